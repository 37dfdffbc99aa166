"""Price and worth of seeds taken from the model's own scores (qap.confident_seeds, csrc/seed_select.hip) on the shapes of the
README's QAP table: Regular N = 50 and N = 200 with ErdosRenyi noise 0.1, 32 relabelled (permute=True) pairs as bit-packed
adjacency (seed 1), scores from a 4-block model of 32 features.

(a) the fgnn_confident_seeds launch against the torch composition that yields the same integers (topk(2) for the margin, two argmax
    calls, a gather for mutual best, an argsort for the order), with the verdict whether the two seed vectors agree;
(b) eval_step_bits(qap_meter=, faq=True) with and without seeds='scores' (and with a SeedMeter on both);
(c) the unseeded step of THIS library and, with --parent-lib, of the parent commit's build (child processes that load it through
    FGNN_LIB and take turns): the unseeded path was not touched, so the expectation is no change beyond the spread;
(d) worth, after the 100-step fit of tools/time_faq_warm.py, for the step with seeds='scores' and the step without:
    seed_precision, seeds per pair, free_acc (the rows WITHOUT a seed the FAQ stage got right; without seeds every row is free), and
    the average FAQ rounds -- also for the untrained model, and for the 8 clearest seeds per pair (count=8).

Protocol (tools/time_pairgen_indexed.py): device events on one stream, warm-up, then WINDOWS = 7 rounds in which the variants take
turns with one window of `reps` calls each; reported per variant: the median window and the spread of the same run.
usage: python tools/time_confident_seeds.py [--reps 5] [--sizes 50,200] [--parent-lib lib.so] [--out profiles/confident_seeds_time.json]"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from graph_neural_net_amd import _lib

if os.environ.get('FGNN_LIB'):
    _lib.load(allow_missing=True)          # (an older build lacks fgnn_confident_seeds; the leg it is asked for does not call it)
from graph_neural_net_amd import qap
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.evaluation import EvalMeter, QapMeter, SeedMeter
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.sampler import EpochSampler
from graph_neural_net_amd.trainer import FgnnTrainer
from time_pairgen_indexed import DEV, WINDOWS, alternate, row

B = 32
FIT_EXAMPLES, FIT_EPOCHS = 640, 5          # 5 epochs of 20 steps = 100 steps


def torch_confident(s):
    """The integers of qap.confident_seeds(s) (no cap, min_margin 0, finite scores) from torch calls -> (seeds, order)"""
    n = s.shape[-1]
    top = torch.topk(s, 2, dim=2).values
    margin = top[:, :, 0] - top[:, :, 1]
    c, r = s.argmax(2), s.argmax(1)
    rows = torch.arange(n, device=s.device).expand_as(c)
    cand = torch.gather(r, 1, c) == rows
    seeds = torch.where(cand, c, torch.full_like(c, -1)).to(torch.int32)
    order = torch.argsort(torch.where(cand, margin, torch.full_like(margin, -1.0)), dim=1, descending=True, stable=True)
    return seeds, order


def setup(N):
    lay = ParamLayout(2, 4, 32, 32, 3)
    gen = PairGenerator(N, 'Regular', 'ErdosRenyi', noise=0.1, seed=1, device=DEV)
    b1, b2, _, lab = gen.bits(0, B, permute=True)
    tr = FgnnTrainer(lay, lay.init_flat(0, DEV), lr=1e-3)
    return gen, tr, b1, b2, lab


def worth(tr, b1, b2, lab):
    out = {}
    for k, kw in (('faq', {}), ('faq_seeds_scores', {'seeds': 'scores'}), ('faq_seeds_top8', {'seeds': {'from': 'scores', 'count': 8}})):
        qm, sm = QapMeter(DEV), SeedMeter(DEV)
        dec = tr.eval_step_bits(b1, b2, labels=lab, qap_meter=qm, faq=True, seed_meter=sm, **kw)['decode']
        q, r = qm.result(), sm.result()
        out[k] = {'seed_precision': r['seed_precision'], 'seeds_per_pair': r['seeds_per_pair'], 'free_acc': r['free_acc'],
                  'clean': r['clean'], 'exact_free': r['exact_free'], 'acc_hungarian': q['acc'], 'acc_faq_all_rows': q['refined_acc'],
                  'faq_nit_mean': float(dec['faq_nit'].double().mean()), 'faq_status_2': int((dec['faq_status'] == 2).sum())}
    return out


def unchanged_leg(sizes, reps):
    """eval_step_bits(qap_meter=, faq=True) without seeds, alone in this process (whatever library FGNN_LIB names)"""
    res = {}
    for N in sizes:
        _, tr, b1, b2, lab = setup(N)
        meter, qm = EvalMeter(DEV), QapMeter(DEV)
        t = alternate({'step': lambda: tr.eval_step_bits(b1, b2, labels=lab, meter=meter, qap_meter=qm, faq=True)},
                      reps if N <= 64 else max(2, reps // 2))
        res[str(N)] = row(t)['step']
    return res


def parent_comparison(parent_lib, sizes, reps):
    """Child processes that take turns: the parent build, this build, twice each -> {'parent': [..], 'own': [..]} per size"""
    out = {'parent': [], 'own': []}
    for who in ('parent', 'own', 'parent', 'own'):
        env = dict(os.environ)
        env.pop('FGNN_LIB', None)
        if who == 'parent':
            env['FGNN_LIB'] = os.path.abspath(parent_lib)
        cmd = [sys.executable, os.path.abspath(__file__), '--leg', 'unchanged', '--sizes', ','.join(map(str, sizes)), '--reps', str(reps)]
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, check=True)
        out[who].append(json.loads(p.stdout.strip().splitlines()[-1]))
    return out


def one_size(N, reps):
    gen, tr, b1, b2, lab = setup(N)
    tr.eval_step_bits(b1, b2, labels=lab)           # (the engine's buffers exist from here on)
    s = tr._eval_forward(B, N, None, bits=torch.cat([b1, b2]).contiguous()).clone()
    # (a)
    mine = qap.confident_seeds(s, return_margin=True)
    seeds, order = torch_confident(s)
    agree = bool(torch.equal(mine['seeds'], seeds))
    ta = alternate({'confident_seeds_launch': lambda: qap.confident_seeds_device(s, None), 'torch_composition': lambda: torch_confident(s)},
                   reps * 4)
    # (d) untrained, then (b), then the fit and (d) again
    quality = {'untrained': worth(tr, b1, b2, lab)}
    meter = EvalMeter(DEV)
    kinds = {'faq': {}, 'faq_seed_meter': {'seed_meter': SeedMeter(DEV)}, 'faq_seeds_scores': {'seeds': 'scores'},
             'faq_seeds_scores_seed_meter': {'seeds': 'scores', 'seed_meter': SeedMeter(DEV)}}
    meters = {k: QapMeter(DEV) for k in kinds}
    steps = {k: (lambda k=k: tr.eval_step_bits(b1, b2, labels=lab, meter=meter, qap_meter=meters[k], faq=True, **kinds[k])) for k in kinds}
    tb = alternate(steps, reps)
    hist = tr.fit(gen, EpochSampler(FIT_EXAMPLES, seed=1), gen, EpochSampler(B, shuffle=False), epochs=FIT_EPOCHS, batch_size=B, permute=True,
                  decode_seeds='scores', decode_faq=True)
    quality['after_fit'] = worth(tr, b1, b2, lab)
    tc = alternate(steps, reps)                     # the same steps on the trained model: more seeds, fewer rounds
    res = {'n_vertices': N, 'pairs': B, 'reps': reps, 'launch_equals_torch': agree, 'seeds_per_pair_untrained': float(mine['nseeds'].double().mean()),
           'select': row(ta), 'steps_untrained': row(tb), 'steps_after_fit': row(tc),
           'fit': {'steps': FIT_EPOCHS * (FIT_EXAMPLES // B), 'lr': 1e-3, 'val_loss': [h['val_loss'] for h in hist],
                   'val_acc': [h['val_acc'] for h in hist], 'val_seed_precision': [h['val_seed_precision'] for h in hist],
                   'val_free_acc': [h['val_free_acc'] for h in hist]}, 'quality': quality}
    for t in (ta, tb, tc):
        print('N %d  ' % N + '  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
    print('N %d  launch equals torch: %s  quality %s' % (N, agree, json.dumps(quality)), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sizes', default='50,200')
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--leg', default=None, choices=[None, 'unchanged'])
    ap.add_argument('--out', default=None)
    o = ap.parse_args()
    sizes = list(map(int, o.sizes.split(',')))
    if o.leg == 'unchanged':
        print(json.dumps(unchanged_leg(sizes, o.reps)))
        return
    res = {'tool': 'time_confident_seeds', 'windows': WINDOWS, 'sizes': []}

    def write():
        line = json.dumps(res)
        if o.out:
            os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
            with open(o.out, 'w') as f:
                f.write(line + '\n')
        return line
    for n in sizes:                                 # (the file is rewritten after every size: a long run leaves what it finished)
        res['sizes'].append(one_size(n, o.reps if n <= 64 else max(2, o.reps // 2)))
        write()
    if o.parent_lib:
        res['unchanged_path'] = parent_comparison(o.parent_lib, sizes, o.reps)
        print('unchanged path %s' % json.dumps(res['unchanged_path']), flush=True)
    print(write())


if __name__ == '__main__':
    main()
