"""Price and quality of the Sinkhorn launch (qap.sinkhorn, csrc/sinkhorn.hip) and of the faq= stage of the decode chain
(evaluation.decode_scores) on the shapes of the README's QAP table: Regular N = 50 and N = 200 with ErdosRenyi noise 0.1, 32
relabelled (permute=True) pairs as bit-packed adjacency (seed 1), scores from a 4-block model of 32 features.

(a) the Sinkhorn launch (tau = 1, 20 iterations) against the torch composition that gives the same matrix (2 x 20 logsumexp calls
    with their broadcast additions, one exp), with the largest difference of the two matrices;
(b) eval_step_bits(qap_meter=) without the stage, with it from the scores and from the barycenter, and each followed by two_opt;
    with --parent-lib the step WITHOUT the stage is also timed against another build of the library (the parent commit's), in child
    processes that take turns -- the path this change must leave alone;
(c) the QAP ratio (sum of the objectives over the sum of the planted ones, over the 32 pairs) of the Hungarian matching, of FAQ from
    the barycenter, of FAQ from the scores, and of each FAQ start followed by two_opt -- once with the scores of the untrained
    model and once after a short fit inside the tool (FIT_EPOCHS epochs of FIT_EXAMPLES / 32 steps on planted pairs, lr 1e-3).

Protocol (tools/time_pairgen_indexed.py): device events on one stream, warm-up, then WINDOWS = 7 rounds in which the variants take
turns with one window of `reps` calls each; reported per variant: the median window and the spread of the same run.
usage: python tools/time_faq_warm.py [--reps 5] [--sizes 50,200] [--parent-lib lib.so] [--out profiles/faq_warm_time.json]"""
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
    _lib.load(allow_missing=True)          # (an older build lacks fgnn_sinkhorn; the leg it is asked for does not call it)
from graph_neural_net_amd import qap
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.evaluation import EvalMeter, QapMeter
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.sampler import EpochSampler
from graph_neural_net_amd.trainer import FgnnTrainer
from time_pairgen_indexed import DEV, WINDOWS, alternate, row

B = 32
TAU, ITERS = 1.0, 20
FIT_EXAMPLES, FIT_EPOCHS = 640, 5          # 5 epochs of 20 steps = 100 steps
CHAINS = {'hungarian': {}, 'faq_barycenter': {'faq': {'P0': 'barycenter'}}, 'faq_scores': {'faq': True},
          'faq_barycenter_two_opt': {'faq': {'P0': 'barycenter'}, 'two_opt': True}, 'faq_scores_two_opt': {'faq': True, 'two_opt': True}}


def torch_sinkhorn(s, tau, iters):
    Z = s / tau
    f = torch.zeros(s.shape[0], s.shape[1], device=s.device)
    g = torch.zeros_like(f)
    for _ in range(iters):
        f = -torch.logsumexp(Z + g[:, None, :], 2)
        g = -torch.logsumexp(Z + f[:, :, None], 1)
    return torch.exp(Z + f[:, :, None] + g[:, None, :])


def setup(N):
    lay = ParamLayout(2, 4, 32, 32, 3)
    gen = PairGenerator(N, 'Regular', 'ErdosRenyi', noise=0.1, seed=1, device=DEV)
    b1, b2, _, lab = gen.bits(0, B, permute=True)
    tr = FgnnTrainer(lay, lay.init_flat(0, DEV), lr=1e-3)
    return gen, tr, b1, b2, lab


def ratios(tr, b1, b2, lab):
    out = {}
    for k, kw in CHAINS.items():
        m = QapMeter(DEV)
        dec = tr.eval_step_bits(b1, b2, labels=lab, qap_meter=m, **kw)['decode']
        r = m.result()
        out[k] = {'qap_ratio': r.get('refined_qap_ratio', r['qap_ratio']), 'acc': r.get('refined_acc', r['acc'])}
        if 'faq' in kw:
            out[k].update({'faq_nit_mean': float(dec['faq_nit'].double().mean()), 'faq_status_2': int((dec['faq_status'] == 2).sum()),
                           'faq_stopped_on_tol': int((dec['faq_status'] == 0).sum())})
            if dec['sinkhorn_err'] is not None:
                out[k]['sinkhorn_err_max'] = float(dec['sinkhorn_err'].max())
    return out


def unchanged_leg(sizes, reps):
    """eval_step_bits(qap_meter=) without the stage, alone in this process (whatever library FGNN_LIB names) -> {N: (median, lo, hi)}"""
    res = {}
    for N in sizes:
        _, tr, b1, b2, lab = setup(N)
        meter, qm = EvalMeter(DEV), QapMeter(DEV)
        t = alternate({'decode': lambda: tr.eval_step_bits(b1, b2, labels=lab, meter=meter, qap_meter=qm)}, reps if N <= 64 else max(2, reps // 2))
        res[str(N)] = row(t)['decode']
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
    scores = tr.eval_step_bits(b1, b2, labels=lab)  # (the engine's buffers exist from here on)
    s = tr._eval_forward(B, N, None, bits=torch.cat([b1, b2]).contiguous()).clone()
    del scores
    # (a)
    mine, theirs = qap.sinkhorn(s, tau=TAU, iters=ITERS), torch_sinkhorn(s, TAU, ITERS)
    ta = alternate({'sinkhorn_launch': lambda: qap.sinkhorn_device(s, None, TAU, ITERS), 'torch_logsumexp': lambda: torch_sinkhorn(s, TAU, ITERS)},
                   reps * 4)
    # (c) untrained, then (b) on the untrained model, then the fit and (c) again
    quality = {'untrained': ratios(tr, b1, b2, lab)}
    meter = EvalMeter(DEV)
    meters = {k: QapMeter(DEV) for k in CHAINS}
    steps = {k: (lambda k=k: tr.eval_step_bits(b1, b2, labels=lab, meter=meter, qap_meter=meters[k], **CHAINS[k])) for k in CHAINS}
    tb = alternate(steps, reps)
    hist = tr.fit(gen, EpochSampler(FIT_EXAMPLES, seed=1), gen, EpochSampler(B, shuffle=False), epochs=FIT_EPOCHS, batch_size=B, permute=True)
    quality['after_fit'] = ratios(tr, b1, b2, lab)
    res = {'n_vertices': N, 'pairs': B, 'reps': reps, 'tau': TAU, 'iters': ITERS, 'sinkhorn': row(ta),
           'sinkhorn_max_abs_diff_to_torch': float((mine['P'] - theirs).abs().max()), 'sinkhorn_err_max': float(mine['err'].max()),
           'steps': row(tb), 'faq_scores_minus_decode_us': round(tb['faq_scores'][0] - tb['hungarian'][0], 2),
           'faq_barycenter_minus_decode_us': round(tb['faq_barycenter'][0] - tb['hungarian'][0], 2),
           'fit': {'steps': FIT_EPOCHS * (FIT_EXAMPLES // B), 'lr': 1e-3, 'val_loss': [h['val_loss'] for h in hist],
                   'val_acc': [h['val_acc'] for h in hist]}, 'quality': quality}
    for t in (ta, tb):
        print('N %d  ' % N + '  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
    print('N %d  quality %s' % (N, json.dumps(quality)), flush=True)
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
    res = {'tool': 'time_faq_warm', 'windows': WINDOWS, 'sizes': []}

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
