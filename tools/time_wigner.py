"""Time of the correlated Gaussian (Wigner) pair launch (fgnn_wigner_pairs, WignerGenerator.weighted) and of the weighted steps, at
32 pairs of N = 50 and N = 200 vertices.

(a) the launch through ``WignerGenerator.weighted`` (two allocations + the launch): `dense`, `levels` (a table of 3 noise values),
    `support` (a Regular / ErdosRenyi PairGenerator's words mask both sides: its own launch rides in the figure, `support_bits_only`
    is that launch alone), `permute` (fgnn_planted_perm + the launch), and `torch_compose`, a torch composition of the same
    distribution -- two randn, symmetrise by triu + transpose, combine, row sums into the diagonal of channel 1;
(b) ``FgnnTrainer.eval_step`` on those pairs without and with a WeightedQapMeter (the fp32 decode chain; plain and with two_opt);
(c) the untouched paths against the parent commit's library (--parent-lib, loaded beside the first; the same Python drives both):
    ``eval_step_bits(qap_meter=)`` on a PairGenerator's words, and the raw fgnn_pairgen_indexed launch, whose vertex-count code moved
    to the header it now shares with wigner.hip;
(d) for the record, not a test: the recovery of ``qap.faq(weighted=True)`` from the barycenter on relabelled Wigner pairs across a few
    noise values s -- accuracy against the planted labels and the objective over the planted one.

Protocol (tools/time_pairgen_indexed.py): device events on one stream, one warm-up call per variant, then WINDOWS = 7 rounds in
which the variants take turns with one window of `reps` calls each; reported per variant: the median window and the spread
(slowest - fastest window) of the same run.  A difference is distinguishable when it exceeds the larger of the two spreads.
usage: python tools/time_wigner.py [--reps 20] [--sizes 50,200] [--parent-lib lib.so] [--out profiles/wigner_time.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from graph_neural_net_amd import _lib, qap
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.evaluation import QapMeter, WeightedQapMeter
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.trainer import FgnnTrainer
from graph_neural_net_amd.wigner import WignerGenerator
from time_pairgen_indexed import DEV, WINDOWS, alternate, check, pairgen_args, row
from time_restarts import load_parent, through

B = 32
NOISES = (0.0, 0.2, 0.4, 0.6)


def torch_compose(N, s):
    """the same law from torch operations: A, Z symmetric N(0, 1/N) with a zero diagonal, B = rho A + s Z, both as (B, 2, N, N)"""
    rho, c = (1.0 - s * s) ** 0.5, N ** -0.5
    def run():
        g = torch.randn(2, B, N, N, device=DEV).triu_(1)
        g = (g + g.transpose(2, 3)) * c
        a, b = g[0], rho * g[0] + s * g[1]
        out = torch.zeros(2, B, 2, N, N, device=DEV)
        out[0, :, 0], out[1, :, 0] = a, b
        torch.diagonal(out[:, :, 1], dim1=2, dim2=3).copy_(torch.stack([a.sum(-1), b.sum(-1)]))
        return out
    return run


def recovery(N):
    out = {}
    for s in NOISES:
        x1, x2, _, lab = WignerGenerator(N, noise=s, seed=1, device=DEV).weighted(0, B, permute=True)
        f = qap.faq(x1, x2, labels=lab, weighted=True)
        planted = qap.objective_weighted(x1, x2, lab, None)['qap']
        out['s%g' % s] = {'acc': float(f['acc'].double().mean()) / N, 'qap_ratio': float((f['qap'].double() / planted.double()).mean()),
                          'recovered_pairs': int((f['acc'] == N).sum())}
    return out


def one_size(N, reps, parent):
    lib = _lib.load()
    stream = _lib.stream_ptr()
    gen = WignerGenerator(N, noise=0.3, seed=1, device=DEV)
    sup = PairGenerator(N, 'Regular', 'ErdosRenyi', noise=0.1, seed=1, device=DEV)
    masked = WignerGenerator(N, noise=0.3, seed=1, support=sup, device=DEV)
    levels = gen.levels((0.0, 0.3, 0.6))
    level = torch.arange(B, dtype=torch.int32, device=DEV) % 3
    index = torch.arange(B, dtype=torch.int64, device=DEV)
    variants = {'dense': lambda: gen.weighted(0, B), 'levels': lambda: gen.weighted(index=index, levels=levels, level=level),
                'support': lambda: masked.weighted(0, B), 'support_bits_only': lambda: sup.bits(0, B),
                'permute': lambda: gen.weighted(0, B, permute=True), 'torch_compose': torch_compose(N, 0.3)}
    # the steps
    lay = ParamLayout(2, 2, 32, 32, 3)
    tr = FgnnTrainer(lay, lay.init_flat(7, DEV))
    x1, x2, _, lab = gen.weighted(0, B, permute=True)
    b1, b2, _, blab = sup.bits(0, B, permute=True)
    wm, bm = WeightedQapMeter(DEV), QapMeter(DEV)
    variants.update({
        'eval_step': lambda: tr.eval_step(x1, x2, labels=lab),
        'eval_step_meter': lambda: tr.eval_step(x1, x2, labels=lab, qap_meter=wm),
        'eval_step_meter_two_opt': lambda: tr.eval_step(x1, x2, labels=lab, qap_meter=wm, two_opt=True),
        'eval_step_bits_meter': lambda: tr.eval_step_bits(b1, b2, labels=blab, qap_meter=bm)})
    outs = [torch.empty(B, N, (N + 31) // 32, dtype=torch.int32, device=DEV) for _ in range(2)]
    a_gen = pairgen_args(sup, 0, outs)
    variants['pairgen_indexed'] = lambda: check(lib.fgnn_pairgen_indexed(a_gen, index.data_ptr(), stream))
    if parent is not None:
        variants['eval_step_bits_meter_parent_lib'] = through(parent, lambda: tr.eval_step_bits(b1, b2, labels=blab, qap_meter=bm))
        variants['pairgen_indexed_parent_lib'] = lambda: check(parent.fgnn_pairgen_indexed(a_gen, index.data_ptr(), stream))
    t = alternate(variants, reps)
    r = row(t)
    res = {'n_vertices': N, 'pairs': B, 'reps': reps, 'bytes_written': 16 * N * N * B, 'times': r, 'faq_recovery': recovery(N)}
    if parent is not None:
        for name in ('eval_step_bits_meter', 'pairgen_indexed'):
            d, spread = round(t[name][0] - t[name + '_parent_lib'][0], 2), max(r[name]['spread_us'], r[name + '_parent_lib']['spread_us'])
            res['%s_minus_parent' % name] = dict(us=d, spread_us=spread, distinguishable=abs(d) > spread)
    print('N %d  ' % N + '  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
    print('N %d  faq recovery %s' % (N, json.dumps(res['faq_recovery'])), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sizes', default='50,200')
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=None)
    o = ap.parse_args()
    _lib.load()
    parent = load_parent(o.parent_lib) if o.parent_lib else None
    res = {'tool': 'time_wigner', 'windows': WINDOWS, 'parent_lib': bool(parent), 'sizes': []}
    line = json.dumps(res)
    for n in map(int, o.sizes.split(',')):          # (the file is rewritten after every size: a long run leaves what it finished)
        res['sizes'].append(one_size(n, o.reps if n <= 64 else max(1, o.reps // 4), parent))
        line = json.dumps(res)
        if o.out:
            os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
            with open(o.out, 'w') as f:
                f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
