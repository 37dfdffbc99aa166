"""Price of the weighted step (fgnn_pair_weights + fgnn_pair_loss_w + fgnn_score_ce_bwd_w instead of
fgnn_score_ce_bwd with the loss job in fgnn_grad_finalize) in the captured cfg2 training step: 4 blocks, Regular N = 50 with
ErdosRenyi noise, 32 pairs handed over as bit-packed adjacency, structured block 1, one replayed graph per step.

Three trainers in one process from the same parameters and on the same batch: `plain` (no weights: the launches and captured graph of
the commit before the weighted step existed -- its kernels are instruction for instruction those of that commit, so it stands for the
parent's step), `weighted` ('mean' with live = B: unit weights, the same numbers as `plain`) and `mean_of_mean`.  Protocol
(tools/time_grad_guard.py): device events on one stream, warm-up steps for all (capture included), then WINDOWS rounds in which the
variants take turns with one window of `reps` steps each; reported per variant: the median window and the spread (fastest - slowest
window) of the same run.  `weighted_minus_plain_us` beside `spread_us` says whether the difference is distinguishable.
usage: python tools/time_pair_weights.py [--reps 200] [--precision fp32|bf16] [--out file.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.trainer import FgnnTrainer
from time_pairgen_indexed import DEV, WINDOWS, alternate, row

B, N = 32, 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--precision', default='fp32', choices=('fp32', 'bf16'))
    ap.add_argument('--out', default=None)
    o = ap.parse_args()
    lay = ParamLayout(2, 4, 32, 32, 3)
    p0 = lay.init_flat(0, DEV)
    gen = PairGenerator(N, 'Regular', 'ErdosRenyi', seed=1, device=DEV)
    b1, b2 = gen.bits(0, B)[:2]
    make = lambda **kw: FgnnTrainer(lay, p0.clone(), lr=1e-3, capture=True, precision=o.precision, block1='structured', **kw)
    trainers = {'plain': make(), 'weighted': make(), 'mean_of_mean': make(loss_reduction='mean_of_mean')}
    live = torch.tensor([B], dtype=torch.int32, device=DEV)
    steps = {'plain': lambda: trainers['plain'].train_step_bits(b1, b2),
             'weighted': lambda: trainers['weighted'].train_step_bits(b1, b2, live=live),
             'mean_of_mean': lambda: trainers['mean_of_mean'].train_step_bits(b1, b2, live=live)}
    for fn in steps.values():            # capture + a few replays
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    assert torch.equal(trainers['plain'].params, trainers['weighted'].params)       # unit weights: the same step, bit for bit
    t = alternate(steps, o.reps)
    assert all(torch.isfinite(tr.params).all().item() for tr in trainers.values())
    assert torch.equal(trainers['plain'].params, trainers['weighted'].params)
    r = row(t)
    r['weighted_minus_plain_us'] = round(t['weighted'][0] - t['plain'][0], 2)
    r['mean_of_mean_minus_plain_us'] = round(t['mean_of_mean'][0] - t['plain'][0], 2)
    r['spread_us'] = max(v['spread_us'] for v in (r['plain'], r['weighted'], r['mean_of_mean']))
    r['distinguishable'] = abs(r['weighted_minus_plain_us']) > r['spread_us']
    res = {'tool': 'time_pair_weights', 'reps': o.reps, 'windows': WINDOWS, 'precision': o.precision, 'pairs': B, 'n_vertices': N,
           'parameters': lay.total, 'cfg2_captured_step': r}
    print('  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
    print('weighted - plain = %.2f us per step, mean_of_mean - plain = %.2f us, spread %.2f us'
          % (r['weighted_minus_plain_us'], r['mean_of_mean_minus_plain_us'], r['spread_us']), flush=True)
    line = json.dumps(res)
    print(line)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
