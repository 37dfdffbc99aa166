"""Price of the guarded optimizer step (FgnnTrainer(max_grad_norm=..., skip_nonfinite=True): fgnn_grad_guard + fgnn_adam_step_guarded
instead of fgnn_adam_step_dev) in the captured cfg2 training step: 4 blocks, Regular N = 50 with ErdosRenyi noise, 32 pairs handed
over as bit-packed adjacency, structured block 1, one replayed graph per step.

Two trainers in one process, `plain` and `guarded`, from the same parameters and on the same batch; both run the same model work, so
the difference is the guard.  Protocol (tools/time_pairgen_indexed.py): device events on one stream, warm-up steps for both (capture
included), then WINDOWS rounds in which the two take turns with one window of `reps` steps each; reported per variant: the median
window and the spread (fastest - slowest window) of the same run.  `guarded_minus_plain_us` beside `spread_us` (the larger of the two
spreads) says whether the difference is distinguishable.  The guard never fires in the timed steps (finite gradients; the clip bound
is below the norm, so the clipped update is what is timed) -- a skipped update only does less.
usage: python tools/time_grad_guard.py [--reps 200] [--precision fp32|bf16] [--out file.json]"""
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
    trainers = {'plain': make(), 'guarded': make(max_grad_norm=1e-2, skip_nonfinite=True)}
    for tr in trainers.values():            # capture + a few replays
        for _ in range(5):
            tr.train_step_bits(b1, b2)
    torch.cuda.synchronize()
    g = trainers['guarded']
    assert g.skipped_steps.item() == 0 and g.opt.clip_coef.item() < 1.0 and torch.isfinite(g.params).all().item()
    t = alternate({k: (lambda tr=tr: tr.train_step_bits(b1, b2)) for k, tr in trainers.items()}, o.reps)
    assert g.skipped_steps.item() == 0 and all(torch.isfinite(tr.params).all().item() for tr in trainers.values())
    r = row(t)
    r['guarded_minus_plain_us'] = round(t['guarded'][0] - t['plain'][0], 2)
    r['spread_us'] = max(r['guarded']['spread_us'], r['plain']['spread_us'])
    r['distinguishable'] = abs(r['guarded_minus_plain_us']) > r['spread_us']
    res = {'tool': 'time_grad_guard', 'reps': o.reps, 'windows': WINDOWS, 'precision': o.precision, 'pairs': B, 'n_vertices': N,
           'parameters': lay.total, 'cfg2_captured_step': r}
    print('  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
    print('guarded - plain = %.2f us per step, spread %.2f us' % (r['guarded_minus_plain_us'], r['spread_us']), flush=True)
    line = json.dumps(res)
    print(line)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
