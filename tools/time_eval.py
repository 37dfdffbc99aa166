"""Price of a validation step on the device (evaluation.py, csrc/eval.hip) on the cfg2 shape: 4 blocks, Regular N = 50 with
ErdosRenyi noise, 32 pairs handed over as bit-packed adjacency, structured block 1.

(a) `eval_step_bits` -- the forward pass of the training engine + evaluate_scores, nothing read back -- against `train_step_bits`
    of the same trainer class (captured: the fastest way the parent commit has to touch a batch; a trainer user without
    eval_step_bits would have to run it, at three times the work and at the price of self.grads).
(b) fgnn_eval_pairs + fgnn_eval_fold on a batch of scores against what the same outputs cost without them: the eager prologue of
    metrics.lsap_device (masked_fill, log_softmax, negation, contiguous), fgnn_accuracy_max and a torch cross-entropy against the
    identity.  The solver launch is the same on both sides and is left out of both.

Protocol (tools/time_pairgen_indexed.py): device events on one stream, warm-up, then WINDOWS rounds in which the variants take turns
with one window of `reps` calls each; reported per variant: the median window and the spread (fastest - slowest window) of the same
run.  A new-path time counts as lower only when it lies below its counterpart by more than the larger spread.
usage: python tools/time_eval.py [--reps 100] [--precision fp32|bf16] [--out file.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from graph_neural_net_amd import _lib
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.evaluation import EvalMeter
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.trainer import FgnnTrainer
from time_pairgen_indexed import DEV, WINDOWS, alternate, row

B, N = 32, 50


def compare(t, new, old):
    r = row(t)
    r['%s_minus_%s_us' % (new, old)] = round(t[new][0] - t[old][0], 2)
    r['spread_us'] = max(r[new]['spread_us'], r[old]['spread_us'])
    r['lower'] = t[old][0] - t[new][0] > r['spread_us']
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--precision', default='fp32', choices=('fp32', 'bf16'))
    ap.add_argument('--out', default=None)
    o = ap.parse_args()
    lay = ParamLayout(2, 4, 32, 32, 3)
    p0 = lay.init_flat(0, DEV)
    gen = PairGenerator(N, 'Regular', 'ErdosRenyi', seed=1, device=DEV)
    b1, b2 = gen.bits(0, B)[:2]
    make = lambda: FgnnTrainer(lay, p0.clone(), lr=1e-3, capture=True, precision=o.precision, block1='structured')
    train, evalr = make(), make()
    meter = EvalMeter(DEV)
    for _ in range(5):
        train.train_step_bits(b1, b2)
        evalr.eval_step_bits(b1, b2, meter=meter)
    torch.cuda.synchronize()
    ta = alternate({'eval_step_bits': lambda: evalr.eval_step_bits(b1, b2, meter=meter),
                    'eval_step_bits_no_solver': lambda: evalr.eval_step_bits(b1, b2, meter=meter, hungarian=False),
                    'train_step_bits': lambda: train.train_step_bits(b1, b2)}, o.reps)
    assert meter.result()['pairs'] > 0 and torch.isfinite(train.params).all().item()

    scores = evalr._engine(2 * B, N, False).scores.clone()
    nvalid = torch.full((B,), N, dtype=torch.int32, device=DEV)
    cost = torch.empty(B, N, N, dtype=torch.float32, device=DEV)
    row_ce = torch.empty(B, N, dtype=torch.float32, device=DEV)
    row_hit = torch.empty(B, N, dtype=torch.int32, device=DEV)
    correct = torch.empty(B, dtype=torch.int32, device=DEV)
    target = torch.arange(N, device=DEV).repeat(B)
    col = torch.arange(N, device=DEV)[None, None, :]

    def new():
        st = _lib.stream_ptr()
        _lib.call('fgnn_eval_pairs', _lib.ptr(scores), _lib.ptr(nvalid), None, B, N, _lib.ptr(cost), N * N, N, _lib.ptr(row_ce),
                  _lib.ptr(row_hit), st)
        _lib.call('fgnn_eval_fold', _lib.ptr(row_ce), _lib.ptr(row_hit), None, _lib.ptr(nvalid), B, N, B, None, None, _lib.ptr(meter.buf), st)

    def old():
        s = scores.masked_fill(~(col < nvalid[:, None, None]), float('-inf'))          # metrics.lsap_device
        c = (-torch.log_softmax(s.float(), -1)).contiguous()
        _lib.call('fgnn_accuracy_max', _lib.ptr(scores), _lib.ptr(nvalid), B, N, _lib.ptr(correct), _lib.stream_ptr())
        loss = torch.nn.functional.cross_entropy(scores.reshape(B * N, N), target, reduction='sum')
        return c, loss

    tb = alternate({'eval_pairs_fold': new, 'parent_chain': old}, o.reps)
    res = {'tool': 'time_eval', 'reps': o.reps, 'windows': WINDOWS, 'precision': o.precision, 'pairs': B, 'n_vertices': N,
           'step': compare(ta, 'eval_step_bits', 'train_step_bits'), 'kernels': compare(tb, 'eval_pairs_fold', 'parent_chain')}
    for t in (ta, tb):
        print('  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
    line = json.dumps(res)
    print(line)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
