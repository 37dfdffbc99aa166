"""Price of the decode epochs (evaluation.decode_scores, csrc/qap_fold.hip) on the cfg2 shape: 4 blocks, Regular N = 50 with
ErdosRenyi noise, 32 pairs handed over as bit-packed adjacency, structured block 1.

(a) fgnn_qap_fold on a batch's per-pair tensors (with perm / refined) against the torch composition that forms the same sums from
    them: the two row comparisons and their per-pair counts, the fp64 ratio, the masks of the matched pairs and the add into an
    epoch vector.
(b) `eval_step_bits` with and without `qap_meter=`, for refine=0 and refine=10.
(c) with --parent-root, the root of a built checkout of the parent commit: that checkout's `eval_step_bits` in the same process,
    taking turns with this one's `eval_step_bits` without the new arguments.

Protocol (tools/time_pairgen_indexed.py): device events on one stream, warm-up, then WINDOWS rounds in which the variants take turns
with one window of `reps` calls each; reported per variant: the median window and the spread (fastest - slowest window) of the same
run.  `exceeds_spread` says whether a difference is larger than the larger of the two spreads.
usage: python tools/time_decode.py [--reps 100] [--precision fp32|bf16] [--parent-root DIR] [--out file.json]"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from graph_neural_net_amd import _lib
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.evaluation import EvalMeter, QapMeter, decode_scores
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.trainer import FgnnTrainer
from time_pairgen_indexed import DEV, WINDOWS, alternate
from time_ranks import added, parent_package

B, N = 32, 50
REFINE = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--precision', default='fp32', choices=('fp32', 'bf16'))
    ap.add_argument('--parent-root', default=None)
    ap.add_argument('--out', default=None)
    o = ap.parse_args()
    lay = ParamLayout(2, 4, 32, 32, 3)
    p0 = lay.init_flat(0, DEV)
    gen = PairGenerator(N, 'Regular', 'ErdosRenyi', seed=1, device=DEV)
    b1, b2 = gen.bits(0, B)[:2]
    tr = FgnnTrainer(lay, p0.clone(), lr=1e-3, capture=True, precision=o.precision, block1='structured')
    meter, qm0, qm10 = EvalMeter(DEV), QapMeter(DEV), QapMeter(DEV)
    steps = {'eval_step_bits_decode': lambda: tr.eval_step_bits(b1, b2, meter=meter, qap_meter=qm0),
             'eval_step_bits_decode_refine': lambda: tr.eval_step_bits(b1, b2, meter=meter, qap_meter=qm10, refine=REFINE),
             'eval_step_bits': lambda: tr.eval_step_bits(b1, b2, meter=meter)}
    if o.parent_root:
        parent_package(o.parent_root)
        ptrainer, pengine, peval = (importlib.import_module('fgnn_parent.' + m) for m in ('trainer', 'engine', 'evaluation'))
        assert not hasattr(peval, 'QapMeter'), 'the parent checkout already has the decode epochs'
        par = ptrainer.FgnnTrainer(pengine.ParamLayout(2, 4, 32, 32, 3), p0.clone(), lr=1e-3, capture=True, precision=o.precision,
                                   block1='structured')
        pmeter = peval.EvalMeter(DEV)
        steps['parent_eval_step_bits'] = lambda: par.eval_step_bits(b1, b2, meter=pmeter)
    for _ in range(5):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()
    ta = alternate(steps, o.reps)
    assert qm0.result()['pairs'] > 0 and qm10.result()['pairs'] > 0 and meter.result()['pairs'] > 0

    # (a) the fold alone, on the per-pair tensors of one decoded batch
    scores = tr._engine(2 * B, N, False).scores.clone()
    d = decode_scores(scores, b1, b2, refine=REFINE)
    assign, perm, q, planted, refined = d['assign'], d['perm'], d['qap'], d['planted'], d['refined']
    record = QapMeter(DEV)
    correct = torch.empty(B, dtype=torch.int32, device=DEV)
    rcorrect = torch.empty(B, dtype=torch.int32, device=DEV)
    ratio = torch.empty(B, dtype=torch.float64, device=DEV)
    target = torch.arange(N, dtype=torch.int32, device=DEV)[None, :]
    epoch = torch.zeros(len(QapMeter.FIELDS) - 1, dtype=torch.float64, device=DEV)

    def new():
        _lib.call('fgnn_qap_fold', _lib.ptr(assign), _lib.ptr(perm), None, _lib.ptr(q), _lib.ptr(planted), _lib.ptr(refined), None, B, N,
                  B, _lib.ptr(correct), _lib.ptr(rcorrect), _lib.ptr(ratio), _lib.ptr(record.buf), _lib.stream_ptr())

    def torch_chain():
        c, rc = (assign == target).sum(1), (perm == target).sum(1)
        ok = q >= 0
        has = ok & (planted > 0)
        r = torch.where(has, q.double() / planted.double(), q.new_zeros((), dtype=torch.float64))
        z = q.new_zeros(())
        sums = [r.sum(), has.sum(), torch.where(ok, q, z).sum(), torch.where(ok, planted, z).sum(), c.sum(), torch.where(ok, refined, z).sum(),
                rc.sum(), (ok & (q >= planted)).sum(), (c == N).sum(), (ok & (refined > q)).sum(), (~ok).sum(), q.new_tensor(B * N),
                q.new_tensor(B)]
        epoch.add_(torch.stack([s.double() for s in sums]))
        return c, rc, r

    new()
    c_t, rc_t, r_t = torch_chain()
    assert torch.equal(correct.long(), c_t) and torch.equal(rcorrect.long(), rc_t) and torch.equal(ratio, r_t), \
        'the two sides do not give the same per-pair values'
    rec = record.record()
    assert [float(rec[k]) for k in QapMeter.FIELDS[1:-1]] == epoch[1:].tolist(), 'the two sides do not give the same sums'
    tb = alternate({'qap_fold': new, 'torch_chain': torch_chain}, o.reps)
    res = {'tool': 'time_decode', 'reps': o.reps, 'windows': WINDOWS, 'precision': o.precision, 'pairs': B, 'n_vertices': N,
           'refine': REFINE, 'kernels': added(tb, 'qap_fold', 'torch_chain'),
           'step': added(ta, 'eval_step_bits_decode', 'eval_step_bits'),
           'step_refine': {k: v for k, v in added(ta, 'eval_step_bits_decode_refine', 'eval_step_bits').items()
                           if k in ('eval_step_bits_decode_refine_minus_eval_step_bits_us', 'spread_us', 'exceeds_spread')}}
    if o.parent_root:
        res['step_vs_parent'] = {k: v for k, v in added(ta, 'eval_step_bits', 'parent_eval_step_bits').items()
                                 if k in ('eval_step_bits_minus_parent_eval_step_bits_us', 'spread_us', 'exceeds_spread')}
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
