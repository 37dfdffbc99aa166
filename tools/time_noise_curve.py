"""Price of the noise curve's two kernels and of the curve itself for K = 8 noise levels on the cfg2 shape: 4 blocks, Regular N = 50
with ErdosRenyi noise, 32 pairs handed over as bit-packed adjacency, structured block 1.

(a) one fgnn_pairgen_levels launch (32 pairs of mixed levels) against fgnn_pairgen_indexed on the same index list: the same work, so
    the expectation is parity.  With --parent-lib, `parent_indexed` = fgnn_pairgen_indexed of another build of the library (the commit
    before the levels entry point; loaded beside the first, only that entry point is taken from it): the kernel the new
    instantiation must not have moved.
(b) fgnn_eval_fold_bins (8 records) against fgnn_eval_fold on the same rows.
(c) FgnnTrainer.noise_curve over K * M = 8 * 64 examples against K separate `evaluate` passes of M = 64 with single-noise generators:
    16 steps of 32 pairs on both sides.  The tool also says whether the two give the same records (a pair's scores in a batch of
    mixed levels against the same pair in a batch of its own level).

Protocol (tools/time_pairgen_indexed.py): device events on one stream, warm-up, then WINDOWS rounds in which the variants take turns
with one window of `reps` calls each; reported per variant: the median window and the spread (fastest - slowest window) of the same
run.  A difference counts only when it exceeds the larger spread.
usage: python tools/time_noise_curve.py [--reps 100] [--precision fp32|bf16] [--parent-lib lib.so] [--out file.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from graph_neural_net_amd import _lib
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.evaluation import BinnedEvalMeter, EvalMeter
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.sampler import EpochSampler, epoch_index
from graph_neural_net_amd.trainer import FgnnTrainer
from time_pairgen_indexed import DEV, EXAMPLES, WINDOWS, alternate, check, pairgen_args, row

B, N, K, M = 32, 50, 8, 64
NOISES = tuple(0.05 * k for k in range(K))


def compare(t, new, old):
    r = row(t)
    r['%s_minus_%s_us' % (new, old)] = round(t[new][0] - t[old][0], 2)
    r['spread_us'] = max(r[new]['spread_us'], r[old]['spread_us'])
    r['distinguishable'] = abs(t[new][0] - t[old][0]) > r['spread_us']
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--precision', default='fp32', choices=('fp32', 'bf16'))
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=None)
    o = ap.parse_args()
    lib = _lib.load()
    parent = None
    if o.parent_lib:
        parent = C.CDLL(os.path.abspath(o.parent_lib))
        parent.fgnn_pairgen_indexed.argtypes = [C.POINTER(_lib.PairgenArgs), C.c_void_p, C.c_void_p]
        parent.fgnn_pairgen_indexed.restype = C.c_int
    stream = _lib.stream_ptr()
    gen = PairGenerator(N, 'Regular', 'ErdosRenyi', noise=NOISES[1], seed=1, device=DEV)
    levels = gen.levels(NOISES)

    # (a) the generator launches, into the same preallocated outputs
    idx = epoch_index(1, 3, EXAMPLES, 5 * B, B, device=DEV)
    level = (torch.arange(B, device=DEV) % K).to(torch.int32)
    outs = [torch.empty(B, N, 2, dtype=torch.int32, device=DEV) for _ in range(2)]
    a = pairgen_args(gen, 0, outs)
    variants = {'levels': lambda: check(lib.fgnn_pairgen_levels(a, idx.data_ptr(), levels.table.data_ptr(), K, level.data_ptr(), stream)),
                'indexed': lambda: check(lib.fgnn_pairgen_indexed(a, idx.data_ptr(), stream))}
    if parent:
        variants['parent_indexed'] = lambda: check(parent.fgnn_pairgen_indexed(a, idx.data_ptr(), stream))
    ones = torch.ones(B, dtype=torch.int32, device=DEV)          # every pair at level 1 is the generator's own launch
    assert all(torch.equal(x, y) for x, y in zip(gen.bits(index=idx, levels=levels, level=ones)[:2], gen.bits(index=idx)[:2]))
    ta = alternate(variants, o.reps)
    ra = compare(ta, 'levels', 'indexed')
    if parent:
        ra['indexed_minus_parent_indexed_us'] = round(ta['indexed'][0] - ta['parent_indexed'][0], 2)
        ra['indexed_equals_parent'] = abs(ta['indexed'][0] - ta['parent_indexed'][0]) <= max(ra['indexed']['spread_us'],
                                                                                                ra['parent_indexed']['spread_us'])

    # (b) the folds, on the rows of one evaluation of real scores
    lay = ParamLayout(2, 4, 32, 32, 3)
    tr = FgnnTrainer(lay, lay.init_flat(0, DEV), lr=1e-3, precision=o.precision, block1='structured')
    b1, b2 = gen.bits(index=idx, levels=levels, level=level)[:2]
    tr.eval_step_bits(b1, b2)
    scores = tr._engine(2 * B, N, False).scores.clone()
    cost = torch.empty(B, N, N, dtype=torch.float32, device=DEV)
    row_ce = torch.empty(B, N, dtype=torch.float32, device=DEV)
    row_hit = torch.empty(B, N, dtype=torch.int32, device=DEV)
    _lib.call('fgnn_eval_pairs', _lib.ptr(scores), None, None, B, N, _lib.ptr(cost), N * N, N, _lib.ptr(row_ce), _lib.ptr(row_hit), stream)
    plain, binned = EvalMeter(DEV), BinnedEvalMeter(DEV, K)
    tb = alternate({'fold_bins': lambda: _lib.call('fgnn_eval_fold_bins', _lib.ptr(row_ce), _lib.ptr(row_hit), None, None, B, N, B,
                                                   _lib.ptr(level), K, None, None, _lib.ptr(binned.buf), stream),
                    'fold': lambda: _lib.call('fgnn_eval_fold', _lib.ptr(row_ce), _lib.ptr(row_hit), None, None, B, N, B, None, None,
                                              _lib.ptr(plain.buf), stream)}, o.reps)
    assert sum(r['pairs'] for r in binned.record()) == plain.record()['pairs']

    # (c) the curve against K single-noise evaluation passes
    singles = [PairGenerator(N, 'Regular', 'ErdosRenyi', noise=v, seed=1, device=DEV) for v in NOISES]
    sampler = EpochSampler(M, shuffle=False)

    def passes():
        return [tr.evaluate(g, sampler, B) for g in singles]

    curve = tr.noise_curve(gen, NOISES, M, B).record()
    apart = [m.record() for m in passes()]
    fields = ('nodes', 'correct_lsap', 'correct_max', 'pairs')
    same = {'counts_equal': all(c[f] == s[f] for c, s in zip(curve, apart) for f in fields),
            'ce_sum_bits_equal': all(c['ce_sum'] == s['ce_sum'] for c, s in zip(curve, apart)),
            'ce_sum_max_rel_diff': max(abs(c['ce_sum'] - s['ce_sum']) / s['ce_sum'] for c, s in zip(curve, apart))}
    tc = alternate({'noise_curve': lambda: tr.noise_curve(gen, NOISES, M, B), 'evaluate_passes': passes}, max(1, o.reps // 10))

    res = {'tool': 'time_noise_curve', 'reps': o.reps, 'windows': WINDOWS, 'precision': o.precision, 'pairs': B, 'n_vertices': N,
           'levels': K, 'examples_per_level': M, 'parent_lib': bool(parent), 'pairgen': ra, 'fold': compare(tb, 'fold_bins', 'fold'),
           'curve': compare(tc, 'noise_curve', 'evaluate_passes'), 'curve_vs_passes': same,
           'result': tr.noise_curve(gen, NOISES, M, B).result()}
    for t in (ta, tb, tc):
        print('  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
    print('noise_curve against the single-noise passes: %r' % (same,), flush=True)
    line = json.dumps(res)
    print(line)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
