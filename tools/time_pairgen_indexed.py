"""Time of pair generation by index list (fgnn_pairgen_indexed, PairGenerator.bits(index=...)) against the contiguous launch
(fgnn_pairgen, bits(first, count)) at the cfg2 batch shape (Regular N = 50, ErdosRenyi noise) with 32 and with 256 pairs, and of the
epoch-index launch (fgnn_epoch_index) alone.  The index list is a window of a shuffled epoch over 20 000 examples; the contiguous
launch makes as many pairs from index 0.

Three variants of the generator launch write into the same preallocated outputs through the raw entry points: `indexed` and
`contiguous` of the library in the tree and, with --parent-lib, `parent` = fgnn_pairgen of another build of the library (the commit
before the indexed entry point; loaded beside the first, only fgnn_pairgen is taken from it).  The Python surface (`bits`, which also
allocates its outputs) is timed in both forms as well.  Protocol: device events on one stream, one warm-up call per variant, then
WINDOWS rounds in which the variants take turns with one window of `reps` calls each; reported per variant: the median window and the
spread (fastest - slowest window) of the same run.  `indexed_minus_contiguous_us` beside `spread_us` (the larger of the two spreads)
says whether a difference is distinguishable.
usage: python tools/time_pairgen_indexed.py [--reps 50] [--parent-lib lib.so] [--out file.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graph_neural_net_amd import _lib
from graph_neural_net_amd.pairgen import FAMILIES, NOISE_MODELS, PairGenerator
from graph_neural_net_amd.sampler import epoch_index

DEV = torch.device('cuda:0')
WINDOWS = 7
EXAMPLES = 20000


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us per call


def alternate(variants, reps):
    """{name: fn} -> {name: (median, fastest, slowest) us}: the variants take turns, one window each per round"""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    w = {k: [] for k in variants}
    for _ in range(WINDOWS):
        for k, fn in variants.items():
            w[k].append(window(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in w.items()}


def pairgen_args(gen, first, outs):
    a = _lib.PairgenArgs()
    a.seed, a.first, a.B, a.N = gen.seed, first, outs[0].shape[0], gen.n_vertices
    a.family, a.noise_model = FAMILIES[gen.generative_model], NOISE_MODELS[gen.noise_model]
    a.edge_density, a.swaps_per_edge = gen.edge_density, gen.swaps_per_edge
    a.thr_edge, a.thr_noise1, a.thr_noise2, a.thr_vertex = gen._thr
    a.bits1, a.bits2, a.nvalid = outs[0].data_ptr(), outs[1].data_ptr(), None
    return a


def check(rc):
    if rc != 0:
        raise RuntimeError(_lib.last_error())


def row(t):
    return {k: dict(us=round(m, 2), us_range=[round(lo, 2), round(hi, 2)], spread_us=round(hi - lo, 2)) for k, (m, lo, hi) in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=None)
    o = ap.parse_args()
    lib = _lib.load()
    parent = None
    if o.parent_lib:
        parent = C.CDLL(os.path.abspath(o.parent_lib))
        parent.fgnn_pairgen.argtypes, parent.fgnn_pairgen.restype = [C.POINTER(_lib.PairgenArgs), C.c_void_p], C.c_int
    gen = PairGenerator(50, 'Regular', 'ErdosRenyi', seed=1, device=DEV)
    stream = _lib.stream_ptr()
    res = {'tool': 'time_pairgen_indexed', 'reps': o.reps, 'windows': WINDOWS, 'parent_lib': bool(parent), 'shapes': {}}
    for B in (32, 256):
        idx = epoch_index(1, 3, EXAMPLES, 5 * B, B, device=DEV)
        outs = [torch.empty(B, 50, 2, dtype=torch.int32, device=DEV) for _ in range(2)]
        a_idx, a_con = pairgen_args(gen, 0, outs), pairgen_args(gen, 0, outs)
        variants = {'indexed': lambda: check(lib.fgnn_pairgen_indexed(a_idx, idx.data_ptr(), stream)),
                    'contiguous': lambda: check(lib.fgnn_pairgen(a_con, stream))}
        if parent:
            variants['parent'] = lambda: check(parent.fgnn_pairgen(a_con, stream))
        variants['bits_indexed'] = lambda: gen.bits(index=idx)
        variants['bits_contiguous'] = lambda: gen.bits(0, B)
        # the two forms make the same pairs when the index is a range
        assert all(torch.equal(x, y) for x, y in zip(gen.bits(7, B)[:2], gen.bits(index=torch.arange(7, 7 + B, device=DEV))[:2]))
        t = alternate(variants, o.reps)
        r = row(t)
        base = 'parent' if parent else 'contiguous'
        r['indexed_minus_%s_us' % base] = round(t['indexed'][0] - t[base][0], 2)
        r['spread_us'] = max(r['indexed']['spread_us'], r[base]['spread_us'])
        r['distinguishable'] = abs(r['indexed_minus_%s_us' % base]) > r['spread_us']
        res['shapes']['cfg2_B%d' % B] = r
        print('B = %3d  ' % B + '  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
        print('         indexed - %s = %.2f us, spread %.2f us' % (base, r['indexed_minus_%s_us' % base], r['spread_us']), flush=True)
    for count in (32, 256, EXAMPLES):
        out = torch.empty(count, dtype=torch.int64, device=DEV)
        t = alternate({'epoch_index': lambda: check(lib.fgnn_epoch_index(1, 3, EXAMPLES, 64, count, out.data_ptr(), stream))}, o.reps)
        res['shapes']['epoch_index_%d' % count] = row(t)
        print('epoch_index, %5d of %d positions: %.2f us (%.2f - %.2f)' % ((count, EXAMPLES) + t['epoch_index']), flush=True)
    line = json.dumps(res)
    print(line)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
