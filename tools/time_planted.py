"""Time of a permuted batch (PairGenerator.bits(permute=True): generate, draw the planted permutations, relabel side 2) against the
plain batch (bits()) at the cfg2 batch shape (Regular N = 50, ErdosRenyi noise) with 32 and with 256 pairs, and of `relabel` on a
(64, 4, 50, 50) spectral side.

With --parent-lib, `parent` is the generator launch of another build of the library (the commit before planted permutations; loaded
beside the first, only fgnn_pairgen is taken from it) writing into preallocated outputs; `generate` is the same raw launch of the
library in the tree.  `bits` and `bits_permuted` are the Python surface, which also allocates its outputs; `perm` and `relabel_bits`
are the two added launches alone.  Protocol (tools/time_pairgen_indexed.py): device events on one stream, one warm-up call per
variant, then WINDOWS rounds in which the variants take turns with one window of `reps` calls each; reported per variant: the median
window and the spread (fastest - slowest window) of the same run.
usage: python tools/time_planted.py [--reps 50] [--parent-lib lib.so] [--out file.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from graph_neural_net_amd import _lib, planted
from graph_neural_net_amd.pairgen import PairGenerator
from time_pairgen_indexed import DEV, WINDOWS, alternate, check, pairgen_args, row


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
    res = {'tool': 'time_planted', 'reps': o.reps, 'windows': WINDOWS, 'parent_lib': bool(parent), 'shapes': {}}
    for B in (32, 256):
        outs = [torch.empty(B, 50, 2, dtype=torch.int32, device=DEV) for _ in range(2)]
        a = pairgen_args(gen, 0, outs)
        b1, b2, _, lab = gen.bits(0, B, permute=True)
        assert torch.equal(b1, gen.bits(0, B)[0]) and torch.equal(planted.relabel(b2, planted.inverse(lab)), gen.bits(0, B)[1])
        variants = {'generate': lambda: check(lib.fgnn_pairgen(a, stream))}
        if parent:
            variants['parent'] = lambda: check(parent.fgnn_pairgen(a, stream))
        variants['bits'] = lambda: gen.bits(0, B)
        variants['bits_permuted'] = lambda: gen.bits(0, B, permute=True)
        variants['perm'] = lambda: planted.planted_permutation(1, 50, 0, B, device=DEV)
        variants['relabel_bits'] = lambda: planted.relabel(b2, lab)
        t = alternate(variants, o.reps)
        r = row(t)
        r['bits_permuted_minus_bits_us'] = round(t['bits_permuted'][0] - t['bits'][0], 2)
        r['spread_us'] = max(r['bits_permuted']['spread_us'], r['bits']['spread_us'])
        res['shapes']['cfg2_B%d' % B] = r
        print('B = %3d  ' % B + '  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
        print('         bits(permute=True) - bits() = %.2f us, spread %.2f us' % (r['bits_permuted_minus_bits_us'], r['spread_us']), flush=True)
    x = gen.spectral(0, 64)[1]['input']
    lab = planted.planted_permutation(1, 50, 0, 64, device=DEV)
    assert x.shape == (64, 4, 50, 50)
    t = alternate({'relabel_dense': lambda: planted.relabel(x, lab), 'clone': lambda: x.clone()}, o.reps)
    res['shapes']['relabel_spectral_64x4x50x50'] = row(t)
    print('relabel (64, 4, 50, 50): %.2f us (%.2f - %.2f); a plain copy of the same tensor: %.2f us (%.2f - %.2f)'
          % (t['relabel_dense'] + t['clone']), flush=True)
    line = json.dumps(res)
    print(line)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
