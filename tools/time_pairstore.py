"""Time of a batch gathered from stored graphs (fgnn_pairstore_gather, PairStore.bits(index=...)) against the generator launch that
makes the same pairs (fgnn_pairgen_indexed of an ErdosRenyi / ErdosRenyi generator) at the cfg2 batch shape (N = 50) with 32 and with
256 pairs.  The store holds that generator's first 20 000 parents; the index list is a window of a shuffled epoch over them.

Variants, all through the raw entry points into the same preallocated outputs: `gather_paired` (a stored second side: two copies),
`gather_er` (ErdosRenyi noise: a strict subset of the generator launch's work), `gather_swap` (EdgeSwap noise), and the three
generator launches `pairgen`, `pairgen_indexed`, `pairgen_levels` of the library in the tree; with --parent-lib the same three of
another build of the library (the commit before the store, loaded beside the first): the generator's device code moved to a shared
header with the store, and its launches should cost what they cost before.  Protocol: device events on one stream, one warm-up call
per variant, then WINDOWS rounds in which the variants take turns with one window of `reps` calls each; reported per variant: the
median window and the spread (slowest - fastest window) of the same run.  A difference is distinguishable when it exceeds the
larger of the two spreads.
usage: python tools/time_pairstore.py [--reps 50] [--parent-lib lib.so] [--out file.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from graph_neural_net_amd import _lib
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.pairstore import PairStore
from graph_neural_net_amd.sampler import epoch_index
from time_pairgen_indexed import DEV, EXAMPLES, WINDOWS, alternate, check, pairgen_args, row

GENERATOR_LAUNCHES = ('pairgen', 'pairgen_indexed', 'pairgen_levels')


def generator_launches(lib, tag, a, idx, table, K, level, stream):
    return {'pairgen' + tag: lambda: check(lib.fgnn_pairgen(a, stream)),
            'pairgen_indexed' + tag: lambda: check(lib.fgnn_pairgen_indexed(a, idx.data_ptr(), stream)),
            'pairgen_levels' + tag: lambda: check(lib.fgnn_pairgen_levels(a, idx.data_ptr(), table.data_ptr(), K, level.data_ptr(), stream))}


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
        for name in ('fgnn_pairgen', 'fgnn_pairgen_indexed', 'fgnn_pairgen_levels'):
            getattr(parent, name).argtypes, getattr(parent, name).restype = _lib._SIGNATURES[name], C.c_int
    gen = PairGenerator(50, 'ErdosRenyi', 'ErdosRenyi', seed=1, device=DEV)
    parents, seconds, _ = gen.bits(0, EXAMPLES)
    settings = dict(noise=gen.noise, seed=gen.seed, edge_density=gen.edge_density)
    stores = {'gather_paired': PairStore.from_bits(parents, seconds=seconds, **settings),
              'gather_er': PairStore.from_bits(parents, noise_model='ErdosRenyi', **settings),
              'gather_swap': PairStore.from_bits(parents, noise_model='EdgeSwap', **settings)}
    levels = gen.levels([gen.noise, 0.0])
    stream = _lib.stream_ptr()
    res = {'tool': 'time_pairstore', 'reps': o.reps, 'windows': WINDOWS, 'parent_lib': bool(parent), 'examples': EXAMPLES,
           'max_edges': stores['gather_swap'].max_edges, 'shapes': {}}
    for B in (32, 256):
        idx = epoch_index(1, 3, EXAMPLES, 5 * B, B, device=DEV)
        level = torch.zeros(B, dtype=torch.int32, device=DEV)
        outs = [torch.empty(B, 50, 2, dtype=torch.int32, device=DEV) for _ in range(2)]
        want = gen.bits(index=idx)
        assert all(torch.equal(x, y) for name in ('gather_paired', 'gather_er') for x, y in zip(stores[name].bits(index=idx)[:2], want[:2]))
        args = {name: s.gather_args(0, idx, None, None, outs[0], outs[1], None) for name, s in stores.items()}
        variants = {name: (lambda a=a: check(lib.fgnn_pairstore_gather(a, stream))) for name, a in args.items()}
        a_gen = pairgen_args(gen, 0, outs)
        variants.update(generator_launches(lib, '', a_gen, idx, levels.table, len(levels), level, stream))
        if parent:
            variants.update(generator_launches(parent, '_parent', a_gen, idx, levels.table, len(levels), level, stream))
        t = alternate(variants, o.reps)
        r = row(t)
        pairs = [('gather_er', 'pairgen_indexed')] + ([(n, n + '_parent') for n in GENERATOR_LAUNCHES] if parent else [])
        for x, y in pairs:
            d, spread = round(t[x][0] - t[y][0], 2), max(r[x]['spread_us'], r[y]['spread_us'])
            r['%s_minus_%s' % (x, y)] = dict(us=d, spread_us=spread, distinguishable=abs(d) > spread)
        res['shapes']['cfg2_B%d' % B] = r
        print('B = %3d  ' % B + '  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
        for x, y in pairs:
            print('         %s - %s = %.2f us, spread %.2f us' % (x, y, r['%s_minus_%s' % (x, y)]['us'], r['%s_minus_%s' % (x, y)]['spread_us']),
                  flush=True)
    line = json.dumps(res)
    print(line)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
