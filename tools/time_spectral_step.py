"""Price of the spectral step from bit words on the cfg2 shape with spectral input: 32 pairs, N = 50, 4 channels, 4 blocks, bf16.

(a) the step route: the captured bf16 train_step_spectral from bit words (fgnn_spectral_slab16 inside the graph) against the route
    that existed before it -- two spectral_features launches, then the captured train_step with its copies into the static input
    and fgnn_to_bf16_pad inside the graph.  Both in this process, taking turns.
(b) the kernel alone on the stacked batch: fgnn_spectral_slab16 against spectral_features + fgnn_to_bf16_pad.
(c) the paths that must not move: the captured train_step_bits (fp32, generic block 1) and the captured 4-channel dense bf16
    train_step.  One library per process: run once as is and once with FGNN_LIB pointing at the build to compare with
    (--legs c: an older build has no fgnn_spectral_slab16), and compare the two JSON lines.

Protocol (tools/time_pairgen_indexed.py): device events on one stream, warm-up, WINDOWS rounds in which the variants take turns with
one window of `reps` calls each; median window and spread per variant.
usage: python tools/time_spectral_step.py [--reps 50] [--legs abc] [--out file.json]"""
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
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.spectral import spectral_features
from graph_neural_net_amd.trainer import FgnnTrainer
from time_pairgen_indexed import DEV, WINDOWS, alternate, row

B, N, C = 32, 50, 4


def show(t):
    print('  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--legs', default='abc')
    ap.add_argument('--out', default=None)
    o = ap.parse_args()
    _lib.load(allow_missing=True)        # an older build: only the legs it has entry points for
    gen = PairGenerator(N, 'Regular', 'ErdosRenyi', seed=1, device=DEV)
    b1, b2, _ = gen.bits(0, B)
    lay32, lay2 = ParamLayout(32, 4, 32, 32, 3), ParamLayout(2, 4, 32, 32, 3)
    res = {'tool': 'time_spectral_step', 'lib': os.path.basename(_lib.LIB_PATH), 'reps': o.reps, 'windows': WINDOWS, 'pairs': B,
           'n_vertices': N, 'channels': C}

    def warm(fns):
        for f in fns.values():
            for _ in range(5):
                f()
        torch.cuda.synchronize()

    if 'a' in o.legs:
        new = FgnnTrainer(lay32, lay32.init_flat(0, DEV), lr=1e-3, capture=True, precision='bf16')
        old = FgnnTrainer(lay32, lay32.init_flat(0, DEV), lr=1e-3, capture=True, precision='bf16')
        fns = {'a_step_from_words': lambda: new.train_step_spectral(b1, b2, n_powers=C),
               'a_features_then_dense_step': lambda: old.train_step(spectral_features(b1, None, C), spectral_features(b2, None, C))}
        warm(fns)
        t = alternate(fns, o.reps)
        res['step_route'] = row(t)
        show(t)
    if 'b' in o.legs:
        G = 2 * B
        bits = torch.cat([b1, b2]).contiguous()
        ldr = (N + 7) // 8 * 8
        ldp = (N * ldr + 63) // 64 * 64
        y = torch.empty(G * 32 * ldp, dtype=torch.bfloat16, device=DEV)
        f = torch.empty(G, C, N, N, device=DEV)

        def one_launch():
            _lib.call('fgnn_spectral_slab16', _lib.ptr(bits), None, G, N, C, 32, ldr, _lib.ptr(y), ldp, _lib.stream_ptr())

        def two_launches():
            _lib.call('fgnn_spectral_features', _lib.ptr(bits), None, G, N, C, _lib.ptr(f), N, _lib.stream_ptr())
            _lib.call('fgnn_to_bf16_pad', _lib.ptr(f), None, G, C, 32, N, ldr, _lib.ptr(y), ldp, _lib.stream_ptr())
        fns = {'b_spectral_slab16': one_launch, 'b_features_plus_to_bf16_pad': two_launches}
        warm(fns)
        t = alternate(fns, 4 * o.reps)
        res['kernel'] = row(t)
        show(t)
    if 'c' in o.legs:
        tr_bits = FgnnTrainer(lay2, lay2.init_flat(0, DEV), lr=1e-3, capture=True)
        tr_dense = FgnnTrainer(lay32, lay32.init_flat(0, DEV), lr=1e-3, capture=True, precision='bf16')
        s1, s2 = spectral_features(b1, None, C), spectral_features(b2, None, C)
        fns = {'c_bits_step_fp32': lambda: tr_bits.train_step_bits(b1, b2), 'c_dense_4ch_step_bf16': lambda: tr_dense.train_step(s1, s2)}
        warm(fns)
        t = alternate(fns, o.reps)
        res['unchanged'] = row(t)
        show(t)
    line = json.dumps(res)
    print(line)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
