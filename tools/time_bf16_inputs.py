"""Price of spectral (4-channel) input in 16 bit on the cfg2 shape: 32 pairs, N = 50, 4 blocks, PairGenerator.spectral batches.

(a) fp32: the captured train_step of FgnnTrainer on the 32-channel padded layout, fed through the zero-padded fp32 staging buffer
    (what the fp32 side does with such a batch: copy 4 channels into a (2 B, 32, N, N) buffer, then the step).
(b) bf16: the captured train_step of FgnnTrainer(precision='bf16') on the same layout, fed the 4-channel batch directly
    (fgnn_to_bf16_pad inside the graph).
(c) the input conversion alone: fgnn_to_bf16_pad against staging copy + fgnn_to_bf16 on 32 channels.
(d) the 2-channel bf16 captured train_step (dense input, generic block 1): the path that must not move.

One library per process: run once as is, and once with FGNN_LIB pointing at the build to compare with (--legs ad for a build without
fgnn_to_bf16_pad), and compare the two JSON lines.  Protocol (tools/time_pairgen_indexed.py): device events on one stream, warm-up,
WINDOWS rounds in which the variants take turns with one window of `reps` calls each; median window and spread per variant.
usage: python tools/time_bf16_inputs.py [--reps 50] [--legs abcd] [--out file.json]"""
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
from graph_neural_net_amd.trainer import FgnnTrainer
from time_pairgen_indexed import DEV, WINDOWS, alternate, row

B, N, C = 32, 50, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--legs', default='abcd')
    ap.add_argument('--out', default=None)
    o = ap.parse_args()
    _lib.load(allow_missing=True)        # an older build: only the legs it has entry points for
    gen = PairGenerator(N, 'Regular', 'ErdosRenyi', seed=1, device=DEV)
    s1, s2 = (d['input'] for d in gen.spectral(0, B, C))
    d1, d2 = (d['input'] for d in gen.dense(0, B))
    lay32, lay2 = ParamLayout(32, 4, 32, 32, 3), ParamLayout(2, 4, 32, 32, 3)
    fns = {}
    if 'a' in o.legs:
        tr32 = FgnnTrainer(lay32, lay32.init_flat(0, DEV), lr=1e-3, capture=True)
        p1, p2 = (torch.zeros(B, 32, N, N, device=DEV) for _ in range(2))

        def fp32_padded():
            p1[:, :C].copy_(s1)
            p2[:, :C].copy_(s2)
            tr32.train_step(p1, p2)
        fns['a_fp32_padded_step'] = fp32_padded
    if 'b' in o.legs:
        tr16 = FgnnTrainer(lay32, lay32.init_flat(0, DEV), lr=1e-3, capture=True, precision='bf16')
        fns['b_bf16_step'] = lambda: tr16.train_step(s1, s2)
    if 'd' in o.legs:
        tr2 = FgnnTrainer(lay2, lay2.init_flat(0, DEV), lr=1e-3, capture=True, precision='bf16')
        fns['d_bf16_2ch_step'] = lambda: tr2.train_step(d1, d2)
    for f in fns.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    res = {'tool': 'time_bf16_inputs', 'lib': os.path.basename(_lib.LIB_PATH), 'reps': o.reps, 'windows': WINDOWS, 'pairs': B, 'n_vertices': N,
           'channels': C}
    if fns:
        t = alternate(fns, o.reps)
        res['steps'] = row(t)
        print('  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
    if 'c' in o.legs:
        G = 2 * B
        x = torch.cat([s1, s2]).contiguous()
        ldr = (N + 7) // 8 * 8
        ldp = (N * ldr + 63) // 64 * 64
        y = torch.empty(G * 32 * ldp, dtype=torch.bfloat16, device=DEV)
        stage = torch.zeros(G, 32, N, N, device=DEV)

        def one_pass():
            _lib.call('fgnn_to_bf16_pad', _lib.ptr(x), None, G, C, 32, N, ldr, _lib.ptr(y), ldp, _lib.stream_ptr())

        def stage_then_convert():
            stage[:, :C].copy_(x)
            _lib.call('fgnn_to_bf16', _lib.ptr(stage), None, G, 32, N, ldr, _lib.ptr(y), 32 * ldp, ldp, _lib.stream_ptr())
        t = alternate({'c_to_bf16_pad': one_pass, 'c_stage_plus_to_bf16': stage_then_convert}, 4 * o.reps)
        res['conversion'] = row(t)
        print('  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
    line = json.dumps(res)
    print(line)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
