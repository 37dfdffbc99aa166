"""Time of the spectral-feature launch (graph_neural_net_amd/spectral.py, csrc/spectral.hip) against the torch composition on the same
GPU -- what a user would write without it: expand_adjacency, then the diag / bmm chain of loaders/data_generator.py:221-232 (with the
isolated-vertex convention, and the crop to the largest n for a ragged batch).  Both start from the same bit rows.  Device events,
one warm-up, the median of five windows of `reps` calls; also the achieved write bandwidth G * n_powers * Nout^2 * 4 B / time.
usage: python tools/gpu_spectral_rate.py [reps] [out.json]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graph_neural_net_amd.inputs import expand_adjacency
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.spectral import spectral_features

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
OUT = sys.argv[2] if len(sys.argv) > 2 else None
DEV = torch.device('cuda:0')
P = 4
SHAPES = [
    ('cfg2', 'cfg2 shape: Regular N=50, 64 graphs', dict(n_vertices=50), 32),
    ('cfg4', 'cfg4 shape: ErdosRenyi N=200, 16 graphs', dict(n_vertices=200, generative_model='ErdosRenyi'), 8),
    ('cfg5', 'cfg5-like ragged: ErdosRenyi N=120, vertex_proba 0.625, 16 graphs',
     dict(n_vertices=120, generative_model='ErdosRenyi', vertex_proba=0.625), 8),
]


def composition(bits, nv, n_out):
    """the reference's arithmetic in torch on the device"""
    N = bits.shape[1]
    w = expand_adjacency(bits, N, nv)[:, 0]
    if n_out != N:
        w = w[:, :n_out, :n_out]
    d = w.sum(-1)
    s = torch.where(d > 0, 1 / torch.sqrt(d), torch.zeros_like(d))
    L = torch.bmm(torch.bmm(torch.diag_embed(s), w), torch.diag_embed(s))
    out = torch.empty(bits.shape[0], P, n_out, n_out, device=bits.device)
    prev = torch.eye(n_out, device=bits.device).expand(bits.shape[0], n_out, n_out)
    for i in range(P):
        prev = torch.bmm(prev, L)
        out[:, i] = prev
    return out


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    w = sorted(window(fn, reps) for _ in range(5))
    return statistics.median(w), w[0], w[-1]


def main():
    res = {'tool': 'gpu_spectral_rate', 'n_powers': P, 'reps': REPS, 'shapes': {}}
    for key, name, kw, B in SHAPES:
        b1, b2, nv = PairGenerator(seed=1, device=DEV, **kw).bits(0, B)
        bits = torch.cat([b1, b2]).contiguous()
        nv = torch.cat([nv, nv]).contiguous() if nv is not None else None
        G, N = bits.shape[0], bits.shape[1]
        n_out = N if nv is None else int(nv.max().item())
        out = torch.empty(G, P, n_out, n_out, device=DEV)
        a, b = spectral_features(bits, nv, P, n_out=n_out), composition(bits, nv, n_out)
        dist = (a - b).abs().max().item()
        k_ms, k_lo, k_hi = timed(lambda: spectral_features(bits, nv, P, n_out=n_out, out=out), REPS)
        c_ms, c_lo, c_hi = timed(lambda: composition(bits, nv, n_out), REPS)
        nbytes = G * P * n_out * n_out * 4
        row = dict(N=N, G=G, n_out=n_out, launch_us=round(k_ms * 1e3, 2), launch_us_range=[round(k_lo * 1e3, 2), round(k_hi * 1e3, 2)],
                   composition_us=round(c_ms * 1e3, 2), composition_us_range=[round(c_lo * 1e3, 2), round(c_hi * 1e3, 2)],
                   composition_over_launch=round(c_ms / k_ms, 2), write_GBps=round(nbytes / (k_ms * 1e-3) / 1e9, 1),
                   composition_write_GBps=round(nbytes / (c_ms * 1e-3) / 1e9, 1), max_abs_difference=dist)
        res['shapes'][key] = row
        print('%-66s launch %8.2f us (%.2f - %.2f)  composition %8.2f us (%.2f - %.2f)  x%.2f  %.1f GB/s written'
              % (name, row['launch_us'], k_lo * 1e3, k_hi * 1e3, row['composition_us'], c_lo * 1e3, c_hi * 1e3,
                 row['composition_over_launch'], row['write_GBps']), flush=True)
    line = json.dumps(res)
    print(line)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
