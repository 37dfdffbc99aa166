#!/usr/bin/env python3
"""Time greedy_qap(T = 10, weighted=True) on spectral pairs: the device chain against the numpy + SciPy float64
loop on the same inputs and against the bit-word path on the underlying 0/1 pairs, plus one improve-cost launch of each kind.
Median of repeated event windows after a warm-up; one JSON line per shape.

Usage:  python tools/time_qap_weighted.py [--windows 20] [--calls 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graph_neural_net_amd import _lib, qap  # noqa: E402
from graph_neural_net_amd.pairgen import PairGenerator  # noqa: E402
from graph_neural_net_amd.spectral import spectral_features  # noqa: E402

DEV = 'cuda:0'


def windows_ms(fn, windows, calls, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=20)
    ap.add_argument('--calls', type=int, default=5)
    a = ap.parse_args()
    T = 10
    for B, N, density in ((32, 50, 0.2), (8, 200, 0.5)):
        gen = PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=density, noise=0.1, seed=1, device=DEV)
        b1, b2, _ = gen.bits(0, B)
        l1, l2 = spectral_features(b1, None, 4), spectral_features(b2, None, 4)
        g = torch.Generator().manual_seed(0)
        a0 = torch.stack([torch.randperm(N, generator=g) for _ in range(B)]).to(torch.int32)
        half = N // 2                                                       # a start that is half right
        a0[:, :half] = torch.sort(a0[:, :half], dim=1).values
        a0 = a0.to(DEV)
        res = {'B': B, 'N': N, 'T': T}
        res['weighted_ms'] = windows_ms(lambda: qap.greedy_qap(l1, l2, a0, T, weighted=True), a.windows, a.calls)
        res['bits_ms'] = windows_ms(lambda: qap.greedy_qap(b1, b2, a0, T), a.windows, a.calls)
        c1, c2, ac = l1.cpu(), l2.cpu(), a0.cpu()
        qap.greedy_qap(c1, c2, ac, T, weighted=True)
        t0 = time.perf_counter()
        qap.greedy_qap(c1, c2, ac, T, weighted=True)
        res['host_float64_ms'] = (time.perf_counter() - t0) * 1e3
        cost = torch.empty(B, N, N, device=DEV)
        x1, x2, gs, ld = qap.weighted_views(l1, l2)
        st = _lib.stream_ptr()
        res['improve_cost_weighted_ms'] = windows_ms(lambda: _lib.call(
            'fgnn_qapw_improve_cost', _lib.ptr(x1), _lib.ptr(x2), gs, ld, _lib.ptr(a0), None, B, N, _lib.ptr(cost), N * N, N, st), a.windows, 20)
        res['improve_cost_bits_ms'] = windows_ms(lambda: _lib.call(
            'fgnn_qap_improve_cost', _lib.ptr(b1), _lib.ptr(b2), _lib.ptr(a0), None, B, N, _lib.ptr(cost), N * N, N, st), a.windows, 20)
        obj = torch.empty(B, device=DEV)
        res['trace_weighted_ms'] = windows_ms(lambda: _lib.call(
            'fgnn_qapw_objective', _lib.ptr(x1), _lib.ptr(x2), gs, ld, _lib.ptr(a0), None, B, N, None, _lib.ptr(obj), None, None, None, st),
            a.windows, 20)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


if __name__ == '__main__':
    main()
