#!/usr/bin/env python3
"""Time the matching decode (graph_neural_net_amd/qap.py: greedy_qap, T = 10) on the GPU and on this machine's CPU, same inputs.

Shapes: cfg2 (N = 50, B = 32, Regular), the cfg4 shape (N = 200, B = 8, ErdosRenyi) and N = 256 (B = 8, ErdosRenyi); pairs from
PairGenerator, starting matchings = the identity with half of the vertices shuffled.  Device chain: warm-up calls, then the median
of five windows of `--reps` calls each, every window bracketed by device events and ended by a synchronise.  The three kernels of a
round (improve cost / solver / objective) are timed the same way, each launched alone on the chain's own data; the chain issues
T + 1 of each (plus T + 1 bookkeeping launches).  The host route (numpy + SciPy loop of qap.py) is timed with a host clock.
Prints ONE JSON line.  Needs a GPU: there is no fallback.

Usage: python tools/gpu_qap_decode_time.py [--reps 20] [--T 10]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graph_neural_net_amd import _lib, qap  # noqa: E402
from graph_neural_net_amd.pairgen import PairGenerator  # noqa: E402

SHAPES = (('cfg2', 50, 32, 'Regular'), ('cfg4', 200, 8, 'ErdosRenyi'), ('n256', 256, 8, 'ErdosRenyi'))


def windows_ms(fn, reps, windows=5, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--T', type=int, default=10)
    ap.add_argument('--host-reps', type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError('gpu_qap_decode_time needs a GPU')
    dev = torch.device('cuda:0')
    T = args.T
    res = {'tool': 'gpu_qap_decode_time', 'T': T, 'reps': args.reps, 'device': torch.cuda.get_device_name(0), 'shapes': {}}
    for name, N, B, family in SHAPES:
        b1, b2, _ = PairGenerator(N, family, 'ErdosRenyi', edge_density=0.2, noise=0.1, seed=1, device=dev).bits(0, B)
        rng = np.random.default_rng(N)
        a0 = np.tile(np.arange(N, dtype=np.int32), (B, 1))
        for b in range(B):
            idx = rng.choice(N, size=N // 2, replace=False)
            a0[b, idx] = a0[b, rng.permutation(idx)]
        a0 = torch.from_numpy(a0).to(dev)
        chain = windows_ms(lambda: qap.greedy_bits(b1, b2, a0, T, None), args.reps)
        # the three kernels of a round, alone
        cost = torch.empty(B, N, N, dtype=torch.float32, device=dev)
        correct = torch.empty(B, dtype=torch.int32, device=dev)
        cur = torch.empty(B, N, dtype=torch.int32, device=dev)
        q = torch.empty(B, dtype=torch.int32, device=dev)
        st = _lib.stream_ptr()
        k_cost = windows_ms(lambda: _lib.call('fgnn_qap_improve_cost', _lib.ptr(b1), _lib.ptr(b2), _lib.ptr(a0), None, B, N,
                                              _lib.ptr(cost), N * N, N, st), 10 * args.reps)
        k_lsap = windows_ms(lambda: _lib.call('fgnn_lsap_accuracy', _lib.ptr(cost), N * N, N, None, B, N, _lib.ptr(correct),
                                              _lib.ptr(cur), st), 2 * args.reps)
        k_obj = windows_ms(lambda: _lib.call('fgnn_qap_objective', _lib.ptr(b1), _lib.ptr(b2), _lib.ptr(cur), None, B, N, _lib.ptr(q),
                                             None, None, None, st), 10 * args.reps)
        dev_out = qap.greedy_bits(b1, b2, a0, T, None)
        # the host route on the same inputs
        h1, h2, ha = b1.cpu(), b2.cpu(), a0.cpu()
        t_host = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            host_out = qap.greedy_qap(h1, h2, ha, T)
            t_host.append((time.perf_counter() - t0) * 1e3)
        same = all(torch.equal(dev_out[k].cpu(), host_out[k]) for k in ('s_best', 'acc_best', 'T_best', 'na', 'nb'))
        res['shapes'][name] = {
            'N': N, 'B': B, 'family': family, 'device_chain_ms': round(chain[0], 4), 'device_chain_ms_min_max': [round(chain[1], 4), round(chain[2], 4)],
            'kernel_us': {'improve_cost': round(1e3 * k_cost[0], 2), 'solver': round(1e3 * k_lsap[0], 2), 'objective': round(1e3 * k_obj[0], 2)},
            'chain_share_of_kernels_ms': {'improve_cost': round((T + 1) * k_cost[0], 4), 'solver': round((T + 1) * k_lsap[0], 4),
                                          'objective': round((T + 1) * k_obj[0], 4)},
            'host_route_ms': round(statistics.median(t_host), 2), 'host_over_device': round(statistics.median(t_host) / chain[0], 1),
            'device_equals_host': bool(same)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
