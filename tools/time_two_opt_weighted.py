"""Price of the pairwise-exchange search on real-weighted pairs (qap.two_opt_weighted, csrc/qap_2opt_weighted.hip): 32 spectral pairs
(PairGenerator.spectral: Regular parents with ErdosRenyi noise 0.1, channel 0 = L = D^-1/2 W D^-1/2, read in place out of the
4-channel batch) at N = 50 (A and Bp in LDS) and N = 200 (Bp in the workspace).  The start is the Hungarian matching of the scores
of a model with initial parameters on the same pairs' bit words, as in tools/time_two_opt.py.

(a) the fgnn_qapw_2opt launch alone;
(b) one round of greedy_weighted (the difference of T = 11 and T = 1, over 10), for comparison;
(c) fgnn_qap_2opt on the same pairs' bit words from the same start;
(d) the exchanges per pair, the share of pairs that end with status 1 (stopped at the bound of n^2 exchanges), the evaluations nit
    and the objective before and after, beside the planted one.

Protocol (tools/time_pairgen_indexed.py): device events on one stream, warm-up, then WINDOWS rounds in which the variants take turns
with one window of `reps` calls each; reported per variant: the median window and the spread of the same run.  One timed probe of
(a) first: `reps` is cut so that its windows stay within --budget seconds.
usage: python tools/time_two_opt_weighted.py [--reps 20] [--sizes 50,200] [--budget 30] [--out profiles/two_opt_weighted_time.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from graph_neural_net_amd import _lib, qap
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.evaluation import EvalMeter, QapMeter
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.trainer import FgnnTrainer
from time_pairgen_indexed import DEV, WINDOWS, alternate, row, window

B = 32


def dist(v):
    return {'min': min(v), 'median': statistics.median(v), 'mean': round(sum(v) / len(v), 2), 'max': max(v)}


def one_size(N, reps, budget):
    lay = ParamLayout(2, 4, 32, 32, 3)
    gen = PairGenerator(N, 'Regular', 'ErdosRenyi', noise=0.1, seed=1, device=DEV)
    b1, b2 = gen.bits(0, B)[:2]
    f1, f2 = (d['input'] for d in gen.spectral(0, B))
    tr = FgnnTrainer(lay, lay.init_flat(0, DEV), lr=1e-3, capture=True, block1='structured' if N == 50 else None)
    assign = tr.eval_step_bits(b1, b2, meter=EvalMeter(DEV), qap_meter=QapMeter(DEV))['decode']['assign'].clone()
    # (d) one search, read before the timing
    out = qap.two_opt_weighted(f1, f2, assign)
    planted = qap.objective_weighted(f1, f2, assign, None)['planted']
    bit = qap.two_opt_bits(b1, b2, assign, None)
    status, swaps = out['status'].cpu().tolist(), out['swaps'].cpu().tolist()
    search = {'swaps': dist(swaps), 'status1_share': round(sum(s == 1 for s in status) / B, 4), 'status': sorted(set(status)),
              'nit_mean': float(out['nit'].double().mean()), 'qap0_mean': float(out['qap0'].mean()), 'qap_mean': float(out['qap'].mean()),
              'planted_mean': float(planted.mean()), 'qap_ratio0': float((out['qap0'] / planted).mean()),
              'qap_ratio': float((out['qap'] / planted).mean()), 'bit_swaps': dist(bit['swaps'].cpu().tolist()),
              'bit_nit_mean': float(bit['nit'].double().mean())}
    # the launches alone
    x1, x2, gs, ld = qap.weighted_views(f1, f2)
    nbytes = _lib.load().fgnn_qapw_2opt_ws_bytes(B, N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV) if nbytes else None
    perm = torch.empty(B, N, dtype=torch.int32, device=DEV)
    o32 = torch.empty(3, B, dtype=torch.int32, device=DEV)
    nit = torch.empty(B, dtype=torch.int64, device=DEV)

    def launch():
        _lib.call('fgnn_qapw_2opt', _lib.ptr(x1), _lib.ptr(x2), gs, ld, _lib.ptr(assign), None, B, N, -1, _lib.ptr(ws), nbytes,
                  _lib.ptr(perm), _lib.ptr(o32[0]), _lib.ptr(nit), _lib.ptr(o32[1]), _lib.stream_ptr())

    def launch_bits():
        _lib.call('fgnn_qap_2opt', _lib.ptr(b1), _lib.ptr(b2), _lib.ptr(assign), None, B, N, -1, _lib.ptr(perm), _lib.ptr(o32[0]),
                  _lib.ptr(o32[1]), _lib.ptr(nit), _lib.ptr(o32[2]), _lib.stream_ptr())
    launch()
    torch.cuda.synchronize()
    probe = window(launch, 1)
    reps = max(1, min(reps, int(budget * 1e6 / (WINDOWS * probe))))
    t = alternate({'two_opt_weighted_launch': launch, 'two_opt_bits_launch': launch_bits,
                   'greedy_weighted_T1': lambda: qap.greedy_weighted(f1, f2, assign, 1, None),
                   'greedy_weighted_T11': lambda: qap.greedy_weighted(f1, f2, assign, 11, None)}, reps)
    res = {'n_vertices': N, 'pairs': B, 'reps': reps, 'probe_us': round(probe, 2), 'launch': row(t),
           'greedy_weighted_round_us': round((t['greedy_weighted_T11'][0] - t['greedy_weighted_T1'][0]) / 10, 2), 'search': search}
    print('N %d  ' % N + '  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
    print('N %d  %r' % (N, search), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sizes', default='50,200')
    ap.add_argument('--budget', type=float, default=30.0)
    ap.add_argument('--out', default=None)
    o = ap.parse_args()
    res = {'tool': 'time_two_opt_weighted', 'windows': WINDOWS, 'sizes': []}
    for n in map(int, o.sizes.split(',')):          # (the file is rewritten after every size: a long run leaves what it finished)
        res['sizes'].append(one_size(n, o.reps, o.budget))
        line = json.dumps(res)
        if o.out:
            os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
            with open(o.out, 'w') as f:
                f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
