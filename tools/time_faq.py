"""Price and quality of the Fast Approximate QAP chain (qap.faq, csrc/qap_faq.hip) on the shapes of the README's QAP table: Regular
N = 50 and N = 200 with ErdosRenyi noise 0.1, 32 pairs as bit-packed adjacency (seed 1, the pairs of tools/time_two_opt.py).

(a) the whole chain (expansion of the bit words, 30 rounds, the last assignment, objective and count) with the default tol, where
    pairs freeze as they converge, and with a tol no pair meets, where all 30 rounds do full work;
(b) the price of a round = (chain of 30 rounds - chain of 1 round) / 29 at that tol, and its split: the solver launch alone
    (fgnn_lsap_accuracy on the cost of fgnn_qapw_improve_cost from FAQ's matching -- for symmetric pairs that cost is G / 2 of a
    permutation P, the same problem), the improve-cost GEMM alone for scale (one product of the gradient's four), and the rest of
    the round (gradient + step kernels), which no entry point issues alone and is therefore a remainder, not a measurement;
(c) the QAP ratio (objective of the found matching over the planted one, mean over the pairs) of FAQ and of FAQ followed by
    `two_opt`, beside the README's Hungarian, refine = 10 and 2-opt rows (constants below: those need a model);
(d) SciPy's host loop, quadratic_assignment(method='faq', maximize=True), on the first --scipy-pairs pairs: seconds per pair and
    its ratio on those pairs beside the device's.

Protocol (tools/time_pairgen_indexed.py): device events on one stream, warm-up, then WINDOWS = 7 rounds in which the variants take
turns with one window of `reps` calls each; reported per variant: the median window and the spread of the same run.
usage: python tools/time_faq.py [--reps 5] [--sizes 50,200] [--scipy-pairs 8] [--out profiles/faq_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from graph_neural_net_amd import _lib, qap
from graph_neural_net_amd.pairgen import PairGenerator
from time_pairgen_indexed import DEV, WINDOWS, alternate, row

B = 32
README_ROWS = {50: {'hungarian': 0.229, 'refine10': 0.262, 'two_opt': 0.554}, 200: {'hungarian': 0.222, 'refine10': 0.232, 'two_opt': 0.417}}
NEVER = 1e-30             # a tol no pair meets


def unpack(words, n):
    w = words.cpu().numpy().view(np.uint32)
    return np.unpackbits(w.view(np.uint8), axis=-1, bitorder='little')[..., :n, :n].astype(np.float64)


def ratio(q, planted):
    return float((q.double() / planted.double()).mean())


def scipy_leg(b1, b2, pairs, N, planted):
    from scipy.optimize import quadratic_assignment
    A, Bm = unpack(b1[:pairs], N), unpack(b2[:pairs], N)
    t0 = time.perf_counter()
    res = [quadratic_assignment(A[b], Bm[b], method='faq', options={'maximize': True}) for b in range(pairs)]
    dt = (time.perf_counter() - t0) / pairs
    funs = torch.tensor([float(r.fun) for r in res], dtype=torch.float64)
    return {'seconds_per_pair': round(dt, 4), 'pairs': pairs, 'qap_ratio': ratio(funs, planted[:pairs].cpu()),
            'nit_mean': float(np.mean([r.nit for r in res]))}


def one_size(N, reps, scipy_pairs):
    gen = PairGenerator(N, 'Regular', 'ErdosRenyi', noise=0.1, seed=1, device=DEV)
    b1, b2 = gen.bits(0, B)[:2]
    ident = torch.arange(N, dtype=torch.int32, device=DEV).expand(B, N).contiguous()
    planted = qap.objective_bits(b1, b2, ident, None)['planted']
    out = qap.faq(b1, b2)
    polished = qap.two_opt(b1, b2, out['perm'])
    assert int(out['status'].max()) < 2 and int(polished['status'].max()) == 0
    quality = {'faq': ratio(out['qap'], planted), 'faq_two_opt': ratio(polished['qap'], planted), 'readme': README_ROWS.get(N),
               'faq_acc': float(out['acc'].double().mean()) / N, 'faq_two_opt_acc': float(polished['acc'].double().mean()) / N,
               'nit': {'min': int(out['nit'].min()), 'mean': float(out['nit'].double().mean()), 'max': int(out['nit'].max())},
               'stopped_on_tol': int((out['status'] == 0).sum()), 'two_opt_swaps_mean': float(polished['swaps'].double().mean())}
    # fp32 operands for the pieces
    x = torch.empty(2, B, 2, N, N, dtype=torch.float32, device=DEV)
    for side, bits in enumerate((b1, b2)):
        _lib.call('fgnn_expand_adjacency', _lib.ptr(bits), None, B, N, _lib.ptr(x[side]), _lib.stream_ptr())
    cost = torch.empty(B, N, N, dtype=torch.float32, device=DEV)
    correct = torch.empty(B, dtype=torch.int32, device=DEV)
    assign = torch.empty(B, N, dtype=torch.int32, device=DEV)
    perm = out['perm'].clone()

    def improve():
        _lib.call('fgnn_qapw_improve_cost', _lib.ptr(x[0]), _lib.ptr(x[1]), 2 * N * N, N, _lib.ptr(perm), None, B, N, _lib.ptr(cost),
                  N * N, N, _lib.stream_ptr())

    def solver():
        _lib.call('fgnn_lsap_accuracy', _lib.ptr(cost), N * N, N, None, B, N, _lib.ptr(correct), _lib.ptr(assign), _lib.stream_ptr())

    improve()
    t = alternate({'chain': lambda: qap.faq(b1, b2), 'chain_two_opt': lambda: qap.two_opt(b1, b2, qap.faq(b1, b2)['perm']),
                   'chain_30_rounds': lambda: qap.faq(b1, b2, tol=NEVER), 'chain_1_round': lambda: qap.faq(b1, b2, tol=NEVER, maxiter=1),
                   'solver_launch': solver, 'improve_cost_launch': improve}, reps)
    round_us = (t['chain_30_rounds'][0] - t['chain_1_round'][0]) / 29
    res = {'n_vertices': N, 'pairs': B, 'reps': reps, 'times': row(t), 'round_us': round(round_us, 2),
           'solver_us': round(t['solver_launch'][0], 2), 'gradient_plus_step_us_remainder': round(round_us - t['solver_launch'][0], 2),
           'improve_cost_us': round(t['improve_cost_launch'][0], 2), 'quality': quality,
           'scipy': scipy_leg(b1, b2, scipy_pairs, N, planted)}
    res['scipy']['device_qap_ratio_same_pairs'] = ratio(out['qap'][:scipy_pairs], planted[:scipy_pairs])
    print('N %d  ' % N + '  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
    print('N %d  quality %s' % (N, json.dumps(quality)), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sizes', default='50,200')
    ap.add_argument('--scipy-pairs', type=int, default=8)
    ap.add_argument('--out', default=None)
    o = ap.parse_args()
    res = {'tool': 'time_faq', 'windows': WINDOWS, 'sizes': []}
    for n in map(int, o.sizes.split(',')):          # (the file is rewritten after every size: a long run leaves what it finished)
        res['sizes'].append(one_size(n, o.reps if n <= 64 else max(2, o.reps // 2), o.scipy_pairs))
        line = json.dumps(res)
        if o.out:
            os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
            with open(o.out, 'w') as f:
                f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
