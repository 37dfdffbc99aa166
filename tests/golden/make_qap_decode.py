#!/usr/bin/env python3
"""Generate tests/golden/qap_decode.npz FROM THE REFERENCE ITSELF: the fixture of the matching decode (graph_neural_net_amd/qap.py,
csrc/qap.hip).  Runs only where the reference is readable (make_golden.py's REF, imported behind the same shims); its files never
travel.

The fixture is a set of groups `<g>/...`, each a batch of seeded pairs (graph_neural_net_amd.synthetic) in the device's wire form:

    bits1, bits2   (B, N, ceil(N/32)) uint32   bit j of word row i = W[i][j], zero outside the pair's n x n corner
    nvalid         (B,) int32                  vertex counts (== N except in the ragged group)
    scores         (B, N, N) float32           identity signal + noise (values exact in bf16, so the file compresses), 0 in the padding
    assign0        (B, N) int32                scipy.optimize.linear_sum_assignment(-log_softmax(scores)) per pair, -1 in the padding
    acc, qap, planted   (B,)                   the per-pair arithmetic of toolbox/metrics.py:168-193 (all_acc_qap) on assign0
    T<k>/s_best, na, nb (float64), T<k>/acc_best, T_best (int64)   toolbox.utils.greedy_qap(A, B, perm_matrix(arange, assign0), k),
                                               k in {0, 1, 10}

Groups: ER pairs at N in {7, 33, 50, 64, 120, 200, 256}, Regular pairs with ER noise at N = 50, a ragged ER group (N = 120, n in
[30, 120]) and `nonsym`: one pair whose second matrix is NOT symmetric (a directed thinning of the noisy graph).  No matching is
recorded for greedy_qap -- the reference returns none; the tests check `perm` by rescoring it.  The script asserts that at least
three pairs have T_best > 0 and at least three keep the initial score through all ten rounds (the reference's quirk case: s_best
is the initial matching's, acc_best a never-scored matching's), and draws scores again until assign0 survives relative
perturbations of 1e-6 of its cost matrix, so that no assign0 depends on the last bits of a log_softmax.

Usage:  python tests/golden/make_qap_decode.py     (from the repo root)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True
from make_golden import OUT, import_reference  # noqa: E402

from graph_neural_net_amd import synthetic  # noqa: E402

TS = (0, 1, 10)
# name -> (family, N, pairs, (n_lo, n_hi) or None)
GROUPS = {'er7': ('ErdosRenyi', 7, 4, None), 'er33': ('ErdosRenyi', 33, 4, None), 'er50': ('ErdosRenyi', 50, 4, None),
          'reg50': ('Regular', 50, 4, None), 'er64': ('ErdosRenyi', 64, 3, None), 'er120': ('ErdosRenyi', 120, 2, None),
          'er200': ('ErdosRenyi', 200, 1, None), 'er256': ('ErdosRenyi', 256, 1, None), 'ragged120': ('ErdosRenyi', 120, 4, (30, 120)),
          'nonsym': ('ErdosRenyi', 33, 1, None)}


def bf16_exact(x):
    return torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()


def pack_rows(w, N):
    n = w.shape[0]
    full = np.zeros((1, N, N), dtype=np.float32)
    full[0, :n, :n] = w
    return synthetic.pack_adjacency(full)[0]


def main():
    import_reference()
    from scipy.optimize import linear_sum_assignment
    from toolbox.utils import greedy_qap, perm_matrix
    out = {}
    improved = kept = 0
    for gi, (name, (family, N, B, ragged)) in enumerate(GROUPS.items()):
        rng = np.random.default_rng(1000 + gi)
        g = {k: [] for k in ('bits1', 'bits2', 'nvalid', 'scores', 'assign0', 'acc', 'qap', 'planted')}
        gq = {T: {k: [] for k in ('s_best', 'na', 'nb', 'acc_best', 'T_best')} for T in TS}
        for b in range(B):
            n = int(rng.integers(ragged[0], ragged[1] + 1)) if ragged else N
            x1, x2 = synthetic.make_pair(rng, n, family, edge_density=0.5 if N >= 200 else 0.2, noise=0.1)
            A, Bm = x1[0].astype(np.float64), x2[0].astype(np.float64)
            if name == 'nonsym':
                Bm = Bm * (1 - np.triu(rng.random((n, n)) < 0.4, 1))          # drop some i < j arcs, keep their reversals
                assert not np.array_equal(Bm, Bm.T) and np.array_equal(A, A.T)
            sigma = (0.6, 1.0, 1.5, 2.2)[b % 4]                               # from nearly right to mostly wrong starting matchings
            while True:
                s = np.zeros((N, N), dtype=np.float32)
                s[:n, :n] = bf16_exact((2.0 * np.eye(n) + sigma * rng.standard_normal((n, n))).astype(np.float32))
                # the reference's arithmetic (toolbox/metrics.py:179-191): log_softmax in torch, the cost to the host, SciPy
                cost = -torch.log_softmax(torch.from_numpy(s[:n, :n]), -1).numpy()
                row, col = linear_sum_assignment(cost)
                # the matching must not hang on the last bits of a log_softmax (another torch build, the device's): scores whose
                # optimum moves under relative perturbations of 1e-6 of the cost are drawn again
                if all(np.array_equal(linear_sum_assignment(cost * (1 + 1e-6 * rng.standard_normal(cost.shape)))[1], col)
                       for _ in range(8)):
                    break
            a0 = np.full(N, -1, dtype=np.int32)
            a0[:n] = col
            g['bits1'].append(pack_rows(A, N))
            g['bits2'].append(pack_rows(Bm, N))
            g['nvalid'].append(n)
            g['scores'].append(s)
            g['assign0'].append(a0)
            g['acc'].append(int(np.sum(col == np.arange(n))))
            g['qap'].append(int((A * (Bm[col, :][:, col])).sum()))
            g['planted'].append(int((A * Bm).sum()))
            for T in TS:
                s_best, na, nb, acc_best, T_best = greedy_qap(A, Bm, perm_matrix(row, col), T)
                for k, v in zip(('s_best', 'na', 'nb', 'acc_best', 'T_best'), (s_best, na, nb, acc_best, T_best)):
                    gq[T][k].append(v)
            s0 = np.trace(A @ perm_matrix(row, col) @ Bm @ perm_matrix(row, col).T) / 2
            improved += gq[10]['T_best'][-1] > 0
            kept += gq[10]['s_best'][-1] == s0
        for k, v in g.items():
            out['%s/%s' % (name, k)] = np.asarray(v, dtype=np.int32 if k in ('nvalid', 'assign0') else None)
        for T in TS:
            for k, v in gq[T].items():
                out['%s/T%d/%s' % (name, T, k)] = np.asarray(v, dtype=np.float64 if k in ('s_best', 'na', 'nb') else np.int64)
    assert improved >= 3, 'only %d pairs with T_best > 0' % improved
    assert kept >= 3, 'only %d pairs where no round improved (the quirk case)' % kept
    path = os.path.join(OUT, 'qap_decode.npz')
    np.savez_compressed(path, **out)
    print('%s: %d bytes, %d pairs with T_best > 0, %d where no round improved' % (path, os.path.getsize(path), improved, kept))


if __name__ == '__main__':
    main()
