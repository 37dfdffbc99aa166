#!/usr/bin/env python3
"""Generate tests/golden/qap_weighted.npz FROM THE REFERENCE ITSELF: the fixture of the matching decode on real-weighted pairs
(graph_neural_net_amd/qap.py with weighted=True, csrc/qap_weighted.hip).  Runs only where the reference is readable (make_golden.py's
REF, imported behind the same shims); its files never travel.  toolbox.utils.perm_matrix / score / greedy_qap and
loaders.data_generator.make_laplacian are imported and evaluated; the per-pair lines of toolbox/metrics.py:184-188 are applied as
they stand.

The fixture is a set of groups `<g>/...`, each a batch of seeded pairs:

    a1, a2         (B, N, N) float32           the matrices, zero outside the pair's n x n corner
    nvalid         (B,) int32                  vertex counts (== N except in the ragged group)
    scores         (B, N, N) float32           identity signal + noise (values exact in bf16, so the file compresses), 0 in the padding
    assign0        (B, N) int32                scipy.optimize.linear_sum_assignment(-log_softmax(scores)) per pair, -1 in the padding
    acc (int64), qap, planted (float64)        the per-pair arithmetic of all_acc_qap on assign0 (on the matrices as float64)
    score0, na, nb (float64)                   toolbox.utils.score(A, B, perm_matrix(arange, assign0))
    T<k>/s_best, na, nb (float64), T<k>/acc_best, T_best (int64)   toolbox.utils.greedy_qap(A, B, perm_matrix(arange, assign0), k),
                                               k in {0, 1, 10} -- NOT in the group `spectral`

Groups (weights: products and partial sums exactly representable in fp32, so the device must reproduce every number exactly):
    int_sym      N = 50, 4 pairs   symmetric, integer weights 0 .. 15 on ER graphs, the second side a noisy re-weighted copy
    int_nonsym   N = 33, 3 pairs   integer weights, NEITHER side symmetric (qap != trace)
    dyadic       N = 64, 3 pairs   symmetric, weights k / 8
    ragged       N = 40, 4 pairs   integer weights, n = 0, 1, 17, 40
    int_sym130   N = 130, 1 pair   symmetric integer weights, beyond one 128-column block of the cost kernel
and `spectral` (N = 50, 2 pairs): L = make_laplacian(W) of ER pairs from synthetic.make_pair, real fp32 weights; objective values
only -- a greedy trajectory on real weights may turn on a near-tie.  An empty pair (n = 0) records zeros.  The script asserts
that at least three pairs have T_best > 0 and at least three keep the initial score through all ten rounds (the reference's quirk
case), and draws scores again until assign0 survives relative perturbations of 1e-6 of its cost matrix.

Usage:  python tests/golden/make_qap_weighted.py     (from the repo root)
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
# name -> (kind, N, vertex counts)
GROUPS = {'int_sym': ('int', 50, [50] * 4), 'int_nonsym': ('nonsym', 33, [33] * 3), 'dyadic': ('dyadic', 64, [64] * 3),
          'ragged': ('int', 40, [0, 1, 17, 40]), 'int_sym130': ('int', 130, [130]), 'spectral': ('spectral', 50, [50] * 2)}


def bf16_exact(x):
    return torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()


def sym_weights(rng, n):
    w = np.triu(rng.integers(1, 16, size=(n, n)), 1)
    return (w + w.T).astype(np.float64)


def draw_pair(rng, kind, n, make_laplacian):
    """-> (A, B) float32 (n, n)"""
    if n == 0:
        return np.zeros((0, 0), np.float32), np.zeros((0, 0), np.float32)
    if kind == 'spectral':
        while True:
            x1, x2 = synthetic.make_pair(rng, n, 'ErdosRenyi', edge_density=0.2, noise=0.1)
            if x1[0].sum(1).min() >= 1 and x2[0].sum(1).min() >= 1:           # an isolated vertex: the reference's L is NaN
                break
        return tuple(make_laplacian(torch.from_numpy(x[0].astype(np.float32))).numpy() for x in (x1, x2))
    if n == 1:
        x1 = x2 = np.zeros((2, 1, 1), np.float32)
    else:
        x1, x2 = synthetic.make_pair(rng, n, 'ErdosRenyi', edge_density=0.3, noise=0.1)
    w = sym_weights(rng, n)
    w2 = np.where(rng.random((n, n)) < 0.15, sym_weights(rng, n), w)          # the noisy side re-weights some edges ...
    w2 = np.triu(w2, 1) + np.triu(w2, 1).T                                   # ... symmetrically
    A, Bm = x1[0] * w, x2[0] * w2
    if kind == 'nonsym':
        A = A * (1 - np.triu(rng.random((n, n)) < 0.4, 1))                    # drop some i < j arcs, keep their reversals
        Bm = Bm * (1 - np.tril(rng.random((n, n)) < 0.4, -1))                 # and some i > j arcs on the other side
        assert not np.array_equal(A, A.T) and not np.array_equal(Bm, Bm.T)
    else:
        assert np.array_equal(A, A.T) and np.array_equal(Bm, Bm.T)
    if kind == 'dyadic':
        A, Bm = A / 8, Bm / 8
    return A.astype(np.float32), Bm.astype(np.float32)


def main():
    import_reference()
    from loaders.data_generator import make_laplacian
    from scipy.optimize import linear_sum_assignment
    from toolbox.utils import greedy_qap, perm_matrix, score
    out = {}
    improved = kept = 0
    for gi, (name, (kind, N, sizes)) in enumerate(GROUPS.items()):
        rng = np.random.default_rng(3000 + gi)
        g = {k: [] for k in ('a1', 'a2', 'nvalid', 'scores', 'assign0', 'acc', 'qap', 'planted', 'score0', 'na', 'nb')}
        gq = {T: {k: [] for k in ('s_best', 'na', 'nb', 'acc_best', 'T_best')} for T in TS}
        for b, n in enumerate(sizes):
            A32, B32 = draw_pair(rng, kind, n, make_laplacian)
            assert A32.dtype == np.float32 and np.isfinite(A32).all() and np.isfinite(B32).all()
            A, Bm = A32.astype(np.float64), B32.astype(np.float64)
            sigma = (0.3, 1.0, 1.5, 2.2)[b % 4]                               # from nearly right to mostly wrong starting matchings
            while n:
                s = np.zeros((N, N), dtype=np.float32)
                s[:n, :n] = bf16_exact((2.0 * np.eye(n) + sigma * rng.standard_normal((n, n))).astype(np.float32))
                cost = -torch.log_softmax(torch.from_numpy(s[:n, :n]), -1).numpy()
                row, col = linear_sum_assignment(cost)
                if all(np.array_equal(linear_sum_assignment(cost * (1 + 1e-6 * rng.standard_normal(cost.shape)))[1], col)
                       for _ in range(8)):
                    break
            if n == 0:
                s, row, col = np.zeros((N, N), dtype=np.float32), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
            a0 = np.full(N, -1, dtype=np.int32)
            a0[:n] = col
            pad = lambda m: np.pad(m, ((0, N - n), (0, N - n)))               # noqa: E731
            g['a1'].append(pad(A32))
            g['a2'].append(pad(B32))
            g['nvalid'].append(n)
            g['scores'].append(s)
            g['assign0'].append(a0)
            g['acc'].append(int(np.sum(col == np.arange(n))))
            g['qap'].append((A * (Bm[col, :][:, col])).sum())                 # toolbox/metrics.py:185-186 on float64 copies
            g['planted'].append((A * Bm).sum())
            P = perm_matrix(row, col)
            s0, na, nb = score(A, Bm, P) if n else (0.0, 0.0, 0.0)
            g['score0'].append(s0)
            g['na'].append(na)
            g['nb'].append(nb)
            if kind == 'spectral':
                continue
            for T in TS:
                res = greedy_qap(A, Bm, P, T) if n else (0.0, 0.0, 0.0, 0, 0)
                for k, v in zip(('s_best', 'na', 'nb', 'acc_best', 'T_best'), res):
                    gq[T][k].append(v)
            improved += gq[10]['T_best'][-1] > 0
            kept += n > 1 and gq[10]['s_best'][-1] == s0
        for k, v in g.items():
            dt = {'nvalid': np.int32, 'assign0': np.int32, 'acc': np.int64, 'a1': np.float32, 'a2': np.float32, 'scores': np.float32}
            out['%s/%s' % (name, k)] = np.asarray(v, dtype=dt.get(k, np.float64))
        if kind != 'spectral':
            for T in TS:
                for k, v in gq[T].items():
                    out['%s/T%d/%s' % (name, T, k)] = np.asarray(v, dtype=np.float64 if k in ('s_best', 'na', 'nb') else np.int64)
    assert improved >= 3, 'only %d pairs with T_best > 0' % improved
    assert kept >= 3, 'only %d pairs where no round improved (the quirk case)' % kept
    path = os.path.join(OUT, 'qap_weighted.npz')
    np.savez_compressed(path, **out)
    print('%s: %d bytes, %d pairs with T_best > 0, %d where no round improved' % (path, os.path.getsize(path), improved, kept))


if __name__ == '__main__':
    main()
