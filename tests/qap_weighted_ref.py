"""numpy + SciPy float64 restatement of the reference's matching decode for REAL matrices (toolbox/utils.py:225-256 perm_matrix /
score / improve / greedy_qap; the per-pair arithmetic of toolbox/metrics.py:168-193 all_acc_qap), in the reference's own matrix form,
plus the error bounds the weighted device path (csrc/qap_weighted.hip) is held to.  tests/test_qap_weighted_host.py holds it to
tests/golden/qap_weighted.npz (made by tests/golden/make_qap_weighted.py from the imported reference)."""
import os

import numpy as np
from scipy.optimize import linear_sum_assignment

TS = (0, 1, 10)                                                     # the T of the fixture's greedy_qap results
GREEDY_KEYS = ('s_best', 'na', 'nb', 'acc_best', 'T_best')
EXACT_GROUPS = ('int_sym', 'int_nonsym', 'dyadic', 'ragged', 'int_sym130')
U = 2.0 ** -24


def fixture_groups():
    """tests/golden/qap_weighted.npz as {group: {key: array}} (tests/golden/make_qap_weighted.py describes the keys)"""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'qap_weighted.npz'))
    groups = {}
    for k in d.files:
        g, rest = k.split('/', 1)
        groups.setdefault(g, {})[rest] = d[k]
    return groups


def perm_matrix(row, preds):
    n = len(row)
    p = np.zeros((n, n))
    p[row, preds] = 1
    return p


def score(A, B, perm):
    return np.trace(A @ perm @ B @ perm.T) / 2, np.sum(A) / 2, np.sum(B) / 2


def improve(A, B, perm):
    r, p = linear_sum_assignment(-A @ perm @ B)
    return perm_matrix(r, p), int(np.sum(p == np.arange(A.shape[0])))


def greedy_qap(A, B, perm, T):
    """-> (s_best, na, nb, acc_best, T_best), and as a sixth value the matching whose score is s_best (the reference returns none)."""
    s_best, na, nb = score(A, B, perm)              # the INITIAL matching's score ...
    perm_best = perm
    perm_p, acc_best = improve(A, B, perm)          # ... next to the fixed points of a matching that is never scored
    T_best = 0
    for i in range(T):
        perm_p, acc = improve(A, B, perm_p)
        s, na, nb = score(A, B, perm_p)
        if s > s_best:
            acc_best, s_best, T_best, perm_best = acc, s, i, perm_p
    return s_best, na, nb, acc_best, T_best, np.argmax(perm_best, 1)


def acc_qap_pair(cost, g1, g2):
    """one pair of all_acc_qap: cost = -log_softmax(scores) -> (col_ind, acc, qap, planted)"""
    _, col = linear_sum_assignment(cost)
    return col, int(np.sum(col == np.arange(len(col)))), (g1 * (g2[col, :][:, col])).sum(), (g1 * g2).sum()


def objective(A, B, pi):
    """float64 (qap, trace, planted, na, nb) of one pair for the matching pi (index form)"""
    Bp = B[np.ix_(pi, pi)]
    return (A * Bp).sum(), (A * Bp.T).sum(), (A * B).sum(), A.sum(), B.sum()


def gamma(m):
    """the any-order summation bound of m fp32 terms (also valid for fma chains): |error| <= gamma(m) * sum |terms|"""
    return m * U / (1 - m * U)


def objective_bounds(A, B, pi):
    """the bounds that go with `objective`: gamma(n^2) * (sum |a||b| per product form, sum |a|, sum |b|)"""
    n = A.shape[0]
    g = gamma(n * n)
    aA, aB = np.abs(A), np.abs(B)
    aBp = aB[np.ix_(pi, pi)]
    return g * (aA * aBp).sum(), g * (aA * aBp.T).sum(), g * (aA * aB).sum(), g * aA.sum(), g * aB.sum()
