"""numpy + SciPy restatement of the reference's matching decode (toolbox/utils.py:225-256 perm_matrix / score / improve /
greedy_qap; the per-pair arithmetic of toolbox/metrics.py:168-193 all_acc_qap), in the reference's own float64 matrix form, for the
cases beyond tests/golden/qap_decode.npz.  tests/test_qap_host.py holds it to the fixture and, where the reference is present, to
the imported reference on fresh seeds."""
import os

import numpy as np
from scipy.optimize import linear_sum_assignment

TS = (0, 1, 10)                                                     # the T of the fixture's greedy_qap results
GREEDY_KEYS = ('s_best', 'na', 'nb', 'acc_best', 'T_best')


def fixture_groups():
    """tests/golden/qap_decode.npz as {group: {key: array}} (tests/golden/make_qap_decode.py describes the keys)"""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'qap_decode.npz'))
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


def unpack_bits(words, n=None):
    """(…, N, ceil(N/32)) 32-bit words -> (…, N, N) float64 0/1 (bit j of word row i = W[i][j]); n: the corner to cut out"""
    w = np.ascontiguousarray(words).view(np.uint32)
    N = w.shape[-2]
    full = np.unpackbits(w.view(np.uint8), axis=-1, bitorder='little')[..., :N]
    full = full.astype(np.float64)
    return full if n is None else full[..., :n, :n]


def pack_bits(w, N=None):
    """(n, n) 0/1 -> (N, ceil(N/32)) uint32 words, zero-padded to N >= n"""
    n = w.shape[0]
    N = n if N is None else N
    words = (N + 31) // 32
    padded = np.zeros((N, words * 32), dtype=bool)
    padded[:n, :n] = w != 0
    return np.packbits(padded.reshape(N, words, 32), axis=-1, bitorder='little').view(np.uint32).reshape(N, words)
