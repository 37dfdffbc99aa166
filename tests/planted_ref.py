"""Numpy restatement of planted permutations (``graph_neural_net_amd/csrc/planted.hip``, ``graph_neural_net_amd/planted.py``) and of
the reference's label-taking metrics (toolbox/metrics.py:92-141) and decode loops with a label.

Test infrastructure only; the package never imports it.  Randomness is the Philox of ``tests/pairgen_ref.py``: the planted
permutation of pair k is Fisher-Yates from the top on the identity, ``j = (u32_t * (t + 1)) >> 32`` for t = n - 1 .. 1, with
``u32_t`` draw t of stream 7 of the pair.
"""
import numpy as np
import torch

import pairgen_ref as PR

STREAM_PLANTED = 7


def planted_perm(seed, k, n):
    p = np.arange(n, dtype=np.int64)
    if n > 1:
        u = PR.draws(seed, k, STREAM_PLANTED, np.arange(n))
        for t in range(n - 1, 0, -1):
            j = int(PR.below(int(u[t]), t + 1))
            p[t], p[j] = p[j], p[t]
    return p


def planted_labels(seed, pairs, N, sizes=None):
    """(len(pairs), N) int32: row b = the permutation of pair pairs[b] on [0, n_b), then -1; a negative pair index gives all -1"""
    out = np.full((len(pairs), N), -1, dtype=np.int32)
    for b, k in enumerate(pairs):
        n = N if sizes is None else int(sizes[b])
        if k >= 0:
            out[b, :n] = planted_perm(seed, int(k), n)
    return out


def inverse(lab, n):
    inv = np.empty(n, dtype=np.int64)
    inv[lab[:n]] = np.arange(n)
    return inv


def relabel_matrix(M, lab, n):
    """out[pi(i)][pi(j)] = M[i][j] on the n x n corner, zeros elsewhere (M: (..., N, N))"""
    out = np.zeros_like(M)
    inv = inverse(lab, n)
    out[..., :n, :n] = M[..., :n, :n][..., inv, :][..., :, inv]
    return out


def unpack_bits(words, N):
    """(B, N, W) uint32/int32 -> (B, N, N) uint8"""
    w = np.ascontiguousarray(words).view(np.uint32)
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], N, -1), axis=-1, bitorder='little')[:, :, :N]


def pack_bits(M):
    """(B, N, N) 0/1 -> (B, N, ceil(N/32)) uint32, padding bits zero"""
    B, N, _ = M.shape
    W = (N + 31) // 32
    full = np.zeros((B, N, 32 * W), dtype=np.uint8)
    full[:, :, :N] = M
    return np.packbits(full, axis=-1, bitorder='little').view(np.uint32).reshape(B, N, W)


def relabel_bits(words, labels, sizes=None):
    B, N, _ = words.shape
    M = unpack_bits(words, N)
    out = np.stack([relabel_matrix(M[b], labels[b], N if sizes is None else int(sizes[b])) for b in range(B)])
    return pack_bits(out)


# ---- the reference's metric loops with a label (toolbox/metrics.py:92-141), per graph on the valid corner --------------------
def _label(labels, b, n):
    return np.arange(n) if labels is None else np.asarray(labels[b])[:n]


def _cost(scores, b, n):
    """the reference's cost matrix: log_softmax where the scores live (toolbox/metrics.py:99,105), then to the host"""
    return -torch.log_softmax(torch.as_tensor(scores[b, :n, :n]).float(), -1).cpu().numpy()


def lsap_counts(scores, sizes, labels=None):
    from scipy.optimize import linear_sum_assignment
    out = []
    for b, n in enumerate(sizes):
        cost = _cost(scores, b, n)
        _, preds = linear_sum_assignment(cost)
        out.append(int(np.sum(preds == _label(labels, b, n))))
    return out


def max_counts(scores, sizes, labels=None):
    out = []
    for b, n in enumerate(sizes):
        preds = np.argmax(torch.as_tensor(scores[b, :n, :n]).cpu().numpy(), 1) if n else np.zeros(0, dtype=np.int64)
        out.append(int(np.sum(preds == _label(labels, b, n))))
    return out


# ---- all_acc_qap / greedy_qap with a label, on exactly representable matrices (0/1 or dyadic): float64 is exact ---------------
def qap_of(A, Bm, pi):
    return (A * Bm[np.ix_(pi, pi)]).sum()


def all_acc_qap(scores, As, Bs, sizes, labels=None):
    from scipy.optimize import linear_sum_assignment
    acc, qap, planted = [], [], []
    for b, n in enumerate(sizes):
        lab = _label(labels, b, n)
        _, col = linear_sum_assignment(_cost(scores, b, n))
        A, Bm = As[b][:n, :n].astype(np.float64), Bs[b][:n, :n].astype(np.float64)
        acc.append(int(np.sum(col == lab)))
        qap.append(qap_of(A, Bm, col))
        planted.append(qap_of(A, Bm, lab))
    return np.array(acc), np.array(qap), np.array(planted)


def greedy_qap(A, Bm, pi0, T, lab):
    """toolbox/utils.py:225-256 with preds == lab in place of preds == arange -> (s_best, acc_best, T_best)"""
    from scipy.optimize import linear_sum_assignment
    n = len(pi0)

    def P(pi):
        m = np.zeros((n, n))
        m[np.arange(n), pi] = 1
        return m

    def score(pi):
        return np.trace(A @ P(pi) @ Bm @ P(pi).T) / 2

    def improve(pi):
        _, col = linear_sum_assignment(-A @ P(pi) @ Bm)
        return col, int(np.sum(col == lab))

    s_best = score(pi0)
    pi, acc_best = improve(pi0)
    T_best = 0
    for i in range(T):
        pi, acc = improve(pi)
        s = score(pi)
        if s > s_best:
            s_best, acc_best, T_best = s, acc, i
    return s_best, acc_best, T_best
