"""fp64 numpy restatement of the cross-entropy against labels, the reference of tests/test_ce_labels_host.py,
tests/test_gpu_ce_labels.py and tests/test_gpu_train_labels.py.

With t_i = labels[b, i], over the live rows i < n_b and live columns j < n_b of pair b:
    lse_i    = log sum_j exp(S_ij)                                  (every live row)
    loss_b   = sum over i with 0 <= t_i < n_b of (lse_i - S[i, t_i])
    dS[i][j] = (exp(S_ij - lse_i) - [j == t_i]) * gscale            (rows with a target; the whole row is 0 without one)
A live row whose label lies outside [0, n_b) has no target (torch's ignore_index).  Nothing outside the n_b x n_b corner is read;
everything outside it is returned as zero."""
import numpy as np


def has_target(labels, nv):
    """(B, N) bool: live rows whose label is a live column"""
    labels = np.asarray(labels)
    nv = np.asarray(nv).reshape(-1, 1)
    rows = np.arange(labels.shape[1])[None, :] < nv
    return rows & (labels >= 0) & (labels < nv)


def batch_ce(S, labels, nv, gscale=1.0, lse=None):
    """S (B, N, N), labels (B, N) ints, nv (B,) -> (lse (B, N), loss (B,), dS (B, N, N)) in fp64.
    lse: take the rows' log-sum-exp as given (the kernel's own fp32 values) instead of computing it, for dS."""
    S = np.asarray(S, dtype=np.float64)
    B, N, _ = S.shape
    labels = np.asarray(labels)
    out_lse = np.zeros((B, N))
    loss = np.zeros(B)
    dS = np.zeros((B, N, N))
    ok = has_target(labels, nv)
    for b in range(B):
        n = int(nv[b])
        if n == 0:
            continue
        blk = S[b, :n, :n]
        if lse is None:
            m = blk.max(1)
            l = m + np.log(np.exp(blk - m[:, None]).sum(1))
        else:
            l = np.asarray(lse, dtype=np.float64)[b, :n]
        out_lse[b, :n] = l
        rows = np.nonzero(ok[b, :n])[0]
        t = labels[b, rows].astype(np.int64)
        loss[b] = (l[rows] - blk[rows, t]).sum()
        p = np.exp(blk[rows] - l[rows, None])
        p[np.arange(len(rows)), t] -= 1.0
        dS[b, rows, :n] = p * gscale
    return out_lse, loss, dS


def ce_scale(S, lse, labels, nv):
    """Per pair the sum of |lse_i| + |S[i, t_i]| over the rows with a target: the magnitude an fp32 sum of the loss terms is rounded
    against (the labelled form of _ce_scale in tests/test_gpu_score_loss.py)"""
    S = np.asarray(S, dtype=np.float64)
    ok = has_target(labels, nv)
    out = np.zeros(S.shape[0])
    for b, i in zip(*np.nonzero(ok)):
        out[b] += abs(lse[b, i]) + abs(S[b, i, int(labels[b, i])])
    return out


def embedding_grads(e1, e2, dS, nv):
    """de1[b, c, i] = sum_j e2[b, c, j] dS[b, i, j], de2[b, c, j] = sum_i e1[b, c, i] dS[b, i, j] over the live corner (fp64); padding
    columns of the embeddings are not read"""
    e1, e2 = np.asarray(e1, dtype=np.float64), np.asarray(e2, dtype=np.float64)
    d1, d2 = np.zeros(e1.shape), np.zeros(e2.shape)
    for b in range(e1.shape[0]):
        n = int(nv[b])
        d1[b, :, :n] = e2[b, :, :n] @ dS[b, :n, :n].T
        d2[b, :, :n] = e1[b, :, :n] @ dS[b, :n, :n]
    return d1, d2


def label_cases(B, N, nv, rng):
    """name -> (B, N) int32 labels, -1 in the padding: a random permutation of each pair's live vertices, the identity, a constant
    row (every t_i = 0: not a permutation), and a permutation with holes: -1 and labels >= n_b (below N where n_b < N, N and N + 5
    otherwise) among the live rows"""
    nv = np.asarray(nv)
    perm = np.full((B, N), -1, dtype=np.int32)
    ident = np.full((B, N), -1, dtype=np.int32)
    const = np.full((B, N), -1, dtype=np.int32)
    for b in range(B):
        n = int(nv[b])
        perm[b, :n] = rng.permutation(n)
        ident[b, :n] = np.arange(n)
        const[b, :n] = 0
    holes = perm.copy()
    for b in range(B):
        n = int(nv[b])
        for i in range(n):
            k = (i + b) % 4
            if k == 1:
                holes[b, i] = -1
            elif k == 3:
                holes[b, i] = n if n < N else (N if i % 2 else N + 5)
    return {'perm': perm, 'identity': ident, 'constant': const, 'holes': holes}
