"""fp64 numpy restatement of the per-pair loss weights of the fused step, the reference of
tests/test_pair_weights_host.py, tests/test_gpu_pair_weights.py and tests/test_gpu_train_weights.py.  It extends the conventions of
tests/ce_labels_ref.py (labels, has_target, batch_ce, embedding_grads).

With w (B,) >= 0 and CE_b, dS_b of ce_labels_ref.batch_ce on the live n_b x n_b corner of pair b:
    loss_sum = sum over b with w_b != 0 of w_b * CE_b
    dS_b     = w_b * gscale * (softmax_row(S_b) - target)     for w_b != 0;   exactly 0 everywhere for w_b == 0
w_b == 0 is a select: nothing of such a pair is read, so NaN or inf in its scores reach neither loss nor gradient.

reduction_weights(mode, nv, live, user): the weights of a reduction and their normaliser D,
    'mean':          w_b = [b < live] u_b,                   D = sum_{b < live} n_b u_b
    'mean_of_mean':  w_b = [b < live and n_b > 0] u_b / n_b, D = sum_{b < live, n_b > 0} u_b
so that loss_sum / D is triplet_loss(mode) over the live pairs (u = 1)."""
import numpy as np

import ce_labels_ref as R


def identity_labels(B, N, nv):
    """(B, N) int32: labels[b, i] = i on the live rows, -1 in the padding (the label-less launches' target)"""
    lab = np.full((B, N), -1, dtype=np.int32)
    for b in range(B):
        lab[b, :int(nv[b])] = np.arange(int(nv[b]))
    return lab


def weighted_ce(S, labels, nv, w, gscale=1.0, lse=None):
    """S (B, N, N) (pairs with w_b == 0 may hold anything), labels (B, N) ints (None: the identity), nv (B,), w (B,)
    -> (loss_sum, per-pair w_b CE_b (B,), dS (B, N, N)) in fp64.  lse: as in ce_labels_ref.batch_ce."""
    S = np.asarray(S, dtype=np.float64)
    B, N, _ = S.shape
    w = np.asarray(w, dtype=np.float64).reshape(B)
    nv = np.asarray(nv).reshape(B)
    on = w != 0
    if labels is None:
        labels = identity_labels(B, N, nv)
    nv_on = np.where(on, nv, 0)                  # the select: a switched-off pair is an empty pair
    S_on = np.where(on[:, None, None], S, 0.0)
    lse_on = None if lse is None else np.where(on[:, None], np.asarray(lse, dtype=np.float64), 0.0)
    _, ce, dS = R.batch_ce(S_on, labels, nv_on, gscale, lse=lse_on)
    pair = np.where(on, w * ce, 0.0)
    return pair.sum(), pair, dS * np.where(on, w, 0.0)[:, None, None]


def weighted_embedding_grads(e1, e2, dS, nv, w):
    """ce_labels_ref.embedding_grads with the switched-off pairs as empty pairs (their embeddings are not read)"""
    on = np.asarray(w).reshape(-1) != 0
    nv_on = np.where(on, np.asarray(nv).reshape(-1), 0)
    return R.embedding_grads(np.where(on[:, None, None], e1, 0.0), np.where(on[:, None, None], e2, 0.0), dS, nv_on)


def reduction_weights(mode, nv, live=None, user=None):
    """-> (w (B,) fp64, D float)"""
    nv = np.asarray(nv, dtype=np.int64).reshape(-1)
    B = len(nv)
    live = B if live is None else max(0, min(B, int(live)))
    u = np.ones(B) if user is None else np.asarray(user, dtype=np.float64).reshape(B)
    on = np.arange(B) < live
    if mode == 'mean':
        return np.where(on, u, 0.0), float((nv * u)[on].sum())
    if mode != 'mean_of_mean':
        raise ValueError(mode)
    on = on & (nv > 0)
    return np.where(on, u / np.maximum(nv, 1), 0.0), float(u[on].sum())
