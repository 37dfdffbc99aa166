"""Float64 restatement of the log-domain Sinkhorn recurrence of fgnn_sinkhorn / qap.sinkhorn and of its degenerate-pair rule, for the
tests.  Written from the specification in include/fgnn_hip.h with numpy's own log-add-exp; it shares no code with the host route
of qap.py (which subtracts the maxima by hand).

Per pair, on the n x n corner: Z = S / tau, f = g = 0, `iters` times f_i = -LSE_j(Z_ij + g_j) then g_j = -LSE_i(Z_ij + f_i);
P = exp(Z + f + g) on the corner, 0 around it; err = max_i |sum_j P_ij - 1|.  A pair with n = 0, a NaN or a +inf in the corner, or
a row or a column whose entries are all -inf is degenerate: status 1, P = 1 / n on the corner, err = 0."""
import numpy as np


def degenerate(Z):
    n = len(Z)
    if n == 0 or np.isnan(Z).any() or np.isposinf(Z).any():
        return True
    dead = np.isneginf(Z)
    return bool(dead.all(axis=1).any() or dead.all(axis=0).any())


def sinkhorn_pair(S, tau, iters):
    """S: (n, n) array -> (P (n, n) float64, err, status)"""
    Z = np.asarray(S, dtype=np.float64) / float(tau)
    n = len(Z)
    if degenerate(Z):
        return np.full((n, n), 1.0 / n if n else 0.0), 0.0, 1
    f, g = np.zeros(n), np.zeros(n)
    for _ in range(int(iters)):
        f = -np.logaddexp.reduce(Z + g[None, :], axis=1)
        g = -np.logaddexp.reduce(Z + f[:, None], axis=0)
    P = np.exp(Z + f[:, None] + g[None, :])
    return P, float(np.abs(P.sum(axis=1) - 1.0).max()), 0


def sinkhorn(scores, nvalid=None, tau=1.0, iters=20):
    """scores: (B, N, N) array; nvalid: B vertex counts or None -> (P (B, N, N) float64, err (B,), status (B,) int64)"""
    scores = np.asarray(scores)
    B, N = scores.shape[0], scores.shape[-1]
    sizes = [N] * B if nvalid is None else [min(max(int(n), 0), N) for n in nvalid]
    P, err, status = np.zeros((B, N, N)), np.zeros(B), np.zeros(B, dtype=np.int64)
    for b, n in enumerate(sizes):
        P[b, :n, :n], err[b], status[b] = sinkhorn_pair(scores[b, :n, :n], tau, iters)
    return P, err, status


SIZES = (1, 2, 31, 32, 33, 64, 65, 192, 193, 256)      # 192 = FGNN_SINKHORN_LDS_MAX_N: the last size whose scores stay in LDS


def batch(N, seed=0, bound=32.0):
    """-> (scores (3, N, N) float32 uniform in [-bound, bound] on each corner and NaN around it, nvalid): a pair of N vertices, a
    ragged one, and one of 0 (odd N) or 1 (even N) vertices"""
    rng = np.random.default_rng(1000 * N + seed)
    nvalid = np.array([N, max(N - N // 3, 1), N % 2 == 0], dtype=np.int64)
    s = np.full((3, N, N), np.nan, dtype=np.float32)
    for b, n in enumerate(nvalid):
        s[b, :n, :n] = rng.uniform(-bound, bound, (n, n)).astype(np.float32)
    return s, nvalid
