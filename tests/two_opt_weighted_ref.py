"""float64 numpy reference of the pairwise-exchange search on real-weighted pairs: SciPy's loop (scipy/optimize/_qap.py,
_quadratic_assignment_2opt, maximize=True, a full partial_guess) -- the scan (0,0), (0,1), .., (0,n-1), (1,1), .., the first pair with
a positive gain exchanged, the scan started over, nit counted per evaluation -- with the gain of an exchange evaluated as a
difference instead of SciPy's O(n^2) objective per candidate.  tests/test_two_opt_weighted_host.py holds it to SciPy itself.

S(p) = sum_{a,k} A[a,k] Bp[a,k] with Bp = B[p][:, p].  The gain of exchanging i < j:
      sum_{k != i,j} (A[i,k] - A[j,k]) (Bp[j,k] - Bp[i,k])                       rows i, j
    + sum_{k != i,j} (A[k,i] - A[k,j]) (Bp[k,j] - Bp[k,i])                       columns i, j
    + (A[i,i] - A[j,j]) (Bp[j,j] - Bp[i,i]) + (A[i,j] - A[j,i]) (Bp[j,i] - Bp[i,j])
No symmetry and no zero diagonal is assumed.  As in the kernel the search is a counted loop: n^2 exchanges without max_swaps.

The module also makes the test pairs (integer weights in [-3, 3], dyadic weights k/8 with |k| <= 8: every product, gain and
objective up to n = 256 is exact in fp32 as in float64) and keeps one reference result per batch (`reference`)."""
import functools

import numpy as np

OPTIMUM, STOPPED, NO_PERMUTATION = 0, 1, 2


def make_pair(n, seed, symmetric, kind='int', noise=0.1):
    """-> (A, B, q) float64: A has weights on 35 % of its entries, B is A relabelled by q (B[q(i), q(k)] = A[i, k]) with a fraction
    `noise` of its entries redrawn.  symmetric: both symmetric with a zero diagonal; else directed with loops."""
    rng = np.random.default_rng(100003 * n + 17 * seed + (kind == 'dyadic'))

    def weights():
        if kind == 'int':
            return rng.integers(-3, 4, (n, n)).astype(np.float64)
        return rng.integers(-8, 9, (n, n)).astype(np.float64) / 8

    A = weights() * (rng.random((n, n)) < 0.35)
    other = weights() * (rng.random((n, n)) < 0.35)
    redraw = rng.random((n, n)) < noise
    M = np.where(redraw, other, A)
    if symmetric:
        A, M = np.triu(A, 1), np.triu(M, 1)
        A, M = A + A.T, M + M.T
    q = rng.permutation(n)
    B = np.zeros_like(A)
    B[np.ix_(q, q)] = M
    return A, B, q


def transposed(q, k, seed):
    """q with k transpositions applied"""
    rng = np.random.default_rng(seed)
    p = q.copy()
    for _ in range(k):
        i, j = rng.choice(len(p), 2, replace=False)
        p[[i, j]] = p[[j, i]]
    return p


def objective(A, B, p):
    return float((A * B[np.ix_(p, p)]).sum())


def terms_of_row(A, Bp, i):
    """-> (n, 2 n + 2) float64: row j holds the terms of the gain of exchanging i and j (zeros for k = i, j; row i is all zero)"""
    n = len(A)
    j = np.arange(n)
    rows = (A[i][None, :] - A) * (Bp - Bp[i][None, :])                     # [j, k]
    cols = (A[:, [i]] - A).T * (Bp - Bp[:, [i]]).T                         # [j, k] = (A[k,i] - A[k,j]) (Bp[k,j] - Bp[k,i])
    keep = np.ones((n, n), dtype=bool)
    keep[:, i] = False
    keep[j, j] = False
    dA, dB = np.diag(A), np.diag(Bp)
    cross = np.stack([(dA[i] - dA) * (dB - dB[i]), (A[i] - A[:, i]) * (Bp[:, i] - Bp[i])], 1)
    t = np.concatenate([np.where(keep, rows, 0.0), np.where(keep, cols, 0.0), cross], 1)
    t[i] = 0.0
    return t


def gains(A, Bp):
    """-> (gain, bound_sum): (n, n) float64, the gain of every pair and the sum of the absolute values of its terms"""
    n = len(A)
    g, s = np.zeros((n, n)), np.zeros((n, n))
    for i in range(n):
        t = terms_of_row(A, Bp, i)
        g[i], s[i] = t.sum(1), np.abs(t).sum(1)
    return g, s


def two_opt(A, B, start, max_swaps=None):
    """A, B: (n, n) matrices; start: n columns -> {'perm', 'qap', 'swaps', 'nit', 'status'}.  status 1: stopped after max_swaps
    (None: n^2) accepted exchanges (nit then holds the accepted positions only); 2: start is no permutation (perm = start, qap -1)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    p = np.array(start, dtype=np.int64)
    n = len(p)
    if sorted(p.tolist()) != list(range(n)):
        return {'perm': p, 'qap': -1.0, 'swaps': 0, 'nit': 0, 'status': NO_PERMUTATION}
    if n == 0:
        return {'perm': p, 'qap': 0.0, 'swaps': 0, 'nit': 0, 'status': OPTIMUM}
    bound = n * n if max_swaps is None else min(max_swaps, n * n)
    Bp = B[np.ix_(p, p)]
    swaps = nit = 0
    while swaps < bound:
        for i in range(n):
            better = np.flatnonzero(terms_of_row(A, Bp, i).sum(1)[i + 1:] > 0)
            if better.size:
                j = i + 1 + int(better[0])
                nit += j - i + 1                                   # (i,i) .. (i,j)
                break
            nit += n - i                                           # (i,i) .. (i,n-1)
        else:
            return {'perm': p, 'qap': float((A * Bp).sum()), 'swaps': swaps, 'nit': nit, 'status': OPTIMUM}
        swaps += 1
        p[[i, j]] = p[[j, i]]
        Bp = B[np.ix_(p, p)]
    return {'perm': p, 'qap': float((A * Bp).sum()), 'swaps': swaps, 'nit': nit, 'status': STOPPED}


KEYS = ('perm', 'qap', 'swaps', 'nit', 'status')


def batch_of(N, B, symmetric, kind):
    """-> (As, Bs, starts): pair b has n_b vertices (0, 1 and N among them when B > 1).  Starts: random up to N = 65; from N = 128
    up the planted matching with 8 random transpositions, so that a search stays short."""
    rng = np.random.default_rng(7 * N + B)
    sizes = [N] * B if B == 1 else ([0, 1, N] + rng.integers(0, N + 1, B).tolist())[:B]
    As, Bs, starts = [], [], []
    for b, n in enumerate(sizes):
        A, Bm, q = make_pair(n, b, symmetric, kind)
        starts.append(rng.permutation(n) if N <= 65 or n < 2 else transposed(q, 8, b))
        As.append(A), Bs.append(Bm)
    return As, Bs, starts


@functools.lru_cache(maxsize=None)
def reference(N, B, symmetric, kind, max_swaps=None):
    """the reference result of every pair of batch_of(N, B, symmetric, kind): a tuple of dicts, computed once, not to be changed"""
    As, Bs, starts = batch_of(N, B, symmetric, kind)
    return tuple(two_opt(A, Bm, s, max_swaps) for A, Bm, s in zip(As, Bs, starts))


# the exact cases of tests/test_gpu_two_opt_weighted.py (the host test asserts that each ends as a local optimum within n^2 exchanges)
CASES = [(1, 5, True, 'int'), (2, 70, False, 'dyadic'), (31, 5, False, 'int'), (32, 1, True, 'dyadic'), (33, 70, True, 'int'),
         (33, 5, False, 'dyadic'), (50, 5, True, 'dyadic'), (50, 1, False, 'int'), (64, 1, False, 'int'), (64, 5, True, 'dyadic'),
         (65, 5, False, 'dyadic'), (65, 1, True, 'int'), (128, 5, True, 'int'), (128, 1, False, 'dyadic'), (129, 5, False, 'int'),
         (129, 1, True, 'dyadic'), (256, 1, True, 'dyadic'), (256, 1, False, 'int')]
