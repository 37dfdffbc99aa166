"""numpy restatement of SciPy's 2-opt for the QAP (scipy/optimize/_qap.py, _quadratic_assignment_2opt) with maximize=True and a full
partial_guess: the same scan order, acceptance rule and evaluation count, with the gain of an exchange evaluated as a difference
instead of SciPy's O(n^2) objective per candidate.  tests/test_two_opt_host.py holds it to SciPy itself.

The objective is S(p) = sum_{a,k} A[a,k] B[p(a),p(k)] = sum A * Bp with Bp = B[p][:, p].  Exchanging p(i) and p(j) swaps rows i, j and
columns i, j of Bp.  For one i and every j at once (vectors over j), with r = sum(A * Bp, 1) and c = sum(A * Bp, 0):
    rows i, j     Bp A[i] + A Bp[i] - r[i] - r      (A[i] against row j of Bp, A[j] against row i)
    columns i, j  A[:,i] Bp + A^T Bp[:,i] - c[i] - c
    crossings     (A[i,i] + A[j,j] - A[i,j] - A[j,i]) (Bp[i,i] + Bp[j,j] - Bp[i,j] - Bp[j,i])
the last line being what the first two count wrongly at (i,i), (i,j), (j,i), (j,j).  No symmetry and no zero diagonal is assumed."""
import numpy as np

OPTIMUM, STOPPED, NO_PERMUTATION = 0, 1, 2


def make_pair(n, seed, symmetric, noise=0.1):
    """-> (A, B, q): B is A relabelled by q (B[q(i), q(k)] = A[i, k]) with a fraction `noise` of its entries flipped"""
    rng = np.random.default_rng(1000 * n + seed)
    A = (rng.random((n, n)) < 0.35).astype(np.int64)
    flip = rng.random((n, n)) < noise
    if symmetric:
        A = np.triu(A, 1)
        A = A + A.T
        flip = np.triu(flip, 1)
        flip = flip | flip.T
    q = rng.permutation(n)
    B = np.zeros_like(A)
    B[np.ix_(q, q)] = A ^ flip
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
    return int((A * B[np.ix_(p, p)]).sum())


def gains_of_row(A, Bp, r, c, i):
    """the gain of exchanging i with every j (entry i itself is 0)"""
    dA, dB = np.diag(A), np.diag(Bp)
    rows = Bp @ A[i] + A @ Bp[i] - r[i] - r
    cols = A[:, i] @ Bp + Bp[:, i] @ A - c[i] - c
    cross = (dA[i] + dA - A[i] - A[:, i]) * (dB[i] + dB - Bp[i] - Bp[:, i])
    return rows + cols + cross


def two_opt(A, B, start, max_swaps=None):
    """A, B: (n, n) integer matrices; start: n columns -> {'perm', 'qap', 'swaps', 'nit', 'status'}.  status 1: stopped after
    max_swaps accepted exchanges (nit then holds the accepted positions only); 2: start is no permutation (perm = start, qap -1)."""
    A, B = np.asarray(A, dtype=np.int64), np.asarray(B, dtype=np.int64)
    p = np.array(start, dtype=np.int64)
    n = len(p)
    if sorted(p.tolist()) != list(range(n)):
        return {'perm': p, 'qap': -1, 'swaps': 0, 'nit': 0, 'status': NO_PERMUTATION}
    if n == 0:
        return {'perm': p, 'qap': 0, 'swaps': 0, 'nit': 0, 'status': OPTIMUM}
    Bp = B[np.ix_(p, p)]
    swaps = nit = 0
    while max_swaps is None or swaps < max_swaps:
        r, c = (A * Bp).sum(1), (A * Bp).sum(0)
        for i in range(n):
            better = np.flatnonzero(gains_of_row(A, Bp, r, c, i)[i + 1:] > 0)
            if better.size:
                j = i + 1 + int(better[0])
                nit += j - i + 1                                   # (i,i) .. (i,j)
                break
            nit += n - i                                           # (i,i) .. (i,n-1)
        else:
            return {'perm': p, 'qap': int((A * Bp).sum()), 'swaps': swaps, 'nit': nit, 'status': OPTIMUM}
        swaps += 1
        p[[i, j]] = p[[j, i]]
        Bp = B[np.ix_(p, p)]
    return {'perm': p, 'qap': int((A * Bp).sum()), 'swaps': swaps, 'nit': nit, 'status': STOPPED}


def batch(As, Bs, starts, max_swaps=None):
    """lists of pairs -> dict of lists, perm as lists"""
    out = [two_opt(A, B, s, max_swaps) for A, B, s in zip(As, Bs, starts)]
    return {k: [o[k].tolist() if k == 'perm' else o[k] for o in out] for k in ('perm', 'qap', 'swaps', 'nit', 'status')}
