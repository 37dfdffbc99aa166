"""Seeds for the QAP solvers: the test seed sets, SciPy with partial_match, float64 numpy pieces of one seeded FAQ round
(scipy/optimize/_qap.py, _quadratic_assignment_faq with partial_match) and the error bounds the GPU tests hold fgnn_qapw_faq_seeded
to.  tests/faq_ref.py has the pairs and the unseeded pieces; DESIGN.md 11.7 derives the bounds.

On the free block, with C = A21 B21^T + A12^T B12:  f(P) = tr(A22^T P B22 P^T) + <C, P>,  G = C + A22 P B22^T + A22^T P B22."""
import numpy as np
from scipy.optimize import quadratic_assignment

import faq_ref as R

U = R.U


# --------------------------------------------------------------------------------------------------------------------- the seeds
def seed_vector(n, m, seed, truth=None):
    """-> (n,) int64: m rows chosen uniformly hold a seed, -1 elsewhere.  The targets are truth[row] when a matching `truth` is
    given, else m distinct columns drawn uniformly (any partial injection is a legal partial_match)."""
    rng = np.random.default_rng(911 * n + 13 * m + seed)
    rows = np.sort(rng.choice(n, size=m, replace=False))
    cols = np.asarray(truth)[rows] if truth is not None else rng.choice(n, size=m, replace=False)
    sd = np.full(n, -1, dtype=np.int64)
    sd[rows] = cols
    return sd


def partial_match_of(sd):
    """a seed vector -> SciPy's (m, 2) array, rows ascending (SciPy's 2opt writes the targets onto the ascending fixed rows)"""
    rows = np.flatnonzero(np.asarray(sd) >= 0)
    return np.stack([rows, np.asarray(sd)[rows]], axis=1).astype(np.int64).reshape(-1, 2)


def lists_of(sd, n):
    """-> (free_a, free_b, seed_a, seed_b) as SciPy takes them: ascending free rows / columns, seeded rows ascending"""
    sd = np.asarray(sd)[:n]
    seed_a = np.flatnonzero(sd >= 0)
    seed_b = sd[seed_a]
    return np.flatnonzero(sd < 0), np.setdiff1d(np.arange(n), seed_b), seed_a, seed_b


def completed(sd, seed):
    """a permutation that holds every seed of sd: the free rows get the free columns in a random order"""
    n = len(sd)
    free_a, free_b, _, _ = lists_of(sd, n)
    p = np.array(sd, dtype=np.int64)
    p[free_a] = np.random.default_rng(seed).permutation(free_b)
    return p


# ----------------------------------------------------------------------------------------------------------------------- SciPy
def scipy_faq(A, B, sd, P0='barycenter', maxiter=30, tol=0.03):
    res = quadratic_assignment(A, B, method='faq', options={'maximize': True, 'partial_match': partial_match_of(sd), 'P0': P0,
                                                            'maxiter': maxiter, 'tol': tol})
    return res.col_ind.astype(np.int64), float(res.fun), int(res.nit)


def scipy_2opt(A, B, sd, assign):
    n = len(A)
    guess = np.stack([np.arange(n), np.asarray(assign)], axis=1)
    res = quadratic_assignment(A, B, method='2opt', options={'maximize': True, 'partial_match': partial_match_of(sd),
                                                             'partial_guess': guess})
    return res.col_ind.astype(np.int64), int(res.fun), int(res.nit)


# ------------------------------------------------------------------------------------------------------- one round, in float64
def blocks(A, B, sd):
    """-> (A22, B22, C, Cabs): the free blocks, SciPy's const_sum and the sum of the absolute values of its terms"""
    free_a, free_b, seed_a, seed_b = lists_of(sd, len(A))
    A22, B22 = A[np.ix_(free_a, free_a)], B[np.ix_(free_b, free_b)]
    A21, A12 = A[np.ix_(free_a, seed_a)], A[np.ix_(seed_a, free_a)]
    B21, B12 = B[np.ix_(free_b, seed_b)], B[np.ix_(seed_b, free_b)]
    return A22, B22, A21 @ B21.T + A12.T @ B12, np.abs(A21) @ np.abs(B21).T + np.abs(A12).T @ np.abs(B12)


def objective(A22, B22, C, P):
    return R.objective(A22, B22, P) + float((C * P).sum())


def gradient(A22, B22, C, P):
    return C + R.gradient(A22, B22, P)


def gradient_abs(A22, B22, Cabs, P):
    return Cabs + R.gradient_abs(A22, B22, P)


def gradient_bound(A22, B22, Cabs, P, m):
    """element-wise bound on |G_fp32 - G|, an any-order summation bound over the 2 u + 2 m products of an entry: the 2 u of the
    quadratic part pass the two chained products of faq_ref.gradient_bound, (1 + u)^(3 u) at most; the 2 m of C one fmaf chain,
    (1 + u)^(2 m); the epilogue's addition rounds once more.  Every product is off by at most gamma_(3 u + 2 m + 1)."""
    return R.gamma(3 * len(A22) + 2 * m + 1) * gradient_abs(A22, B22, Cabs, P)


def line_coefficients(A22, B22, C, P, q):
    """(a, b) of f(Q + x (P - Q)) = f(Q) + b x + a x^2"""
    a, b = R.line_coefficients(A22, B22, P, q)
    Q = np.eye(len(A22))[q]
    return a, b + float((C * (P - Q)).sum())


def segment_maximum(A22, B22, C, P, q):
    a, b = line_coefficients(A22, B22, C, P, q)
    x = R.step_size(a, b)
    return objective(A22, B22, C, np.eye(len(A22))[q]) + b * x + a * x * x, x


def line_search_tolerance(A22, B22, C, Cabs, P, q, P1, m):
    """How far f(P1) of the device's P1 may lie from segment_maximum.  The device forms, in fp64 from its fp32 G and C,
    a = (<G,P> - <C,P>) / 2 - (<G,Q> - <C,Q>) + q(Q) and b = (<G,Q> - <C,Q>) - 2 q(Q) + <C,P> - <C,Q>.  With d = gradient_bound (which
    also bounds the error of C alone): |a' - a| <= <d,P> + 2 <d,Q> and |b' - b| <= <d,P> + 3 <d,Q>, so the quadratic it maximises is
    within E = 2 <d,P> + 5 <d,Q> of the true one on [0, 1] and the true value at its maximiser within 2 E of the true maximum.  P1 is
    rounded once to fp32: f moves by at most u <|G|(P1), P1> (1 + O(u)); the factor 2 covers the second-order term."""
    d = gradient_bound(A22, B22, Cabs, P, m)
    n = len(A22)
    E = 2 * float((d * P).sum()) + 5 * float(d[np.arange(n), q].sum())
    return 2 * E + 2 * U * float((gradient_abs(A22, B22, Cabs, P1) * np.abs(P1)).sum())
