"""float64 numpy pieces of one FAQ round (scipy/optimize/_qap.py, _quadratic_assignment_faq, maximize=True, no seeds, no shuffling),
the test pairs, and the error bounds the GPU tests of fgnn_qapw_faq hold the kernels to (DESIGN.md 11.5 derives them).
tests/test_faq_host.py holds the host route of qap.faq to SciPy itself.

f(P) = tr(A^T P B P^T);  G = A P B^T + A^T P B;  q = argmax_Q <G, Q>;  with R = P - Q: f(Q + x R) = f(Q) + b x + a x^2."""
import functools

import numpy as np
from scipy.optimize import linear_sum_assignment, quadratic_assignment

import two_opt_weighted_ref as W
from graph_neural_net_amd import synthetic

U = 2.0 ** -24
STOPPED_ON_TOL, MAXITER, FAILED = 0, 1, 2


def gamma(m):
    return m * U / (1 - m * U)


# ------------------------------------------------------------------------------------------------------------------ the pairs
def zero_one_pair(n, seed, family='Regular'):
    """-> (A, B) float64 0/1, symmetric, zero diagonal: a `family` parent and its noise-0.1 copy (synthetic.make_pair)"""
    rng = np.random.default_rng(1000 * n + seed)
    x, y = synthetic.make_pair(rng, n, family, 0.2, 0.1)
    return x[0].astype(np.float64), y[0].astype(np.float64)


def directed_pair(n, seed):
    """-> (A, B) float64 0/1, directed, with loops: B is A relabelled with a tenth of its entries redrawn"""
    rng = np.random.default_rng(77 * n + seed)
    A = (rng.random((n, n)) < 0.3).astype(np.float64)
    M = np.where(rng.random((n, n)) < 0.1, (rng.random((n, n)) < 0.3).astype(np.float64), A)
    q = rng.permutation(n)
    B = np.zeros_like(A)
    B[np.ix_(q, q)] = M
    return A, B


def real_pair(n, seed, symmetric=True):
    """-> (A, B) float64 holding fp32 values: real weights in (-0.5, 1.5) on 40 % of the entries, B = A relabelled plus noise"""
    rng = np.random.default_rng(31 * n + seed)
    A = (rng.random((n, n)) * 2 - 0.5) * (rng.random((n, n)) < 0.4)
    M = A + 0.05 * rng.standard_normal((n, n)) * (rng.random((n, n)) < 0.5)
    if symmetric:
        A, M = np.triu(A, 1), np.triu(M, 1)
        A, M = A + A.T, M + M.T
    q = rng.permutation(n)
    B = np.zeros_like(A)
    B[np.ix_(q, q)] = M
    return A.astype(np.float32).astype(np.float64), B.astype(np.float32).astype(np.float64)


def exact_pair(n, seed, symmetric, kind):
    """integer ('int') or dyadic ('dyadic') weights: tests/two_opt_weighted_ref.py's pairs"""
    A, B, _ = W.make_pair(n, seed, symmetric, kind)
    return A, B


def interior_start(n, seed):
    """a doubly stochastic P inside the polytope: half the barycenter, a quarter each of two permutations; as fp32 values"""
    rng = np.random.default_rng(5 * n + seed)
    P = np.full((n, n), 0.5 / max(n, 1))
    for _ in range(2):
        P[np.arange(n), rng.permutation(n)] += 0.25
    return P.astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------------- one round, in float64
def objective(A, B, P):
    return float((A * (P @ B @ P.T)).sum())                       # tr(A^T P B P^T)


def gradient(A, B, P):
    return A @ P @ B.T + A.T @ P @ B


def gradient_abs(A, B, P):
    """|A| |P| |B|^T + |A|^T |P| |B|: what the rounding errors of G scale with"""
    A, B, P = np.abs(A), np.abs(B), np.abs(P)
    return A @ P @ B.T + A.T @ P @ B


def gradient_bound(A, B, P):
    """element-wise bound on |G_fp32 - G|: T = P [B^T | B] is an fmaf chain of n terms per entry, G = [A | A^T] [T0; T1] one of 2 n
    terms over the rounded T: gamma_2n (1 + gamma_n) + gamma_n <= gamma_3n, so m = 3 n"""
    return gamma(3 * len(A)) * gradient_abs(A, B, P)


def direction(G):
    return linear_sum_assignment(G, maximize=True)[1]


def line_coefficients(A, B, P, q):
    """(a, b) as SciPy forms them, with two more products"""
    Q = np.eye(len(A))[q]
    R = P - Q
    AR, BR = A.T @ R, B @ R.T
    return float((AR.T * BR).sum()), float((AR * B.T[q]).sum() + (A * BR[q]).sum())


def step_size(a, b):
    if -a > 0 and 0 <= -b / (2 * a) <= 1:
        return -b / (2 * a)
    return float(np.argmin([0, -(b + a)]))


def segment_maximum(A, B, P, q):
    """max over x in [0, 1] of f(Q + x (P - Q)) -> (value, x)"""
    a, b = line_coefficients(A, B, P, q)
    x = step_size(a, b)
    return objective(A, B, np.eye(len(A))[q]) + b * x + a * x * x, x


def line_search_tolerance(A, B, P, q, P1):
    """How far f(P1) of the device's P1 may lie from segment_maximum: the device forms a = <G, P> / 2 - <G, Q> + f(Q) and
    b = <G, Q> - 2 f(Q) from its fp32 G in fp64, so with d = gradient_bound: |a' - a| <= <d, P> / 2 + <d, Q>, |b' - b| <= <d, Q>, the
    quadratic it maximises is within E = <d, P> / 2 + 2 <d, Q> of the true one on [0, 1], and the true value at its maximiser within
    2 E of the true maximum.  P1 is rounded once to fp32: f moves by at most u <|G|(P1), P1> (1 + O(u)); the factor 2 covers the
    second-order term and the fp64 roundings."""
    d = gradient_bound(A, B, P)
    E = float((d * P).sum()) / 2 + 2 * float(d[np.arange(len(A)), q].sum())
    return 2 * E + 2 * U * float((gradient_abs(A, B, P1) * np.abs(P1)).sum())


def scipy_faq(A, B, P0='barycenter', maxiter=30, tol=0.03):
    res = quadratic_assignment(A, B, method='faq', options={'maximize': True, 'P0': P0, 'maxiter': maxiter, 'tol': tol})
    return res.col_ind.astype(np.int64), float(res.fun), int(res.nit)


# ---------------------------------------------------------------------------------------------------------- the quality pairs
QUALITY_N, QUALITY_PAIRS = 33, 32


@functools.lru_cache(maxsize=None)
def quality_set(seed_set):
    """-> (As, Bs, funs): the 32 real-weighted pairs of seed set `seed_set` and float64 SciPy's objective on each; computed once"""
    pairs = [real_pair(QUALITY_N, 1000 * seed_set + k) for k in range(QUALITY_PAIRS)]
    funs = tuple(scipy_faq(A, B)[1] for A, B in pairs)
    return tuple(p[0] for p in pairs), tuple(p[1] for p in pairs), funs
