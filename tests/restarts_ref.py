"""Numpy float64 restatement of the random restarts of ``qap.faq`` (``graph_neural_net_amd/csrc/qap_restarts.hip``).

Test infrastructure only; the package never imports it.  Written from the rule, on the draws of ``pairgen_ref`` (a Philox of its
own), so that both routes of the package can be compared with it:

* ``uniform``: U_k[i, j] = ((u32 >> 8) + 1) 2^-24, u32 = raw draw (k << 32) | (i << 16) | j of pair stream 9 of pair p;
* ``doubly_stochastic``: SciPy's ``_doubly_stochastic``, the Sinkhorn-Knopp loop whose first test runs on the unscaled matrix;
* ``starts``: start 0 = the base (or the barycenter), start k >= 1 = (base + K_k) / 2; n = 1: K = [[1]]; n = 0: nothing;
* ``best_of``: among the restarts whose status is not 2 the largest objective wins, a NaN never, ties go to the smallest k; without
  a candidate restart 0 stands.
"""
import numpy as np

import pairgen_ref

RESTART_STREAM = 9
TOL, ROUNDS = 1e-3, 1000


def uniform(seed, p, k, n):
    i, j = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64), indexing='ij')
    u32 = pairgen_ref.draws(seed, p, RESTART_STREAM, ((k << 32) | (i << 16) | j).reshape(-1))
    return ((u32 >> 8) + 1).reshape(n, n) / 16777216.0


def doubly_stochastic(P):
    """-> (K, the updates performed)"""
    c = 1 / P.sum(axis=0)
    r = 1 / (P @ c)
    K, rounds = P, 0
    for rounds in range(ROUNDS + 1):
        if rounds == ROUNDS or ((np.abs(K.sum(axis=1) - 1) < TOL).all() and (np.abs(K.sum(axis=0) - 1) < TOL).all()):
            break
        c = 1 / (r @ P)
        r = 1 / (P @ c)
        K = r[:, None] * P * c
    return K, rounds


def starts(seed, p, R, n, N, base=None):
    """-> (R, N, N) float64, zeros outside the n x n corner; base: (n, n) or None for the barycenter"""
    out = np.zeros((R, N, N))
    if n == 0:
        return out
    J = np.asarray(base, dtype=np.float64) if base is not None else np.full((n, n), 1.0 / n)
    out[0, :n, :n] = J
    for k in range(1, R):
        K = doubly_stochastic(uniform(seed, p, k, n))[0] if n > 1 else np.ones((1, 1))
        out[k, :n, :n] = (J + K) / 2
    return out


class _FixedUniform(np.random.Generator):
    """a generator whose uniform() hands out U: SciPy's randomized start then IS (J + _doubly_stochastic(U)) / 2"""

    def __init__(self, U):
        super().__init__(np.random.PCG64(0))
        self.U = U

    def uniform(self, low=0.0, high=1.0, size=None):
        assert tuple(size) == self.U.shape
        return self.U


def scipy_restart(A, B, seed, p, k, maxiter=30, tol=0.03):
    """SciPy's FAQ from restart k of pair p -> (col_ind, fun, nit).  Restart 0 is its barycenter.  A start k >= 1 cannot be handed
    in as a matrix -- SciPy's check of a P0 matrix asks for sums within 1e-5 of 1, K's own tolerance is 1e-3 -- so it goes in as
    SciPy's own 'randomized' start, built from U_k."""
    from scipy.optimize import quadratic_assignment
    options = {'maximize': True, 'maxiter': maxiter, 'tol': tol, 'P0': 'barycenter'}
    if k > 0:
        options.update(P0='randomized', rng=_FixedUniform(uniform(seed, p, k, len(A))))
    res = quadratic_assignment(A, B, method='faq', options=options)
    return res.col_ind.astype(np.int64), float(res.fun), int(res.nit)


def best_of(q, status, veto=None):
    """one pair's R objectives and statuses -> the winner's k"""
    best = None
    for k in range(len(q)):
        if status[k] == 2 or (veto is not None and veto[k] == 2) or q[k] != q[k]:
            continue
        if best is None or q[k] > q[best]:
            best = k
    return 0 if best is None else best
