"""Independent restatements of GRAMPA (csrc/grampa.hip, qap.grampa) for the tests:

(a) `eig`: the float64 eigen formula X = sum_ij u_i u_i^T H v_j v_j^T / ((lambda_i - mu_j)^2 + eta^2) for symmetric A, B;
(b) `kron_solve`: for any square A, B the dense float64 solve of the n^2 x n^2 system (T^T T + eta^2 I) vec(X) = vec(H) with
    T = I (x) A - B^T (x) I (column-major vec: vec(A X - X B) = T vec(X));
(c) `cg32`: the conjugate-gradient recurrence the kernels run, in numpy with fp32 operands and fp64 sums -- a YARDSTICK for what fp32
    conjugate gradient reaches on given inputs, not a bit-exact model: its products are numpy's fp32 matmul, whose summation order need
    not be the matrix cores' (up to 33 vertices the chain is cheap enough to walk as the kernel does, k ascending, one fp32 rounding per
    term).  The elementwise updates are single-rounded fmas, formed in float64 from fp32 inputs and rounded once.

`standardize64` is the float64 (w - m) / (sqrt(n) sd) of the prologue, `true_residual` the float64 ||H - (T^T T + eta^2) X|| / ||H||.
"""
import numpy as np

CHAIN_MAX_N = 33


def eta2_of(eta):
    """eta^2 as the launch forms it: the fp32 eta squared in double, rounded once to fp32"""
    e = float(np.float32(eta))
    return np.float32(e * e)


def eig(A, B, eta=0.2, H=None):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    n = len(A)
    H = np.ones((n, n)) if H is None else np.asarray(H, dtype=np.float64)
    lam, U = np.linalg.eigh(A)
    mu, V = np.linalg.eigh(B)
    K = 1.0 / ((lam[:, None] - mu[None, :]) ** 2 + eta * eta)
    return U @ (K * (U.T @ H @ V)) @ V.T


def kron_solve(A, B, eta=0.2, H=None):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    n = len(A)
    H = np.ones((n, n)) if H is None else np.asarray(H, dtype=np.float64)
    I = np.eye(n)
    T = np.kron(I, A) - np.kron(B.T, I)
    x = np.linalg.solve(T.T @ T + eta * eta * np.eye(n * n), H.reshape(-1, order='F'))
    return x.reshape(n, n, order='F')


def true_residual(A, B, X, eta=0.2, H=None):
    A, B, X = (np.asarray(m, dtype=np.float64) for m in (A, B, X))
    n = len(A)
    H = np.ones((n, n)) if H is None else np.asarray(H, dtype=np.float64)
    S = A @ X - X @ B
    return np.linalg.norm(H - (A.T @ S - S @ B.T + eta * eta * X)) / np.linalg.norm(H)


def standardize64(W):
    """-> the standardised matrix (float64), or None where the off-diagonal entries have no variance (or n < 2)"""
    W = np.asarray(W, dtype=np.float64)
    n = len(W)
    if n < 2:
        return None
    off = ~np.eye(n, dtype=bool)
    m = W[off].sum() / (n * (n - 1))
    sd = np.sqrt(((W[off] - m) ** 2).sum() / (n * (n - 1)))
    if not sd > 0:
        return None
    out = (W - m) / (np.sqrt(float(n)) * sd)
    out[~off] = 0.0
    return out


def _fma32(a, b, c):
    """fp32 inputs -> a b + c rounded once to fp32 (the product of two fp32 values is exact in float64)"""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def _mm32(X, Y):
    n = X.shape[1]
    if n > CHAIN_MAX_N:
        return X @ Y
    acc = np.zeros((X.shape[0], Y.shape[1]), dtype=np.float32)
    for k in range(n):
        acc = _fma32(X[:, k:k + 1], Y[k:k + 1, :], acc)
    return acc


def cg32(A, B, eta=0.2, H=None, maxiter=256, tol=1e-6):
    """-> (X float32, nit, res, status) of the recurrence of csrc/grampa.hip on the fp32 images of A, B, H"""
    A, B = np.asarray(A, dtype=np.float32), np.asarray(B, dtype=np.float32)
    n = len(A)
    H = np.ones((n, n), dtype=np.float32) if H is None else np.asarray(H, dtype=np.float32)
    e2 = eta2_of(eta)
    X, R, P = np.zeros((n, n), dtype=np.float32), H.copy(), H.copy()
    r0 = rr = float((H.astype(np.float64) ** 2).sum())
    nit, res, status = 0, 1.0, 1
    for _ in range(maxiter):
        S = _mm32(A, P) - _mm32(P, B)
        Q = _fma32(e2, P, _mm32(A.T, S) - _mm32(S, B.T))
        pq = float((P.astype(np.float64) * Q.astype(np.float64)).sum())
        if not (np.isfinite(pq) and pq > 0):
            return X, nit, res, 3
        alpha = np.float32(rr / pq)
        R = _fma32(-alpha, Q, R)
        rn = float((R.astype(np.float64) ** 2).sum())
        if not np.isfinite(rn):
            return X, nit, res, 3
        X = _fma32(alpha, P, X)
        nit, res = nit + 1, float(np.sqrt(rn / r0))
        if res < float(np.float32(tol)):
            status = 0
            break
        P = _fma32(np.float32(rn / rr), P, R)
        rr = rn
    return X, nit, res, status


def rel_err(X, Xa):
    return float(np.abs(np.asarray(X, dtype=np.float64) - Xa).max() / np.abs(Xa).max())
