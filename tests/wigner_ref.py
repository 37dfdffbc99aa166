"""Numpy restatement of csrc/wigner.hip (graph_neural_net_amd/wigner.py): the correlated Gaussian (Wigner) pairs.

The integer part is exact -- Philox words from tests/pairgen_ref.py, the addressing t = i N + j -> block t >> 3, 64-bit word
(t & 7) >> 1, the 24-bit uniforms -- and Box-Muller is evaluated in float64 from those uniforms, so `normals` is the value the
kernel's fp32 logf / sqrtf / sinpif / cospif approximate.  rho, sig and the scale c are rounded to float32 as the host and the
kernel round them; the products and the fma that follow are taken in float64 on those float32 inputs.
"""
import math

import numpy as np

import pairgen_ref as R

PARENT_STREAM, NOISE_STREAM = 10, 11


def uniforms(seed, k, stream, t):
    """(u, v) of the normals with linear indices t (any integer array): exact float64 images of the 24-bit uniforms."""
    t = np.asarray(t, dtype=np.int64).reshape(-1)
    w0 = R.draws(seed, k, stream, t & ~np.int64(1))          # the 64-bit word (t & 7) >> 1 of block t >> 3: its low half ...
    w1 = R.draws(seed, k, stream, t | np.int64(1))           # ... and its high half
    return ((w0 >> 8) + 1) * 2.0 ** -24, (w1 >> 8) * 2.0 ** -24


def normals(seed, k, stream, t):
    """z_stream(t) in float64: sqrt(-2 ln u) cos(2 pi v) for even t, sqrt(-2 ln u) sin(2 pi v) for odd t."""
    t = np.asarray(t, dtype=np.int64).reshape(-1)
    u, v = uniforms(seed, k, stream, t)
    r = np.sqrt(-2.0 * np.log(u))
    return r * np.where(t & 1, np.sin(2.0 * np.pi * v), np.cos(2.0 * np.pi * v))


def coefficients(noise):
    """(rho, sig) as the float32 values the launch receives (computed in double, rounded once)."""
    s = float(noise)
    return np.float32(math.sqrt(max(0.0, 1.0 - s * s))), np.float32(s)


def scale_of(n, scale='wigner'):
    """c_b: float32 1 / sqrtf(n) (a correctly rounded division of a correctly rounded root), or 1."""
    return np.float32(1.0) / np.sqrt(np.float32(n)) if scale == 'wigner' else np.float32(1.0)


def pair(seed, k, N, noise, vertex_proba=1.0, scale='wigner', support=None, labels=None):
    """Pair k of dataset `seed` -> (A, B, n): (N, N) float64 matrices, zero outside the n x n corner and on the diagonal.
    support: None or (S1, S2), (N, N) bool masks (unpermuted); labels: None or the (>= n,) planted permutation -- B is then returned
    relabelled, out[pi(i)][pi(j)] = B_ij."""
    n = R.vertex_count(seed, k, N, R.threshold(vertex_proba))
    rho, sig = coefficients(noise)
    c = float(scale_of(n, scale))
    A, B = np.zeros((N, N)), np.zeros((N, N))
    i, j = np.triu_indices(n, 1)
    t = i * N + j
    a = c * normals(seed, k, PARENT_STREAM, t)
    b = float(rho) * a + float(sig) * (c * normals(seed, k, NOISE_STREAM, t))
    A[i, j] = A[j, i] = a
    B[i, j] = B[j, i] = b
    if support is not None:
        A, B = A * support[0], B * support[1]
    if labels is not None:
        pi = np.asarray(labels[:n], dtype=np.int64)
        out = np.zeros_like(B)
        out[np.ix_(pi, pi)] = B[:n, :n]
        B = out
    return A, B, n


def pairs(seed, index, N, noise, **kw):
    """pair() for every index -> (A (B, N, N), B (B, N, N), n (B,)); noise may be one value or one per pair."""
    index = list(index)
    noises = list(noise) if np.ndim(noise) else [noise] * len(index)
    labels = kw.pop('labels', None)
    support = kw.pop('support', None)
    out = [pair(seed, k, N, s, labels=None if labels is None else labels[b],
                support=None if support is None else (support[0][b], support[1][b]), **kw)
           for b, (k, s) in enumerate(zip(index, noises))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out])


def row_sums64(W):
    """float64 row sums of (..., N, N)"""
    return np.asarray(W, dtype=np.float64).sum(-1)


def row_sums32(W):
    """The kernel's fp32 order on the float32 matrix W (..., N, N), N <= 256: lane l < 64 adds its columns l, l + 64, l + 128,
    l + 192 (those < N) in ascending order onto +0, then six butterfly steps s_l += s_(l ^ o), o = 32, 16, 8, 4, 2, 1; every
    addition rounds to float32.  -> (..., N) float32"""
    W = np.asarray(W, dtype=np.float32)
    N = W.shape[-1]
    s = np.zeros(W.shape[:-1] + (64,), dtype=np.float32)
    for m in range((N + 63) // 64):
        chunk = W[..., 64 * m:min(N, 64 * m + 64)]
        s[..., :chunk.shape[-1]] = s[..., :chunk.shape[-1]] + chunk
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lanes ^ o]
    return s[..., 0]


def standardised(W, n):
    """The off-diagonal entries above the diagonal of the n x n corners of (B, N, N), times sqrt(n): unit normals (scale 'wigner')"""
    out = []
    for w, m in zip(W, n):
        i, j = np.triu_indices(int(m), 1)
        out.append(np.asarray(w, dtype=np.float64)[i, j] * math.sqrt(float(m)))
    return np.concatenate(out)


def moments(x):
    """(mean, variance about the mean, standardised fourth moment m4 = E[(x - mean)^4] / var^2)"""
    x = np.asarray(x, dtype=np.float64)
    mu = x.mean()
    d = x - mu
    var = (d * d).mean()
    return mu, var, (d ** 4).mean() / (var * var)
