"""Restatement of the reference's spectral input (loaders/data_generator.py:221-232 make_laplacian / make_spectral_feature) on
numpy arrays, in fp32 and in fp64, for the cases beyond tests/golden/spectral_features.npz:

    D = W @ ones,  L = diag(1 / sqrt(D)) @ W @ diag(1 / sqrt(D)),  F_1 = eye @ L,  F_{p+1} = F_p @ L    (left to right)

with ONE convention the reference does not have: 1 / sqrt(0) is taken as 0, so an isolated vertex has a zero row and column (the
reference computes inf * 0 = NaN there and every later power is NaN in every entry).  On a graph without isolated vertices the
statements are the reference's, operation for operation (1 / sqrt(D) is evaluated by numpy, correctly rounded on every host); the
matrix products run through torch's CPU matmul like the reference's, so the fp32 form has the reference's summation order (tests/test_spectral_host.py holds it bit for bit to the fixture and, where the
reference is present, to the imported reference)."""
import os

import numpy as np
import torch

N_POWERS = 4                  # the reference's default
FIXTURE_POWERS = 8            # ref_err is recorded for this many


def fixture_groups():
    """tests/golden/spectral_features.npz as {group: {key: array}} (tests/golden/make_spectral_features.py describes the keys)"""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'spectral_features.npz'))
    groups = {}
    for k in d.files:
        g, rest = k.split('/', 1)
        groups.setdefault(g, {})[rest] = d[k]
    return groups


def unpack_bits(words, n=None):
    """(N, ceil(N/32)) uint32 / int32 bit rows -> the (n, n) 0/1 corner as float64 (n = N by default)"""
    w = np.ascontiguousarray(words).view(np.uint32)
    N = w.shape[0]
    full = np.unpackbits(w.view(np.uint8).reshape(N, -1), axis=-1, bitorder='little')[:, :N]
    n = N if n is None else int(n)
    return full[:n, :n].astype(np.float64)


def pack_bits(W, N=None):
    """(n, n) 0/1 matrix -> (N, ceil(N/32)) uint32 bit rows, bit j of word row i = W[i][j], zero outside the corner"""
    n = W.shape[0]
    N = n if N is None else N
    full = np.zeros((N, 32 * ((N + 31) // 32)), dtype=np.uint8)
    full[:n, :n] = W != 0
    return np.packbits(full, axis=-1, bitorder='little').view(np.uint32).reshape(N, -1)


def laplacian(W, dtype):
    W = torch.from_numpy(np.ascontiguousarray(W)).to(dtype)
    D = (W @ torch.ones(W.shape[-1], dtype=dtype)).numpy()
    # 1 / sqrt(D) in numpy: IEEE sqrt and division on every host.  torch's vectorised CPU kernels are not correctly rounded on
    # every instruction set (on an AVX-512 host `1 / torch.sqrt(D)` was measured one ulp off at D = 19), and the first power is
    # compared bit for bit.  The convention: 0 where the reference has inf.
    with np.errstate(divide='ignore'):
        s = torch.from_numpy(np.where(D > 0, D.dtype.type(1) / np.sqrt(D), D.dtype.type(0)).astype(D.dtype))
    return torch.diag(s) @ W @ torch.diag(s)


def spectral_feature(L, n=N_POWERS):
    out = torch.zeros((n, *L.shape), dtype=L.dtype)
    L_prev = torch.eye(L.shape[-1], dtype=L.dtype)
    for i in range(n):
        L_prev = L_prev @ L
        out[i, :, :] = L_prev
    return out


def features(W, n_powers=N_POWERS, dtype=torch.float32):
    """(n, n) 0/1 matrix (any numpy dtype) -> (n_powers, n, n) numpy array of `dtype` (torch.float32 or torch.float64)"""
    return spectral_feature(laplacian(W, dtype), n_powers).numpy()


def padded_features(bits, nvalid=None, n_powers=N_POWERS, n_out=None, dtype=torch.float32):
    """what the device writes for a batch of bit rows: (G, n_powers, n_out, n_out), the features of every n_g x n_g corner and zeros
    around them (bits outside a corner are ignored)"""
    G, N = bits.shape[0], bits.shape[1]
    n_out = N if n_out is None else n_out
    out = np.zeros((G, n_powers, N, N), dtype=np.float32 if dtype == torch.float32 else np.float64)
    for g in range(G):
        n = N if nvalid is None else min(max(int(nvalid[g]), 0), N)
        if n:
            out[g, :, :n, :n] = features(unpack_bits(bits[g], n), n_powers, dtype)
    return out[:, :, :n_out, :n_out]


def own_error(bits, nvalid=None, n_powers=N_POWERS):
    """per power, the max-abs distance of the fp32 restatement from the fp64 one over the batch: the yard-stick of a shape the
    fixture does not hold"""
    f32 = padded_features(bits, nvalid, n_powers, dtype=torch.float32).astype(np.float64)
    f64 = padded_features(bits, nvalid, n_powers, dtype=torch.float64)
    return np.abs(f32 - f64).max(axis=(0, 2, 3)), f64
