"""numpy restatement of the bf16 input slab that fgnn_spectral_slab16 (csrc/spectral_slab.hip) and fgnn_to_bf16_pad write: fp32
features (G, c, N, N) -> round-to-nearest-even bf16 -> (G, CP, ldp) uint16 with row pitch ldr, everything outside the n_g x n_g
corner of the first c channels exact +0.  Shared by tests/test_spectral_step_host.py (checked there against torch's own bfloat16
conversion) and readable next to the kernel's header comment."""
import numpy as np


def pitches(N, extra_ldr=0, extra_ldp=0):
    """The engine's pitches: ldr = N rounded up to 8, ldp = N * ldr rounded up to 64 (+ optional slack in the same granules)."""
    ldr = (N + 7) // 8 * 8 + extra_ldr
    return ldr, (N * ldr + 63) // 64 * 64 + extra_ldp


def bf16_rne(x):
    """fp32 array -> the uint16 bit patterns of its bf16 roundings (nearest, ties to even; NaN stays a quiet NaN)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(x)
    if nan.any():
        r[nan] = ((u[nan] >> 16) | 0x40).astype(np.uint16)
    return r


def slab(features, nvalid, CP, ldr, ldp):
    """features: (G, c, N, N) fp32; nvalid: None or G integers (clamped to [0, N]) -> (G, CP, ldp) uint16"""
    G, c, N, _ = features.shape
    assert c <= CP and ldr >= N and ldr % 8 == 0 and ldp >= N * ldr and ldp % 64 == 0
    out = np.zeros((G, CP, ldp), dtype=np.uint16)
    plane = out[:, :, :N * ldr].reshape(G, CP, N, ldr)          # (a view: ldp >= N * ldr and the slice is contiguous per channel)
    for g in range(G):
        n = N if nvalid is None else min(max(int(nvalid[g]), 0), N)
        plane[g, :c, :n, :n] = bf16_rne(features[g, :, :n, :n])
    out[:, :, :N * ldr] = plane.reshape(G, CP, N * ldr)
    return out
