"""CPU reference of the per-channel bf16 products (csrc/matmul16.hip): numpy only, fp64 and exact integer / rational arithmetic.

The kernels compute, per (g, c) matrix and inside the graph's nv x nv corner,
    y  = RNE_bf16(fp32(fma(z, a, b))),  b = fp32(beta - mean * a)                      (mm_src, norm8 / norm_dword)
    M  = Ya Yb,   dA = dM Yb^T,   dB = Ya^T dM        fp32 accumulation (v_mfma_f32_32x32x16_bf16), one final RNE to bf16 (cvt_pk)
Operands outside the corner are zero.  `operands` restates the load stage bit for bit, `products` forms the three products in
fp64, `rne_bf16` the final rounding without a double rounding, `accum_bound` the order-independent bound on the fp32
accumulation.  `grid_case` draws inputs on a dyadic grid on which every fp32 partial sum is exact in any order, so that the
stored output must equal rne_bf16(exact product) with no tolerance; it asserts that precondition for every case it returns.
"""
from fractions import Fraction

import numpy as np

U32 = 2.0 ** -24                      # unit roundoff of fp32
GRID_LIMIT = 2 ** 24                  # integers below it are exact in fp32


# the shapes of tests/test_gpu_matmul16_exact.py (shared with the host test that checks the exactness condition at each of them)
G, CH = 3, 3
DENSE = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160, 193, 200, 224, 225, 240, 255, 256)
RAGGED = ((64, (64, 33, 0)), (120, (120, 72, 1)), (128, (127, 64, 31)), (200, (200, 129, 96)), (224, (224, 193, 8)),
          (256, (256, 225, 40)))
SHAPES = [(n, None) for n in DENSE] + list(RAGGED)


def shape_id(s):
    return 'N%d' % s[0] if s[1] is None else 'N%d_nv%s' % (s[0], '_'.join(map(str, s[1])))


def case_seed(N, nvalid, tag=16):
    return [tag, N] + list(nvalid or ())


def ceil8(n):
    return (n + 7) // 8 * 8


# ---- roundings ------------------------------------------------------------------------------------------------------------
def _rne_to(x64, p, emin):
    """x64 (exact fp64 values) rounded to nearest even on the grid of a binary format with p significant bits and smallest
    normal exponent emin; returned as fp64 (exact: the result has at most p bits).  frexp / ldexp / rint are exact, so the
    fp64 input is rounded exactly once."""
    x = np.asarray(x64, dtype=np.float64)
    _, e = np.frexp(x)                                     # |x| = m 2^e, m in [0.5, 1): the leading bit has weight 2^(e-1)
    q = np.maximum(e - p, emin - (p - 1)).astype(np.int32)  # exponent of the last kept bit (subnormals: fixed quantum)
    return np.ldexp(np.rint(np.ldexp(x, -q)), q)


def bf16_round(x64):
    """RNE to bf16 of exact fp64 values, as fp64."""
    return _rne_to(x64, 8, -126)


def f32_round(x64):
    """RNE to fp32 of exact fp64 values, as fp64."""
    return _rne_to(x64, 24, -126)


def rne_bf16(x64):
    """bf16 bit pattern (uint16) of the round-to-nearest-even of fp64 values.  The fp64 value is rounded once, on the bf16
    grid itself (no intermediate fp32 rounding); the result is fp32-exact, so taking the high half of its fp32 image is exact.
    Values beyond the bf16 range become infinities, like the hardware conversion."""
    r = bf16_round(x64)
    with np.errstate(over='ignore'):
        bits = r.astype(np.float32).view(np.uint32)
    return (bits >> 16).astype(np.uint16)


def bf16_value(bits):
    """fp64 value of bf16 bit patterns (uint16 or int16)."""
    b = np.asarray(bits).astype(np.uint16).astype(np.uint32) << 16
    return b.view(np.float32).astype(np.float64)


def bf16_ulp(x64):
    """Spacing of the bf16 grid in the binade of |x| (fp64): 2^(floor(log2 |x|) - 7); subnormal spacing below 2^-126."""
    _, e = np.frexp(np.abs(np.asarray(x64, dtype=np.float64)))
    return np.ldexp(1.0, np.maximum(e - 8, -133).astype(np.int32))


def f32_ulp(x64):
    _, e = np.frexp(np.abs(np.asarray(x64, dtype=np.float64)))
    return np.ldexp(1.0, np.maximum(e - 24, -149).astype(np.int32))


def _f32_of_fraction(q):
    """RNE to fp32 of an exact rational in the normal range (Fraction.__round__ rounds half to even)."""
    if q == 0:
        return 0.0
    e = abs(q.numerator).bit_length() - q.denominator.bit_length()          # 2^(e-1) <= |q| < 2^(e+1)
    if abs(q) < Fraction(2) ** e:
        e -= 1                                                              # now 2^e <= |q| < 2^(e+1)
    quantum = Fraction(2) ** (e - 23)
    return float(round(q / quantum) * quantum)


def affine_b(mean, a, beta):
    """b = fp32(beta - mean * a): ONE rounding.  mm_src writes `be - n.x * n.y`; the build contracts it into a single
    v_fma_f32 (-ffp-contract=fast, the HIP default; checked in the ISA), so the product is not rounded on its own.
    Evaluated in exact rational arithmetic (a handful of values per case)."""
    mean, a, beta = np.broadcast_arrays(np.asarray(mean, np.float64), np.asarray(a, np.float64), np.asarray(beta, np.float64))
    out = np.empty(mean.shape, np.float64)
    for i in np.ndindex(mean.shape):
        out[i] = _f32_of_fraction(Fraction(float(beta[i])) - Fraction(float(mean[i])) * Fraction(float(a[i])))
    return out


# ---- the load stage -------------------------------------------------------------------------------------------------------
def operands(z, mean, a, beta, nv):
    """y = RNE_bf16(fp32(fma(z, a, beta - mean a))) inside the nv x nv corner, 0 outside (fp64 array of bf16-exact values).
    z: (G, C, N, N) bf16-exact values; mean, a: (G, C) fp32 values; beta: (C,) fp32 values; nv: (G,) ints.
    The fma is evaluated in fp64: a bf16 times an fp32 is exact there (32 bits), and the sum with the fp32 `b` is checked to be
    exact with the error-free TwoSum; it is then rounded to fp32 and to bf16, the two roundings of the kernel."""
    z = np.asarray(z, np.float64)
    G, C, N, _ = z.shape
    a = np.asarray(a, np.float64).reshape(G, C, 1, 1)
    b = affine_b(np.asarray(mean, np.float64).reshape(G, C), a.reshape(G, C),
                 np.broadcast_to(np.asarray(beta, np.float64).reshape(1, C), (G, C))).reshape(G, C, 1, 1)
    p = z * a
    s = p + b
    bb = s - p
    err = (p - (s - bb)) + (b - bb)                        # TwoSum: p + b == s + err exactly
    assert not err.any(), 'operands: z * a + b is not exact in fp64 for these ranges'
    y = bf16_round(f32_round(s))
    return mask_corner(y, nv)


def mask_corner(x, nv):
    """x (G, C, N, N) with everything outside the per-graph nv x nv corner replaced by +0."""
    x = np.array(x, dtype=np.float64)
    for g, n in enumerate(nv):
        x[g, :, n:, :] = 0.0
        x[g, :, :, n:] = 0.0
    return x


def products(ya, yb, dm):
    """M = Ya Yb, dA = dM Yb^T, dB = Ya^T dM in fp64 (exact on grid data: every partial sum is a small integer multiple of the unit)."""
    M = np.matmul(ya, yb)
    dA = np.matmul(dm, np.swapaxes(yb, -1, -2))
    dB = np.matmul(np.swapaxes(ya, -1, -2), dm)
    return M, dA, dB


def accum_bound(absA, absB, K):
    """K 2^-24 (|A| @ |B|): bound on the error of a K-term fp32 dot product accumulated in any order (each of the at most K
    additions an element takes part in perturbs the running sum by at most 2^-24 of a partial sum of |a_k b_k|; the products of
    two bf16 values are exact in fp32).  K: the contracted length rounded up to the 16 of the MFMA k-step."""
    return K * U32 * np.matmul(absA, absB)


def k_steps(nv):
    return (int(nv) + 15) // 16 * 16


# ---- grid inputs ----------------------------------------------------------------------------------------------------------
def grid_load(opA, opB, unit):
    """max over the output elements of sum_k |OpA||OpB| / unit: the largest integer a partial sum can reach, in units of the
    term grid.  Below 2^24 every fp32 partial sum is exact whatever the order."""
    return float(np.matmul(np.abs(opA), np.abs(opB)).max() / unit) if opA.size else 0.0


def grid_case(rng, G, C, N, ldr, nvalid=None):
    """Inputs on a dyadic grid: z, dM multiples of 1/8 with |.| <= 2; mean, beta multiples of 1/8 with |.| <= 1; a in {1/2, 1, 2}
    per (g, c).  Then y = (z - mean) a + beta is a multiple of 1/16 with |y| <= 7 (bf16-exact: at most 7 significant bits), a
    forward term a multiple of 1/256 and a backward term (dM y) a multiple of 1/128.
    Returns a dict; `load` holds sum_k |OpA||OpB| / unit for the three products, asserted < 2^24 here, for every case."""
    assert ldr == ceil8(N)
    nv = np.asarray(nvalid if nvalid is not None else [N] * G, dtype=np.int64)
    assert len(nv) == G and (nv >= 0).all() and (nv <= N).all()
    eighths = lambda lim, shape: rng.integers(-8 * lim, 8 * lim + 1, size=shape).astype(np.float64) / 8.0
    c = dict(G=G, C=C, N=N, ldr=ldr, nv=nv, ragged=nvalid is not None)
    c['za'], c['zb'], c['dm'] = eighths(2, (G, C, N, N)), eighths(2, (G, C, N, N)), mask_corner(eighths(2, (G, C, N, N)), nv)
    for s in 'ab':
        c['mean_' + s] = eighths(1, (G, C))
        c['a_' + s] = rng.choice(np.array([0.5, 1.0, 2.0]), size=(G, C))
        c['beta_' + s] = eighths(1, (C,))
        y = operands(c['z' + s], c['mean_' + s], c['a_' + s], c['beta_' + s], nv)
        exact = mask_corner((c['z' + s] - c['mean_' + s][:, :, None, None]) * c['a_' + s][:, :, None, None]
                            + c['beta_' + s][None, :, None, None], nv)
        assert np.array_equal(y, exact) and np.abs(y).max(initial=0.0) <= 7 and not np.mod(y * 16, 1).any()
        c['y' + s] = y
    ya, yb, dm = c['ya'], c['yb'], c['dm']
    c['load'] = dict(M=grid_load(ya, yb, 1 / 256), dA=grid_load(dm, np.swapaxes(yb, -1, -2), 1 / 128),
                     dB=grid_load(np.swapaxes(ya, -1, -2), dm, 1 / 128))
    assert max(c['load'].values()) < GRID_LIMIT, c['load']
    c['M'], c['dA'], c['dB'] = products(ya, yb, dm)
    return c


def random_case(rng, G, C, N, ldr, nvalid=None):
    """Ordinary data: z = bf16(randn * scale + shift) (the scales of tests/diag/gpu_mm16_kernel_check.py), arbitrary fp32 mean / a /
    beta, so that the staging fma rounds for real."""
    assert ldr == ceil8(N)
    nv = np.asarray(nvalid if nvalid is not None else [N] * G, dtype=np.int64)
    c = dict(G=G, C=C, N=N, ldr=ldr, nv=nv, ragged=nvalid is not None)
    f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)
    c['za'] = bf16_round(rng.standard_normal((G, C, N, N)) * 0.3 + 1.5)
    c['zb'] = bf16_round(rng.standard_normal((G, C, N, N)) * 0.2 - 0.7)
    c['dm'] = mask_corner(bf16_round(rng.standard_normal((G, C, N, N)) * 0.05), nv)
    c['mean_a'], c['a_a'] = f32(1.5 + 0.1 * rng.standard_normal((G, C))), f32(0.8 * (1 + 0.2 * rng.standard_normal((G, C))))
    c['mean_b'], c['a_b'] = f32(-0.7 + 0.1 * rng.standard_normal((G, C))), f32(1.3 * (1 + 0.2 * rng.standard_normal((G, C))))
    c['beta_a'], c['beta_b'] = f32(0.1 * rng.standard_normal(C)), f32(0.1 * rng.standard_normal(C))
    for s in 'ab':
        c['y' + s] = operands(c['z' + s], c['mean_' + s], c['a_' + s], c['beta_' + s], nv)
    c['M'], c['dA'], c['dB'] = products(c['ya'], c['yb'], c['dm'])
    return c


def element_gate(ref64, absA, absB, K):
    """Per-element gate of a bf16 output computed with fp32 accumulation: half a bf16 ulp + accum_bound.  The fp32 sum lies within
    `acc` of ref64 and is then rounded once, by at most half the bf16 spacing of ITS binade -- which can be the next one up when
    ref64 sits just under a power of two: the spacing is taken at |ref64| + acc, the largest magnitude the sum can have."""
    acc = accum_bound(absA, absB, K)
    return 0.5 * bf16_ulp(np.abs(ref64) + acc) + acc


# ---- GraphNorm finalize folded into the forward launch (fgnn_chan_matmul_fwd16_fin) ---------------------------------------
def tile_partials(z, nv, tpg, rng, empty_frac=0.3):
    """Any partition of each graph's nv x nv corner into tpg pieces, some of them empty (the kernel only combines the pieces):
    cnt (G, tpg) and, per (g, c), {mean_t, M2_t} in fp64 rounded to fp32 -- (G, C, tpg, 2), the layout the kernel reads.
    Empty pieces carry {0, 0}."""
    G, C, N, _ = z.shape
    cnt = np.zeros((G, tpg), np.float64)
    part = np.zeros((G, C, tpg, 2), np.float64)
    for g in range(G):
        n = int(nv[g])
        if n == 0:
            continue
        live = np.flatnonzero(rng.random(tpg) >= empty_frac)
        if len(live) == 0:
            live = np.array([tpg - 1])
        owner = live[rng.integers(0, len(live), size=n * n)]
        owner[:len(live)] = live[:n * n]                    # when there is room, every live piece owns at least one element
        cnt[g] = np.bincount(owner, minlength=tpg)
        for c in range(C):
            v = z[g, c, :n, :n].reshape(-1)
            s = np.bincount(owner, weights=v, minlength=tpg)
            m = np.divide(s, cnt[g], out=np.zeros(tpg), where=cnt[g] > 0)
            part[g, c, :, 0] = m
            part[g, c, :, 1] = np.bincount(owner, weights=(v - m[owner]) ** 2, minlength=tpg)
    return f32_round(part), cnt


def nrm_records(part, cnt, nv, w, eps):
    """fp64 two-level combination of the tile partials pushed through nrm_record (csrc/fgnn_norm.h:8-18, finalize_reduce :46-64):
        m = sum n_t;  mean = sum n_t mean_t / m;  M2 = sum [M2_t + n_t (mean_t - mean)^2];  var = M2 / m;  ve = var + eps
        q = 1 / (2 sqrt(nv ve))  (0 for an empty graph);  record = {mean, w q, q, 1 / ve}
    Returns (rec (G, C, 4), gate (G, C, 4)).  The gate counts the fp32 roundings of chan_matmul_fwd16_kernel<FIN> (u = 2^-24):
      * a workgroup sum of 1024 slots is 1 in-thread addition, 6 wave levels and 7 fixed-order additions: 14 roundings on any
        path; m is a sum of small integers and exact;
      * mean: product n_t mean_t (1) + sum (14) + division (1) = 16 u, relative to sum |n_t mean_t| / m;
      * M2: each d_t = mean_t - mean inherits err(mean) and one rounding, which counts twice in d^2; n d, (n d) d and the addition
        of M2_t are 3 more, the sum 14:  err(M2) <= sum n_t 2 |d_t| err(mean) + (2 + 3 + 14) u M2   (all terms are non-negative);
      * ve: division (1) and addition (1): err(ve) <= err(M2) / m + u var + u ve;
      * r2 = 1 / ve: err(ve) / ve + 1 u relative;
      * q: product nv ve (1), sqrtf (1), division (1), the factor 2 is exact; the square root halves the relative error it receives:
        (err(ve) / ve + u) / 2 + 2 u relative;   a = w q: one more.
    One further u is added to every relative figure for the second-order terms dropped above."""
    G, C, tpg, _ = part.shape
    rec, gate = np.zeros((G, C, 4)), np.zeros((G, C, 4))
    u = U32
    for g in range(G):
        n_t = cnt[g]
        m = n_t.sum()
        for c in range(C):
            mt, m2t = part[g, c, :, 0], part[g, c, :, 1]
            mean = (n_t * mt).sum() / m if m > 0 else 0.0
            e_mean = 16 * u * (np.abs(n_t * mt).sum() / m if m > 0 else 0.0)
            d = mt - mean
            M2 = (m2t + n_t * d * d).sum()
            e_M2 = (n_t * 2 * np.abs(d)).sum() * e_mean + 19 * u * M2
            var = M2 / m if m > 0 else 0.0
            ve = var + eps
            e_ve = (e_M2 / m if m > 0 else 0.0) + u * var + u * ve
            q = 1.0 / (2.0 * np.sqrt(nv[g] * ve)) if nv[g] > 0 else 0.0
            rel_q = 0.5 * (e_ve / ve + u) + 2 * u
            wc = 1.0 if w is None else w[c]
            rec[g, c] = (mean, wc * q, q, 1.0 / ve)
            gate[g, c] = (e_mean + u * abs(mean), abs(wc * q) * (rel_q + 2 * u), q * (rel_q + u), (e_ve / ve + 2 * u) / ve)
    return rec, gate
