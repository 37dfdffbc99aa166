"""fp64 restatement of the GraphNorm statistics chain (csrc/norm.hip, csrc/fgnn_norm.h), the rounding-error bounds of its
kernels, and a float32 emulation of the kernels' summation order.  numpy only: no GPU, no library.

The record of channel c of graph g is {mean, a, q, r2} (include/fgnn_hip.h, models/layers.py:71-80):
    mean = sum_t n_t mean_t / sum_t n_t          M2 = sum_t [M2_t + n_t (mean_t - mean)^2]        m = sum_t n_t
    var = M2 / m      r2 = 1 / (var + eps)       q = 1 / (2 sqrt(n (var + eps)))                  a = w q
with q = a = 0 and mean = 0 for an empty graph (n = 0).

Error bounds.  u = 2^-24 is the unit round-off of fp32.  A sum of k terms that a kernel forms with `A` serial adds per lane
followed by the 6-level wave butterfly passes every term through at most A + 6 additions, so its error is at most
(A + 6 + r) u sum|term| to first order, r being the roundings of the term itself.  The second-order remainder and the
roundings an fma saves are what the tests' safety factor of 2 is for; no bound below is fitted to a measured error.

  finalize (gn_finalize_kernel, finalize_wave, finalize_wave_any): L = ceil(tpg / 64) adds per lane, K = L + 9.
    sn = sum n_t is exact (integers below 2^24).  sm = sum n_t mean_t: 1 rounding of the product, L + 6 additions, 1 division:
        eps_mean = |d mean| <= K u (sum n_t |mean_t| / sum n_t)                                  (K = L + 8, one spare)
    M2 is summed with the computed mean, mean + e, |e| <= eps_mean:
        sum n_t (mean_t - mean - e)^2 = sum n_t (mean_t - mean)^2 - 2 e sum n_t (mean_t - mean) + m e^2
    and the cross term vanishes (e is the same for every tile, mean is the weighted mean).  Every term is non-negative and
    costs 4 roundings (difference, square, times n_t, plus M2_t) and L + 6 additions:
        |d M2| <= (K + 4) u M2 + m eps_mean^2
    var = M2 / m, var + eps, 1 / (.) are 3 roundings:  rel(r2) <= dM2 / (m (var + eps)) + 3 u
    q = 1 / (2 sqrt(n (var + eps))) takes half of that through the root, and product, root and division round once each
    (4 u covers them and the halved 2 u of var + eps):  rel(q) <= rel(r2) / 2 + 4 u,   rel(a) <= rel(q) + u.
  two-pass statistics (gn_stats_kernel) and plane kernels: the same composition with K = A + 8, A the serial adds per lane:
    ceil(N^2 / 64) on a dense plane, n ceil(n / 64) on a ragged one, 16 per thread in the plane kernels (whose 4-wave LDS
    combine adds 2 levels, inside the 8).
  wave sums over a plane or over tile partials (S1, S2): (A + 8) u sum|term|.
  reduce_cols: ceil(rows / 4) serial adds per row group, 2 levels of the LDS combine, the scale product and the product of
    the two scales:  (ceil(rows / 4) + 5) u sum_r |in[r][i]| |scale|.
  affine_reduce: 1 product, ceil(G / 8) serial adds, 8 serial adds of the LDS combine:  (ceil(G / 8) + 10) u sum_g |term|.
  y = (v - mean) a + beta:  |dy| <= |a| eps_mean + |v - mean| |a| (rel(a) + 3 u) + u |y|.
  dz = a dy + cb (z - mean) + cc with cb = -a S2 r2 / m, cc = -a S1 / m: see dz_bound.
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
EPS32 = np.float32(1e-5)
EPS = float(EPS32)          # the kernels receive eps as a float
F32, F64 = np.float32, np.float64


def tiles_of(N, T=32, pitch=None):
    return (N * (pitch or N) + T - 1) // T


def nv_list(G, N, nvalid):
    return [N] * G if nvalid is None else [int(v) for v in nvalid]


# ---------------------------------------------------------------------------------------------- fp64 restatement
class Partials:
    """Per-tile statistics of a (G, C, N, N) tensor: mean_t, M2_t (G, C, tpg) and cnt (G, tpg)."""

    def __init__(self, mean_t, m2_t, cnt):
        self.mean_t, self.m2_t, self.cnt = mean_t, m2_t, cnt
        self.G, self.C, self.tpg = mean_t.shape

    def part(self, tr):
        """(G, tpg, C, 2) for tr = 0 (the fp32 kernels), (G, C, tpg, 2) for tr = 1 (the `_tpg` entry points)."""
        p = np.stack([self.mean_t, self.m2_t], axis=-1)
        return np.ascontiguousarray(p if tr else p.transpose(0, 2, 1, 3))


def tile_partials(x, nvalid=None, T=32, pitch=None, dtype=F32):
    """Tile t of a plane is its T consecutive elements [tT, tT + T) at row pitch `pitch`; only the valid n x n corner counts,
    a tile without a valid element is {0, 0} with count 0.  Computed in fp64, returned in `dtype`."""
    x = np.asarray(x, dtype=F64)
    G, C, N, _ = x.shape
    pitch = pitch or N
    tpg = tiles_of(N, T, pitch)
    val = np.zeros((G, C, tpg * T))
    msk = np.zeros((G, tpg * T))
    for g, n in enumerate(nv_list(G, N, nvalid)):
        plane = np.zeros((C, N, pitch))
        plane[:, :n, :n] = x[g, :, :n, :n]
        val[g, :, :N * pitch] = plane.reshape(C, -1)
        mk = np.zeros((N, pitch))
        mk[:n, :n] = 1
        msk[g, :N * pitch] = mk.reshape(-1)
    val = val.reshape(G, C, tpg, T)
    mk = msk.reshape(G, 1, tpg, T)
    cnt = mk.sum(-1)
    mean_t = (val * mk).sum(-1) / np.maximum(cnt, 1)
    m2_t = (mk * (val - mean_t[..., None]) ** 2).sum(-1)
    return Partials(mean_t.astype(dtype), m2_t.astype(dtype), cnt[:, 0].astype(dtype))


def unpack_part(part, tr, G, C, tpg):
    """the two storage orders -> (G, C, tpg) arrays of the two fields, fp64"""
    p = np.asarray(part, dtype=F64).reshape((G, C, tpg, 2) if tr else (G, tpg, C, 2))
    if not tr:
        p = p.transpose(0, 2, 1, 3)
    return p[..., 0], p[..., 1]


def record_of(mean, M2, m, nv, w, eps=EPS):
    """fp64 record from mean / M2 / m (G, C), vertex counts (G) and weights (C) or None; also what the bounds need"""
    G, C = mean.shape
    nvc = np.asarray(nv, dtype=F64).reshape(G, 1) * np.ones((1, C))
    var = np.where(m > 0, M2 / np.maximum(m, 1), 0.0)
    ve = var + eps
    q = np.where(nvc > 0, 1.0 / (2.0 * np.sqrt(np.maximum(nvc, 1) * ve)), 0.0)
    wv = np.ones(C) if w is None else np.asarray(w, dtype=F64)
    return dict(mean=mean, a=wv[None, :] * q, q=q, r2=1.0 / ve, M2=M2, m=m * np.ones_like(mean), ve=ve)


def finalize_ref(part, cnt, nvalid, N, tr, C, w=None, eps=EPS):
    """record of every (g, c) from the fp32 tile partials as the kernel reads them, in fp64.  `mabs` = sum n_t |mean_t| / m."""
    cnt = np.asarray(cnt, dtype=F64)
    G, tpg = cnt.shape
    mean_t, m2_t = unpack_part(part, tr, G, C, tpg)
    n_t = cnt[:, None, :]
    m = n_t.sum(-1)
    mean = np.where(m > 0, (n_t * mean_t).sum(-1) / np.maximum(m, 1), 0.0)
    M2 = (m2_t + n_t * (mean_t - mean[..., None]) ** 2).sum(-1)
    rec = record_of(mean, M2, m, nv_list(G, N, nvalid), w, eps)
    rec['mabs'] = np.where(m > 0, (n_t * np.abs(mean_t)).sum(-1) / np.maximum(m, 1), 0.0)
    return rec


def direct_ref(x, nvalid, w=None, eps=EPS):
    """the same record straight from the tensor: fp64 mean / biased variance over the valid corner"""
    x = np.asarray(x, dtype=F64)
    G, C, N, _ = x.shape
    nv = nv_list(G, N, nvalid)
    mean, M2, m, mabs = (np.zeros((G, C)) for _ in range(4))
    for g, n in enumerate(nv):
        if n == 0:
            continue
        v = x[g, :, :n, :n].reshape(C, -1)
        mean[g] = v.mean(-1)
        M2[g] = ((v - mean[g][:, None]) ** 2).sum(-1)
        m[g] = n * n
        mabs[g] = np.abs(v).mean(-1)
    rec = record_of(mean, M2, m, nv, w, eps)
    rec['mabs'] = mabs
    return rec


def s12_of_tiles(s12part, tr, G, C, tpg):
    """S1, S2 (G, C) as fp64 sums of the per-tile partials, and the sums of their magnitudes"""
    p1, p2 = unpack_part(s12part, tr, G, C, tpg)
    return p1.sum(-1), p2.sum(-1), np.abs(p1).sum(-1), np.abs(p2).sum(-1)


def coef_ref(S1, S2, rec, nvalid, N):
    """{mean, a, -a S2 r2 / m, -a S1 / m} (G, C, 4); zeros in the last two for an empty graph"""
    G, C = S1.shape
    nv = np.asarray(nv_list(G, N, nvalid), dtype=F64).reshape(G, 1) * np.ones((1, C))
    m = nv * nv
    ms = np.maximum(m, 1)
    z = np.where(m > 0, -rec['a'] * S2 * rec['r2'] / ms, 0.0)
    w = np.where(m > 0, -rec['a'] * S1 / ms, 0.0)
    return np.stack([rec['mean'], rec['a'], z, w], axis=-1)


def affine_ref(q, S1, S2):
    """dgw[c] = sum_g q S2, dgb[c] = sum_g S1, and the sums of magnitudes"""
    q, S1, S2 = (np.asarray(v, dtype=F64) for v in (q, S1, S2))
    return (q * S2).sum(0), S1.sum(0), np.abs(q * S2).sum(0), np.abs(S1).sum(0)


def reduce_ref(inp, scale=1.0):
    """out[i] = scale sum_r in[r][i], and |scale| sum_r |in[r][i]|"""
    a = np.asarray(inp, dtype=F64)
    return scale * a.sum(0), abs(scale) * np.abs(a).sum(0)


def norm_fwd_ref(x, nvalid, w, beta, eps=EPS):
    """y = w (x - mean) / (2 sqrt(n (var + eps))) + b on the valid corner, 0 in the padding; and the record"""
    x = np.asarray(x, dtype=F64)
    G, C, N, _ = x.shape
    rec = direct_ref(x, nvalid, w, eps)
    be = np.zeros(C) if beta is None else np.asarray(beta, dtype=F64)
    y = np.zeros_like(x)
    for g, n in enumerate(nv_list(G, N, nvalid)):
        y[g, :, :n, :n] = (x[g, :, :n, :n] - rec['mean'][g][:, None, None]) * rec['a'][g][:, None, None] + be[:, None, None]
    return y, rec


def norm_bwd_ref(dy, z, rec, nvalid):
    """S1 = sum dy, S2 = sum dy (z - mean) over the valid corner; dz = a dy + cb (z - mean) + cc; sums of magnitudes"""
    dy, z = np.asarray(dy, dtype=F64), np.asarray(z, dtype=F64)
    G, C, N, _ = z.shape
    S1, S2, A1, A2 = (np.zeros((G, C)) for _ in range(4))
    nv = nv_list(G, N, nvalid)
    for g, n in enumerate(nv):
        d = dy[g, :, :n, :n].reshape(C, -1)
        t = d * (z[g, :, :n, :n].reshape(C, -1) - rec['mean'][g][:, None])
        S1[g], S2[g], A1[g], A2[g] = d.sum(-1), t.sum(-1), np.abs(d).sum(-1), np.abs(t).sum(-1)
    coef = coef_ref(S1, S2, rec, nvalid, N)
    dz = np.zeros_like(z)
    for g, n in enumerate(nv):
        k = coef[g][:, None, None, :]
        dz[g, :, :n, :n] = k[..., 1] * dy[g, :, :n, :n] + k[..., 2] * (z[g, :, :n, :n] - k[..., 0]) + k[..., 3]
    return dict(S1=S1, S2=S2, A1=A1, A2=A2, coef=coef, dz=dz)


# ---------------------------------------------------------------------------------------------- bounds (module docstring)
def finalize_K(tpg):
    return (tpg + 63) // 64 + 9


def stats_adds(N, n):
    """serial adds per lane of gn_stats_kernel / gn_bwd_stats_kernel for a graph of n valid vertices"""
    return (N * N + 63) // 64 if n == N else n * ((n + 63) // 64)


PLANE_ADDS = 16


def record_bounds(rec, K):
    """absolute bounds of the four record fields, (G, C) each; K per graph (G) or a scalar"""
    K = np.asarray(K, dtype=F64).reshape(-1, 1)
    em = K * U * rec['mabs']
    dM2 = (K + 4) * U * rec['M2'] + rec['m'] * em ** 2
    rel_r2 = dM2 / (np.maximum(rec['m'], 1) * rec['ve']) + 3 * U
    rel_q = rel_r2 / 2 + 4 * U
    rel_a = rel_q + U
    return dict(mean=em, r2=rel_r2 * rec['r2'], q=rel_q * np.abs(rec['q']), a=rel_a * np.abs(rec['a']), rel_a=rel_a, rel_r2=rel_r2)


def wave_sum_bound(adds, abs_sum):
    return (np.asarray(adds, dtype=F64) + 8) * U * abs_sum


def coef_bounds(coef, rec, dS1, dS2, nvalid, N):
    """bounds of the z and w fields of a coefficient record whose mean, a, r2 inputs are exact (the kernel reads them) and
    whose S1 / S2 carry the errors dS1 / dS2: two products and a division (3 u), one and one (2 u); 4 u covers both"""
    G, C = dS1.shape
    nv = np.asarray(nv_list(G, N, nvalid), dtype=F64).reshape(G, 1)
    ms = np.maximum(nv * nv, 1)
    live = nv > 0
    z = np.where(live, np.abs(rec['a']) * rec['r2'] / ms * dS2 + 4 * U * np.abs(coef[..., 2]), 0.0)
    w = np.where(live, np.abs(rec['a']) / ms * dS1 + 4 * U * np.abs(coef[..., 3]), 0.0)
    return z, w


def reduce_bound(rows, abs_sum):
    return ((rows + 3) // 4 + 5) * U * abs_sum


def affine_bound(G, abs_sum):
    return ((G + 7) // 8 + 10) * U * abs_sum


def _per_plane(v):
    return np.asarray(v, dtype=F64)[:, :, None, None]


def y_bound(x, y, rec, rb):
    """|dy| <= |a| eps_mean + |v - mean| |a| (rel_a + 3 u) + u |y|, elementwise"""
    x = np.asarray(x, dtype=F64)
    return (_per_plane(np.abs(rec['a']) * rb['mean']) + np.abs(x - _per_plane(rec['mean'])) * _per_plane(np.abs(rec['a']) * (rb['rel_a'] + 3 * U))
            + U * np.abs(y))


def dz_bound(dy, z, rec, rb, bw, adds):
    """dz = a dy + cb (z - mean) + cc computed from the kernels' own record, S1 and S2.  With e = eps_mean, v = z - mean:
      S1: dS1 <= (A + 8) u sum|dy|
      S2 is summed with mean + e: sum dy (v - e) = S2 - e S1, so dS2 <= (A + 8) u sum|dy| (|v| + e) + e |S1|
      cb = -a S2 r2 / m: |d cb| <= |cb| (rel_a + rel_r2 + 4 u) + |a| r2 / m dS2       cc = -a S1 / m: |d cc| <= |cc| (rel_a + 4 u) + |a| / m dS1
      |d dz| <= |a dy| (rel_a + u) + |d cb| |v| + |cb| e + |d cc| + 3 u (|a dy| + |cb v| + |cc|)      (difference, product, two sums)"""
    dy, z = np.asarray(dy, dtype=F64), np.asarray(z, dtype=F64)
    adds = np.asarray(adds, dtype=F64).reshape(-1, 1)
    e = rb['mean']
    ms = np.maximum(rec['m'], 1)
    dS1 = (adds + 8) * U * bw['A1']
    dS2 = (adds + 8) * U * (bw['A2'] + e * bw['A1']) + e * np.abs(bw['S1'])
    cb, cc = np.abs(bw['coef'][..., 2]), np.abs(bw['coef'][..., 3])
    a, r2 = np.abs(rec['a']), rec['r2']
    dcb = cb * (rb['rel_a'] + rb['rel_r2'] + 4 * U) + a * r2 / ms * dS2
    dcc = cc * (rb['rel_a'] + 4 * U) + a / ms * dS1
    v = np.abs(z - _per_plane(rec['mean']))
    t1, t2 = _per_plane(a) * np.abs(dy), _per_plane(cb) * v
    return (t1 * _per_plane(rb['rel_a'] + U) + _per_plane(dcb) * v + _per_plane(cb * e) + _per_plane(dcc)
            + 3 * U * (t1 + t2 + _per_plane(cc)))


SAFETY = 2.0       # every test applies its bound per element with this factor


def within(got, ref, bound, what):
    """asserts |got - ref| <= SAFETY * bound in every element; returns the largest error / bound ratio"""
    err = np.abs(np.asarray(got, dtype=F64) - ref)
    bound = np.broadcast_to(bound, err.shape)
    bad = ~(err <= SAFETY * bound)
    assert not bad.any(), '%s: %d cells outside the bound, worst error %g at bound %g' % (
        what, bad.sum(), err[bad].max(), bound[bad][err[bad].argmax()])
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


# ---------------------------------------------------------------------------------------------- float32 emulation
def _mirror(width):
    i = np.arange(64)
    return (i & ~(width - 1)) | (width - 1 - (i & (width - 1)))


_BUTTERFLY = [np.arange(64) ^ 1, np.arange(64) ^ 2, _mirror(8), _mirror(16), np.arange(64) ^ 16, np.arange(64) ^ 32]


def emu_wave_sum(v):
    """wave_sum of fgnn_common.h: quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror, xor 16, xor 32; (..., 64) -> (...)"""
    v = np.asarray(v, dtype=F32)
    for perm in _BUTTERFLY:
        v = (v + v[..., perm]).astype(F32)
    return v[..., 0]


def emu_lane_sum(terms):
    """lane l adds terms l, l + 64, l + 128, ... in order, then the butterfly; (..., k) float32 -> (...)"""
    terms = np.asarray(terms, dtype=F32)
    k = terms.shape[-1]
    L = max(1, (k + 63) // 64)
    t = np.zeros(terms.shape[:-1] + (L * 64,), dtype=F32)
    t[..., :k] = terms
    t = t.reshape(terms.shape[:-1] + (L, 64))
    acc = np.zeros(terms.shape[:-1] + (64,), dtype=F32)
    for j in range(L):
        acc = (acc + t[..., j, :]).astype(F32)
    return emu_wave_sum(acc)


def emu_record(mean, m2, m, nv, w, eps=EPS32):
    """nrm_record of fgnn_norm.h in float32; (...,) arrays -> (..., 4)"""
    mean, m2, m, nv, w = (np.asarray(v, dtype=F32) for v in (mean, m2, m, nv, w))
    one, two = F32(1), F32(2)
    with np.errstate(divide='ignore', invalid='ignore'):
        var = np.where(m > 0, m2 / np.where(m > 0, m, one), F32(0)).astype(F32)
        ve = (var + eps).astype(F32)
        q = np.where(nv > 0, one / (two * np.sqrt((nv * ve).astype(F32))).astype(F32), F32(0)).astype(F32)
    return np.stack([mean * np.ones_like(q), (w * q).astype(F32), q, (one / ve).astype(F32)], axis=-1).astype(F32)


def emu_finalize(part, cnt, nvalid, N, tr, C, w=None):
    """gn_finalize_kernel: both of its paths add tile t = lane + 64 j in increasing j"""
    cnt = np.asarray(cnt, dtype=F32)
    G, tpg = cnt.shape
    p = np.asarray(part, dtype=F32).reshape((G, C, tpg, 2) if tr else (G, tpg, C, 2))
    if not tr:
        p = p.transpose(0, 2, 1, 3)
    mean_t, m2_t, n_t = p[..., 0], p[..., 1], cnt[:, None, :] * np.ones((1, C, 1), dtype=F32)
    sn = emu_lane_sum(n_t)
    sm = emu_lane_sum((n_t * mean_t).astype(F32))
    with np.errstate(divide='ignore', invalid='ignore'):
        mean = np.where(sn > 0, sm / np.where(sn > 0, sn, F32(1)), F32(0)).astype(F32)
    d = (mean_t - mean[..., None]).astype(F32)
    m2 = emu_lane_sum((m2_t + ((n_t * d).astype(F32) * d).astype(F32)).astype(F32))
    nv = np.asarray(nv_list(G, N, nvalid), dtype=F32).reshape(G, 1) * np.ones((1, C), dtype=F32)
    wv = np.ones(C, dtype=F32) if w is None else np.asarray(w, dtype=F32)
    return emu_record(mean, m2, sn, nv, wv[None, :] * np.ones((G, 1), dtype=F32))


def emu_coef(s1, s2, nrm, nvalid, N):
    """the coefficient arithmetic of gn_bwd_coef_kernel / gn_bwd_coef_tiles_kernel; nrm (G, C, 4) float32"""
    s1, s2, nrm = (np.asarray(v, dtype=F32) for v in (s1, s2, nrm))
    G, C = s1.shape
    nv = np.asarray(nv_list(G, N, nvalid), dtype=F32).reshape(G, 1) * np.ones((1, C), dtype=F32)
    m = (nv * nv).astype(F32)
    ms = np.where(m > 0, m, F32(1))
    a, r2 = nrm[..., 1], nrm[..., 3]
    z = np.where(m > 0, (((-a * s2).astype(F32) * r2).astype(F32) / ms).astype(F32), F32(0))
    w = np.where(m > 0, ((-a * s1).astype(F32) / ms).astype(F32), F32(0))
    return np.stack([nrm[..., 0], a, z, w], axis=-1).astype(F32)


def emu_coef_tiles(s12part, nrm, nvalid, N, tr, G, C, tpg):
    p = np.asarray(s12part, dtype=F32).reshape((G, C, tpg, 2) if tr else (G, tpg, C, 2))
    if not tr:
        p = p.transpose(0, 2, 1, 3)
    s1, s2 = emu_lane_sum(p[..., 0]), emu_lane_sum(p[..., 1])
    return s1, s2, emu_coef(s1, s2, nrm, nvalid, N)


def emu_reduce_cols(inp, scale=1.0, scale_dev=None):
    """reduce_cols: row group rg adds rows rg, rg + 4, ... in order (its 32-way, 8-way and scalar loops keep that order),
    then (s0 + s1) + (s2 + s3), then the scale"""
    a = np.asarray(inp, dtype=F32)
    rows, cols = a.shape
    s = np.zeros((4, cols), dtype=F32)
    for r in range(rows):
        s[r & 3] = (s[r & 3] + a[r]).astype(F32)
    sc = F32(F32(scale if scale != 0 else 1.0) * F32(1.0 if scale_dev is None else scale_dev))
    return ((((s[0] + s[1]).astype(F32) + (s[2] + s[3]).astype(F32)).astype(F32)) * sc).astype(F32)


def emu_affine(q, S1, S2):
    """affine_reduce: group gg adds graphs gg, gg + 8, ... in order, then the eight groups in order"""
    q, S1, S2 = (np.asarray(v, dtype=F32) for v in (q, S1, S2))
    G, C = q.shape
    aw, ab = np.zeros((8, C), dtype=F32), np.zeros((8, C), dtype=F32)
    for g in range(G):
        aw[g & 7] = (aw[g & 7] + (q[g] * S2[g]).astype(F32)).astype(F32)
        ab[g & 7] = (ab[g & 7] + S1[g]).astype(F32)
    w, b = np.zeros(C, dtype=F32), np.zeros(C, dtype=F32)
    for k in range(8):
        w, b = (w + aw[k]).astype(F32), (b + ab[k]).astype(F32)
    return w, b


def _lane_terms(v, N, n):
    """the valid elements of a (C, N, N) plane stack in the order one wave of the two-pass kernels walks them, laid out so
    that emu_lane_sum reproduces it: the dense plane flat, the ragged one row by row with each row padded to whole waves"""
    C = v.shape[0]
    if n == N:
        return v.reshape(C, N * N)
    Lr = (n + 63) // 64
    t = np.zeros((C, n, Lr * 64), dtype=F32)
    t[:, :, :n] = v[:, :n, :n]
    return t.reshape(C, n * Lr * 64)


def emu_stats(x, nvalid, w=None):
    """gn_stats_kernel in float32 -> nrm (G, C, 4)"""
    x = np.asarray(x, dtype=F32)
    G, C, N, _ = x.shape
    out = np.zeros((G, C, 4), dtype=F32)
    wv = np.ones(C, dtype=F32) if w is None else np.asarray(w, dtype=F32)
    for g, n in enumerate(nv_list(G, N, nvalid)):
        m = F32(F32(n) * F32(n))
        if n == 0:
            out[g] = emu_record(np.zeros(C), np.zeros(C), np.zeros(C), np.zeros(C), wv)
            continue
        mean = (emu_lane_sum(_lane_terms(x[g], N, n)) / m).astype(F32)
        d = np.zeros_like(x[g])
        d[:, :n, :n] = (x[g, :, :n, :n] - mean[:, None, None]).astype(F32)
        s2 = emu_lane_sum(_lane_terms((d * d).astype(F32), N, n))
        out[g] = emu_record(mean, s2, np.full(C, m), np.full(C, F32(n)), wv)
    return out


def emu_apply(x, nrm, beta, nvalid):
    x, nrm = np.asarray(x, dtype=F32), np.asarray(nrm, dtype=F32)
    G, C, N, _ = x.shape
    be = np.zeros(C, dtype=F32) if beta is None else np.asarray(beta, dtype=F32)
    y = np.zeros_like(x)
    for g, n in enumerate(nv_list(G, N, nvalid)):
        v = (x[g, :, :n, :n] - nrm[g, :, 0][:, None, None]).astype(F32)
        y[g, :, :n, :n] = ((v * nrm[g, :, 1][:, None, None]).astype(F32) + be[:, None, None]).astype(F32)
    return y


def emu_bwd_stats(dy, z, nrm, nvalid):
    dy, z, nrm = (np.asarray(v, dtype=F32) for v in (dy, z, nrm))
    G, C, N, _ = z.shape
    s1, s2 = np.zeros((G, C), dtype=F32), np.zeros((G, C), dtype=F32)
    for g, n in enumerate(nv_list(G, N, nvalid)):
        if n == 0:
            continue
        d = np.zeros_like(dy[g])
        d[:, :n, :n] = dy[g, :, :n, :n]
        t = np.zeros_like(d)
        t[:, :n, :n] = (d[:, :n, :n] * (z[g, :, :n, :n] - nrm[g, :, 0][:, None, None]).astype(F32)).astype(F32)
        s1[g], s2[g] = emu_lane_sum(_lane_terms(d, N, n)), emu_lane_sum(_lane_terms(t, N, n))
    return s1, s2


def emu_bwd_apply(dy, z, coef, nvalid):
    dy, z, coef = (np.asarray(v, dtype=F32) for v in (dy, z, coef))
    G, C, N, _ = z.shape
    dz = np.zeros_like(z)
    for g, n in enumerate(nv_list(G, N, nvalid)):
        k = coef[g][:, None, None, :]
        v = (z[g, :, :n, :n] - k[..., 0]).astype(F32)
        dz[g, :, :n, :n] = (((k[..., 1] * dy[g, :, :n, :n]).astype(F32) + (k[..., 2] * v).astype(F32)).astype(F32) + k[..., 3]).astype(F32)
    return dz


def emu_plane_sum(v):
    """plane kernels: thread tid adds elements tid, tid + 256, ... (16 of them), wave butterfly, (w0 + w1) + (w2 + w3); (C, P) -> (C)"""
    v = np.asarray(v, dtype=F32)
    C, P = v.shape
    t = np.zeros((C, 16 * 256), dtype=F32)
    t[:, :P] = v
    t = t.reshape(C, 16, 256)
    acc = np.zeros((C, 256), dtype=F32)
    for k in range(16):
        acc = (acc + t[:, k]).astype(F32)
    ws = emu_wave_sum(acc.reshape(C, 4, 64))
    return ((ws[:, 0] + ws[:, 1]).astype(F32) + (ws[:, 2] + ws[:, 3]).astype(F32)).astype(F32)


def _masked(v, n):
    o = np.zeros_like(v)
    o[:, :n, :n] = v[:, :n, :n]
    return o


def emu_plane_fwd(x, nvalid, w=None):
    """the record of gn_plane_fwd_kernel (its y is emu_apply of that record)"""
    x = np.asarray(x, dtype=F32)
    G, C, N, _ = x.shape
    out = np.zeros((G, C, 4), dtype=F32)
    wv = np.ones(C, dtype=F32) if w is None else np.asarray(w, dtype=F32)
    for g, n in enumerate(nv_list(G, N, nvalid)):
        m = F32(F32(n) * F32(n))
        xm = _masked(x[g], n)
        mean = (emu_plane_sum(xm.reshape(C, -1)) / m).astype(F32) if n else np.zeros(C, dtype=F32)
        d = _masked((x[g] - mean[:, None, None]).astype(F32), n)
        out[g] = emu_record(mean, emu_plane_sum((d * d).astype(F32).reshape(C, -1)), np.full(C, m), np.full(C, F32(n)), wv)
    return out


def emu_plane_bwd_stats(dy, z, nrm, nvalid):
    dy, z, nrm = (np.asarray(v, dtype=F32) for v in (dy, z, nrm))
    G, C, N, _ = z.shape
    s1, s2 = np.zeros((G, C), dtype=F32), np.zeros((G, C), dtype=F32)
    for g, n in enumerate(nv_list(G, N, nvalid)):
        d = _masked(dy[g], n)
        u = _masked((z[g] - nrm[g, :, 0][:, None, None]).astype(F32), n)
        s1[g], s2[g] = emu_plane_sum(d.reshape(C, -1)), emu_plane_sum((d * u).astype(F32).reshape(C, -1))
    return s1, s2


# ---------------------------------------------------------------------------------------------- shared input sets
FIN_N = (1, 5, 8, 46, 90, 91, 128, 129, 200)                   # tpg = 1, 1, 2, 67, 254, 259, 512, 521, 1250
FIN_TPG = (1, 63, 64, 65, 256, 257, 512, 513, 1250)
FIN_GC = (1, 5, 15, 37)
# (G, C) of a G*C: dense batches put the product in the channels (where the two storage orders differ), ragged batches
# need the graphs for the vertex counts {N, N // 2, 1, 0}
GC_DENSE = {1: (1, 1), 5: (1, 5), 15: (3, 5), 37: (1, 37)}
GC_RAGGED = {1: (1, 1), 5: (5, 1), 15: (3, 5), 37: (37, 1)}
TPG_N = 6                                                      # the `_tpg` entry points take N only for nvalid_of


def ragged_counts(G, N):
    """vertex counts cycling through {N // 2, 0, 1, N}; a single graph gets the partly filled N // 2"""
    cyc = (N // 2, 0, 1, N)
    return [cyc[g % 4] for g in range(G)]


@functools.lru_cache(maxsize=None)
def plane_for_tpg(tpg):
    """(N, ldr) of a bf16-layout plane (tiles of 64 at row pitch ldr >= N) with exactly tpg tiles"""
    for n in range(max(1, int(math.sqrt(64 * tpg)) + 1), 0, -1):
        for ldr in range(n, n + 64):
            if (n * ldr + 63) // 64 == tpg:
                return n, ldr
    raise ValueError(tpg)


def _data(seed, G, C, N, shift=False):
    rng = np.random.default_rng(seed)
    if shift:
        return (1000.0 + 0.01 * rng.standard_normal((G, C, N, N))).astype(F32)
    ch = rng.uniform(0.5, 2.0, (1, C, 1, 1)), rng.uniform(-1.0, 1.0, (1, C, 1, 1))
    return (ch[0] * rng.standard_normal((G, C, N, N)) + ch[1]).astype(F32)


@functools.lru_cache(maxsize=None)
def finalize_case(size, gc, ragged, tr, shift=False):
    """One finalize input set, built once and shared: `size` is N for the fp32 layout (tr = 0), tpg for the `_tpg` forms.
    Two partial sets over the same counts (finalize2), the kernel-side N and vertex counts, channel weights."""
    G, C = (GC_RAGGED if ragged else GC_DENSE)[gc]
    if tr:
        Nd, pitch, T, N = plane_for_tpg(size) + (64, TPG_N)
    else:
        Nd, pitch, T, N = size, size, 32, size
    nvd = ragged_counts(G, Nd) if ragged else None
    # the kernel-side counts only feed q; a live graph stays live, an empty one empty
    nvk = None if not ragged else ([{Nd: N, 0: 0, 1: 1}.get(n, max(1, N // 2)) for n in nvd] if tr else nvd)
    seed = (size * 64 + gc) * 8 + ragged * 4 + tr * 2 + int(shift)
    x0 = _data(seed, G, C, Nd, shift)
    x1 = (F32(1.25) - F32(0.75) * x0).astype(F32)
    p0, p1 = tile_partials(x0, nvd, T, pitch), tile_partials(x1, nvd, T, pitch)
    w = np.random.default_rng(seed + 1).uniform(0.5, 1.5, C).astype(F32)
    for a in (p0.mean_t, p0.m2_t, p0.cnt, p1.mean_t, p1.m2_t, w, x0, x1):
        a.setflags(write=False)
    return dict(G=G, C=C, N=N, tpg=p0.tpg, tr=tr, nvalid=nvk, data_nvalid=nvd, x=(x0, x1), parts=(p0, p1), cnt=p0.cnt, w=w)


@functools.lru_cache(maxsize=None)
def s12_case(size, gc, ragged, tr):
    """per-tile {S1, S2} partials with random signs, and a record set, for the coefficient-tile kernels"""
    fc = finalize_case(size, gc, ragged, tr)
    G, C, tpg = fc['G'], fc['C'], fc['tpg']
    rng = np.random.default_rng(size * 1000 + gc * 10 + ragged * 2 + tr + 77)
    p = Partials(rng.standard_normal((G, C, tpg)).astype(F32), (3 * rng.standard_normal((G, C, tpg))).astype(F32), fc['cnt'])
    rec = finalize_ref(fc['parts'][0].part(tr), fc['cnt'], fc['nvalid'], fc['N'], tr, C, fc['w'])
    nrm = np.stack([rec['mean'], rec['a'], rec['q'], rec['r2']], axis=-1).astype(F32)
    for a in (p.mean_t, p.m2_t, nrm):
        a.setflags(write=False)
    return dict(fc=fc, s12=p, nrm=nrm)


def nrm_as_rec(nrm):
    """an fp32 record array (G, C, 4) as the fp64 dict the coefficient references take"""
    n = np.asarray(nrm, dtype=F64)
    return dict(mean=n[..., 0], a=n[..., 1], q=n[..., 2], r2=n[..., 3])


RED_ROWS = (1, 3, 4, 5, 31, 32, 33, 127, 128, 129, 256, 300)
RED_COUNTS = (1, 63, 64, 65, 200)
RED_NUM_WG = 6
RED_SCALES = (0.0, 1.0, 0.375, -2.5)
RED_SCALE_DEV = 0.3


@functools.lru_cache(maxsize=None)
def reduce_launches():
    """four launches of 16 jobs: every (rows, count) pair once, counts mixed inside a launch; the sixteenth job has rows = 0
    (= num_wg).  A job is (rows field, count, scale field, uses scale_dev, input (rows, count))."""
    pairs = [(r, c) for r in RED_ROWS for c in RED_COUNTS]
    rng = np.random.default_rng(2024)
    out = []
    for l in range(4):
        jobs = []
        for i, (r, c) in enumerate(pairs[l::4] + [(0, RED_COUNTS[l])]):
            a = rng.standard_normal((r or RED_NUM_WG, c)).astype(F32)
            a.setflags(write=False)
            jobs.append(dict(rows=r, count=c, scale=RED_SCALES[(i + l) % 4], dev=(i // 2 + l) % 2 == 1, inp=a))
        out.append(jobs)
    return out


AFF_C = (1, 32, 33, 70)
AFF_G = (1, 7, 8, 9, 20)


@functools.lru_cache(maxsize=None)
def affine_case(G, C):
    rng = np.random.default_rng(G * 100 + C)
    nrm = np.zeros((G, C, 4), dtype=F32)
    nrm[..., 0] = rng.standard_normal((G, C))
    nrm[..., 2] = rng.uniform(0.01, 2.0, (G, C))
    nrm[..., 1] = nrm[..., 2] * rng.uniform(0.5, 1.5, (1, C)).astype(F32)
    nrm[..., 3] = rng.uniform(0.1, 10.0, (G, C))
    s12 = rng.standard_normal((G, C, 2)).astype(F32)
    nrm.setflags(write=False)
    s12.setflags(write=False)
    return nrm, s12


# two-pass and plane kernels: (name, ragged, strided, affine parameters given)
SLAB_VARIANTS = (('dense', False, False, True), ('ragged_strided', True, True, True), ('dense_strided_null', False, True, False),
                 ('ragged_null', True, False, False))
TWO_PASS_N = (65, 91)
PLANE_N = (1, 33)
SLAB_GC = (3, 2)


@functools.lru_cache(maxsize=None)
def slab_case(N, ragged):
    G, C = SLAB_GC
    rng = np.random.default_rng(N * 2 + ragged)
    nv = [N, N // 2, 0] if ragged else None
    x = (2 * rng.standard_normal((G, C, N, N)) + 0.5).astype(F32)
    dy = rng.standard_normal((G, C, N, N)).astype(F32)
    w, b = rng.uniform(0.5, 1.5, C).astype(F32), rng.standard_normal(C).astype(F32)
    for a in (x, dy, w, b):
        a.setflags(write=False)
    return dict(G=G, C=C, N=N, nvalid=nv, x=x, dy=dy, w=w, b=b)
