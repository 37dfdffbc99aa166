"""CPU reference of the per-channel fp32 products (csrc/matmul.hip): numpy only, fp64.

The kernels compute, per (g, c) matrix and inside the graph's nv x nv corner,
    y  = (z - mean) * a + beta                     fp32, on load (norm_of / FGNN_W_RECORDS / big_stage)
    M  = Ya Yb,   dA = dM Yb^T,   dB = Ya^T dM     fp32 accumulation (v_mfma_f32_32x32x2_f32)
    S1 = sum dA,  S2 = sum dA (z_a - mean_a)       (s12a; s12b likewise with dB and z_b), over the corner
Operands outside the corner count as zero whatever the slab holds there.

Two data families.  `grid_case`: integer z and dM, records {integer mean, a in {1/2, 1, 2}, integer beta}, so that y is exact
in fp32 with or without FMA contraction and every partial sum of every product is an integer multiple of a fixed unit below
2^24 units -- exact in fp32 in ANY order; the expected output is the fp64 result, whose cast to fp32 is lossless.  The builder
asserts that precondition for the three products of every case, and computes the same load figure for the S sums (flag
`s_exact`; a case whose S sums are not exact is checked with the bound instead, the assert is not relaxed).
`random_case`: ordinary data, expected fp64 result plus the worst-case per-element bound of `finish`.

Layout of every case (`strides`, `slab`, `render`): row pitch N (mat[row * N + col], the fp32 slab contract); the two operand
slabs, dM and the outputs each have their own (gstride, ld).  The C ABI has ONE (ogstride, ldo) for dA and dB (two buffers,
one pair).  Operand slabs and dM hold finite garbage of magnitude 1e30, mixed signs, everywhere outside the corner; outputs
are prefilled with the sentinel SENT."""
import functools

import numpy as np

U32 = 2.0 ** -24                      # unit roundoff of fp32
GRID_LIMIT = 2 ** 24                  # integers below it are exact in fp32
SENT = 0x5A5A5A5A                     # sentinel bit pattern of the output buffers (a finite float, about 1.5e16)
G, CH = 3, 3
TM, BIG_MAX = 64, 256                 # matmul.hip: TM, big_path()

# ---- the shapes of tests/test_gpu_matmul32.py ---------------------------------------------------------------------------------
# N <= 64: 9, 24 and 55 are there for KQ = ceil(N / 8) = 2, 3 and 7 of launch_fwd_w (1, 4, 5, 6, 8 come with the edge sizes)
SMALL_N = (1, 2, 7, 9, 24, 31, 32, 33, 48, 55, 63, 64)
NT4_N = (65, 96, 127, 128)
NT8_N = (129, 200, 255, 256)


def _small_ragged(N):
    r = [(N, 1, N - 1), (N, 0, (N + 1) // 2)]
    if N > 32:
        r.append((33, 32, 31))
    return r


SMALL = [(N, None) for N in SMALL_N] + [(N, nv) for N in SMALL_N for nv in _small_ragged(N)]
BIG = ([(N, None) for N in NT4_N + NT8_N] + [(N, nv) for N in NT4_N for nv in ((N, 64, 1), (N, 65, 0))]
       + [(N, nv) for N in NT8_N for nv in ((N, 128, 97), (N, 129, 1))])
GENERIC = [(257, None), (257, (257,)), (257, (200,))]          # G = 1, C = 2
ODD = [(33, None), (64, (64, 33, 1)), (96, (96, 65, 0)), (200, (200, 129, 1)), (257, (200,))]    # strides odd in floats
FIN = [(33, (33, 17, 0)), (64, None), (64, (64, 33, 0)), (65, (65, 64, 1)), (128, None), (129, (129, 128, 0)), (200, (200, 129, 1)),
       (256, None)]
SHAPES = SMALL + BIG + GENERIC


def shape_id(s):
    return 'N%d' % s[0] if s[1] is None else 'N%d_nv%s' % (s[0], '_'.join(map(str, s[1])))


def dims(N):
    """(G, C) of a case: 3 x 3 = 9 matrices (an odd count: the last workgroup of the wave-per-matrix kernel has an idle wave),
    1 x 2 on the generic-tile path."""
    return (1, 2) if N > BIG_MAX else (G, CH)


def case_seed(N, nvalid, tag=32):
    return [tag, N] + list(nvalid or ())


def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def f32_ulp(x64):
    _, e = np.frexp(np.abs(np.asarray(x64, dtype=np.float64)))
    return np.ldexp(1.0, np.maximum(e - 24, -149).astype(np.int32))


def mask_corner(x, nv):
    """x (G, C, N, N) with everything outside the per-graph nv x nv corner replaced by +0."""
    x = np.array(x, dtype=np.float64)
    for g, n in enumerate(nv):
        x[g, :, n:, :] = 0.0
        x[g, :, :, n:] = 0.0
    return x


# ---- reference ------------------------------------------------------------------------------------------------------------------
def _T(x):
    return np.swapaxes(x, -1, -2)


def products(ya, yb, dm):
    return np.matmul(ya, yb), np.matmul(dm, _T(yb)), np.matmul(_T(ya), dm)


def finish(c):
    """Expected outputs and bounds of a case from its z / dm / records (all fp32-exact values held in fp64).

    Bound (u = 2^-24, K = nv of the graph), worst case, no margin:  yhat = |(z - mean) a| + |beta| bounds |y| and the size of
    every intermediate of its evaluation; y evaluated in fp32 (subtraction, product, sum -- or subtraction and one FMA) is off by
    at most 3 u yhat.  A K-term fp32 dot product accumulated in any order adds at most (K + 1) u sum |ya||yb| (one rounding per
    product, at most K additions on the path of a term).  Two perturbed operands: 3 + 3 + (K + 1) = K + 7, one more for the
    second-order terms:
        bound_M[i][j]  = u (K + 8) sum_k yhat_a[i][k] yhat_b[k][j]  +  ulp(M[i][j])
        bound_dA[i][k] = u (K + 8) sum_j |dM[i][j]| yhat_b[k][j]    +  ulp(dA[i][k])         (dB alike)
    S1 = sum dA: the errors of its terms, plus an nv^2-term accumulation in any order;  S2 = sum dA (z - mean) alike, each
    term's error scaled by |z - mean| (the subtraction's own rounding is among the + 8):
        bound_S1 = sum bound_dA + u (nv^2 + 8) sum |dA|,   bound_S2 = sum bound_dA |z - mean| + u (nv^2 + 8) sum |dA (z - mean)|"""
    nv = c['nv']
    Gc, Cc = c['G'], c['C']
    K = np.asarray(nv, np.float64).reshape(Gc, 1, 1, 1)
    dm = c['dm'] = mask_corner(c['dm_raw'], nv)
    hat, u = {}, {}
    for s in 'ab':
        mean, a = c['mean_' + s][:, :, None, None], c['a_' + s][:, :, None, None]
        beta = c['beta_' + s][None, :, None, None]
        d = c['z' + s] - mean
        c['y' + s] = mask_corner(d * a + beta, nv)
        hat[s] = mask_corner(np.abs(d * a) + np.abs(beta), nv)
        u[s] = mask_corner(d, nv)
    c['M'], c['dA'], c['dB'] = products(c['ya'], c['yb'], dm)
    absM, absA, absB = products(hat['a'], hat['b'], np.abs(dm))
    c['bound'] = dict(M=U32 * (K + 8) * absM + f32_ulp(c['M']), dA=U32 * (K + 8) * absA + f32_ulp(c['dA']),
                      dB=U32 * (K + 8) * absB + f32_ulp(c['dB']))
    c['absdot'] = dict(M=absM, dA=absA, dB=absB)
    K2 = K.reshape(Gc, 1) ** 2
    for s, d in (('a', c['dA']), ('b', c['dB'])):
        t2 = d * u[s]
        c['s12' + s] = np.stack([d.sum((-1, -2)), t2.sum((-1, -2))], -1)
        bd = c['bound']['d' + s.upper()]
        bd = mask_corner(bd, nv)
        c['bound']['s12' + s] = np.stack([bd.sum((-1, -2)) + U32 * (K2 + 8) * np.abs(d).sum((-1, -2)),
                                          (bd * np.abs(u[s])).sum((-1, -2)) + U32 * (K2 + 8) * np.abs(t2).sum((-1, -2))], -1)
        c['sload_' + s] = (np.abs(d).sum((-1, -2)), np.abs(t2).sum((-1, -2)))
    for s in 'ab':          # the record buffers {mean, a, q, r2}: the products read the first two only
        c['nrm_' + s] = np.stack([c['mean_' + s], c['a_' + s], np.full_like(c['a_' + s], 0.25), np.full_like(c['a_' + s], 4.0)], -1)
    return c


def _blank(N, nvalid):
    Gc, Cc = dims(N)
    nv = np.asarray(nvalid if nvalid is not None else [N] * Gc, dtype=np.int64)
    assert len(nv) == Gc and (nv >= 0).all() and (nv <= N).all()
    return dict(G=Gc, C=Cc, N=N, nv=nv, ragged=nvalid is not None)


def grid_ranges(N):
    """(|z| <=, |dM| <=, density of dM): chosen per N so that the S-sum loads stay below 2^24 up to N = 257 -- sum |dA| grows like
    nv^2 sqrt(density nv)."""
    return (3, 2, 1.0) if N <= TM else (2, 1, 16.0 / N)


def grid_case(rng, N, nvalid=None):
    c = _blank(N, nvalid)
    Gc, Cc = c['G'], c['C']
    zr, dr, dens = grid_ranges(N)
    ints = lambda lim, shape: rng.integers(-lim, lim + 1, size=shape).astype(np.float64)
    c['za'], c['zb'] = ints(zr, (Gc, Cc, N, N)), ints(zr, (Gc, Cc, N, N))
    c['dm_raw'] = ints(dr, (Gc, Cc, N, N)) * (rng.random((Gc, Cc, N, N)) < dens)
    for s in 'ab':
        c['mean_' + s] = ints(1, (Gc, Cc))
        c['a_' + s] = rng.choice(np.array([0.5, 1.0, 2.0]), size=(Gc, Cc))
        c['beta_' + s] = ints(1, (Cc,))
    finish(c)
    # y is a multiple of 1/2: forward terms are multiples of 1/4, backward terms (integer dM) and S terms (integer z - mean) of 1/2
    for s in 'ab':
        assert not np.mod(c['y' + s] * 2, 1).any()
    c['load'] = dict(M=float(np.matmul(np.abs(c['ya']), np.abs(c['yb'])).max(initial=0.0) * 4), dA=float(np.matmul(np.abs(c['dm']), np.abs(_T(c['yb']))).max(initial=0.0) * 2),
                     dB=float(np.matmul(np.abs(_T(c['ya'])), np.abs(c['dm'])).max(initial=0.0) * 2))
    assert max(c['load'].values()) < GRID_LIMIT, c['load']
    c['load']['S'] = float(max(np.max(x, initial=0.0) for s in 'ab' for x in c['sload_' + s]) * 2)
    c['exact'] = True
    c['s_exact'] = c['load']['S'] < GRID_LIMIT
    return c


def random_case(rng, N, nvalid=None):
    c = _blank(N, nvalid)
    Gc, Cc = c['G'], c['C']
    c['za'], c['zb'] = f32(rng.standard_normal((Gc, Cc, N, N))), f32(rng.standard_normal((Gc, Cc, N, N)))
    c['dm_raw'] = f32(rng.standard_normal((Gc, Cc, N, N)))
    for s in 'ab':
        c['mean_' + s] = f32(rng.standard_normal((Gc, Cc)))
        c['a_' + s] = f32(rng.uniform(0.5, 1.5, (Gc, Cc)))
        c['beta_' + s] = f32(rng.standard_normal(Cc))
    finish(c)
    c['exact'] = c['s_exact'] = False
    return c


@functools.lru_cache(maxsize=6)          # (a 256-vertex case holds about 100 MB of fp64 arrays)
def case(family, N, nvalid):
    rng = np.random.default_rng(case_seed(N, nvalid, tag=32 if family == 'grid' else 33))
    return (grid_case if family == 'grid' else random_case)(rng, N, nvalid)


def with_records(c, nrm_a, nrm_b):
    """The case with the records replaced by {mean, a} of (G, C, 4) fp32 record buffers (the folded-finalize tests)."""
    d = {k: c[k] for k in ('G', 'C', 'N', 'nv', 'ragged', 'za', 'zb', 'dm_raw', 'beta_a', 'beta_b')}
    for s, n in (('a', nrm_a), ('b', nrm_b)):
        n = np.asarray(n, np.float64).reshape(c['G'], c['C'], 4)
        d['mean_' + s], d['a_' + s] = n[:, :, 0].copy(), n[:, :, 1].copy()
    finish(d)
    d['exact'] = d['s_exact'] = False
    return d


# ---- buffers --------------------------------------------------------------------------------------------------------------------
def strides(N, C, odd=False):
    """(gstride, ld) of the two operand slabs, dM and the outputs, in floats: all different, multiples of 4 (16-byte accesses stay
    aligned), all but b's ld above the minimum.  odd: every one of them odd (matrices start on 4-byte boundaries only)."""
    P = (N * N + 3) // 4 * 4
    if odd:
        P = N * N | 1                    # odd and >= N * N
        return dict(a=((C * (P + 2) + 2) | 1, P + 2), b=((C * P) | 1, P), dm=((C * (P + 6) + 4) | 1, P + 6),
                    out=((C * (P + 4) + 6) | 1, P + 4))
    return dict(a=(C * (P + 8) + 16, P + 8), b=(C * P + 8, P), dm=(C * (P + 24), P + 24), out=(C * (P + 16) + 24, P + 16))


def garbage(rng, n):
    """finite fp32 values of magnitude 1e30 .. 2e30, mixed signs"""
    return ((1.0 + rng.random(n)) * 1e30 * rng.choice(np.array([-1.0, 1.0]), n)).astype(np.float32)


def slab(values, nv, gs, ld, rng):
    """(G * gs) fp32: garbage everywhere except the nv x nv corners, which hold `values` (G, C, N, N)."""
    Gc, Cc, N, _ = values.shape
    buf = garbage(rng, Gc * gs)
    for g in range(Gc):
        n = int(nv[g])
        for c in range(Cc):
            img = buf[g * gs + c * ld:g * gs + c * ld + N * N].reshape(N, N)
            img[:n, :n] = values[g, c, :n, :n]
    return buf


def sentinel(n):
    return np.full(n, SENT, np.uint32).view(np.float32)


def big(N):
    return TM < N <= BIG_MAX


def zero_mask(N, nv, fill):
    """The N x N boolean image of what a product entry point must leave as exact +0 outside the nv x nv corner (the rest of the
    frame must still hold what was there).  fill = 0, and every N outside 64 < N <= 256: the whole frame.  fill = 1
    (include/fgnn_hip.h, fgnn_chan_matmul_fwd_ord; csrc/matmul.hip, big_zero_fill): with X = 32 ceil(nv / 32), the X x X block of
    32 x 32 tiles that hold the corner is written whole (products of zero padding), the tails [X, N) of the valid rows are zeroed,
    and when nv = X the first 32 pixels of row nv."""
    z = np.ones((N, N), bool)
    if fill and big(N):
        X = (nv + 31) // 32 * 32
        z[:] = False
        z[:X, :X] = True
        z[:nv, X:] = True
        if nv == X and nv < N:
            z[nv, :min(32, N)] = True
    z[:nv, :nv] = False
    return z


def consumer_reach(N, nv):
    """The padding pixels a consumer that steps over padding-only tiles can read (include/fgnn_hip.h, fgnn_ragged_tile_ranges): a
    tile is 32 consecutive pixels of the N x N plane; every pixel of a tile that holds a valid pixel, less the valid ones."""
    valid = np.zeros((N, N), bool)
    valid[:nv, :nv] = True
    flat = valid.reshape(-1)
    tiles = np.zeros((N * N + 31) // 32, bool)
    tiles[np.flatnonzero(flat) // 32] = True
    reach = np.repeat(tiles, 32)[:N * N] & ~flat
    return reach.reshape(N, N)


def render(values, nv, gs, ld, fill=0):
    """What a correct kernel leaves in a sentinel-filled output buffer for the corner values `values` (G, C, N, N)."""
    Gc, Cc, N, _ = values.shape
    buf = sentinel(Gc * gs).copy()
    for g in range(Gc):
        n = int(nv[g])
        zm = zero_mask(N, n, fill)
        for c in range(Cc):
            img = buf[g * gs + c * ld:g * gs + c * ld + N * N].reshape(N, N)
            img[zm] = 0.0
            img[:n, :n] = values[g, c, :n, :n]
    return buf


# ---- checkers -------------------------------------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    pass


def _first(mask):
    return tuple(int(i) for i in np.argwhere(mask)[0])


def _check_buffer(name, buf, c, gs, ld, fill, exact):
    Gc, Cc, N, nv = c['G'], c['C'], c['N'], c['nv']
    buf = np.asarray(buf)
    assert buf.dtype == np.float32 and buf.shape == (Gc * gs,), (name, buf.dtype, buf.shape)
    bits = buf.view(np.uint32)
    covered = np.zeros(Gc * gs, bool)
    ref, bound = c[name], c['bound'][name]
    for g in range(Gc):
        n = int(nv[g])
        zm = zero_mask(N, n, fill)
        keep = ~zm
        keep[:n, :n] = False
        for ch in range(Cc):
            lo = g * gs + ch * ld
            covered[lo:lo + N * N] = True
            img, ibits = buf[lo:lo + N * N].reshape(N, N), bits[lo:lo + N * N].reshape(N, N)
            got = img[:n, :n].astype(np.float64)
            err = np.abs(got - ref[g, ch, :n, :n])
            bad = (err != 0) if exact else ~(err <= bound[g, ch, :n, :n])
            if bad.any():
                i, j = _first(bad)
                raise Mismatch('%s[g=%d, c=%d, i=%d, j=%d] = %r, expected %r%s' % (
                    name, g, ch, i, j, got[i, j], ref[g, ch, i, j], '' if exact else ' +- %.3g (error / bound = %.3g)' % (
                        bound[g, ch, i, j], err[i, j] / bound[g, ch, i, j])))
            bad = zm & (ibits != 0)
            if bad.any():
                i, j = _first(bad)
                raise Mismatch('%s[g=%d, c=%d, i=%d, j=%d]: padding holds %r (bits %08x), not +0' % (name, g, ch, i, j, img[i, j], ibits[i, j]))
            bad = keep & (ibits != SENT)
            if bad.any():
                i, j = _first(bad)
                raise Mismatch('%s[g=%d, c=%d, i=%d, j=%d]: the frame outside the fill = 1 region was written (%r)' % (name, g, ch, i, j, img[i, j]))
    bad = ~covered & (bits != SENT)
    if bad.any():
        e = int(np.flatnonzero(bad)[0])
        g, r = divmod(e, gs)
        raise Mismatch('%s: word %d (g=%d, c=%d, offset %d of the channel) outside every image was written' % (name, e, g, min(r // ld, Cc), r - min(r // ld, Cc) * ld))
    return float((np.abs(_images(buf, c, gs, ld) - ref) / bound)[_corner(c)].max(initial=0.0))


def _images(buf, c, gs, ld):
    Gc, Cc, N = c['G'], c['C'], c['N']
    out = np.empty((Gc, Cc, N, N))
    for g in range(Gc):
        for ch in range(Cc):
            out[g, ch] = buf[g * gs + ch * ld:g * gs + ch * ld + N * N].reshape(N, N)
    return out


def _corner(c):
    m = np.zeros((c['G'], c['C'], c['N'], c['N']), bool)
    for g, n in enumerate(c['nv']):
        m[g, :, :n, :n] = True
    return m


def _check_s12(name, got, c, exact):
    got = np.asarray(got, np.float64).reshape(c['G'], c['C'], 2)
    ref, bound = c[name], c['bound'][name]
    err = np.abs(got - ref)
    bad = (err != 0) if exact else ~(err <= bound)
    if bad.any():
        g, ch, k = _first(bad)
        raise Mismatch('%s[g=%d, c=%d].S%d = %r, expected %r%s' % (name, g, ch, k + 1, got[g, ch, k], ref[g, ch, k],
                                                                  '' if exact else ' +- %.3g' % bound[g, ch, k]))
    return float((err / np.where(bound > 0, bound, 1.0)).max(initial=0.0))


def _check(dev, c, exact):
    """dev: {'st': (gstride, ld) of the outputs, 'fill': 0 / 1, and any of 'M', 'dA', 'dB' (flat fp32 buffers of G * gstride floats)
    and 's12a', 's12b' (G * C * 2)}.  Returns {name: largest error / bound}; raises Mismatch naming the first offending element."""
    gs, ld = dev['st']
    ratios = {}
    for name in ('M', 'dA', 'dB'):
        if dev.get(name) is not None:
            ratios[name] = _check_buffer(name, dev[name], c, gs, ld, dev.get('fill', 0), exact)
    for name in ('s12a', 's12b'):
        if dev.get(name) is not None:
            ratios[name] = _check_s12(name, dev[name], c, exact and c['s_exact'])
    return ratios


def check_exact(dev, c):
    """Grid cases: every corner element equals the exact product, S1 / S2 the exact sums (the bound where the case is marked
    `s_exact` False); the frame and the sentinels as in zero_mask."""
    assert c['exact']
    return _check(dev, c, True)


def check_bounded(dev, c):
    """Every corner element within its derived bound of the fp64 product, S1 / S2 within theirs; the frame and the sentinels
    as in zero_mask (exact, like check_exact)."""
    return _check(dev, c, False)


# ---- fp32 emulation (tests/test_matmul32_ref_host.py) -------------------------------------------------------------------------
def emulate(c, interleave):
    """The three products in numpy fp32 with operands normalised in fp32: k in sequence, or (interleave) as the kernels' MFMA steps
    take it -- step s adds the pair k = 2 s + h, h = 0, 1, to the accumulator in one go."""
    F = np.float32
    nv = c['nv']
    y = {}
    for s in 'ab':
        mean, a = c['mean_' + s].astype(F)[:, :, None, None], c['a_' + s].astype(F)[:, :, None, None]
        beta = c['beta_' + s].astype(F)[None, :, None, None]
        y[s] = mask_corner((c['z' + s].astype(F) - mean) * a + beta, nv).astype(F)
    dm = c['dm'].astype(F)

    def dot(A, B):          # A (.., n, K), B (.., K, m)
        K = A.shape[-1]
        acc = np.zeros(A.shape[:-1] + (B.shape[-1],), F)
        if not interleave:
            for k in range(K):
                acc = acc + A[..., :, k, None] * B[..., k, None, :]
            return acc
        for k in range(0, K, 2):
            p = A[..., :, k, None] * B[..., k, None, :]
            if k + 1 < K:
                p = p + A[..., :, k + 1, None] * B[..., k + 1, None, :]
            acc = acc + p
        return acc
    return dict(M=dot(y['a'], y['b']), dA=dot(dm, _T(y['b'])), dB=dot(_T(y['a']), dm))
