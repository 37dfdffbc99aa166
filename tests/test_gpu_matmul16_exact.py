"""GPU: the per-channel bf16 products of csrc/matmul16.hip, through the C ABI, against tests/matmul16_ref.py -- bit for bit on
grid operands, element by element on ordinary data, in all four compiled forms (NT=2, NT=4, strip <8,7>, strip <8,8>), both
staging routes and both `nv % 8` branches, the three statistics modes, the coefficient records and the folded finalize.

Bit-exactness: on the dyadic grid of matmul16_ref.grid_case every fp32 partial sum is exact in any order (the precondition
sum_k |OpA||OpB| / unit < 2^24 is asserted by the reference for every case, tests/test_matmul16_ref_host.py), so the only
rounding is the final RNE to bf16 and the stored bits must equal rne_bf16(exact product): no tolerance, no allowance.

Set-up of every case: G = 3, C = 3; ldr = ceil8(N); the two operand slabs, dM and the outputs each have their own graph
and channel strides (multiples of 8 elements, all but one above the minimum).  The operand slabs hold finite garbage (bf16
values of magnitude about 1e30, mixed signs) everywhere outside the nv x nv corner: rows >= nv, columns >= nv, the pitch
columns N..ldr, the tail of every channel up to its stride and the gap between graphs.  Garbage is FINITE only: the slab
contract (include/fgnn_hip.h, "Columns j >= N, like all padding of a ragged graph, are stored as exact zeros") does not promise
that non-finite padding is ignored, and the staging multiplies a straddling piece's padding by 0.  dM is a raw slab that the
kernels do not mask: by the same contract its N x ldr image is exact zeros outside the corner; only its tails hold garbage.
Outputs are prefilled with a sentinel bit pattern."""
import ctypes as ct
import functools
import os
import re

import numpy as np
import pytest
import torch

import matmul16_ref as R
from graph_neural_net_amd import _lib
from graph_neural_net_amd.engine import EPS
from matmul16_ref import CH, DENSE, G, RAGGED, SHAPES, case_seed, shape_id

gpu = pytest.mark.gpu
DEV = 'cuda:0'
SENT = 0x5A5A                       # sentinel bit pattern of the output buffers
U = R.U32
RANDOM_SHAPES = [(n, None) for n in (33, 64, 65, 129, 225, 256)] + list(RAGGED)
FIN_SHAPES = [(n, None) for n in (50, 128, 200, 256)] + [(200, (200, 129, 0))]


# ---- slabs ------------------------------------------------------------------------------------------------------------------
def strides(N, ldr):
    """(gstride, ld) of the two operand slabs, dM and the outputs: all different, multiples of 8, one at the minimum."""
    img = N * ldr
    return dict(a=(CH * (img + 8) + 16, img + 8), b=(CH * img + 8, img), dm=(CH * (img + 24), img + 24),
                out=(CH * (img + 16) + 24, img + 16))


def garbage(rng, n):
    """finite bf16 bit patterns of magnitude about 1e30, mixed signs"""
    base = int(R.rne_bf16(np.array([1e30]))[0]) & 0xff80
    return (base | rng.integers(0, 128, n) | (rng.integers(0, 2, n) << 15)).astype(np.uint16)


def host_slab(bits, nv, gs, ld, N, ldr, rng, zero_image=False):
    """(G * gs) uint16: garbage everywhere except the nv x nv corners (zero_image: except the whole N x ldr images, which are
    exact zeros outside the corner)."""
    buf = garbage(rng, G * gs)
    for g in range(G):
        for c in range(CH):
            img = buf[g * gs + c * ld:g * gs + c * ld + N * ldr].reshape(N, ldr)
            if zero_image:
                img[:] = 0
            img[:nv[g], :nv[g]] = bits[g, c, :nv[g], :nv[g]]
    return buf


def dev16(buf):
    return torch.from_numpy(buf.view(np.int16)).to(DEV)


def dev32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


class Launch:
    """Device buffers of one case and the launches on them."""

    def __init__(self, case, with_nrm=True, nrm_out=False):
        _lib.load()
        N, ldr, nv = case['N'], case['ldr'], case['nv']
        self.case, self.N, self.ldr = case, N, ldr
        self.st = strides(N, ldr)
        rng = np.random.default_rng(case_seed(N, [int(n) for n in nv], tag=77))
        self.za = dev16(host_slab(case['za_bits'], nv, *self.st['a'], N, ldr, rng))
        self.zb = dev16(host_slab(case['zb_bits'], nv, *self.st['b'], N, ldr, rng))
        self.dm = dev16(host_slab(case['dm_bits'], nv, *self.st['dm'], N, ldr, rng, zero_image=True))
        self.nvalid = torch.from_numpy(nv.astype(np.int32)).to(DEV) if case['ragged'] else None
        self.beta = [dev32(case['beta_a']), dev32(case['beta_b'])]
        self.nrm = [None, None]
        if nrm_out:
            self.nrm = [torch.full((G * CH * 4,), 123.0, device=DEV), torch.full((G * CH * 4,), 123.0, device=DEV)]
        elif with_nrm:
            self.nrm = [dev32(case['nrm_a']), dev32(case['nrm_b'])]
        self.sa = _lib.make_slab16(self.za, *self.st['a'], CH, nrm=self.nrm[0], beta=self.beta[0])
        self.sb = _lib.make_slab16(self.zb, *self.st['b'], CH, nrm=self.nrm[1], beta=self.beta[1])

    def out(self):
        return torch.full((G * self.st['out'][0],), SENT, dtype=torch.int16, device=DEV)

    def fwd(self):
        o = self.out()
        _lib.call('fgnn_chan_matmul_fwd16', ct.byref(self.sa), ct.byref(self.sb), _lib.ptr(self.nvalid), G, self.N, self.ldr,
                  _lib.ptr(o), *self.st['out'], _lib.stream_ptr())
        torch.cuda.synchronize()
        return o.cpu().numpy()

    def fwd_fin(self, part_a, part_b, cnt, w_a, w_b, tpg):
        o = self.out()
        keep = [dev32(part_a), dev32(part_b), dev32(cnt), None if w_a is None else dev32(w_a), None if w_b is None else dev32(w_b)]
        _lib.call('fgnn_chan_matmul_fwd16_fin', ct.byref(self.sa), ct.byref(self.sb), _lib.ptr(keep[0]), _lib.ptr(keep[1]),
                  _lib.ptr(keep[2]), _lib.ptr(keep[3]), _lib.ptr(keep[4]), EPS, tpg, _lib.ptr(self.nvalid), G, self.N, self.ldr,
                  _lib.ptr(o), *self.st['out'], _lib.stream_ptr())
        torch.cuda.synchronize()
        return o.cpu().numpy(), [n.cpu().numpy().astype(np.float64).reshape(G, CH, 4) for n in self.nrm]

    def bwd(self, mode, tpart=None, tpg=0):
        """mode 0: no statistics; 1: _bwd16 with s12; 2: _bwd16_t; 3: _bwd16_tc"""
        da, db = self.out(), self.out()
        s12 = [torch.full((G * CH * 2,), 77.0, device=DEV) for _ in range(2)] if mode else [None, None]
        coef = [torch.full((G * CH * 4,), 77.0, device=DEV) for _ in range(2)] if mode == 3 else [None, None]
        head = (ct.byref(self.sa), ct.byref(self.sb), _lib.ptr(self.dm), *self.st['dm'])
        tail = (_lib.ptr(self.nvalid), G, self.N, self.ldr, _lib.ptr(da), _lib.ptr(db), *self.st['out'], _lib.ptr(s12[0]),
                _lib.ptr(s12[1]))
        if mode < 2:
            _lib.call('fgnn_chan_matmul_bwd16', *head, *tail, _lib.stream_ptr())
        else:
            tp = dev32(tpart)
            extra = (_lib.ptr(coef[0]), _lib.ptr(coef[1])) if mode == 3 else ()
            _lib.call('fgnn_chan_matmul_bwd16_tc' if mode == 3 else 'fgnn_chan_matmul_bwd16_t', *head, _lib.ptr(tp), tpg, *tail, *extra,
                      _lib.stream_ptr())
        torch.cuda.synchronize()
        f = lambda t, k: None if t is None else t.cpu().numpy().reshape(G, CH, k)
        return dict(da=da.cpu().numpy(), db=db.cpu().numpy(), s12=[f(t, 2) for t in s12], coef=[f(t, 4) for t in coef])


# ---- checks -----------------------------------------------------------------------------------------------------------------
def first_bad(mask):
    return tuple(int(i) for i in np.argwhere(mask)[0])


def images(out, N, ldr):
    """stored (G, C, N, ldr) images as uint16 and everything of the buffer that lies outside them"""
    gs, ld = strides(N, ldr)['out']
    o = out.view(np.uint16)
    inside = np.zeros(o.shape, bool)
    img = np.empty((G, CH, N, ldr), np.uint16)
    for g in range(G):
        for c in range(CH):
            s = g * gs + c * ld
            img[g, c] = o[s:s + N * ldr].reshape(N, ldr)
            inside[s:s + N * ldr] = True
    return img, o[~inside]


def check_frame(what, out, case):
    """every element of the N x ldr images outside the corner is +0 and every sentinel outside the images is intact; returns the images"""
    N, ldr, nv = case['N'], case['ldr'], case['nv']
    img, rest = images(out, N, ldr)
    assert (rest == SENT).all(), '%s: sentinel overwritten, first at %s' % (what, first_bad(rest != SENT))
    pad = np.ones(img.shape, bool)
    for g in range(G):
        pad[g, :, :nv[g], :nv[g]] = False
    bad = pad & (img != 0)
    assert not bad.any(), '%s: (g, c, row, col) = %s outside the corner holds 0x%04x, not +0 (%d such)' % (
        what, first_bad(bad), img[first_bad(bad)], bad.sum())
    return img


def check_bits(what, out, ref64, case):
    """the three assertions of the bit-exact tests; returns the stored corner values (fp64, zeros outside)"""
    img = check_frame(what, out, case)
    N = case['N']
    want = R.rne_bf16(ref64)
    got = img[..., :N]
    bad = (got != want) & corner_mask(case)
    assert not bad.any(), '%s: (g, c, row, col) = %s stores 0x%04x, RNE_bf16(exact) = 0x%04x (%d of %d differ)' % (
        what, first_bad(bad), got[first_bad(bad)], want[first_bad(bad)], bad.sum(), corner_mask(case).sum())
    return R.bf16_value(got)


def corner_mask(case):
    m = np.zeros((G, CH, case['N'], case['N']), bool)
    for g, n in enumerate(case['nv']):
        m[g, :, :n, :n] = True
    return m


def check_elements(what, out, ref64, absA, absB, case):
    """|got - ref64| <= half a bf16 ulp + accum_bound, every element, no allowance; returns the largest error / gate"""
    img = check_frame(what, out, case)
    got = R.bf16_value(img[..., :case['N']])
    K = np.array([R.k_steps(n) for n in case['nv']], np.float64).reshape(G, 1, 1, 1)
    gate = R.element_gate(ref64, absA, absB, K)
    err = np.abs(got - ref64)
    m = corner_mask(case)
    ratio = float((err[m] / gate[m]).max()) if m.any() else 0.0
    print('RATIO %s %s: max error / gate = %.4f' % (what, shape_id((case['N'], tuple(case['nv']) if case['ragged'] else None)), ratio))
    bad = m & ~(err <= gate)
    assert not bad.any(), '%s: (g, c, row, col) = %s: got %r, reference %r, gate %r (%d elements over the gate, worst ratio %.3f)' % (
        what, first_bad(bad), got[first_bad(bad)], ref64[first_bad(bad)], gate[first_bad(bad)], bad.sum(), ratio)
    return ratio


# ---- cases ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid(N, nvalid):
    """The grid case of a shape, computed once and shared by the tests (read only): inputs as bf16 bits, the fp64 products."""
    rng = np.random.default_rng(case_seed(N, nvalid))
    c = R.grid_case(rng, G, CH, N, R.ceil8(N), nvalid)
    slim = {k: c[k] for k in ('G', 'C', 'N', 'ldr', 'nv', 'ragged', 'load', 'mean_a', 'mean_b', 'a_a', 'a_b', 'beta_a', 'beta_b')}
    for k in ('za', 'zb', 'dm'):
        slim[k + '_bits'] = R.rne_bf16(c[k])
        assert np.array_equal(R.bf16_value(slim[k + '_bits']), c[k])
    for k in ('M', 'dA', 'dB'):
        slim[k] = c[k].astype(np.float32)                   # multiples of 1/256 below 2^16: exact in fp32
        assert np.array_equal(slim[k], c[k])
    # records {mean, a, q, r2}: q and r2 only enter the coefficient records
    r2 = rng.choice(np.array([0.5, 1.0, 2.0, 4.0]), size=(2, G, CH))
    for i, s in enumerate('ab'):
        slim['nrm_' + s] = np.stack([c['mean_' + s], c['a_' + s], c['a_' + s], r2[i]], -1)
    for v in slim.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return slim


def pack_random(c):
    for k in ('za', 'zb', 'dm'):
        c[k + '_bits'] = R.rne_bf16(c[k])
    for s in 'ab':
        c['nrm_' + s] = np.stack([c['mean_' + s], c['a_' + s], c['a_' + s], np.ones((G, CH))], -1)
    return c


def tpart_of(case, tpg, rng):
    """T = <dM, M> of the stored product (scaled into the exact range if need be), spread over several tile entries in multiples
    of 1/16 so that the kernel's fp32 sum of the partials is exact in any order: T is what the test says it is."""
    M = R.bf16_value(R.rne_bf16(case['M'].astype(np.float64)))
    T = (R.bf16_value(case['dm_bits']) * M).sum((-1, -2))
    slots = sorted({0, tpg // 3, tpg // 2, min(600, tpg - 1), tpg - 1})      # 600: the second sweep of the kernel's load (t >= 512)
    tp = np.zeros((G, CH, tpg))
    for g in range(G):
        for c in range(CH):
            t = T[g, c]
            while abs(t) * 16 * 4 >= 2 ** 24:
                t /= 2
            share = np.rint(16 * t / len(slots)) / 16
            tp[g, c, slots] = share + rng.integers(-32, 33, len(slots)) / 16
    assert (np.abs(tp).sum(-1) * 16 < 2 ** 24).all() and not np.mod(tp * 16, 1).any()
    return tp


# ---- (a), (b) -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
def test_forward_is_bit_exact_on_grid_operands(shape):
    """fgnn_chan_matmul_fwd16: the nv x nv corner equals rne_bf16(M) bit for bit, every other element of the N x ldr image is +0
    ("the whole N x ldr output is defined"), every sentinel outside the images is intact."""
    case = grid(*shape)
    check_bits('M', Launch(case).fwd(), case['M'], case)


@gpu
@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
def test_backward_is_bit_exact_on_grid_operands(shape):
    """fgnn_chan_matmul_bwd16 without statistics: the same three assertions for dA = dM Yb^T and for dB = Ya^T dM."""
    case = grid(*shape)
    r = Launch(case).bwd(0)
    check_bits('dA', r['da'], case['dA'], case)
    check_bits('dB', r['db'], case['dB'], case)


# ---- (c) ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
def test_backward_statistics(shape):
    """STATS 1 (_bwd16 with s12), STATS 2 (_bwd16_t) and _bwd16_tc on the grid case.  dA and dB are bit-identical to the plain
    launch in all three (the same three assertions against the same reference bits).  With t the STORED values of the corner,
    n = nv^2 their number and u = 2^-24:
      * S1 = sum t within n u sum |t| of the fp64 sum (n - 1 fp32 additions in any order); bit-identical between the modes;
      * STATS 1: S2 = sum t (z - mean) within n u sum |t| |z - mean| (on the grid z - mean and the products are exact in fp32);
      * STATS 2: S2 = (T - beta S1) / a, the kernel's stated identity, evaluated in fp64 with T = sum tpart as given and the fp64
        S1; gate = |beta / a| x (bound on S1) + 4 fp32 ulps of the result (the kernel rounds beta S1, the difference and the quotient);
      * _tc: records {n.x, n.y, -n.y S2 n.w / m, -n.y S1 / m}, m = nv^2, against fp64 with the S1 / S2 gates propagated through
        the factors + 4 fp32 ulps (three roundings each); all-zero at nv = 0."""
    case = grid(*shape)
    N, ldr, nv = case['N'], case['ldr'], case['nv']
    L = Launch(case)
    tpg = _lib.load().fgnn_tiles_per_graph16(N, ldr)
    assert tpg == -(-N * ldr // 64)
    tpart = tpart_of(case, tpg, np.random.default_rng(case_seed(N, shape[1], tag=5)))
    runs = [L.bwd(1), L.bwd(2, tpart, tpg), L.bwd(3, tpart, tpg)]
    T = tpart.sum(-1)
    n = (nv.astype(np.float64) ** 2).reshape(G, 1)
    worst = {}
    def gated(name, got, ref, gate):
        err = np.abs(got - ref)
        worst[name] = max(worst.get(name, 0.0), float(np.max(np.where(gate > 0, err / np.where(gate > 0, gate, 1), 0.0))))
        assert (err <= gate).all(), '%s: (g, c) = %s: got %r, reference %r, gate %r' % (
            name, first_bad(err > gate), got[first_bad(err > gate)], ref[first_bad(err > gate)], gate[first_bad(err > gate)])
    for side, key, ref_key, s in ((0, 'da', 'dA', 'a'), (1, 'db', 'dB', 'b')):
        t = None
        for mode, r in zip((1, 2, 3), runs):
            t = check_bits('%s (mode %d)' % (ref_key, mode), r[key], case[ref_key], case)
        mean, a, beta = case['mean_' + s][:, :, None, None], case['a_' + s], case['beta_' + s][None, :]
        zc = (R.bf16_value(case['z%s_bits' % s]) - mean) * corner_mask(case)
        s1_64, g1 = t.sum((-1, -2)), n * U * np.abs(t).sum((-1, -2))
        s2_64, g2 = (t * zc).sum((-1, -2)), n * U * np.abs(t * zc).sum((-1, -2))
        s1 = [r['s12'][side][..., 0].astype(np.float64) for r in runs]
        s2 = [r['s12'][side][..., 1].astype(np.float64) for r in runs]
        for k in range(3):
            gated('S1', s1[k], s1_64, g1)
        assert np.array_equal(s1[0], s1[1]) and np.array_equal(s1[1], s1[2])                  # same sums, bit for bit
        gated('S2 (STATS 1)', s2[0], s2_64, g2)
        ident = (T - beta * s1_64) / a
        gi = np.abs(beta / a) * g1 + 4 * R.f32_ulp(ident)
        gated('S2 (STATS 2)', s2[1], ident, gi)
        assert np.array_equal(s2[1], s2[2])
        coef, rec = runs[2]['coef'][side].astype(np.float64), case['nrm_' + s]
        assert np.array_equal(coef[..., 0], rec[..., 0]) and np.array_equal(coef[..., 1], rec[..., 1])
        m = np.where(n > 0, n, 1.0)
        live = (n > 0).astype(np.float64)
        cz = -rec[..., 1] * ident * rec[..., 3] / m * live
        cw = -rec[..., 1] * s1_64 / m * live
        gated('coef.z', coef[..., 2], cz, np.abs(rec[..., 1] * rec[..., 3] / m) * gi * live + 4 * R.f32_ulp(cz) * live)
        gated('coef.w', coef[..., 3], cw, np.abs(rec[..., 1] / m) * g1 * live + 4 * R.f32_ulp(cw) * live)
    print('RATIO statistics %s: %s' % (shape_id(shape), ', '.join('%s %.4f' % kv for kv in sorted(worst.items()))))


# ---- (d) ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('shape', RANDOM_SHAPES, ids=shape_id)
def test_random_operands_element_wise(shape):
    """Forward and backward on ordinary data (randn scaled and shifted, arbitrary fp32 mean / a / beta: the staging rounds for
    real), reference operands from matmul16_ref.operands.  Every element: |got - ref64| <= half a bf16 ulp of ref64 (the spacing
    of the binade the fp32 sum can reach) + accum_bound; no allowance for outliers, no L2 gate."""
    N, nvalid = shape
    case = pack_random(R.random_case(np.random.default_rng(case_seed(N, nvalid, tag=4)), G, CH, N, R.ceil8(N), nvalid))
    L = Launch(case)
    ya, yb, dm = np.abs(case['ya']), np.abs(case['yb']), np.abs(case['dm'])
    check_elements('M', L.fwd(), case['M'], ya, yb, case)
    r = L.bwd(0)
    check_elements('dA', r['da'], case['dA'], dm, np.swapaxes(yb, -1, -2), case)
    check_elements('dB', r['db'], case['dB'], np.swapaxes(ya, -1, -2), dm, case)


# ---- (e) ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('weights', [False, True], ids=['unit_weight', 'weights'])
@pytest.mark.parametrize('shape', FIN_SHAPES, ids=shape_id)
def test_forward_with_folded_finalize(shape, weights):
    """fgnn_chan_matmul_fwd16_fin.  The tile statistics {mean_t, M2_t}, cnt are formed in fp64 from the raw z over a random
    partition of the corner into tpg pieces (some empty) and rounded to fp32.
    Step 1: the records written to slab.nrm against the fp64 two-level combination pushed through the nrm_record formula
    (matmul16_ref.nrm_records restates csrc/fgnn_norm.h:8-18 and derives the gate from the kernel's operation count; the 14
    roundings of a workgroup sum dominate it: 13 to 22 fp32 ulps on `a` at these shapes, more only where mean_t - mean cancels).
    Step 2: the product, element by element as in test_random_operands_element_wise, with reference operands formed from the
    records READ BACK from step 1."""
    N, nvalid = shape
    ldr = R.ceil8(N)
    rng = np.random.default_rng(case_seed(N, nvalid, tag=6))
    case = R.random_case(rng, G, CH, N, ldr, nvalid)
    for k in ('za', 'zb', 'dm'):
        case[k + '_bits'] = R.rne_bf16(case[k])
    nv = case['nv']
    tpg = _lib.load().fgnn_tiles_per_graph16(N, ldr)
    part, cnt = R.tile_partials(np.concatenate([case['za'], case['zb']], 1), nv, tpg, rng)
    assert (cnt == 0).any() and (cnt.sum(1) == nv ** 2).all()
    w = [1 + 0.2 * rng.standard_normal(CH), 1 + 0.2 * rng.standard_normal(CH)] if weights else [None, None]
    w = [None if x is None else np.asarray(x, np.float32).astype(np.float64) for x in w]
    L = Launch(case, nrm_out=True)
    out, recs = L.fwd_fin(part[:, :CH], part[:, CH:], cnt, w[0], w[1], tpg)
    eps = float(np.float32(EPS))
    worst = 0.0
    for i, s in enumerate('ab'):
        ref, gate = R.nrm_records(part[:, i * CH:(i + 1) * CH], cnt, nv, w[i], eps)
        err = np.abs(recs[i] - ref)
        worst = max(worst, float(np.max(np.where(gate > 0, err / np.where(gate > 0, gate, 1), 0.0))))
        assert (err <= gate).all(), 'record %s: (g, c, field) = %s: got %r, reference %r, gate %r (%.1f fp32 ulps)' % (
            s, first_bad(err > gate), recs[i][first_bad(err > gate)], ref[first_bad(err > gate)], gate[first_bad(err > gate)],
            gate[first_bad(err > gate)] / R.f32_ulp(ref[first_bad(err > gate)]))
        case['y' + s] = R.operands(case['z' + s], recs[i][..., 0], recs[i][..., 1], case['beta_' + s], nv)
    print('RATIO records %s %s: max error / gate = %.4f' % (shape_id(shape), 'weights' if weights else 'unit', worst))
    M, _, _ = R.products(case['ya'], case['yb'], case['dm'])
    check_elements('M (fin)', out, M, np.abs(case['ya']), np.abs(case['yb']), case)


# ---- (f) ----------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals():
    """Each bad argument returns the error code without launching: the outputs keep their sentinel."""
    lib = _lib.load()
    N, ldr, Gs, Cs = 16, 16, 1, 2
    room = Gs * Cs * 264 * 264                                             # enough for every shape named below
    z = torch.zeros(room, dtype=torch.int16, device=DEV)
    outs = [torch.full((room,), SENT, dtype=torch.int16, device=DEV) for _ in range(2)]
    f = torch.zeros(4096, device=DEV)
    st, p, pf = _lib.stream_ptr(), _lib.ptr(z), _lib.ptr(f)
    o0, o1 = _lib.ptr(outs[0]), _lib.ptr(outs[1])
    def slab(C=Cs, gs=None, ld=None, nrm=True, N=N, ldr=ldr):
        ld = N * ldr if ld is None else ld
        return _lib.make_slab16(z, Cs * ld if gs is None else gs, ld, C, nrm=f if nrm else None, beta=f)
    def fwd(sa=None, sb=None, N=N, ldr=ldr):
        sa, sb = sa or slab(N=N, ldr=ldr), sb or slab(N=N, ldr=ldr)
        return lib.fgnn_chan_matmul_fwd16(ct.byref(sa), ct.byref(sb), None, Gs, N, ldr, o0, Cs * N * ldr, N * ldr, st)
    def fin(tpg, N=N, ldr=ldr):
        sa, sb = slab(N=N, ldr=ldr), slab(N=N, ldr=ldr)
        return lib.fgnn_chan_matmul_fwd16_fin(ct.byref(sa), ct.byref(sb), pf, pf, pf, None, None, EPS, tpg, None, Gs, N, ldr, o0,
                                              Cs * N * ldr, N * ldr, st)
    def bwd(sa=None, sb=None, N=N, ldr=ldr, dmg=None, ldm=None, s12=(None, None), tpart=None, tpg=0, coef=None, name=None):
        sa, sb = sa or slab(N=N, ldr=ldr), sb or slab(N=N, ldr=ldr)
        img = N * ldr
        head = (ct.byref(sa), ct.byref(sb), p, Cs * img if dmg is None else dmg, img if ldm is None else ldm)
        tail = (None, Gs, N, ldr, o0, o1, Cs * img, img, s12[0], s12[1])
        if name == 'tc':
            return lib.fgnn_chan_matmul_bwd16_tc(*head, tpart, tpg, *tail, coef[0], coef[1], st)
        if name == 't':
            return lib.fgnn_chan_matmul_bwd16_t(*head, tpart, tpg, *tail, st)
        return lib.fgnn_chan_matmul_bwd16(*head, *tail, st)
    tpg = lib.fgnn_tiles_per_graph16(N, ldr)
    s12 = (pf, pf)
    bad = {
        'ldr % 8 != 0': [lambda: fwd(N=12, ldr=12), lambda: bwd(N=12, ldr=12)],
        'ldr < N': [lambda: fwd(N=16, ldr=8), lambda: bwd(N=16, ldr=8)],
        'N = 257': [lambda: fwd(N=257, ldr=264), lambda: bwd(N=257, ldr=264), lambda: fin(tpg, N=257, ldr=264)],
        'C mismatch': [lambda: fwd(sb=slab(C=1)), lambda: bwd(sb=slab(C=1))],
        'stride % 8 != 0': [lambda: fwd(sa=slab(ld=N * ldr + 4)), lambda: fwd(sb=slab(gs=Cs * N * ldr + 4)),
                            lambda: bwd(sa=slab(gs=Cs * N * ldr + 4)), lambda: bwd(sb=slab(ld=N * ldr + 4)),
                            lambda: bwd(ldm=N * ldr + 4), lambda: bwd(dmg=Cs * N * ldr + 4)],
        's12a without s12b': [lambda: bwd(s12=(pf, None)), lambda: bwd(s12=(None, pf))],
        's12 without nrm': [lambda: bwd(sa=slab(nrm=False), s12=s12), lambda: bwd(sb=slab(nrm=False), s12=s12)],
        'tpart without s12': [lambda: bwd(tpart=pf, tpg=tpg, name='t')],
        'missing tpart': [lambda: bwd(s12=s12, tpart=None, tpg=tpg, name='t'), lambda: bwd(s12=s12, tpart=None, tpg=tpg, coef=s12, name='tc')],
        'tpg = 1025': [lambda: bwd(s12=s12, tpart=pf, tpg=1025, name='t'), lambda: bwd(s12=s12, tpart=pf, tpg=0, name='t'),
                       lambda: fin(1025), lambda: fin(0)],
        'coef without s12': [lambda: bwd(tpart=pf, tpg=tpg, coef=(pf, pf), name='tc')],
        'one coef': [lambda: bwd(s12=s12, tpart=pf, tpg=tpg, coef=(pf, None), name='tc')],
    }
    for what, calls in bad.items():
        for i, fn in enumerate(calls):
            assert fn() == 1, '%s (call %d) was not refused' % (what, i)
            assert _lib.last_error(), what
    torch.cuda.synchronize()
    assert all((o.cpu().numpy().view(np.uint16) == SENT).all() for o in outs) and not f.cpu().numpy().any()
    # the baseline the refusals perturb is itself accepted
    assert fwd() == 0 and bwd() == 0 and bwd(s12=s12) == 0 and fin(tpg) == 0
    torch.cuda.synchronize()


# ---- (g) ----------------------------------------------------------------------------------------------------------------------
FORMS = ((64, (2, 2)), (128, (4, 4)), (224, (8, 7)), (256, (8, 8)))       # N <= bound -> <NT, NCOL>


def form_of(N):
    """The dispatch of matmul_fwd16_common / matmul_bwd16_common (csrc/matmul16.hip, `if (N <= 64) return launch_fwd16<2>` ...
    `if (N <= 224) return launch_fwd16<8, 7>`, else <8>; N <= 256 checked above it)."""
    return next(f for bound, f in FORMS if N <= bound)


def test_cases_reach_every_form():
    """Host-side bookkeeping: the size tables cover each of the four dispatch ranges from both sides of its thresholds, both
    `nv % 8` branches, ntv < NT (a tile row / column left out) and nv = 0 -- and the thresholds restated in FORMS are the
    ones in the source, so that a changed threshold fails here instead of silently shrinking the coverage."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'graph_neural_net_amd', 'csrc',
                            'matmul16.hip')).read()
    for kind in ('fwd16', 'bwd16'):
        body = src[src.index('static int matmul_%s_common' % kind):]
        body = body[:body.index('extern "C"')]
        assert 'N <= 256' in body
        found = re.findall(r'if \(N <= (\d+)\)\s*return launch_%s<(\d+)(?:, (\d+))?>' % kind, body)
        last = re.findall(r'\n    return launch_%s<(\d+)(?:, (\d+))?>' % kind, body)
        got = [(int(b), (int(nt), int(nc or nt))) for b, nt, nc in found] + [(256, (int(last[0][0]), int(last[0][1] or last[0][0])))]
        assert tuple(got) == FORMS, (kind, got)
    pairs = [(N, N) for N in DENSE] + [(N, n) for N, nvs in RAGGED for n in nvs]
    for table, name in ((pairs, 'bit-exact'), ([(N, n) for N, nvs in RANDOM_SHAPES for n in (nvs or (N,))], 'element-wise')):
        for bound, form in FORMS:
            mine = [(N, n) for N, n in table if form_of(N) == form and n > 0]
            assert mine, (name, form)
            assert any(n % 8 == 0 for _, n in mine) and any(n % 8 for _, n in mine), (name, form)
            if name == 'bit-exact':
                assert any(-(-n // 32) < form[1] for _, n in mine), form                     # ntv < NT
                assert any(-(-n // 32) == form[1] for _, n in mine), form                    # every tile row and column
        assert any(n == 0 for _, n in table) and any(n == 1 for _, n in table), name
    assert {64, 65, 128, 129, 224, 225, 256} <= set(DENSE)                                   # both sides of every threshold
    # the finalize shapes reach all four forms and nv = 0
    assert {form_of(N) for N, _ in FIN_SHAPES} == {(2, 2), (4, 4), (8, 7), (8, 8)}
    assert any(nvs and 0 in nvs for _, nvs in FIN_SHAPES)
