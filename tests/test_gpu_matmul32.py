"""GPU: the per-channel fp32 products of csrc/matmul.hip, through the C ABI, against tests/matmul32_ref.py -- exactly on grid
operands, element by element inside the derived bound on ordinary data, in every compiled form: the wave-per-matrix forward
(every KQ instance, its eight-byte form, its four-byte form at every N), the workgroup-per-matrix forward, the whole-matrix
kernels (NT = 4, 8; plain and longest-first order; fill 0 and 1; backward split and not), the single-tile backward with and
without S1 / S2, the generic tiles with their fgnn_gn_bwd_stats passes, and the folded finalize.

Set-up of every case (matmul32_ref): G = 3, C = 3 -- nine matrices, so the last workgroup of the wave-per-matrix kernel has an
idle wave -- (1 x 2 at N = 257); row pitch N; the operand slabs, dM and the outputs each have their own (gstride, ld), all but
one above the minimum (dA and dB are two buffers with the ONE (ogstride, ldo) of the C ABI); operand slabs and dM hold finite
garbage of magnitude 1e30 everywhere outside the nv x nv corner -- rows and columns >= nv of the image, channel tails, graph
gaps; every output is prefilled with a sentinel, and the checkers assert the frame (exact +0, or what fill = 1 leaves alone) and
the intact sentinels with every product.  No tolerance here is a constant: a result is bit-equal to another, equal to the
exact product, or inside matmul32_ref.finish's bound."""
import ctypes as ct
import os
import re

import numpy as np
import pytest
import torch

import matmul32_ref as R
from graph_neural_net_amd import _lib
from matmul32_ref import shape_id

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 1e-5
FAMILIES = ('grid', 'random')
VARIANTS = (1, 9, 0)                    # fgnn_debug_matmul_variant: shipped, four-byte form, workgroup per matrix

# (shape, odd strides)
SMALL = [(s, False) for s in R.SMALL] + [(s, True) for s in R.ODD if s[0] <= R.TM]
BIG = [(s, False) for s in R.BIG] + [(s, True) for s in R.ODD if R.big(s[0])]
GENERIC = [(s, False) for s in R.GENERIC] + [(s, True) for s in R.ODD if s[0] > R.BIG_MAX]
FIN = [(s, False) for s in R.FIN] + [((64, (64, 33, 1)), True), ((200, (200, 129, 1)), True)]
ids = dict(ids=lambda p: shape_id(p[0]) + ('_odd' if p[1] else '') if isinstance(p, tuple) else str(p))

RATIO = {}                              # (form, output) -> largest error / bound seen (test_ratio_table prints it)


def note(form, ratios):
    for k, v in ratios.items():
        RATIO[(form, k)] = max(RATIO.get((form, k), 0.0), v)


def dev32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


class Launch:
    """Device buffers of one case and the launches on them."""

    def __init__(self, case, odd=False, nrm_out=False, raw=False):
        self.lib = _lib.load()
        c = self.case = case
        self.G, self.C, self.N, nv = c['G'], c['C'], c['N'], c['nv']
        self.st = R.strides(self.N, self.C, odd)
        rng = np.random.default_rng(R.case_seed(self.N, [int(n) for n in nv], tag=77))
        f = lambda x: x.astype(np.float32)
        self.za = dev32(R.slab(f(c['za']), nv, *self.st['a'], rng))
        self.zb = dev32(R.slab(f(c['zb']), nv, *self.st['b'], rng))
        self.dm = dev32(R.slab(f(c['dm_raw']), nv, *self.st['dm'], rng))
        self.nv_all = torch.from_numpy(nv.astype(np.int32)).to(DEV)
        self.nvalid = self.nv_all if c['ragged'] else None
        self.beta = [dev32(c['beta_a']), dev32(c['beta_b'])]
        if nrm_out:
            self.nrm = [torch.full((self.G * self.C * 4,), float('nan'), device=DEV) for _ in range(2)]
        elif raw:
            self.nrm = [None, None]
        else:
            self.nrm = [dev32(c['nrm_a']), dev32(c['nrm_b'])]
        self.sa = _lib.make_slab(self.za, *self.st['a'], self.C, nrm=self.nrm[0], beta=self.beta[0])
        self.sb = _lib.make_slab(self.zb, *self.st['b'], self.C, nrm=self.nrm[1], beta=self.beta[1])
        self._order = None

    def order(self):
        """the longest-first schedule of fgnn_ragged_tile_ranges_order for this case's vertex counts"""
        if self._order is None:
            ranges = torch.empty(_lib.FGNN_RANGE_WG + 1, dtype=torch.int32, device=DEV)
            self._order = torch.full((self.G,), -1, dtype=torch.int32, device=DEV)
            _lib.call('fgnn_ragged_tile_ranges_order', _lib.ptr(self.nv_all), self.G, self.N, _lib.ptr(ranges), _lib.ptr(self._order),
                      _lib.stream_ptr())
            want = sorted(range(self.G), key=lambda g: (-int(self.case['nv'][g]), g))
            assert self._order.cpu().tolist() == want
        return self._order

    def out(self):
        return torch.from_numpy(R.sentinel(self.G * self.st['out'][0]).copy()).to(DEV)

    def _nv(self, ordered):
        return self.nv_all if ordered else self.nvalid

    def fwd(self, ordered=False, fill=0):
        o = self.out()
        _lib.call('fgnn_chan_matmul_fwd_ord', ct.byref(self.sa), ct.byref(self.sb), _lib.ptr(self._nv(ordered)), self.G, self.N,
                  _lib.ptr(o), *self.st['out'], _lib.ptr(self.order() if ordered else None), fill, _lib.stream_ptr())
        torch.cuda.synchronize()
        return dict(st=self.st['out'], fill=fill, M=o.cpu().numpy())

    def fwd_fin(self, part_a, part_b, cnt, gw_a, gw_b, ordered=False, fill=0):
        o = self.out()
        for n in self.nrm:
            n.fill_(float('nan'))
        _lib.call('fgnn_chan_matmul_fwd_fin_ord', ct.byref(self.sa), ct.byref(self.sb), _lib.ptr(part_a), _lib.ptr(part_b),
                  _lib.ptr(cnt), _lib.ptr(gw_a), _lib.ptr(gw_b), EPS, _lib.ptr(self._nv(ordered)), self.G, self.N, _lib.ptr(o),
                  *self.st['out'], _lib.ptr(self.order() if ordered else None), fill, _lib.stream_ptr())
        torch.cuda.synchronize()
        return dict(st=self.st['out'], fill=fill, M=o.cpu().numpy()), [n.cpu().numpy().copy() for n in self.nrm]

    def bwd(self, s12=True, ordered=False, fill=0):
        da, db = self.out(), self.out()
        s = [torch.full((self.G * self.C * 2,), 77.0, device=DEV) for _ in range(2)] if s12 else [None, None]
        _lib.call('fgnn_chan_matmul_bwd_ord', ct.byref(self.sa), ct.byref(self.sb), _lib.ptr(self.dm), *self.st['dm'],
                  _lib.ptr(self._nv(ordered)), self.G, self.N, _lib.ptr(da), _lib.ptr(db), *self.st['out'], _lib.ptr(s[0]),
                  _lib.ptr(s[1]), _lib.ptr(self.order() if ordered else None), fill, _lib.stream_ptr())
        torch.cuda.synchronize()
        return dict(st=self.st['out'], fill=fill, dA=da.cpu().numpy(), dB=db.cpu().numpy(),
                    s12a=None if s[0] is None else s[0].cpu().numpy(), s12b=None if s[1] is None else s[1].cpu().numpy())


def check(dev, case):
    return (R.check_exact if case['exact'] else R.check_bounded)(dev, case)


def same_bits(x, y):
    return np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))


# ---- which kernel a call reaches ------------------------------------------------------------------------------------------------
def fwd_form(N, variant=1, ordered=False, fill=0, fin=False):
    """The decision of chan_matmul_fwd_dispatch / launch_fwd_w (csrc/matmul.hip) restated."""
    f = '_fin' if fin else ''
    if N <= R.TM:
        if not variant & 1:
            return 'fwd1' + f
        KQ = (N + 7) // 8
        return ('w2<8>' if KQ == 8 and not variant & 8 and N % 2 == 0 else 'w<%d>' % KQ) + f
    if R.big(N):
        return 'fwd_big<%d>%s order=%d fill=%d' % (4 if N <= 128 else 8, f, ordered, fill)
    assert not fin
    return 'fwd_generic'


def bwd_form(N, s12, ordered=False, fill=0, matrices=R.G * R.CH):
    """The decision of fgnn_chan_matmul_bwd_ord restated (split: an order, and at most BIG_SPLIT_MAX_MATRICES = 2048 matrices)."""
    if N <= R.TM:
        return 'bwd1 s12=%d' % s12
    if R.big(N):
        return 'bwd_big<%d> split=%d fill=%d s12=%d' % (4 if N <= 128 else 8, ordered and matrices <= 2048, fill, s12)
    return 'bwd_generic' + (' + gn_bwd_stats' if s12 else '')


# ---- forward --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('p', SMALL, **ids)
def test_forward_small(p, family):
    (N, nvalid), odd = p
    case = R.case(family, N, nvalid)
    L = Launch(case, odd)
    outs = []
    try:
        for variant in VARIANTS:
            L.lib.fgnn_debug_matmul_variant(variant)
            dev = L.fwd()
            note(fwd_form(N, variant), check(dev, case))
            outs.append(dev['M'])
    finally:
        L.lib.fgnn_debug_matmul_variant(1)
    assert same_bits(outs[0], outs[1]) and same_bits(outs[0], outs[2])


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('p', BIG + GENERIC, **ids)
def test_forward_big(p, family):
    (N, nvalid), odd = p
    case = R.case(family, N, nvalid)
    L = Launch(case, odd)
    outs = {}
    for ordered in (False, True):
        for fill in (0, 1):
            dev = L.fwd(ordered, fill)
            note(fwd_form(N, 1, ordered, fill), check(dev, case))
            outs[ordered, fill] = dev['M']
    for fill in (0, 1):
        assert same_bits(outs[False, fill], outs[True, fill])


# ---- backward -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('p', SMALL, **ids)
def test_backward_small(p, family):
    (N, nvalid), odd = p
    case = R.case(family, N, nvalid)
    L = Launch(case, odd)
    with_s, without = L.bwd(True), L.bwd(False)
    note(bwd_form(N, True), check(with_s, case))
    note(bwd_form(N, False), check(without, case))
    assert same_bits(with_s['dA'], without['dA']) and same_bits(with_s['dB'], without['dB'])


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('p', BIG, **ids)
def test_backward_big(p, family):
    """order == NULL: one workgroup per matrix; an order: one per product (split).  Same bits on the live region and in S1 / S2."""
    (N, nvalid), odd = p
    case = R.case(family, N, nvalid)
    L = Launch(case, odd)
    res = {}
    for ordered in (False, True):
        for fill in (0, 1):
            for s12 in (True, False):
                dev = res[ordered, fill, s12] = L.bwd(s12, ordered, fill)
                note(bwd_form(N, s12, ordered, fill), check(dev, case))
    base = res[False, 0, True]
    for key, dev in res.items():
        for name in ('dA', 'dB'):
            if key[1] == 0:
                assert same_bits(dev[name], base[name]), (key, name)
            else:
                assert same_bits(dev[name], res[False, 1, True][name]), (key, name)
            live = R._corner(case)
            assert same_bits(R._images(dev[name], case, *dev['st'])[live].astype(np.float32),
                             R._images(base[name], case, *base['st'])[live].astype(np.float32)), (key, name)
        if key[2]:
            assert same_bits(dev['s12a'], base['s12a']) and same_bits(dev['s12b'], base['s12b']), key


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('p', GENERIC, **ids)
def test_backward_generic(p, family):
    """N = 257: the tiled kernel, and with s12 its two fgnn_gn_bwd_stats passes."""
    (N, nvalid), odd = p
    case = R.case(family, N, nvalid)
    L = Launch(case, odd)
    with_s, without = L.bwd(True), L.bwd(False)
    note(bwd_form(N, True), check(with_s, case))
    note(bwd_form(N, False), check(without, case))
    assert same_bits(with_s['dA'], without['dA']) and same_bits(with_s['dB'], without['dB'])


# ---- folded finalize ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', FIN, **ids)
def test_forward_fin(p):
    """fgnn_chan_matmul_fwd_fin_ord = fgnn_gn_finalize2 + fgnn_chan_matmul_fwd_ord bit for bit (records and product), and the
    product inside the element bound of the fp64 reference evaluated with the records the device published."""
    (N, nvalid), odd = p
    base = R.case('random', N, nvalid)
    G, C, nv = base['G'], base['C'], base['nv']
    L = Launch(base, odd, nrm_out=True)
    tpg = L.lib.fgnn_tiles_per_graph(N)
    g = torch.Generator().manual_seed(3000 + N)
    parts = [torch.stack([torch.randn(G, tpg, C, generator=g), torch.rand(G, tpg, C, generator=g) + 0.1], dim=-1).contiguous().to(DEV)
             for _ in range(2)]
    w = torch.rand(G, tpg, generator=g) + 0.1               # positive counts that sum to nv^2 per graph
    cnt = (w / w.sum(dim=1, keepdim=True) * torch.tensor([float(n * n) for n in nv]).view(G, 1)).contiguous().to(DEV)
    gw = [(torch.rand(C, generator=g) + 0.5).to(DEV) for _ in range(2)]
    rec = [torch.full((G * C * 4,), float('nan'), device=DEV) for _ in range(2)]
    _lib.call('fgnn_gn_finalize2', _lib.ptr(parts[0]), _lib.ptr(parts[1]), _lib.ptr(cnt), _lib.ptr(gw[0]), _lib.ptr(gw[1]),
              _lib.ptr(L.nvalid), G, C, N, EPS, _lib.ptr(rec[0]), _lib.ptr(rec[1]), _lib.stream_ptr())
    torch.cuda.synchronize()
    rec = [r.cpu().numpy() for r in rec]
    assert np.isfinite(rec[0]).all() and np.isfinite(rec[1]).all()
    case = R.with_records(base, rec[0], rec[1])
    two = Launch(dict(case, dm_raw=base['dm_raw']), odd)     # the two-launch path: slabs that carry the finalized records
    modes = [(v, False, 0) for v in VARIANTS] if N <= R.TM else [(1, o, f) for o in (False, True) for f in (0, 1)]
    try:
        for variant, ordered, fill in modes:
            L.lib.fgnn_debug_matmul_variant(variant)
            dev, nrm = L.fwd_fin(parts[0], parts[1], cnt, gw[0], gw[1], ordered, fill)
            ref = two.fwd(ordered, fill)
            assert same_bits(nrm[0], rec[0]) and same_bits(nrm[1], rec[1]), (variant, ordered, fill)
            assert same_bits(dev['M'], ref['M']), (variant, ordered, fill)
            note(fwd_form(N, variant, ordered, fill, fin=True), R.check_bounded(dev, case))
    finally:
        L.lib.fgnn_debug_matmul_variant(1)


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def test_argument_checks_refuse_without_writing():
    lib = _lib.load()
    small, gen = Launch(R.case('random', 33, None)), Launch(R.case('random', 257, None))
    raw = Launch(R.case('random', 33, None), raw=True)
    st = _lib.stream_ptr()

    def run(L, what):
        o, o2 = L.out(), L.out()
        s = [torch.from_numpy(R.sentinel(L.G * L.C * 2).copy()).to(DEV) for _ in range(2)]
        nrm = [torch.from_numpy(R.sentinel(L.G * L.C * 4).copy()).to(DEV) for _ in range(2)]
        sa = _lib.make_slab(L.za, *L.st['a'], L.C, nrm=nrm[0] if what.startswith('fin') else L.nrm[0], beta=L.beta[0])
        sb = _lib.make_slab(L.zb, *L.st['b'], 1 if what.endswith('C') else L.C, nrm=nrm[1] if what.startswith('fin') else L.nrm[1],
                            beta=L.beta[1])
        a, b = ct.byref(sa), ct.byref(sb)
        tpg = lib.fgnn_tiles_per_graph(L.N)
        part, cnt = torch.ones(L.G * tpg * L.C * 2, device=DEV), torch.ones(L.G * tpg, device=DEV)
        order = _lib.ptr(L.order()) if 'order' in what else None
        out, dm = (_lib.ptr(o), *L.st['out']), (_lib.ptr(L.dm), *L.st['dm'])
        p = _lib.ptr
        rc = {
            'fwd C': lambda: lib.fgnn_chan_matmul_fwd(a, b, None, L.G, L.N, *out, st),
            'fwd_ord C': lambda: lib.fgnn_chan_matmul_fwd_ord(a, b, None, L.G, L.N, *out, None, 0, st),
            'fin C': lambda: lib.fgnn_chan_matmul_fwd_fin(a, b, p(part), p(part), p(cnt), None, None, EPS, None, L.G, L.N, *out, st),
            'fin_ord C': lambda: lib.fgnn_chan_matmul_fwd_fin_ord(a, b, p(part), p(part), p(cnt), None, None, EPS, None, L.G, L.N, *out, None, 0, st),
            'bwd C': lambda: lib.fgnn_chan_matmul_bwd(a, b, *dm, None, L.G, L.N, p(o), p(o2), *L.st['out'], None, None, st),
            'bwd_ord C': lambda: lib.fgnn_chan_matmul_bwd_ord(a, b, *dm, None, L.G, L.N, p(o), p(o2), *L.st['out'], None, None, None, 0, st),
            'fwd_ord order': lambda: lib.fgnn_chan_matmul_fwd_ord(a, b, None, L.G, L.N, *out, order, 0, st),
            'fin_ord order': lambda: lib.fgnn_chan_matmul_fwd_fin_ord(a, b, p(part), p(part), p(cnt), None, None, EPS, None, L.G, L.N, *out, order, 0, st),
            'bwd_ord order': lambda: lib.fgnn_chan_matmul_bwd_ord(a, b, *dm, None, L.G, L.N, p(o), p(o2), *L.st['out'], None, None, order, 0, st),
            'bwd s12a only': lambda: lib.fgnn_chan_matmul_bwd(a, b, *dm, None, L.G, L.N, p(o), p(o2), *L.st['out'], p(s[0]), None, st),
            'bwd s12b only': lambda: lib.fgnn_chan_matmul_bwd_ord(a, b, *dm, None, L.G, L.N, p(o), p(o2), *L.st['out'], None, p(s[1]), None, 0, st),
            'bwd s12 raw': lambda: lib.fgnn_chan_matmul_bwd(a, b, *dm, None, L.G, L.N, p(o), p(o2), *L.st['out'], p(s[0]), p(s[1]), st),
            'fin 257': lambda: lib.fgnn_chan_matmul_fwd_fin(a, b, p(part), p(part), p(cnt), None, None, EPS, None, L.G, L.N, *out, st),
            'fin_ord 257': lambda: lib.fgnn_chan_matmul_fwd_fin_ord(a, b, p(part), p(part), p(cnt), None, None, EPS, None, L.G, L.N, *out, None, 0, st),
        }[what]()
        torch.cuda.synchronize()
        assert rc == 1 and _lib.last_error(), '%s was not refused' % what
        for t in [o, o2] + s + nrm:
            assert (t.cpu().numpy().view(np.uint32) == R.SENT).all(), '%s wrote to an output' % what

    for what in ('fwd C', 'fwd_ord C', 'fin C', 'fin_ord C', 'bwd C', 'bwd_ord C', 'fwd_ord order', 'fin_ord order', 'bwd_ord order',
                 'bwd s12a only', 'bwd s12b only'):
        run(small, what)
    run(raw, 'bwd s12 raw')
    assert lib.fgnn_chan_matmul_fwd_fin_supported(256) == 1 and lib.fgnn_chan_matmul_fwd_fin_supported(257) == 0
    run(gen, 'fin 257')
    run(gen, 'fin_ord 257')
    # the baseline the refusals perturb is itself accepted
    check(small.fwd(), small.case)
    check(small.bwd(True), small.case)


# ---- coverage -------------------------------------------------------------------------------------------------------------------
def test_cases_reach_every_form():
    """Host-side bookkeeping: the case lists reach every compiled form of csrc/matmul.hip, and the dispatch restated in fwd_form /
    bwd_form is the one in the source -- a changed threshold fails here instead of silently shrinking the coverage."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'graph_neural_net_amd', 'csrc', 'matmul.hip')).read()
    assert 'constexpr int TM = 64;' in src and 'inline bool big_path(int N) { return N > TM && N <= 256; }' in src
    assert 'constexpr int BIG_SPLIT_MAX_MATRICES = 8 * 256;' in src and 'constexpr int W_WAVES = 2;' in src
    d = src[src.index('static int chan_matmul_fwd_dispatch'):src.index('extern "C" int fgnn_chan_matmul_fwd(')]
    assert re.search(r'if \(N <= TM\) \{\s*if \(mm_wave_variant\(\)\) launch_fwd_w<FIN>.*?else hipLaunchKernelGGL\(chan_matmul_fwd1_kernel<FIN>', d, re.S)
    assert re.search(r'else if \(big_path\(N\)\) \{\s*if \(N <= 128\) launch_fwd_big<4, FIN>.*?else launch_fwd_big<8, FIN>', d, re.S)
    assert 'hipLaunchKernelGGL(chan_matmul_fwd_kernel,' in d
    w = src[src.index('int launch_fwd_w('):src.index('// Whole matrix per workgroup')]
    assert 'const int KQ = (N + 7) / 8' in w and 'if (KQ == 8 && !mm_narrow() && (N & 1) == 0)' in w
    kqs = [int(k) for k in re.findall(r'FGNN_W\((\d)\)', w[w.index('switch (KQ)'):])]
    assert kqs == list(range(1, 9))
    b = src[src.index('extern "C" int fgnn_chan_matmul_bwd_ord'):]
    assert 'const int t = (N + TM - 1) / TM;' in b and re.search(r'if \(t == 1\) \{.*?chan_matmul_bwd1_kernel', b, re.S)
    assert 'const int split = (order && (long long)G * ya->C <= BIG_SPLIT_MAX_MATRICES) ? 1 : 0;' in b
    assert re.search(r'if \(N <= 128\) FGNN_BIG_BWD\(4\)\s*else FGNN_BIG_BWD\(8\)', b)
    assert 'fgnn_gn_bwd_stats(da,' in b and 'fgnn_gn_bwd_stats(db,' in b

    fwd = {fwd_form(s[0], v) for s, _ in SMALL for v in VARIANTS}
    fwd |= {fwd_form(s[0], 1, o, f) for s, _ in BIG + GENERIC for o in (False, True) for f in (0, 1)}
    want = {'w<%d>' % k for k in kqs} | {'w2<8>', 'fwd1', 'fwd_generic'}
    want |= {'fwd_big<%d> order=%d fill=%d' % (nt, o, f) for nt in (4, 8) for o in (0, 1) for f in (0, 1)}
    assert fwd == want, fwd ^ want
    bwd = {bwd_form(s[0], s12) for s, _ in SMALL + GENERIC for s12 in (True, False)}
    bwd |= {bwd_form(s[0], s12, o, f) for s, _ in BIG for o in (False, True) for f in (0, 1) for s12 in (True, False)}
    want = {'bwd1 s12=0', 'bwd1 s12=1', 'bwd_generic', 'bwd_generic + gn_bwd_stats'}
    want |= {'bwd_big<%d> split=%d fill=%d s12=%d' % (nt, sp, f, s) for nt in (4, 8) for sp in (0, 1) for f in (0, 1) for s in (0, 1)}
    assert bwd == want, bwd ^ want
    fin = {fwd_form(s[0], v, fin=True) for s, _ in FIN if s[0] <= R.TM for v in VARIANTS}
    fin |= {fwd_form(s[0], 1, o, f, fin=True) for s, _ in FIN if s[0] > R.TM for o in (False, True) for f in (0, 1)}
    want = {'w<5>_fin', 'w<8>_fin', 'w2<8>_fin', 'fwd1_fin'} | {'fwd_big<%d>_fin order=%d fill=%d' % (nt, o, f) for nt in (4, 8) for o in (0, 1) for f in (0, 1)}
    assert fin == want, fin ^ want
    # the shapes: both sides of every threshold, every N dense and ragged, nv straddling 32 below N = 64 and the tile edges above,
    # an empty graph, a single vertex, an odd number of matrices, strides odd in floats in every range
    Ns = {s[0] for s, _ in SMALL + BIG + GENERIC}
    assert {1, 2, 7, 31, 32, 33, 48, 63, 64, 65, 96, 127, 128, 129, 200, 255, 256, 257} <= Ns
    for N in Ns:
        assert any(s[0] == N and s[1] is None for s, _ in SMALL + BIG + GENERIC)
        assert any(s[0] == N and s[1] is not None for s, _ in SMALL + BIG + GENERIC)
    rag = {s for s, _ in SMALL + BIG + GENERIC if s[1] is not None}
    for N in R.SMALL_N:
        assert {(N, (N, 1, N - 1)), (N, (N, 0, (N + 1) // 2))} <= rag and (N <= 32 or (N, (33, 32, 31)) in rag)
    for N in R.NT4_N:
        assert {(N, (N, 64, 1)), (N, (N, 65, 0))} <= rag
    for N in R.NT8_N:
        assert {(N, (N, 128, 97)), (N, (N, 129, 1))} <= rag
    assert {(257, (257,)), (257, (200,))} <= rag
    assert (R.G * R.CH) % 2 == 1
    for lst in (SMALL, BIG, GENERIC, FIN):
        assert any(odd for _, odd in lst)
    for N in (64, 96, 200, 257):
        assert all(x % 2 for pair in R.strides(N, R.dims(N)[1], True).values() for x in pair)
        st = R.strides(N, R.dims(N)[1])
        assert all(x % 4 == 0 for pair in st.values() for x in pair) and len(set(st.values())) == 4
        assert sum(ld == (N * N + 3) // 4 * 4 for _, ld in st.values()) == 1


def test_ratio_table():
    """Largest error / bound per form over the ordinary cases above (printed with -s; DESIGN.md quotes it)."""
    for form, name in sorted(RATIO):
        print('measured  %-44s %-4s error / bound <= %.3f' % (form, name, RATIO[form, name]))
        assert RATIO[form, name] <= 1.0
