"""GPU: the GraphNorm record, coefficient and gradient-reduction kernels of csrc/norm.hip through the C ABI, each output
element against the fp64 restatement of tests/graphnorm_ref.py within the rounding bound derived there from the kernel's
operation order (safety factor 2; tests/test_graphnorm_ref_host.py shows a float32 emulation inside the same bounds on the
same inputs).  Every output buffer lies between NaN guard cells and starts as NaN: the guards must stay, and exactly the
expected cells must be written."""
import numpy as np
import pytest
import torch

import graphnorm_ref as R
from graph_neural_net_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 512                 # floats on either side of a buffer (a multiple of 4: float4 records stay aligned)
FIELDS = ('mean', 'a', 'q', 'r2')
EPS = 1e-5


class Out:
    """n floats of NaN between two NaN guards"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
        self.t = self.buf[GUARD:GUARD + n]

    @property
    def ptr(self):
        return _lib.ptr(self.t)

    def read(self, written=None):
        """the n floats, after checking that the guards are untouched and that exactly the cells of the boolean mask `written`
        (default: all) were written"""
        b = self.buf.cpu().numpy()
        assert np.isnan(b[:GUARD]).all() and np.isnan(b[GUARD + self.n:]).all(), 'a guard cell was written'
        body = b[GUARD:GUARD + self.n].copy()
        w = np.ones(self.n, dtype=bool) if written is None else np.asarray(written, dtype=bool).reshape(-1)
        assert not np.isnan(body[w]).any(), '%d expected cells were not written' % np.isnan(body[w]).sum()
        assert np.isnan(body[~w]).all(), '%d cells were written that must stay untouched' % (~np.isnan(body[~w])).sum()
        return body


def dev(a, dtype=np.float32):
    """an input on the device, between NaN guards of its own (a kernel that reads past its input sums a NaN)"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
    if dtype != np.float32:
        return torch.from_numpy(a.copy()).to(DEV)
    buf = torch.full((a.size + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    buf[GUARD:GUARD + a.size] = torch.from_numpy(a.copy())
    return buf[GUARD:GUARD + a.size]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def note(family, ratio):
    print('graphnorm-ratio %s %.3f' % (family, ratio))


# ------------------------------------------------------------------------------------------------------------ finalize
def _finalize(tr, part, cnt, w, nv, fc, out):
    if tr:
        _lib.call('fgnn_gn_finalize_tpg', _lib.ptr(part), _lib.ptr(cnt), _lib.ptr(w), _lib.ptr(nv), fc['G'], fc['C'], fc['N'], fc['tpg'],
                  EPS, out.ptr, _lib.stream_ptr())
    else:
        _lib.call('fgnn_gn_finalize', _lib.ptr(part), _lib.ptr(cnt), _lib.ptr(w), _lib.ptr(nv), fc['G'], fc['C'], fc['N'], EPS, out.ptr,
                  _lib.stream_ptr())


def _finalize2(tr, p0, p1, cnt, w0, w1, nv, fc, o0, o1):
    if tr:
        _lib.call('fgnn_gn_finalize2_tpg', _lib.ptr(p0), _lib.ptr(p1), _lib.ptr(cnt), _lib.ptr(w0), _lib.ptr(w1), _lib.ptr(nv), fc['G'],
                  fc['C'], fc['N'], fc['tpg'], EPS, o0.ptr, o1.ptr, _lib.stream_ptr())
    else:
        _lib.call('fgnn_gn_finalize2', _lib.ptr(p0), _lib.ptr(p1), _lib.ptr(cnt), _lib.ptr(w0), _lib.ptr(w1), _lib.ptr(nv), fc['G'],
                  fc['C'], fc['N'], EPS, o0.ptr, o1.ptr, _lib.stream_ptr())


def _check_finalize(fc):
    """all of one input set: both partial sets, with and without weights, single launches twice, the paired launch"""
    tr, G, Cc = fc['tr'], fc['G'], fc['C']
    assert _lib.load().fgnn_tiles_per_graph(fc['N']) == fc['tpg'] or tr
    parts = [fc['parts'][k].part(tr) for k in (0, 1)]
    pd = [dev(p) for p in parts]
    cnt, nv = dev(fc['cnt']), dev(fc['nvalid'], np.int32)
    ws = (fc['w'], np.ascontiguousarray(fc['w'][::-1]))
    worst = 0.0
    for weighted in (True, False):
        wd = [dev(w) if weighted else None for w in ws]
        single = []
        for k in (0, 1):
            o, again = Out(G * Cc * 4), Out(G * Cc * 4)
            _finalize(tr, pd[k], cnt, wd[k], nv, fc, o)
            _finalize(tr, pd[k], cnt, wd[k], nv, fc, again)
            got = o.read()
            assert np.array_equal(bits(got), bits(again.read())), 'a second launch differs'
            ref = R.finalize_ref(parts[k], fc['cnt'], fc['nvalid'], fc['N'], tr, Cc, ws[k] if weighted else None)
            bnd = R.record_bounds(ref, R.finalize_K(fc['tpg']))
            got = got.reshape(G, Cc, 4)
            for i, f in enumerate(FIELDS):
                worst = max(worst, R.within(got[..., i], ref[f], bnd[f], 'finalize tr=%d set %d weighted=%s %s' % (tr, k, weighted, f)))
            for g, n in enumerate(R.nv_list(G, fc['N'], fc['nvalid'])):
                if n == 0:
                    assert (got[g, :, :3] == 0).all(), 'an empty graph must give mean = a = q = 0'
            single.append(got)
        o0, o1 = Out(G * Cc * 4), Out(G * Cc * 4)
        _finalize2(tr, pd[0], pd[1], cnt, wd[0], wd[1], nv, fc, o0, o1)
        assert np.array_equal(bits(o0.read()), bits(single[0]).reshape(-1)), 'finalize2 differs from finalize (first set)'
        assert np.array_equal(bits(o1.read()), bits(single[1]).reshape(-1)), 'finalize2 differs from finalize (second set)'
    return worst


@pytest.mark.parametrize('gc', R.FIN_GC)
@pytest.mark.parametrize('tr,size', [(0, n) for n in R.FIN_N] + [(1, t) for t in R.FIN_TPG])
def test_finalize_records_against_fp64(tr, size, gc):
    """fgnn_gn_finalize / fgnn_gn_finalize2 (fp32 tile layout, size = N) and fgnn_gn_finalize_tpg / fgnn_gn_finalize2_tpg
    (size = tpg): every field of every record within its bound of finalize_ref, dense and ragged (dead and partly filled
    tiles, empty graphs), with gn_weight and with NULL; finalize2 = two finalize launches and relaunches bit for bit."""
    worst = max(_check_finalize(R.finalize_case(size, gc, ragged, tr)) for ragged in (False, True))
    note('finalize', worst)


@pytest.mark.parametrize('tr,size', [(0, 46), (0, 129), (0, 200), (1, 1250)])
def test_finalize_of_shifted_data_keeps_r2(tr, size):
    """mean 1000, std 0.01: the error of the mean enters M2 as m eps_mean^2, which dominates the bound of r2 here"""
    worst = max(_check_finalize(R.finalize_case(size, 15, ragged, tr, True)) for ragged in (False, True))
    note('finalize-shift', worst)


# ------------------------------------------------------------------------------------------------------------ coefficient tiles
@pytest.mark.parametrize('gc', R.FIN_GC)
@pytest.mark.parametrize('tr,size', [(0, n) for n in R.FIN_N] + [(1, t) for t in R.FIN_TPG])
def test_coefficient_tiles_against_fp64(tr, size, gc):
    """fgnn_gn_bwd_coef_tiles / fgnn_gn_bwd_coef_tiles_tpg: s12 against the fp64 sums of the per-tile partials (random
    signs), coef against coef_ref; an empty graph gives zero z and w fields."""
    worst = 0.0
    for ragged in (False, True):
        sc = R.s12_case(size, gc, ragged, tr)
        fc = sc['fc']
        G, Cc, tpg, N = fc['G'], fc['C'], fc['tpg'], fc['N']
        part = sc['s12'].part(tr)
        s12, coef = Out(G * Cc * 2), Out(G * Cc * 4)
        pd, nd, nvd = dev(part), dev(sc['nrm']), dev(fc['nvalid'], np.int32)
        args = (_lib.ptr(pd), _lib.ptr(nd), _lib.ptr(nvd), G, Cc, N)
        if tr:
            _lib.call('fgnn_gn_bwd_coef_tiles_tpg', *args, tpg, s12.ptr, coef.ptr, _lib.stream_ptr())
        else:
            _lib.call('fgnn_gn_bwd_coef_tiles', *args, s12.ptr, coef.ptr, _lib.stream_ptr())
        S1, S2, A1, A2 = R.s12_of_tiles(part, tr, G, Cc, tpg)
        L = (tpg + 63) // 64
        d1, d2 = R.wave_sum_bound(L, A1), R.wave_sum_bound(L, A2)
        rec = R.nrm_as_rec(sc['nrm'])
        want = R.coef_ref(S1, S2, rec, fc['nvalid'], N)
        bz, bw = R.coef_bounds(want, rec, d1, d2, fc['nvalid'], N)
        got_s, got_c = s12.read().reshape(G, Cc, 2), coef.read().reshape(G, Cc, 4)
        tag = 'coef tiles tr=%d ragged=%s ' % (tr, ragged)
        worst = max(worst, R.within(got_s[..., 0], S1, d1, tag + 'S1'), R.within(got_s[..., 1], S2, d2, tag + 'S2'),
                    R.within(got_c[..., 2], want[..., 2], bz, tag + 'z'), R.within(got_c[..., 3], want[..., 3], bw, tag + 'w'))
        assert np.array_equal(bits(got_c[..., :2]), bits(sc['nrm'][..., :2])), 'mean and a are copied from the record'
        for g, n in enumerate(R.nv_list(G, N, fc['nvalid'])):
            if n == 0:
                assert (got_c[g, :, 2:] == 0).all()
    note('coef-tiles', worst)


# ------------------------------------------------------------------------------------------------------------ grad_finalize
def _job(jobs, i, **kw):
    for k, v in kw.items():
        setattr(jobs[i], k, v.data_ptr() if isinstance(v, torch.Tensor) else v)


@pytest.mark.parametrize('launch', range(4))
def test_grad_finalize_column_sums_against_fp64(launch):
    """fgnn_grad_finalize: sixteen jobs of different row and column counts in one launch, every out[i] within the reduce_cols
    bound of scale * sum_r in[r][i]; rows = 0 means num_wg, scale = 0 means 1, scale_dev is multiplied in; the surplus column
    blocks of the narrower jobs write nothing (guards); a job without s12 leaves its dgn buffers alone; where the arguments
    coincide the sums equal fgnn_reduce_partials / fgnn_sum_scale bit for bit."""
    spec = R.reduce_launches()[launch]
    jobs = (_lib.GradJob * len(spec))()
    sdev = dev(np.array([R.RED_SCALE_DEV]))
    ins, outs, keep = [], [], []
    dgw, dgb = Out(8), Out(8)
    for i, j in enumerate(spec):
        ins.append(dev(j['inp']))
        outs.append(Out(j['count']))
        _job(jobs, i, wpart=ins[i], count=j['count'], out=outs[i].t, rows=j['rows'], scale=j['scale'], dgn_w=dgw.t, dgn_b=dgb.t)
        if j['dev']:
            _job(jobs, i, scale_dev=sdev)
    _lib.call('fgnn_grad_finalize', jobs, len(spec), R.RED_NUM_WG, 2, 4, _lib.stream_ptr())
    dgw.read(np.zeros(8, dtype=bool))
    dgb.read(np.zeros(8, dtype=bool))
    worst = 0.0
    for i, j in enumerate(spec):
        rows = j['rows'] or R.RED_NUM_WG
        assert j['inp'].shape == (rows, j['count'])
        scale = (j['scale'] or 1.0) * (float(np.float32(R.RED_SCALE_DEV)) if j['dev'] else 1.0)
        ref, ab = R.reduce_ref(j['inp'], scale)
        got = outs[i].read()
        worst = max(worst, R.within(got, ref, R.reduce_bound(rows, ab), 'grad_finalize job %d rows=%d count=%d' % (i, rows, j['count'])))
        if not j['dev']:
            same = Out(j['count'])
            if j['scale'] in (0.0, 1.0):
                _lib.call('fgnn_reduce_partials', _lib.ptr(ins[i]), rows, j['count'], same.ptr, _lib.stream_ptr())
            else:
                _lib.call('fgnn_sum_scale', _lib.ptr(ins[i]), rows, j['count'], j['scale'], same.ptr, _lib.stream_ptr())
            assert np.array_equal(bits(same.read()), bits(got)), 'job %d differs from the stand-alone reduction' % i
    note('reduce-cols', worst)


def test_grad_finalize_takes_sixteen_jobs_and_refuses_seventeen():
    a = dev(np.ones((3, 5)))
    for n in (16, 17):
        jobs = (_lib.GradJob * n)()
        outs = [Out(5) for _ in range(n)]
        for i in range(n):
            _job(jobs, i, wpart=a, count=5, out=outs[i].t, rows=3, scale=0.0)
        if n == 16:
            _lib.call('fgnn_grad_finalize', jobs, n, 3, 1, 1, _lib.stream_ptr())
            for o in outs:
                assert (o.read() == 3).all()
        else:
            with pytest.raises(RuntimeError):
                _lib.call('fgnn_grad_finalize', jobs, n, 3, 1, 1, _lib.stream_ptr())
            torch.cuda.synchronize()
            for o in outs:
                o.read(np.zeros(5, dtype=bool))


@pytest.mark.parametrize('Cc', R.AFF_C)
def test_affine_gradients_against_fp64(Cc):
    """the affine block of fgnn_grad_finalize and fgnn_gn_bwd_coef's affine launch against affine_ref, for graph counts on
    either side of the eight accumulation groups and channel counts on either side of the 32-channel chunk; only dgn_w or
    only dgn_b given writes only that one."""
    worst = 0.0
    for G in R.AFF_G:
        nrm, s12 = R.affine_case(G, Cc)
        dgw, dgb, aw, ab = R.affine_ref(nrm[..., 2], s12[..., 0], s12[..., 1])
        bw, bb = R.affine_bound(G, aw), R.affine_bound(G, ab)
        nd, sd = dev(nrm), dev(s12)
        part = dev(np.ones((2, 70)))
        jobs = (_lib.GradJob * 2)()
        ow, ob, o0, o1, uw, ub = Out(Cc), Out(Cc), Out(70), Out(3), Out(Cc), Out(Cc)
        _job(jobs, 0, wpart=part, count=70, out=o0.t, s12=sd, nrm=nd, dgn_w=ow.t, dgn_b=ob.t)
        _job(jobs, 1, wpart=part, count=3, out=o1.t, dgn_w=uw.t, dgn_b=ub.t)          # no s12: its dgn buffers stay untouched
        _lib.call('fgnn_grad_finalize', jobs, 2, 2, G, Cc, _lib.stream_ptr())
        gw, gb = ow.read(), ob.read()
        worst = max(worst, R.within(gw, dgw, bw, 'grad_finalize dgn_w G=%d C=%d' % (G, Cc)), R.within(gb, dgb, bb, 'grad_finalize dgn_b G=%d' % G))
        assert (o0.read() == 2).all() and (o1.read() == 2).all()
        uw.read(np.zeros(Cc, dtype=bool))
        ub.read(np.zeros(Cc, dtype=bool))
        for give_w, give_b in ((True, False), (False, True)):
            cw, cb, coef = Out(Cc), Out(Cc), Out(G * Cc * 4)
            _lib.call('fgnn_gn_bwd_coef', _lib.ptr(sd), _lib.ptr(nd), None, G, Cc, 3, coef.ptr, cw.ptr if give_w else None,
                      cb.ptr if give_b else None, _lib.stream_ptr())
            hw, hb = cw.read(np.full(Cc, give_w)), cb.read(np.full(Cc, give_b))
            worst = max(worst, R.within(hw, dgw, bw, 'gn_bwd_coef dgn_w') if give_w else R.within(hb, dgb, bb, 'gn_bwd_coef dgn_b'))
            S1, S2 = s12[..., 0].astype(np.float64), s12[..., 1].astype(np.float64)
            rec = R.nrm_as_rec(nrm)
            want = R.coef_ref(S1, S2, rec, None, 3)
            bz, bwd = R.coef_bounds(want, rec, np.zeros_like(S1), np.zeros_like(S2), None, 3)
            got = coef.read().reshape(G, Cc, 4)
            R.within(got[..., 2], want[..., 2], bz, 'gn_bwd_coef z')
            R.within(got[..., 3], want[..., 3], bwd, 'gn_bwd_coef w')
    note('affine', worst)


# ------------------------------------------------------------------------------------------------------------ two-pass / plane
class Slab:
    """a (G, C, N, N) tensor on the device at plane pitch ldp and graph stride gs, every other cell NaN"""

    def __init__(self, G, Cc, N, strided, a=None):
        self.G, self.C, self.N, self.P = G, Cc, N, N * N
        self.ldp = self.P + 7 if strided else self.P
        self.gs = Cc * self.ldp + 5 if strided else Cc * self.P
        self.o = Out(G * self.gs)
        self.cells = (np.arange(G)[:, None, None] * self.gs + np.arange(Cc)[None, :, None] * self.ldp + np.arange(self.P)[None, None, :]).reshape(-1)
        if a is not None:
            self.o.t[torch.from_numpy(self.cells).to(DEV)] = torch.from_numpy(np.array(a, dtype=np.float32).reshape(-1)).to(DEV)

    @property
    def ptr(self):
        return self.o.ptr

    def read(self):
        """(G, C, N, N), after checking the guards, that every plane cell was written and no cell between the planes was"""
        w = np.zeros(self.o.n, dtype=bool)
        w[self.cells] = True
        return self.o.read(w)[self.cells].reshape(self.G, self.C, self.N, self.N)


def _padding(G, N, nv):
    m = np.ones((G, 1, N, N), dtype=bool)
    for g, n in enumerate(R.nv_list(G, N, nv)):
        m[g, :, :n, :n] = False
    return m


def _slab_refs(sc, affine):
    w, b = (sc['w'], sc['b']) if affine else (None, None)
    y, rec = R.norm_fwd_ref(sc['x'], sc['nvalid'], w, b)
    return w, b, y, rec, R.norm_bwd_ref(sc['dy'], sc['x'], rec, sc['nvalid'])


def _check_record(got, rec, rb, tag):
    return max(R.within(got[..., i], rec[f], rb[f], tag + ' ' + f) for i, f in enumerate(FIELDS))


@pytest.mark.parametrize('name,ragged,strided,affine', R.SLAB_VARIANTS)
@pytest.mark.parametrize('N', R.TWO_PASS_N)
def test_two_pass_kernels_against_fp64(N, name, ragged, strided, affine):
    """fgnn_gn_stats, _apply, _bwd_stats, _bwd_coef and _bwd_apply above N = 64 (the unrolled dense loops with a tail), on
    ragged batches with an empty graph, on strided slabs and with NULL gn_weight / beta / nvalid: record, y, s12 and dz
    elementwise against fp64, exact zeros in the padding, nothing written between the planes."""
    sc = R.slab_case(N, ragged)
    G, Cc, nv = sc['G'], sc['C'], sc['nvalid']
    w, b, y_ref, rec, bw = _slab_refs(sc, affine)
    adds = [R.stats_adds(N, n) for n in R.nv_list(G, N, nv)]
    rb = R.record_bounds(rec, np.asarray(adds) + 8)
    x, dy = Slab(G, Cc, N, strided, sc['x']), Slab(G, Cc, N, strided, sc['dy'])
    y, dz = Slab(G, Cc, N, strided), Slab(G, Cc, N, strided)
    wd, bd, nvd, st = dev(w), dev(b), dev(nv, np.int32), _lib.stream_ptr()
    nrm, s12, coef = Out(G * Cc * 4), Out(G * Cc * 2), Out(G * Cc * 4)
    assert _lib.load().fgnn_gn_plane_supported(N) == 0
    _lib.call('fgnn_gn_stats', x.ptr, x.gs, x.ldp, _lib.ptr(wd), _lib.ptr(nvd), G, Cc, N, EPS, nrm.ptr, st)
    _lib.call('fgnn_gn_apply', x.ptr, x.gs, x.ldp, nrm.ptr, _lib.ptr(bd), _lib.ptr(nvd), G, Cc, N, y.ptr, y.gs, y.ldp, st)
    _lib.call('fgnn_gn_bwd_stats', dy.ptr, dy.gs, dy.ldp, x.ptr, x.gs, x.ldp, nrm.ptr, _lib.ptr(nvd), G, Cc, N, s12.ptr, st)
    _lib.call('fgnn_gn_bwd_coef', s12.ptr, nrm.ptr, _lib.ptr(nvd), G, Cc, N, coef.ptr, None, None, st)
    _lib.call('fgnn_gn_bwd_apply', dy.ptr, dy.gs, dy.ldp, x.ptr, x.gs, x.ldp, coef.ptr, _lib.ptr(nvd), G, Cc, N, dz.ptr, dz.gs, dz.ldp, st)
    worst = _check_record(nrm.read().reshape(G, Cc, 4), rec, rb, 'gn_stats N=%d %s' % (N, name))
    got_y, got_dz = y.read(), dz.read()
    worst = max(worst, R.within(got_y, y_ref, R.y_bound(sc['x'], y_ref, rec, rb), 'gn_apply N=%d %s' % (N, name)),
                R.within(got_dz, bw['dz'], R.dz_bound(sc['dy'], sc['x'], rec, rb, bw, adds), 'gn_bwd_apply N=%d %s' % (N, name)))
    pad = np.broadcast_to(_padding(G, N, nv), got_y.shape)
    assert (got_y[pad] == 0).all() and (got_dz[pad] == 0).all()
    # s12 against the fp64 sums formed with the record the kernel was given
    nrm_np = nrm.read().reshape(G, Cc, 4)
    own = R.norm_bwd_ref(sc['dy'], sc['x'], R.nrm_as_rec(nrm_np), nv)
    got_s = s12.read().reshape(G, Cc, 2)
    a8 = np.asarray(adds, dtype=np.float64).reshape(-1, 1)
    worst = max(worst, R.within(got_s[..., 0], own['S1'], R.wave_sum_bound(a8, own['A1']), 'gn_bwd_stats S1'),
                R.within(got_s[..., 1], own['S2'], R.wave_sum_bound(a8, own['A2']), 'gn_bwd_stats S2'))
    x.read(), dy.read()              # the inputs are still what they were: nothing was written into them
    note('two-pass', worst)
    for entry in ('fgnn_gn_plane_fwd', 'fgnn_gn_plane_bwd'):
        o = Out(G * Cc * 4)
        with pytest.raises(RuntimeError):
            if entry == 'fgnn_gn_plane_fwd':
                _lib.call(entry, x.ptr, x.gs, x.ldp, None, None, None, G, Cc, N, EPS, y.ptr, y.gs, y.ldp, o.ptr, st)
            else:
                _lib.call(entry, dy.ptr, dy.gs, dy.ldp, x.ptr, x.gs, x.ldp, nrm.ptr, None, G, Cc, N, dz.ptr, dz.gs, dz.ldp, o.ptr, None, None, st)
        o.read(np.zeros(o.n, dtype=bool))


@pytest.mark.parametrize('name,ragged,strided,affine', R.SLAB_VARIANTS)
@pytest.mark.parametrize('N', R.PLANE_N)
def test_plane_kernels_against_fp64(N, name, ragged, strided, affine):
    """fgnn_gn_plane_fwd / _bwd at N = 1 and on strided slabs, empty graphs and NULL parameters at N = 33: record, y, s12, dz
    and the affine gradients elementwise against fp64."""
    sc = R.slab_case(N, ragged)
    G, Cc, nv = sc['G'], sc['C'], sc['nvalid']
    w, b, y_ref, rec, bw = _slab_refs(sc, affine)
    rb = R.record_bounds(rec, R.PLANE_ADDS + 8)
    x, dy = Slab(G, Cc, N, strided, sc['x']), Slab(G, Cc, N, strided, sc['dy'])
    y, dz = Slab(G, Cc, N, strided), Slab(G, Cc, N, strided)
    wd, bd, nvd, st = dev(w), dev(b), dev(nv, np.int32), _lib.stream_ptr()
    nrm, s12, dgw, dgb = Out(G * Cc * 4), Out(G * Cc * 2), Out(Cc), Out(Cc)
    assert _lib.load().fgnn_gn_plane_supported(N) == 1
    _lib.call('fgnn_gn_plane_fwd', x.ptr, x.gs, x.ldp, _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(nvd), G, Cc, N, EPS, y.ptr, y.gs, y.ldp, nrm.ptr, st)
    _lib.call('fgnn_gn_plane_bwd', dy.ptr, dy.gs, dy.ldp, x.ptr, x.gs, x.ldp, nrm.ptr, _lib.ptr(nvd), G, Cc, N, dz.ptr, dz.gs, dz.ldp,
              s12.ptr, dgw.ptr, dgb.ptr, st)
    nrm_np = nrm.read().reshape(G, Cc, 4)
    worst = _check_record(nrm_np, rec, rb, 'gn_plane_fwd N=%d %s' % (N, name))
    got_y, got_dz = y.read(), dz.read()
    worst = max(worst, R.within(got_y, y_ref, R.y_bound(sc['x'], y_ref, rec, rb), 'gn_plane_fwd y N=%d %s' % (N, name)),
                R.within(got_dz, bw['dz'], R.dz_bound(sc['dy'], sc['x'], rec, rb, bw, R.PLANE_ADDS), 'gn_plane_bwd dz N=%d %s' % (N, name)))
    pad = np.broadcast_to(_padding(G, N, nv), got_y.shape)
    assert (got_y[pad] == 0).all() and (got_dz[pad] == 0).all()
    own = R.norm_bwd_ref(sc['dy'], sc['x'], R.nrm_as_rec(nrm_np), nv)
    got_s = s12.read().reshape(G, Cc, 2)
    worst = max(worst, R.within(got_s[..., 0], own['S1'], R.wave_sum_bound(R.PLANE_ADDS, own['A1']), 'gn_plane_bwd S1'),
                R.within(got_s[..., 1], own['S2'], R.wave_sum_bound(R.PLANE_ADDS, own['A2']), 'gn_plane_bwd S2'))
    # the affine gradients are affine_reduce of the kernel's own q and s12
    aw, ab, sw, sb = R.affine_ref(nrm_np[..., 2], got_s[..., 0], got_s[..., 1])
    worst = max(worst, R.within(dgw.read(), aw, R.affine_bound(G, sw), 'gn_plane_bwd dgn_w'), R.within(dgb.read(), ab, R.affine_bound(G, sb), 'gn_plane_bwd dgn_b'))
    x.read(), dy.read()
    note('plane', worst)
