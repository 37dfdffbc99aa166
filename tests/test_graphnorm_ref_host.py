"""CPU: the fp64 GraphNorm restatement of tests/graphnorm_ref.py against the direct definition and fp64 autograd, and its error
bounds against a float32 emulation of the kernels' summation order on every input set of tests/test_gpu_graphnorm.py -- the
bounds must be attainable by a correct float32 implementation before any kernel is held to them."""
import numpy as np
import pytest
import torch

import graphnorm_ref as R

SAFETY, _within = R.SAFETY, R.within
FIELDS = ('mean', 'a', 'q', 'r2')


@pytest.mark.parametrize('T,pitch_extra', [(32, 0), (64, 0), (64, 5)])
@pytest.mark.parametrize('N,nvalid', [(8, None), (13, None), (46, None), (13, [13, 6, 1, 0]), (46, [23, 0, 46, 1]), (1, [1, 0])])
def test_finalize_of_the_tile_partials_is_the_direct_mean_and_variance(N, nvalid, T, pitch_extra):
    """finalize_ref(tile_partials(x)) in fp64 equals the mean / biased variance of x over the valid corner to 1e-12, in both
    tile layouts and storage orders, with vertex counts of 0 and 1."""
    G, C = (len(nvalid) if nvalid else 2), 3
    x = R._data(N * 10 + T + pitch_extra, G, C, N)
    w = np.linspace(0.5, 1.5, C)
    p = R.tile_partials(x, nvalid, T, N + pitch_extra, dtype=np.float64)
    assert p.tpg == -(-N * (N + pitch_extra) // T)
    want = R.direct_ref(x, nvalid, w)
    for tr in (0, 1):
        got = R.finalize_ref(p.part(tr), p.cnt, nvalid, N, tr, C, w)
        for f in FIELDS + ('M2', 'm'):
            assert np.allclose(got[f], want[f], rtol=1e-12, atol=1e-12 * np.abs(want[f]).max()), (f, tr)
    for g, n in enumerate(R.nv_list(G, N, nvalid)):
        if n == 0:
            assert (want['q'][g] == 0).all() and (want['a'][g] == 0).all() and (want['mean'][g] == 0).all()
            assert (p.cnt[g] == 0).all() and (p.mean_t[g] == 0).all() and (p.m2_t[g] == 0).all()
    # dead tiles are {0, 0} with count 0, every valid element is counted once
    assert ((p.cnt == 0)[:, None, :] <= ((p.mean_t == 0) & (p.m2_t == 0))).all()
    assert np.array_equal(p.cnt.sum(-1), np.array([n * n for n in R.nv_list(G, N, nvalid)], dtype=np.float64))


@pytest.mark.parametrize('N,nvalid', [(7, None), (12, [12, 5, 1, 0])])
def test_coefficients_and_affine_sums_are_the_fp64_autograd(N, nvalid):
    """coef_ref / affine_ref against torch autograd in fp64 of w (x - mean) / (2 sqrt(n (var + eps))) + b
    (models/layers.py:71-80): dz, dw and db."""
    G, C = (len(nvalid) if nvalid else 3), 4
    x, dy = R._data(N, G, C, N), R._data(N + 1, G, C, N)
    w, b = np.linspace(0.5, 1.5, C), np.linspace(-1, 1, C)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    wt, bt = torch.from_numpy(w).requires_grad_(True), torch.from_numpy(b).requires_grad_(True)
    ys = []
    for g, n in enumerate(R.nv_list(G, N, nvalid)):
        xb = xt[g, :, :n, :n]
        if n == 0:
            ys.append(torch.zeros(C, N, N, dtype=torch.float64))
            continue
        mean = xb.mean((-1, -2), keepdim=True)
        var = ((xb - mean) ** 2).mean((-1, -2), keepdim=True)
        yb = wt[:, None, None] * (xb - mean) / (2 * torch.sqrt(n * (var + R.EPS))) + bt[:, None, None]
        ys.append(torch.nn.functional.pad(yb, (0, N - n, 0, N - n)))
    yt = torch.stack(ys)
    yt.backward(torch.from_numpy(dy).double())
    y, rec = R.norm_fwd_ref(x, nvalid, w, b)
    assert np.allclose(y, yt.detach().numpy(), rtol=1e-12, atol=1e-12)
    bw = R.norm_bwd_ref(dy, x, rec, nvalid)
    assert np.allclose(bw['dz'], xt.grad.numpy(), rtol=1e-10, atol=1e-12)
    dgw, dgb, _, _ = R.affine_ref(rec['q'], bw['S1'], bw['S2'])
    assert np.allclose(dgw, wt.grad.numpy(), rtol=1e-10, atol=1e-12)
    assert np.allclose(dgb, bt.grad.numpy(), rtol=1e-10, atol=1e-12)
    # the same S1 / S2 from per-tile partials in both storage orders
    p = R.Partials(*(np.random.default_rng(3).standard_normal((G, C, 9)) for _ in range(2)), None)
    for tr in (0, 1):
        s1, s2, a1, a2 = R.s12_of_tiles(p.part(tr), tr, G, C, 9)
        assert np.allclose(s1, p.mean_t.sum(-1)) and np.allclose(s2, p.m2_t.sum(-1))
        assert np.allclose(a1, np.abs(p.mean_t).sum(-1)) and np.allclose(a2, np.abs(p.m2_t).sum(-1))
    out, ab = R.reduce_ref(np.arange(12.0).reshape(3, 4) - 5, -0.5)
    assert np.array_equal(out, -0.5 * np.array([-3.0, 0, 3, 6])) and np.array_equal(ab, 0.5 * np.array([9.0, 8, 9, 10]))


def test_the_butterfly_emulation_sums_every_lane_once():
    v = np.random.default_rng(0).integers(-1000, 1000, (5, 64)).astype(np.float32)
    assert np.array_equal(R.emu_wave_sum(v), v.sum(-1))           # integers: exact in any order
    t = np.random.default_rng(1).integers(-100, 100, (3, 1250)).astype(np.float32)
    assert np.array_equal(R.emu_lane_sum(t), t.sum(-1))
    assert np.array_equal(R.emu_plane_sum(t), t.sum(-1))
    assert np.array_equal(R.emu_reduce_cols(t.T.copy(), 2.0), 2 * t.sum(-1))


def _check_finalize(size, gc, ragged, tr, shift=False):
    fc = R.finalize_case(size, gc, ragged, tr, shift)
    worst = 0.0
    for k in (0, 1):
        part = fc['parts'][k].part(tr)
        for w in (fc['w'], None):
            ref = R.finalize_ref(part, fc['cnt'], fc['nvalid'], fc['N'], tr, fc['C'], w)
            bnd = R.record_bounds(ref, R.finalize_K(fc['tpg']))
            got = R.emu_finalize(part, fc['cnt'], fc['nvalid'], fc['N'], tr, fc['C'], w)
            for i, f in enumerate(FIELDS):
                worst = max(worst, _within(got[..., i], ref[f], bnd[f], 'finalize %s %s' % ((size, gc, ragged, tr, shift), f)))
    return worst


@pytest.mark.parametrize('tr,size', [(0, n) for n in R.FIN_N] + [(1, t) for t in R.FIN_TPG])
def test_float32_finalize_stays_inside_its_bounds(tr, size):
    """the emulated gn_finalize_kernel on every finalize input set of the GPU tests, and the tile counts they rely on"""
    for gc in R.FIN_GC:
        for ragged in (False, True):
            fc = R.finalize_case(size, gc, ragged, tr)
            assert fc['G'] * fc['C'] == gc and fc['tpg'] == (size if tr else -(-size * size // 32))
            assert _check_finalize(size, gc, ragged, tr) <= SAFETY


def test_float32_finalize_of_shifted_data_stays_inside_its_bounds():
    """mean 1000, std 0.01: the m eps_mean^2 term carries the bound of r2"""
    for tr, size in ((0, 46), (0, 129), (0, 200), (1, 1250)):
        for ragged in (False, True):
            assert _check_finalize(size, 15, ragged, tr, shift=True) <= SAFETY
            fc = R.finalize_case(size, 15, ragged, tr, True)
            ref = R.finalize_ref(fc['parts'][0].part(tr), fc['cnt'], fc['nvalid'], fc['N'], tr, fc['C'])
            K = R.finalize_K(fc['tpg'])
            live = ref['m'] > 1
            assert (ref['m'] * (K * R.U * ref['mabs']) ** 2 > (K + 4) * R.U * ref['M2'])[live].all()


@pytest.mark.parametrize('tr,size', [(0, n) for n in R.FIN_N] + [(1, t) for t in R.FIN_TPG])
def test_float32_coefficient_tiles_stay_inside_their_bounds(tr, size):
    for gc in R.FIN_GC:
        for ragged in (False, True):
            sc = R.s12_case(size, gc, ragged, tr)
            fc = sc['fc']
            G, C, tpg, L = fc['G'], fc['C'], fc['tpg'], (fc['tpg'] + 63) // 64
            part = sc['s12'].part(tr)
            S1, S2, A1, A2 = R.s12_of_tiles(part, tr, G, C, tpg)
            d1, d2 = R.wave_sum_bound(L, A1), R.wave_sum_bound(L, A2)
            rec = R.nrm_as_rec(sc['nrm'])
            coef = R.coef_ref(S1, S2, rec, fc['nvalid'], fc['N'])
            bz, bw = R.coef_bounds(coef, rec, d1, d2, fc['nvalid'], fc['N'])
            s1, s2, got = R.emu_coef_tiles(part, sc['nrm'], fc['nvalid'], fc['N'], tr, G, C, tpg)
            tag = 'coef tiles %s' % ((size, gc, ragged, tr),)
            _within(s1, S1, d1, tag + ' S1')
            _within(s2, S2, d2, tag + ' S2')
            _within(got[..., 2], coef[..., 2], bz, tag + ' z')
            _within(got[..., 3], coef[..., 3], bw, tag + ' w')
            assert np.array_equal(got[..., :2], sc['nrm'][..., :2])


def test_float32_column_sums_stay_inside_their_bounds():
    for jobs in R.reduce_launches():
        assert len(jobs) == 16 and len({j['count'] for j in jobs}) > 1
        for j in jobs:
            scale = (j['scale'] or 1.0) * (float(np.float32(R.RED_SCALE_DEV)) if j['dev'] else 1.0)
            ref, ab = R.reduce_ref(j['inp'], scale)
            got = R.emu_reduce_cols(j['inp'], j['scale'], np.float32(R.RED_SCALE_DEV) if j['dev'] else None)
            _within(got, ref, R.reduce_bound(j['inp'].shape[0], ab), 'reduce_cols rows=%d count=%d' % (j['rows'], j['count']))
    assert {(j['rows'], j['count']) for jobs in R.reduce_launches() for j in jobs} >= {(r, c) for r in R.RED_ROWS for c in R.RED_COUNTS}


def test_float32_affine_sums_stay_inside_their_bounds():
    for C in R.AFF_C:
        for G in R.AFF_G:
            nrm, s12 = R.affine_case(G, C)
            dgw, dgb, aw, ab = R.affine_ref(nrm[..., 2], s12[..., 0], s12[..., 1])
            w, b = R.emu_affine(nrm[..., 2], s12[..., 0], s12[..., 1])
            _within(w, dgw, R.affine_bound(G, aw), 'affine dgw G=%d C=%d' % (G, C))
            _within(b, dgb, R.affine_bound(G, ab), 'affine dgb G=%d C=%d' % (G, C))


@pytest.mark.parametrize('N', R.TWO_PASS_N + R.PLANE_N)
def test_float32_two_pass_and_plane_chains_stay_inside_their_bounds(N):
    """statistics -> apply -> backward statistics -> coefficients -> backward apply in float32, held to the composed y and dz
    bounds elementwise; the plane kernels' order too where they run (N * N <= 4096)"""
    for _, ragged, _, affine in R.SLAB_VARIANTS:
        sc = R.slab_case(N, ragged)
        w, b = (sc['w'], sc['b']) if affine else (None, None)
        nv = sc['nvalid']
        y, rec = R.norm_fwd_ref(sc['x'], nv, w, b)
        bw = R.norm_bwd_ref(sc['dy'], sc['x'], rec, nv)
        chains = [('two-pass', [R.stats_adds(N, n) for n in R.nv_list(sc['G'], N, nv)], R.emu_stats, R.emu_bwd_stats)]
        if N * N <= 4096:
            chains.append(('plane', R.PLANE_ADDS, R.emu_plane_fwd, R.emu_plane_bwd_stats))
        for name, adds, fwd, bwd_stats in chains:
            rb = R.record_bounds(rec, np.asarray(adds) + 8)
            nrm = fwd(sc['x'], nv, w)
            for i, f in enumerate(FIELDS):
                _within(nrm[..., i], rec[f], rb[f], '%s N=%d %s' % (name, N, f))
            _within(R.emu_apply(sc['x'], nrm, b, nv), y, R.y_bound(sc['x'], y, rec, rb), '%s N=%d y' % (name, N))
            s1, s2 = bwd_stats(sc['dy'], sc['x'], nrm, nv)
            coef = R.emu_coef(s1, s2, nrm, nv, N)
            dz = R.emu_bwd_apply(sc['dy'], sc['x'], coef, nv)
            _within(dz, bw['dz'], R.dz_bound(sc['dy'], sc['x'], rec, rb, bw, adds), '%s N=%d dz' % (name, N))
