"""CPU: tests/matmul32_ref.py on its own -- the exactness precondition at every shape the GPU file uses, the fp32 emulation of
the products inside the derived bound, the fill = 1 frame against the consumer it is made for, and the checkers against
host-made wrong answers (the suite's mutation check: no GPU, no modified kernel)."""
import numpy as np
import pytest

import matmul32_ref as R

ALL = R.SHAPES + R.ODD + R.FIN
EMU = [s for s in ALL if s[1] is None or s[0] in (33, 64, 96, 200)]           # every dense N, some ragged ones
IDS = dict(ids=R.shape_id)


@pytest.mark.parametrize('shape', sorted(set(ALL), key=str), **IDS)
def test_grid_precondition(shape):
    """Every partial sum of every product, and of S1 / S2, is an integer number of units below 2^24 (grid_case asserts the
    products itself); the entry ranges keep the S sums exact at every shape, so no GPU case falls back to the bound."""
    c = R.case('grid', *shape)
    assert max(c['load'].values()) < R.GRID_LIMIT and c['s_exact'], c['load']
    for name in ('M', 'dA', 'dB', 's12a', 's12b'):
        assert np.array_equal(c[name].astype(np.float32).astype(np.float64), c[name]), name      # the cast is lossless
    nvmax = int(c['nv'].max())
    assert nvmax == 0 or np.abs(c['dA']).max() > 0


EMU_RATIO = {}


@pytest.mark.parametrize('interleave', (False, True), ids=('sequential', 'pairs'))
@pytest.mark.parametrize('shape', sorted(set(EMU), key=str), **IDS)
def test_fp32_emulation_is_inside_the_bound(shape, interleave):
    c = R.case('random', *shape)
    emu = R.emulate(c, interleave)
    for name in ('M', 'dA', 'dB'):
        ratio = np.abs(emu[name].astype(np.float64) - c[name]) / c['bound'][name]
        r = float(ratio[R._corner(c)].max(initial=0.0))
        key = (name, 'N<=64' if shape[0] <= 64 else 'N<=128' if shape[0] <= 128 else 'N<=256' if shape[0] <= 256 else 'N>256')
        EMU_RATIO[key] = max(EMU_RATIO.get(key, 0.0), r)
        assert r <= 1.0, (name, shape, r)
    # the emulation on grid data is exact
    g = R.case('grid', *shape)
    emu = R.emulate(g, interleave)
    for name in ('M', 'dA', 'dB'):
        assert np.array_equal(emu[name].astype(np.float64), g[name]), name


def test_emulation_ratio_table():
    """Largest error / bound of the emulation per form (printed with -s; DESIGN.md quotes it).  Runs after the cases above."""
    for key in sorted(EMU_RATIO):
        print('emulation  %-3s %-7s  error / bound <= %.3f' % (key + (EMU_RATIO[key],)))
        assert EMU_RATIO[key] <= 1.0


@pytest.mark.parametrize('N', (65, 96, 127, 128, 129, 200, 255, 256))
def test_fill1_frame_covers_what_a_tile_skipping_consumer_reads(N):
    for nv in sorted({0, 1, 31, 32, 33, 64, 65, 96, 97, 128, 129, N - 1, N} & set(range(N + 1))):
        zm, reach = R.zero_mask(N, nv, 1), R.consumer_reach(N, nv)
        assert not (reach & ~zm).any(), (N, nv, R._first(reach & ~zm))
        assert not zm[:nv, :nv].any()
        full = R.zero_mask(N, nv, 0)
        assert full.sum() == N * N - nv * nv and not (zm & ~full).any()


# ---- the checkers reject wrong answers ------------------------------------------------------------------------------------------
def good(c, fill=0, odd=False):
    st = R.strides(c['N'], c['C'], odd)['out']
    dev = dict(st=st, fill=fill)
    for name in ('M', 'dA', 'dB'):
        dev[name] = R.render(c[name].astype(np.float32), c['nv'], *st, fill=fill)
    dev['s12a'], dev['s12b'] = c['s12a'].astype(np.float32).reshape(-1), c['s12b'].astype(np.float32).reshape(-1)
    return dev


def check(dev, c):
    return (R.check_exact if c['exact'] else R.check_bounded)(dev, c)


MUT_SHAPES = [(33, (33, 32, 31)), (64, None), (64, (64, 33, 1)), (96, (96, 65, 0)), (200, (200, 129, 1)), (257, (200,))]
FAMILIES = ('grid', 'random')


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('shape', MUT_SHAPES, **IDS)
def test_checkers_accept_the_reference(shape, family):
    c = R.case(family, *shape)
    for fill in (0, 1):
        for odd in (False, True):
            check(good(c, fill, odd), c)


def reject(dev, c, what):
    with pytest.raises(R.Mismatch, match=what):
        check(dev, c)


def rerender(dev, c, name, values, fill=0):
    dev[name] = R.render(values.astype(np.float32), c['nv'], *dev['st'], fill=fill)


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('shape', MUT_SHAPES, **IDS)
def test_checkers_reject_wrong_products(shape, family):
    c = R.case(family, *shape)
    Gc, Cc, N, nv = c['G'], c['C'], c['N'], c['nv']
    g = int(np.argmax(nv))
    n = int(nv[g])
    ch = Cc - 1
    # one k-term dropped from ONE element of each product (grid: a k whose term is not zero)
    for name, opA, opB in (('M', c['ya'], c['yb']), ('dA', c['dm'], R._T(c['yb'])), ('dB', R._T(c['ya']), c['dm'])):
        A, B = opA[g, ch, :n, :n], opB[g, ch, :n, :n]
        i, j = next((i, j) for i in range(n - 1, -1, -1) for j in range(n - 1, -1, -1) if (A[i] * B[:, j]).any())
        k = int(np.flatnonzero(A[i] * B[:, j])[-1])
        bad = c[name].copy()
        bad[g, ch, i, j] -= A[i, k] * B[k, j]
        dev = good(c)
        rerender(dev, c, name, bad)
        reject(dev, c, r'%s\[g=%d, c=%d, i=%d, j=%d\]' % (name, g, ch, i, j))
    # operands transposed / swapped
    for bad in (np.matmul(R._T(c['ya']), c['yb']), np.matmul(c['yb'], c['ya'])):
        if n > 1:
            dev = good(c)
            rerender(dev, c, 'M', bad)
            reject(dev, c, r'M\[g=')
    dev = good(c)
    rerender(dev, c, 'dA', c['dB'])
    if n > 1:
        reject(dev, c, r'dA\[g=')
    # the last column block (columns >= 32) taken from the neighbouring matrix
    if n > 32:
        bad = c['M'].copy()
        bad[g, ch, :, 32:] = c['M'][g, ch - 1, :, 32:]
        dev = good(c)
        rerender(dev, c, 'M', bad)
        reject(dev, c, r'M\[g=%d, c=%d, i=0, j=3[2-9]\]' % (g, ch))


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('shape', [s for s in MUT_SHAPES if s[1] is not None], **IDS)
def test_checkers_reject_leaks_and_wrong_strides(shape, family):
    c = R.case(family, *shape)
    Gc, Cc, N, nv = c['G'], c['C'], c['N'], c['nv']
    st = R.strides(N, Cc)
    rng = np.random.default_rng(5)
    # one padding row of A leaked in from the garbage: row nv of the output is garbage @ Yb instead of 0
    g = next(g for g in range(Gc) if 0 < nv[g] < N)
    n = int(nv[g])
    for fill in (0, 1):
        dev = good(c, fill)
        leak = (R.garbage(rng, n).astype(np.float64) - c['mean_a'][g, 0]) * c['a_a'][g, 0] + c['beta_a'][0]
        img = dev['M'][g * st['out'][0]:][:N * N].reshape(N, N)
        with np.errstate(over='ignore', invalid='ignore'):
            img[n, :n] = (leak @ c['yb'][g, 0, :n, :n]).astype(np.float32)
        reject(dev, c, r'M\[g=%d, c=0, i=%d, j=\d+\]: (padding holds|the frame)' % (g, n))
    # ld replaced by N * N: an operand read that way, and an output written that way
    za = R.slab(c['za'].astype(np.float32), nv, *st['a'], rng)
    wrong = np.zeros_like(c['za'])
    for gg in range(Gc):
        for ch in range(Cc):
            wrong[gg, ch] = za[gg * st['a'][0] + ch * N * N:][:N * N].reshape(N, N)
    d = dict(c, za=wrong)
    with np.errstate(over='ignore', invalid='ignore'):
        R.finish(d)
    dev = good(c)
    rerender(dev, c, 'M', np.clip(np.nan_to_num(d['M'], nan=1e30), -3e38, 3e38))
    reject(dev, c, r'M\[g=\d, c=1,')
    dev = good(c)
    dev['dB'] = R.render(c['dB'].astype(np.float32), nv, st['out'][0], N * N)
    reject(dev, c, r'dB')
    # dA written with dM's strides (ogstride / dmgstride mixed up)
    dev = good(c)
    big = R.render(c['dA'].astype(np.float32), nv, *st['dm'])
    dev['dA'] = R.sentinel(Gc * st['out'][0]).copy()
    m = min(len(big), len(dev['dA']))
    dev['dA'][:m] = big[:m]
    reject(dev, c, r'dA')
    # one sentinel word overwritten: behind a matrix in the channel gap, in the graph gap, and in the fill = 1 frame
    gs, ld = st['out']
    for off in (N * N, ld - 1, Cc * ld, gs - 1):
        dev = good(c)
        dev['dB'][g * gs + off] = 0.0
        reject(dev, c, r'outside every image')
    keep = ~R.zero_mask(N, n, 1)
    keep[:n, :n] = False
    if keep.any():                                          # (nothing of the frame is left alone when 32 ceil(nv / 32) >= N)
        e = g * gs + int(np.flatnonzero(keep.reshape(-1))[0])
        dev = good(c, 1)
        assert dev['M'].view(np.uint32)[e] == R.SENT
        dev['M'][e] = 0.0
        reject(dev, c, r'the frame outside the fill = 1 region')
        dev = good(c, 1)                                    # and a fill = 1 answer is no fill = 0 answer, nor the reverse
        dev['fill'] = 0
        reject(dev, c, r'padding holds')
        dev = good(c, 0)
        dev['fill'] = 1
        reject(dev, c, r'the frame outside the fill = 1 region')
    # a negative zero in the padding
    dev = good(c)
    dev['M'][g * gs + N * N - 1] = -0.0
    reject(dev, c, r'not \+0')


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('shape', [s for s in MUT_SHAPES if s[0] <= 64], **IDS)
def test_checkers_reject_s1_missing_one_row(shape, family):
    """(Ordinary data at N <= 64 only: the worst-case bound of an nv^2-term sum outgrows one row's share beyond that -- the grid
    cases, where S1 / S2 are exact, are what catches a missing row at every N; next test.)"""
    c = R.case(family, *shape)
    _reject_s_rows(c)


@pytest.mark.parametrize('shape', [s for s in MUT_SHAPES if s[0] > 64], **IDS)
def test_checkers_reject_s1_missing_one_row_exactly(shape):
    _reject_s_rows(R.case('grid', *shape))


def _reject_s_rows(c):
    g = int(np.argmax(c['nv']))
    n = int(c['nv'][g])
    for name, prod, z, mean in (('s12a', c['dA'], c['za'], c['mean_a']), ('s12b', c['dB'], c['zb'], c['mean_b'])):
        for k in (0, 1):
            rows = prod[g, 1, :n, :n] * ((z[g, 1, :n, :n] - mean[g, 1]) if k else 1.0)
            i = int(np.argmax(np.abs(rows.sum(1))))
            dev = good(c)
            s = c[name].copy()
            s[g, 1, k] -= rows[i].sum()
            dev[name] = s.astype(np.float32).reshape(-1)
            reject(dev, c, r'%s\[g=%d, c=1\]\.S%d' % (name, g, k + 1))
