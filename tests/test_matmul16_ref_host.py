"""Host checks of tests/matmul16_ref.py, the CPU reference of the per-channel bf16 products: its roundings against torch, its
load stage and its exactness precondition on grid data at every shape of the GPU table, its products against a triple loop."""
import numpy as np
import pytest
import torch

import matmul16_ref as R
from matmul16_ref import CH as C, G, SHAPES, case_seed, shape_id


def _torch_bits(x32):
    return torch.from_numpy(x32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_rne_bf16_agrees_with_torch_on_fp32_exact_inputs():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(200000) * np.exp2(rng.integers(-30, 30, 200000))).astype(np.float32)
    # exact ties (bit 15 set, nothing below) on even and odd kept mantissas, both signs; binade tops that carry into the exponent
    hi = rng.integers(0x0080, 0x7f00, 4096).astype(np.uint32)
    ties = ((hi << 16) | 0x8000).view(np.float32)
    near = np.concatenate([((hi << 16) | 0x7fff).view(np.float32), ((hi << 16) | 0x8001).view(np.float32)])
    carry = np.array([0x3fff8000, 0x3fffffff, 0x407f8000, 0x3f7f8000], np.uint32).view(np.float32)
    small = np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -126, 2.0 ** -133, 3 * 2.0 ** -134, 2.0 ** -134, 2.0 ** -140], np.float32)
    allx = np.concatenate([x, ties, -ties, near, -near, carry, -carry, small, -small])
    assert np.array_equal(R.rne_bf16(allx.astype(np.float64)), _torch_bits(allx))
    # a tie is decided to even: both neighbours occur among the results
    t = R.rne_bf16(ties.astype(np.float64))
    assert ((t == hi) & (hi % 2 == 0)).any() and ((t == hi + 1) & (hi % 2 == 1)).any()
    assert np.array_equal(R.bf16_value(t), R.bf16_round(ties.astype(np.float64)))


def test_rne_bf16_rounds_an_fp64_value_once():
    """1 + 2^-8 + 2^-30 lies above the tie 1 + 2^-8: rounding through fp32 first would land ON the tie and then go to even (1.0)."""
    x = np.array([1 + 2.0 ** -8 + 2.0 ** -30, -(1 + 2.0 ** -8 + 2.0 ** -30), 1 + 2.0 ** -8])
    assert np.array_equal(R.bf16_value(R.rne_bf16(x)), [1 + 2.0 ** -7, -(1 + 2.0 ** -7), 1.0])
    assert _torch_bits(x.astype(np.float32))[0] == R.rne_bf16(np.array([1.0]))[0]


def test_f32_round_and_affine_b():
    rng = np.random.default_rng(2)
    x = rng.standard_normal(100000) * np.exp2(rng.integers(-40, 40, 100000))
    assert np.array_equal(R.f32_round(x), x.astype(np.float32).astype(np.float64))
    # one rounding of beta - mean a: against fp64 where that is exact, and a case where rounding the product first differs
    mean, a, beta = (rng.standard_normal(2000).astype(np.float32).astype(np.float64) for _ in range(3))
    b = R.affine_b(mean, a, beta)
    assert np.array_equal(b, R.f32_round(b))
    exact64 = beta - mean * a
    resid = np.abs(b - exact64)
    assert (resid <= 0.5 * R.f32_ulp(exact64) * (1 + 2.0 ** -20)).all()
    m1, a1 = 1 + 2.0 ** -23, 1 + 2.0 ** -22                # product 1 + 3 2^-23 + 2^-45: rounds to 1 + 2^-21 when rounded alone
    assert R.affine_b([m1], [a1], [1.0])[0] == -(3 * 2.0 ** -23 + 2.0 ** -45)


def test_operands_are_exact_on_grid_data():
    rng = np.random.default_rng(3)
    c = R.grid_case(rng, G, C, 40, 40, (40, 17, 0))
    for s in 'ab':
        z, mean, a, beta = c['z' + s], c['mean_' + s], c['a_' + s], c['beta_' + s]
        y64 = (z - mean[:, :, None, None]) * a[:, :, None, None] + beta[None, :, None, None]
        y = R.operands(z, mean, a, beta, c['nv'])
        for g, n in enumerate(c['nv']):
            assert np.array_equal(y[g, :, :n, :n], y64[g, :, :n, :n])
            assert not y[g, :, n:, :].any() and not y[g, :, :, n:].any()
        assert np.array_equal(R.bf16_value(R.rne_bf16(y)), y)
        # the extremes of the ranges are reached by the formula: |y| <= (2 + 1) 2 + 1
        ext = R.operands(np.full((1, 1, 1, 1), -2.0), [[1.0]], [[2.0]], [-1.0], [1])
        assert ext[0, 0, 0, 0] == -7.0


def test_operands_round_twice_like_the_kernel():
    """fma -> fp32 -> bf16: a value whose fp32 rounding lands on a bf16 tie goes to even, unlike a single rounding."""
    z = np.full((1, 1, 1, 1), 1.0)
    a = np.float32(1 + 2.0 ** -8)                                # z a = 1 + 2^-8, the bf16 tie between 1 and 1 + 2^-7
    b_small = 2.0 ** -40                                          # fp32(1 + 2^-8 + 2^-40) = 1 + 2^-8: the tie, then to even
    mean = np.float32(-b_small / float(a))
    y = R.operands(z, [[mean]], [[a]], [0.0], [1])
    bb = R.affine_b([[mean]], [[a]], [[0.0]])[0, 0]
    assert bb > 0 and y[0, 0, 0, 0] == 1.0
    assert R.bf16_round(np.array([1.0 * float(a) + bb]))[0] == 1 + 2.0 ** -7


@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
def test_grid_case_stays_inside_the_exactness_condition(shape, record_property):
    """grid_case asserts sum_k |OpA||OpB| / unit < 2^24 itself; here every shape of the GPU table is drawn with the GPU test's
    seed, the figure recomputed independently and the reference's own outputs shown to be multiples of the unit."""
    N, nvalid = shape
    c = R.grid_case(np.random.default_rng(case_seed(N, nvalid)), G, C, N, R.ceil8(N), nvalid)
    ya, yb, dm = c['ya'], c['yb'], c['dm']
    load = 0.0
    for opA, opB, unit, out in ((ya, yb, 1 / 256, c['M']), (dm, np.swapaxes(yb, -1, -2), 1 / 128, c['dA']),
                                (np.swapaxes(ya, -1, -2), dm, 1 / 128, c['dB'])):
        s = np.einsum('gcik,gckj->gcij', np.abs(opA), np.abs(opB)) / unit
        load = max(load, float(s.max(initial=0.0)))
        assert not np.mod(out / unit, 1).any() and (np.abs(out) / unit <= s).all()
    assert load == max(c['load'].values()) and load < 2 ** 24
    assert load <= 256 * 49 * 256                            # the worst case of the ranges
    record_property('grid_load', load)
    print('grid load %s: %.0f of %d' % (shape_id(shape), load, 2 ** 24))


def test_products_agree_with_a_triple_loop():
    rng = np.random.default_rng(5)
    N = 9
    ya, yb, dm = (rng.integers(-20, 21, (2, 2, N, N)).astype(np.float64) / 4 for _ in range(3))
    M, dA, dB = R.products(ya, yb, dm)
    for g in range(2):
        for c in range(2):
            for i in range(N):
                for j in range(N):
                    m = da = db = 0.0
                    for k in range(N):
                        m += ya[g, c, i, k] * yb[g, c, k, j]
                        da += dm[g, c, i, k] * yb[g, c, j, k]
                        db += ya[g, c, k, i] * dm[g, c, k, j]
                    assert (M[g, c, i, j], dA[g, c, i, j], dB[g, c, i, j]) == (m, da, db)


def test_gates_are_what_they_say():
    a, b = np.array([[1.0, -2.0]]), np.array([[3.0], [0.5]])
    assert R.accum_bound(np.abs(a), np.abs(b), 16)[0, 0] == 16 * 2.0 ** -24 * 4.0
    assert R.k_steps(1) == 16 and R.k_steps(16) == 16 and R.k_steps(17) == 32 and R.k_steps(0) == 0
    assert R.bf16_ulp(np.array([1.0, 1.99, 2.0, 0.75]))[:].tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8]
    # just under a power of two the spacing of the next binade is used
    ref, one = np.array([[2.0 - 2.0 ** -20]]), np.array([[1.0]])
    g = R.element_gate(ref, one * 1024, one, 16)              # accumulation bound 2^-10 reaches past 2.0
    assert g[0, 0] == 0.5 * 2.0 ** -6 + 16 * 2.0 ** -24 * 1024


def test_nrm_records_against_a_direct_evaluation():
    """The two-level combination is exact: from exact partials it reproduces mean and variance of the whole corner."""
    rng = np.random.default_rng(6)
    nv = np.array([12, 5, 0])
    z = rng.integers(-16, 17, (3, 2, 12, 12)).astype(np.float64) / 8
    tpg = 7
    part, cnt = R.tile_partials(z, nv, tpg, rng)
    assert (cnt.sum(1) == nv ** 2).all() and (cnt == 0).any() and not part[cnt.sum(1) == 0].any()
    w = np.array([0.5, 1.5])
    rec, gate = R.nrm_records(part, cnt, nv, w, 1e-5)
    for g in range(2):
        for c in range(2):
            v = z[g, c, :nv[g], :nv[g]]
            ve = v.var() + 1e-5
            want = (v.mean(), w[c] / (2 * np.sqrt(nv[g] * ve)), 1 / (2 * np.sqrt(nv[g] * ve)), 1 / ve)
            assert np.allclose(rec[g, c], want, rtol=1e-6, atol=0)          # the partials were rounded to fp32
            assert (gate[g, c] > 0).all() and (gate[g, c][1:] < 1e-4 * np.abs(rec[g, c][1:])).all()
    assert rec[2].tolist() == [[0.0, 0.0, 0.0, 1 / 1e-5]] * 2
