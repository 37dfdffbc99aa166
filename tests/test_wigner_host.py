"""CPU: WignerGenerator's argument checks (they run before any device call) and the numpy restatement's own properties --
symmetry, a value that depends on (seed, pair, i, j) only, the fp32 row-sum order -- and the moment bounds of the GPU statistics
test asserted on the restatement alone, for the exact seed and shape that test uses: the bounds are satisfiable."""
import numpy as np
import pytest
import torch

import pairgen_ref as R
import wigner_ref as WR
from graph_neural_net_amd import _lib
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.wigner import WignerGenerator, WignerLevels

STAT = dict(N=64, B=64, noise=0.6, seed=2024)          # tests/test_gpu_wigner.py: test_statistics


def _gen(**kw):
    kw.setdefault('n_vertices', 12)
    return WignerGenerator(device='cpu', **kw)


@pytest.mark.parametrize('kw', [dict(n_vertices=0), dict(n_vertices=257), dict(noise=-0.1), dict(noise=1.5), dict(vertex_proba=0.0),
                                dict(vertex_proba=1.2), dict(n_vertices=1, vertex_proba=0.5), dict(scale='goe'), dict(scale=1.0),
                                dict(seed=-1), dict(seed=1 << 64), dict(support='Regular')])
def test_constructor_refusals(kw):
    with pytest.raises(ValueError):
        _gen(**kw)


def test_support_must_match():
    sup = PairGenerator(12, 'Regular', 'ErdosRenyi', device='cpu')
    assert _gen(support=sup).support is sup
    with pytest.raises(ValueError):
        _gen(n_vertices=13, support=sup)
    with pytest.raises(ValueError):
        _gen(vertex_proba=0.7, support=sup)                 # binomial against constant
    rag = PairGenerator(12, 'ErdosRenyi', 'ErdosRenyi', vertex_proba=0.7, seed=3, device='cpu')
    assert _gen(vertex_proba=0.7, seed=3, support=rag).constant_n_vertices is False
    with pytest.raises(ValueError):
        _gen(vertex_proba=0.7, seed=4, support=rag)         # the two would draw different vertex counts
    with pytest.raises(ValueError):
        _gen(vertex_proba=0.8, seed=3, support=rag)


def test_attributes_and_the_package_export():
    import graph_neural_net_amd
    assert graph_neural_net_amd.WignerGenerator is WignerGenerator
    g = _gen(noise=0.25, seed=9)
    assert (g.seed, g.n_vertices, g.noise, g.constant_n_vertices, g.device) == (9, 12, 0.25, True, torch.device('cpu'))
    assert _gen(vertex_proba=0.5).constant_n_vertices is False
    for call in (g.bits, g.spectral):
        with pytest.raises(RuntimeError, match='weighted'):
            call(0, 1)
    with pytest.raises(RuntimeError, match='GPU'):
        g.weighted(0, 1)                                    # there is no CPU path


def test_levels_validation():
    g = _gen()
    lv = g.levels((0, 0.3, 1))
    assert isinstance(lv, WignerLevels) and len(lv) == 3 and lv.noises == (0.0, 0.3, 1.0)
    assert lv.table.dtype == torch.float32 and tuple(lv.table.shape) == (3, 2)
    want = np.array([[float(v) for v in WR.coefficients(s)] for s in lv.noises], dtype=np.float32)
    assert np.array_equal(lv.table.numpy().view(np.int32), want.view(np.int32))
    for bad in ((), [0.1] * (_lib.FGNN_MAX_LEVELS + 1), (0.1, 1.1), (-0.1,)):
        with pytest.raises(ValueError):
            g.levels(bad)
    # the checks of a mixed call run before the device
    with pytest.raises(ValueError, match='go together'):
        g.weighted(0, 2, levels=lv)
    with pytest.raises(ValueError, match='go together'):
        g.weighted(0, 2, level=[0, 1])
    with pytest.raises(ValueError, match='this generator'):
        g.weighted(0, 2, levels=_gen().levels((0, 0.3, 1)), level=[0, 1])
    with pytest.raises(ValueError, match='integer tensor'):
        g.weighted(0, 2, levels=lv, level=[0, 1, 2])
    with pytest.raises(ValueError):
        g.weighted(0, 2, index=[1, 2])
    with pytest.raises(ValueError):
        g.weighted()


def test_reference_is_symmetric_and_an_entry_depends_on_its_address_only():
    N, seed = 33, 5
    A, B, n = WR.pairs(seed, [4, 5, 6], N, 0.4)
    assert np.array_equal(A, A.transpose(0, 2, 1)) and np.array_equal(B, B.transpose(0, 2, 1))
    assert not np.diagonal(A, axis1=1, axis2=2).any() and (n == N).all()
    # count and first: pair 5 alone
    A5, B5, _ = WR.pairs(seed, [5], N, 0.4)
    assert np.array_equal(A5[0], A[1]) and np.array_equal(B5[0], B[1])
    # n_b: the standardised entry at (i, j) is the same normal whatever the vertex count (the scale c_b aside)
    Ar, _, nr = WR.pairs(seed, [4, 5, 6, 7], N, 0.4, vertex_proba=0.6)
    assert (nr < N).any()
    Au, _, _ = WR.pairs(seed, [4, 5, 6, 7], N, 0.4, scale=None)
    for b in range(4):
        m = int(nr[b])
        c = float(WR.scale_of(m))
        assert np.array_equal(Ar[b, :m, :m], c * Au[b, :m, :m]) and not Ar[b, m:].any() and not Ar[b, :, m:].any()
    # the noise does not move a draw: side 1 is the same, side 2 at s = 0 is side 1
    A0, B0, _ = WR.pairs(seed, [4, 5, 6], N, 0.0)
    assert np.array_equal(A0, A) and np.array_equal(B0, A)
    # t and t ^ 1 share their uniforms and take the two Box-Muller branches
    u0, v0 = WR.uniforms(seed, 4, WR.PARENT_STREAM, [6])
    u1, v1 = WR.uniforms(seed, 4, WR.PARENT_STREAM, [7])
    z = WR.normals(seed, 4, WR.PARENT_STREAM, [6, 7])
    assert u0 == u1 and v0 == v1 and 0 < u0 <= 1 and 0 <= v0 < 1
    assert np.allclose(z[0] ** 2 + z[1] ** 2, -2 * np.log(u0), rtol=1e-12)


def test_reference_relabelling_and_support():
    N, seed = 12, 5
    pi = np.random.RandomState(0).permutation(N)
    _, B, _ = WR.pairs(seed, [2], N, 0.4)
    _, Bp, _ = WR.pairs(seed, [2], N, 0.4, labels=[pi])
    assert np.array_equal(Bp[0][np.ix_(pi, pi)], B[0])
    S = np.triu(np.random.RandomState(1).rand(N, N) < 0.4, 1)
    S = S | S.T
    As, Bs, _ = WR.pairs(seed, [2], N, 0.4, support=([S], [S.T]))
    A, _, _ = WR.pairs(seed, [2], N, 0.4)
    assert np.array_equal(As[0], np.where(S, A[0], 0.0)) and np.array_equal(Bs[0] != 0, S)


def test_row_sum_order():
    rng = np.random.RandomState(3)
    for N in (2, 5, 64, 65, 200):
        W = rng.standard_normal((3, N, N)).astype(np.float32)
        s32, s64 = WR.row_sums32(W), WR.row_sums64(W)
        assert s32.dtype == np.float32 and s32.shape == (3, N)
        assert (np.abs(s32 - s64) <= (N - 1) * 2.0 ** -24 * np.abs(W.astype(np.float64)).sum(-1)).all()
        # the order written out for one row: per-lane partial sums, then the butterfly
        lane = [np.float32(0)] * 64
        for j in range(N):
            lane[j % 64] = np.float32(lane[j % 64] + W[0, 0, j])
        for o in (32, 16, 8, 4, 2, 1):
            lane = [np.float32(lane[l] + lane[l ^ o]) for l in range(64)]
        assert all(v.view(np.int32) == s32[0, 0].view(np.int32) for v in lane)


def test_moment_bounds_hold_on_the_reference():
    """M = 64 * 2016 = 129 024 standardised entries per side; five standard errors of each figure"""
    N, B = STAT['N'], STAT['B']
    A, Bm, n = WR.pairs(STAT['seed'], range(B), N, STAT['noise'])
    a, b = WR.standardised(A, n), WR.standardised(Bm, n)
    assert a.size == 129024
    for x in (a, b):
        mu, var, m4 = WR.moments(x)
        assert abs(mu) <= 0.014 and abs(var - 1) <= 0.02 and abs(m4 - 3) <= 0.14, (mu, var, m4)
    assert abs(np.corrcoef(a, b)[0, 1] - 0.8) <= 0.005
