"""GPU: correlated Gaussian (Wigner) pairs (csrc/wigner.hip, fgnn_wigner_pairs; WignerGenerator) against the numpy restatement
tests/wigner_ref.py: structure bit for bit, values within the fp32 error of Box-Muller, row sums in the documented fp32 order,
addressing, noise levels, planted relabelling, supports, moments, and the collate structures of ``dense``.

The value tolerance |x_dev - x_ref64| <= 1e-5 max(1, |x_ref64|) c_b: a wrong word, branch or index gives an O(1) error; the right
one a few ulp of logf / sinpif / cospif times r <= 5.77 (u >= 2^-24), below 1e-6 -- a tenfold margin."""
import numpy as np
import pytest
import torch

import pairgen_ref as R
import wigner_ref as WR
from graph_neural_net_amd import WignerGenerator
from graph_neural_net_amd.inputs import expand_adjacency
from graph_neural_net_amd.masked import MaskedTensor
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.planted import planted_permutation

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SEED = 29
SHAPES = [(2, 3, 1.0), (5, 3, 1.0), (33, 3, 1.0), (64, 3, 1.0), (65, 3, 1.0), (40, 6, 0.7)]
IDS = ['N%d-B%d-vp%g' % s for s in SHAPES]
FIRST = 3


def _gen(N, vp=1.0, noise=0.4, **kw):
    return WignerGenerator(N, noise=noise, vertex_proba=vp, seed=SEED, device=DEV, **kw)


def _n(nv, B, N):
    return np.full(B, N) if nv is None else nv.cpu().numpy()


def _check_structure(x, n):
    """channel 0 symmetric with a zero diagonal, channel 1 diagonal, +0.0 outside every corner"""
    B, _, N, _ = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous()
    assert torch.equal(x[:, 0], x[:, 0].transpose(1, 2))
    assert not bool(torch.diagonal(x[:, 0], dim1=1, dim2=2).any())
    off = ~torch.eye(N, dtype=torch.bool, device=x.device)
    assert not bool((x[:, 1].view(torch.int32) * off).any())
    bits = x.view(torch.int32).cpu().numpy()
    for b in range(B):
        m = int(n[b])
        assert not bits[b, :, m:, :].any() and not bits[b, :, :, m:].any(), b


def _check_row_sums(x, n):
    """channel 1's diagonal: bit-equal to the documented fp32 order on the device's channel 0; within (n - 1) 2^-24 sum |w| of fp64"""
    w = x[:, 0].cpu().numpy()
    d = torch.diagonal(x[:, 1], dim1=1, dim2=2).cpu().numpy()
    assert np.array_equal(WR.row_sums32(w).view(np.int32), d.view(np.int32))
    for b in range(x.shape[0]):
        bound = max(int(n[b]) - 1, 0) * 2.0 ** -24 * np.abs(w[b].astype(np.float64)).sum(-1)
        assert (np.abs(d[b].astype(np.float64) - WR.row_sums64(w[b])) <= bound).all(), b


def _check_values(x, ref, n, scale='wigner'):
    got = x[:, 0].cpu().numpy().astype(np.float64)
    worst = 0.0
    for b in range(got.shape[0]):
        c = float(WR.scale_of(max(int(n[b]), 1), scale))
        err = np.abs(got[b] - ref[b]) / (np.maximum(1.0, np.abs(ref[b])) * c)
        worst = max(worst, float(err.max()))
    print('max |x_dev - x_ref64| / (max(1, |x_ref64|) c_b) = %.3e' % worst)
    assert worst <= 1e-5
    return worst


@pytest.mark.parametrize('N,B,vp', SHAPES, ids=IDS)
def test_structure_values_and_row_sums(N, B, vp):
    x1, x2, nv = _gen(N, vp).weighted(FIRST, B)
    assert x1.shape == x2.shape == (B, 2, N, N) and (nv is None) == (vp == 1.0)
    n = _n(nv, B, N)
    if nv is not None:
        _, _, pnv = PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, vertex_proba=vp, seed=SEED, device=DEV).bits(FIRST, B)
        assert nv.dtype == torch.int32 and torch.equal(nv, pnv)
    A, Bm, nref = WR.pairs(SEED, range(FIRST, FIRST + B), N, 0.4, vertex_proba=vp)
    assert np.array_equal(n, nref)
    for x, ref in ((x1, A), (x2, Bm)):
        _check_structure(x, n)
        _check_values(x, ref, n)
        _check_row_sums(x, n)
    if N > 2:
        assert bool((x1[:, 0] != x2[:, 0]).any())


def test_scale_none_is_the_unit_normal():
    N, B = 33, 3
    x1, x2, _ = _gen(N, scale=None).weighted(FIRST, B)
    A, Bm, n = WR.pairs(SEED, range(FIRST, FIRST + B), N, 0.4, scale=None)
    _check_values(x1, A, n, None)
    _check_values(x2, Bm, n, None)
    _check_row_sums(x2, n)


@pytest.mark.parametrize('N,B,vp', [(33, 6, 1.0), (40, 6, 0.7)], ids=['N33', 'N40-vp0.7'])
def test_addressing(N, B, vp):
    g = _gen(N, vp)
    whole = g.weighted(FIRST, B)

    def same(got, rows=slice(None)):
        for a, b in zip(got, whole):
            assert (a is None and b is None) or torch.equal(a, b[rows])
    same(g.weighted(index=torch.arange(FIRST, FIRST + B, device=DEV)))
    h = B // 2
    lo, hi = g.weighted(FIRST, h), g.weighted(FIRST + h, B - h)
    same([None if a is None else torch.cat([a, b]) for a, b in zip(lo, hi)])
    order = torch.tensor([4, 0, 5, 2, 1, 3], device=DEV)
    shuffled = g.weighted(index=(FIRST + order).tolist())
    inv = torch.argsort(order)
    same([None if a is None else a[inv] for a in shuffled])
    dup = g.weighted(index=[FIRST + 1, FIRST + 1, FIRST])
    same(dup[:3], rows=torch.tensor([1, 1, 0], device=DEV))
    # a large index: the pair number is 64 bits wide
    big = g.weighted(index=[2 ** 33 + 1])
    A, _, n = WR.pairs(SEED, [2 ** 33 + 1], N, 0.4, vertex_proba=vp)
    _check_values(big[0], A, n)
    # a negative index: the empty graph and nvalid = 0
    x1, x2, nv = g.weighted(index=[FIRST, -1, FIRST + 2])
    assert not bool(x1[1].view(torch.int32).any()) and not bool(x2[1].view(torch.int32).any())
    assert torch.equal(x1[0], whole[0][0]) and torch.equal(x2[2], whole[1][2])
    if nv is not None:
        assert int(nv[1]) == 0 and int(nv[0]) == int(whole[2][0])


@pytest.mark.parametrize('N,vp', [(33, 1.0), (40, 0.7)], ids=['N33', 'N40-vp0.7'])
def test_levels(N, vp):
    noises, level = (0.0, 0.3, 1.0), [2, 0, 1, 1, 0, 2]
    index = [FIRST + b for b in range(len(level))]
    g = _gen(N, vp, noise=0.77)                      # (its own noise value must not matter)
    x1, x2, nv = g.weighted(index=index, levels=g.levels(noises), level=level)
    plain = g.weighted(index=index)
    assert torch.equal(x1, plain[0])                 # side 1 is the same at every level
    for b, l in enumerate(level):
        e1, e2, env = _gen(N, vp, noise=noises[l]).weighted(index=[index[b]])
        assert torch.equal(x1[b:b + 1], e1) and torch.equal(x2[b:b + 1], e2), b
        assert nv is None or torch.equal(nv[b:b + 1], env)
        if l == 0:
            assert torch.equal(x2[b], x1[b])
    # a level outside the table: the empty graph
    y1, y2, ynv = g.weighted(index=index[:2], levels=g.levels(noises), level=[3, 1])
    assert not bool(y1[0].view(torch.int32).any()) and not bool(y2[0].view(torch.int32).any()) and torch.equal(y1[1], x1[1])
    assert ynv is None or int(ynv[0]) == 0
    lv = _gen(N, vp).levels(noises)
    with pytest.raises(ValueError):
        g.weighted(index=index, levels=lv, level=level)


@pytest.mark.parametrize('N,B,vp', [(5, 3, 1.0), (65, 3, 1.0), (40, 6, 0.7)], ids=['N5', 'N65', 'N40-vp0.7'])
def test_permute(N, B, vp):
    g = _gen(N, vp)
    x1, x2, nv = g.weighted(FIRST, B)
    p1, p2, pnv, labels = g.weighted(FIRST, B, permute=True)
    assert torch.equal(p1, x1) and (nv is None or torch.equal(pnv, nv))
    assert torch.equal(labels, planted_permutation(SEED, N, FIRST, B, nvalid=nv, device=DEV))
    n = _n(nv, B, N)
    lab = labels.cpu().numpy()
    w, wp = x2[:, 0].cpu().numpy(), p2[:, 0].cpu().numpy()
    for b in range(B):
        pi = lab[b, :n[b]]
        assert np.array_equal(np.sort(pi), np.arange(n[b]))
        assert np.array_equal(wp[b][np.ix_(pi, pi)].view(np.int32), w[b, :n[b], :n[b]].view(np.int32)), b
    assert bool((p2[:, 0] != x2[:, 0]).any())
    _check_structure(p2, n)
    _check_row_sums(p2, n)
    # by index, the same relabelled pairs
    q = g.weighted(index=list(range(FIRST, FIRST + B)), permute=True)
    assert torch.equal(q[1], p2) and torch.equal(q[3], labels)


@pytest.mark.parametrize('N,vp', [(33, 1.0), (40, 0.7)], ids=['N33', 'N40-vp0.7'])
def test_support(N, vp):
    B = 4
    sup = PairGenerator(N, 'Regular', 'ErdosRenyi', edge_density=0.3, noise=0.2, vertex_proba=vp, seed=SEED, device=DEV)
    g = _gen(N, vp, support=sup)
    x1, x2, nv = g.weighted(FIRST, B)
    d1, d2, _ = _gen(N, vp).weighted(FIRST, B)
    b1, b2, bnv = sup.bits(FIRST, B)
    assert nv is None or torch.equal(nv, bnv)
    for x, d, bits in ((x1, d1, b1), (x2, d2, b2)):
        mask = expand_adjacency(bits, N, bnv)[:, 0] != 0
        assert bool(mask.any()) and torch.equal(x[:, 0] != 0, mask)
        assert torch.equal(x[:, 0], torch.where(mask, d[:, 0], torch.zeros_like(d[:, 0])))
        _check_row_sums(x, _n(nv, B, N))
    # relabelled: the mask moves with the values
    p1, p2, _, labels = g.weighted(FIRST, B, permute=True)
    lab, n = labels.cpu().numpy(), _n(nv, B, N)
    w, wp = x2[:, 0].cpu().numpy(), p2[:, 0].cpu().numpy()
    for b in range(B):
        pi = lab[b, :n[b]]
        assert np.array_equal(wp[b][np.ix_(pi, pi)], w[b, :n[b], :n[b]])


STAT = dict(N=64, B=64, noise=0.6, seed=2024)          # tests/test_wigner_host.py asserts the same bounds on the reference alone


def test_statistics():
    N, B = STAT['N'], STAT['B']
    x1, x2, _ = WignerGenerator(N, noise=STAT['noise'], seed=STAT['seed'], device=DEV).weighted(0, B)
    n = np.full(B, N)
    a, b = WR.standardised(x1[:, 0].cpu().numpy(), n), WR.standardised(x2[:, 0].cpu().numpy(), n)
    assert a.size == 129024
    for x in (a, b):
        mu, var, m4 = WR.moments(x)
        print('mean %.5f var %.5f m4 %.4f' % (mu, var, m4))
        assert abs(mu) <= 0.014 and abs(var - 1) <= 0.02 and abs(m4 - 3) <= 0.14
    corr = np.corrcoef(a, b)[0, 1]
    print('corr %.5f' % corr)
    assert abs(corr - 0.8) <= 0.005


def test_dense_wraps_the_same_tensors():
    g = _gen(12)
    x1, x2, _ = g.weighted(FIRST, 3)
    d1, d2 = g.dense(FIRST, 3)
    assert isinstance(d1, dict) and torch.equal(d1['input'], x1) and torch.equal(d2['input'], x2)
    d1, d2, labels = g.dense(FIRST, 3, permute=True)
    assert torch.equal(d2['input'], g.weighted(FIRST, 3, permute=True)[1]) and labels.shape == (3, 12)
    g = _gen(40, 0.7)
    x1, x2, nv = g.weighted(FIRST, 6)
    m1, m2 = g.dense(index=list(range(FIRST, FIRST + 6)))
    n = int(nv.max())
    assert isinstance(m1, MaskedTensor) and isinstance(m2, MaskedTensor)
    assert torch.equal(m1.tensor.rename(None), x1[:, :, :n, :n]) and torch.equal(m2.tensor.rename(None), x2[:, :, :n, :n])
    assert torch.equal(m1.nvalid, nv) and torch.equal(m2.nvalid, nv)


def test_bits_and_spectral_point_to_weighted():
    g = _gen(12)
    for call in (g.bits, g.spectral):
        with pytest.raises(RuntimeError, match='weighted'):
            call(0, 2)
