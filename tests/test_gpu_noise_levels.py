"""GPU: pairs of several noise levels in one launch (fgnn_pairgen_levels, PairGenerator.bits(levels=, level=)): every pair of a
mixed launch is, bit for bit, the pair a single-noise generator makes for the same dataset index."""
import ctypes as C

import numpy as np
import pytest
import torch

import pairgen_ref as R
from graph_neural_net_amd import _lib, synthetic
from graph_neural_net_amd.inputs import expand_adjacency
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.planted import relabel_bits
from graph_neural_net_amd.spectral import spectral_features

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NOISES = (0.0, 0.1, 1.0)
INDEX = [3, 0, 3, 11, 2, 2 ** 33 + 1, 5]          # a duplicate and an index past 2^32
LEVEL = [0, 1, 2, 2, 0, 1, 1]
FIRST = 2


def _kw(family, noise_model, N, vertex_proba=1.0):
    p = 0.5 if family == 'BarabasiAlbert' and N == 5 else 0.3          # BarabasiAlbert at N = 5 needs m = int(p * 4 / 2) >= 1
    return dict(n_vertices=N, generative_model=family, noise_model=noise_model, edge_density=p, vertex_proba=vertex_proba, seed=17)


def _accepted(kw):
    try:
        PairGenerator(device='cpu', **kw)
    except ValueError:
        return False
    return True


CASES = [_kw(f, m, N) for N in (5, 33, 64) for f in ('ErdosRenyi', 'Regular', 'BarabasiAlbert') for m in ('ErdosRenyi', 'EdgeSwap')]
CASES = [kw for kw in CASES if _accepted(kw)] + [_kw('ErdosRenyi', 'ErdosRenyi', 33, vertex_proba=0.7)]


def _same(a, b):
    return (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize('kw', CASES, ids=lambda kw: '%s-%s-N%d-vp%g' % (kw['generative_model'], kw['noise_model'], kw['n_vertices'],
                                                                         kw['vertex_proba']))
def test_mixed_launch_equals_single_noise_launches(kw):
    gen = PairGenerator(noise=0.37, device=DEV, **kw)          # (its own noise value must not matter)
    single = [PairGenerator(noise=v, device=DEV, **kw) for v in NOISES]
    lv = gen.levels(NOISES)
    level = torch.tensor(LEVEL, dtype=torch.int64, device=DEV)
    b1, b2, nv = gen.bits(index=INDEX, levels=lv, level=level)
    c1, c2, cnv = gen.bits(FIRST, len(LEVEL), levels=lv, level=LEVEL)
    assert (nv is None) == (kw['vertex_proba'] == 1.0) and b1.shape == (7, kw['n_vertices'], (kw['n_vertices'] + 31) // 32)
    for b, (k, l) in enumerate(zip(INDEX, LEVEL)):
        e1, e2, env = single[l].bits(index=[k])
        assert torch.equal(b1[b:b + 1], e1) and torch.equal(b2[b:b + 1], e2) and _same(None if nv is None else nv[b:b + 1], env), b
        e1, e2, env = single[l].bits(index=[FIRST + b])
        assert torch.equal(c1[b:b + 1], e1) and torch.equal(c2[b:b + 1], e2) and _same(None if cnv is None else cnv[b:b + 1], env), b
        if l == 0 and kw['noise_model'] == 'ErdosRenyi':
            assert torch.equal(b2[b], b1[b]) and torch.equal(c2[b], c1[b])
    if kw['noise_model'] == 'ErdosRenyi' and kw['n_vertices'] >= 33:
        assert bool(b1[2].any()) and not bool((b1[2] & b2[2]).any())          # noise 1.0 (the threshold 2^32) removes every edge


def test_mixed_launch_equals_the_host_restatement():
    kw = _kw('Regular', 'ErdosRenyi', 33)
    gen = PairGenerator(noise=0.37, device=DEV, **kw)
    b1, b2, _ = gen.bits(index=INDEX, levels=gen.levels(NOISES), level=LEVEL)
    for b, (k, l) in enumerate(zip(INDEX, LEVEL)):
        W1, W2, n = R.generate_pair(kw['seed'], k, 33, 'Regular', 'ErdosRenyi', kw['edge_density'], NOISES[l])
        assert n == 33
        for got, want in ((b1[b], W1), (b2[b], W2)):
            assert torch.equal(got.cpu(), torch.from_numpy(synthetic.pack_adjacency(want[None]).view(np.int32))[0]), (b, k, l)


@pytest.mark.parametrize('vertex_proba', [1.0, 0.7])
def test_permute_with_levels(vertex_proba):
    gen = PairGenerator(noise=0.37, device=DEV, **_kw('ErdosRenyi', 'ErdosRenyi', 33, vertex_proba))
    lv = gen.levels(NOISES)
    b1, b2, nv = gen.bits(index=INDEX, levels=lv, level=LEVEL)
    p1, p2, pnv, labels = gen.bits(index=INDEX, permute=True, levels=lv, level=LEVEL)
    plain = gen.bits(index=INDEX, permute=True)
    assert torch.equal(labels, plain[3]) and torch.equal(p1, b1) and _same(pnv, nv)          # the labels depend on (seed, index) only
    assert torch.equal(p2, relabel_bits(b2, labels, nv)) and not torch.equal(p2, b2)


def test_a_level_outside_the_table_gives_the_empty_graph():
    gen = PairGenerator(noise=0.37, device=DEV, **_kw('Regular', 'EdgeSwap', 33, 0.7))
    lv = gen.levels(NOISES)
    good = gen.bits(index=INDEX, levels=lv, level=LEVEL)
    bad_level = list(LEVEL)
    bad_level[1], bad_level[4] = -1, len(NOISES)
    b1, b2, nv = gen.bits(index=INDEX, levels=lv, level=bad_level)
    for b in range(len(LEVEL)):
        if b in (1, 4):
            assert not bool(b1[b].any()) and not bool(b2[b].any()) and nv[b].item() == 0
        else:
            assert torch.equal(b1[b], good[0][b]) and torch.equal(b2[b], good[1][b]) and nv[b].item() == good[2][b].item()
    with pytest.raises(RuntimeError, match='fgnn_pairgen_levels'):
        _lib.call('fgnn_pairgen_levels', C.byref(_lib.PairgenArgs()), None, _lib.ptr(lv.table), 65, None, _lib.stream_ptr())


def test_dense_and_spectral_with_levels():
    N = 12
    for vp in (1.0, 0.7):
        gen = PairGenerator(noise=0.37, device=DEV, **_kw('ErdosRenyi', 'ErdosRenyi', N, vp))
        lv = gen.levels(NOISES)
        b1, b2, nv = gen.bits(index=INDEX, levels=lv, level=LEVEL)
        x1, x2 = gen.dense(index=INDEX, levels=lv, level=LEVEL)
        f1, f2 = gen.spectral(index=INDEX, levels=lv, level=LEVEL)
        if nv is None:
            assert torch.equal(x1['input'], expand_adjacency(b1, N, None)) and torch.equal(x2['input'], expand_adjacency(b2, N, None))
            assert torch.equal(f1['input'], spectral_features(b1, None, 4)) and torch.equal(f2['input'], spectral_features(b2, None, 4))
        else:
            n = int(nv.max().item())
            assert torch.equal(x2.tensor, expand_adjacency(b2, N, nv)[:, :, :n, :n]) and torch.equal(x2.nvalid, nv)
            assert torch.equal(x1.tensor, expand_adjacency(b1, N, nv)[:, :, :n, :n])
            assert torch.equal(f1.tensor, spectral_features(b1, nv, 4, n_out=n)) and torch.equal(f2.tensor, spectral_features(b2, nv, 4, n_out=n))


def test_a_generator_on_the_current_device_takes_its_own_levels():
    """device='cuda' keeps no index while the table reports cuda:0: the same device (pairgen.same_device)"""
    kw = _kw('Regular', 'ErdosRenyi', 33)
    here, named = PairGenerator(noise=0.37, device='cuda', **kw), PairGenerator(noise=0.37, device=DEV, **kw)
    got = here.bits(index=INDEX, levels=here.levels(NOISES), level=LEVEL)
    want = named.bits(index=INDEX, levels=named.levels(NOISES), level=LEVEL)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    x1, x2 = here.dense(index=INDEX, levels=named.levels(NOISES), level=LEVEL)          # (either generator's table: one device)
    assert torch.equal(x2['input'], expand_adjacency(want[1], 33, None))
