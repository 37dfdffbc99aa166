"""Host: the numpy float64 routes of qap.faq(seeds=) and qap.two_opt(seeds=) (CPU tensors) against
scipy.optimize.quadratic_assignment(..., options={'maximize': True, 'partial_match': ...}): col_ind, nit and fun, exactly -- the
routes restate SciPy's seeded loops -- on 0/1 pairs (Regular, ErdosRenyi, directed with loops) and on integer / dyadic weighted
pairs, with n = 12 and 0, 1, 4, 11, 12 seeds and n = 24 and 8 seeds.  Also seeds_from_partial_match, the invalid-seed statuses,
the ValueErrors, and that the C interface is declared and bound."""
import os
import re

import numpy as np
import pytest
import torch

import faq_ref as R
import seeds_ref as S
from graph_neural_net_amd import _lib, qap, synthetic

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'fgnn_hip.h')
CASES = [(12, 0), (12, 1), (12, 4), (12, 11), (12, 12), (24, 8)]
PAD = 3
SYMBOLS = ('fgnn_seed_index', 'fgnn_seed_gather', 'fgnn_seed_const', 'fgnn_qapw_faq_seeded', 'fgnn_qapw_faq_seeded_ws_bytes',
           'fgnn_qap_2opt_seeded', 'fgnn_reveal_seeds')


def pairs_of(kind, n):
    if kind in ('Regular', 'ErdosRenyi'):
        return [R.zero_one_pair(n, s, kind) for s in (0, 1)]
    if kind == 'directed':
        return [R.directed_pair(n, s) for s in (0, 1)]
    what, sym = kind.split('-')
    return [R.exact_pair(n, s, sym == 'sym', what) for s in (0, 1)]


def dense01(mats):
    """0/1 matrices -> (B, 2, N, N) tensor representations, garbage in the padding"""
    return torch.stack([torch.from_numpy(np.pad(synthetic.tensor_representation(m.astype(np.float32)),
                                                ((0, 0), (0, PAD), (0, PAD)), constant_values=7.0)) for m in mats])


def padded(mats, N):
    x = torch.full((len(mats), N, N), float('nan'), dtype=torch.float64)
    for b, m in enumerate(mats):
        x[b, :len(m), :len(m)] = torch.from_numpy(np.asarray(m))
    return x


def seeds_tensor(sds, N):
    t = torch.full((len(sds), N), -1, dtype=torch.int64)
    for b, sd in enumerate(sds):
        t[b, :len(sd)] = torch.from_numpy(sd)
    t[:, -1] = 5                                      # rows at or beyond n_b are ignored
    return t


def inputs(kind, pairs, N):
    if '-' in kind:
        return padded([p[0] for p in pairs], N), padded([p[1] for p in pairs], N), True
    return dense01([p[0] for p in pairs]), dense01([p[1] for p in pairs]), False


@pytest.mark.parametrize('start', ['barycenter', 'perm', 'matrix'])
@pytest.mark.parametrize('kind', ['Regular', 'ErdosRenyi', 'directed', 'int-sym', 'dyadic-sym', 'dyadic-dir'])
@pytest.mark.parametrize('n,m', CASES)
def test_faq_host_route_equals_scipy(n, m, kind, start):
    N = n + PAD
    pairs = pairs_of(kind, n)
    sds = [S.seed_vector(n, m, s) for s in range(len(pairs))]
    x1, x2, weighted = inputs(kind, pairs, N)
    u = n - m
    if start == 'barycenter':
        P0, starts = 'barycenter', ['barycenter'] * len(pairs)
    elif start == 'perm':
        full = [S.completed(sd, s) for s, sd in enumerate(sds)]
        P0 = torch.full((len(pairs), N), -1, dtype=torch.int64)
        starts = []
        for b, (sd, p) in enumerate(zip(sds, full)):
            P0[b, :n] = torch.from_numpy(p)
            free_a, free_b, _, _ = S.lists_of(sd, n)
            starts.append(np.eye(u)[np.searchsorted(free_b, p[free_a])])
    else:
        starts = [R.interior_start(u, s) for s in range(len(pairs))]
        P0 = torch.full((len(pairs), N, N), float('nan'), dtype=torch.float64)
        for b, sd in enumerate(sds):
            free_a, free_b, _, _ = S.lists_of(sd, n)
            P0[b][np.ix_(free_a, free_b)] = torch.from_numpy(starts[b])
    want = [S.scipy_faq(A, B, sd, P0=st) for (A, B), sd, st in zip(pairs, sds, starts)]
    out = qap.faq(x1, x2, nvalid=torch.full((len(pairs),), n), P0=P0, weighted=weighted, seeds=seeds_tensor(sds, N), return_P=True)
    assert set(out) == {'perm', 'qap', 'acc', 'nit', 'status', 'seeded', 'P'}
    assert out['seeded'].tolist() == [m] * len(pairs) and out['seeded'].dtype == torch.int64
    for b, (col, fun, nit) in enumerate(want):
        assert out['perm'][b].tolist() == col.tolist() + [-1] * PAD, (b, nit)
        assert int(out['nit'][b]) == nit and float(out['qap'][b]) == fun
        assert int(out['status'][b]) in ((0, 1) if nit == 30 else (0,))
        assert int(out['acc'][b]) == int((col == np.arange(n)).sum())
        held = sds[b] >= 0
        assert np.array_equal(out['perm'][b, :n].numpy()[held], sds[b][held])
        assert not out['P'][b, u:].any() and not out['P'][b, :, u:].any()


def test_faq_without_seeds_is_untouched():
    A, B = R.zero_one_pair(12, 0)
    x1, x2 = dense01([A]), dense01([B])
    nv = torch.tensor([12])
    plain = qap.faq(x1, x2, nvalid=nv, return_P=True)
    none = qap.faq(x1, x2, nvalid=nv, return_P=True, seeds=None)
    free = qap.faq(x1, x2, nvalid=nv, return_P=True, seeds=torch.full((1, 12 + PAD), -1))
    assert set(plain) == set(none) == {'perm', 'qap', 'acc', 'nit', 'status', 'P'}
    for k in plain:
        assert torch.equal(plain[k], none[k]) and torch.equal(plain[k], free[k]), k
    assert free['seeded'].tolist() == [0]


@pytest.mark.parametrize('kind', ['Regular', 'ErdosRenyi', 'directed'])
@pytest.mark.parametrize('n,m', CASES)
def test_two_opt_host_route_equals_scipy(n, m, kind):
    N = n + PAD
    pairs = pairs_of(kind, n)
    sds = [S.seed_vector(n, m, 10 + s) for s in range(len(pairs))]
    assigns = [S.completed(sd, 20 + s) for s, sd in enumerate(sds)]
    want = [S.scipy_2opt(A, B, sd, p) for (A, B), sd, p in zip(pairs, sds, assigns)]
    x1, x2, _ = inputs(kind, pairs, N)
    a = torch.full((len(pairs), N), -1, dtype=torch.int64)
    for b, p in enumerate(assigns):
        a[b, :n] = torch.from_numpy(p)
    out = qap.two_opt(x1, x2, a, nvalid=torch.full((len(pairs),), n), seeds=seeds_tensor(sds, N))
    for b, (col, fun, nit) in enumerate(want):
        assert out['perm'][b].tolist() == col.tolist() + [-1] * PAD, b
        assert int(out['qap'][b]) == fun and int(out['nit'][b]) == nit and int(out['status'][b]) == 0
        held = sds[b] >= 0
        assert np.array_equal(col[held], sds[b][held])
    if 0 < m < n - 1:
        assert any(int(s) > 0 for s in out['swaps'])


def test_two_opt_start_against_a_seed_is_status_2():
    n = 12
    A, B = R.zero_one_pair(n, 0)
    sd = S.seed_vector(n, 4, 0)
    p = S.completed(sd, 1)
    row = int(np.flatnonzero(sd >= 0)[0])
    other = int(np.flatnonzero(sd < 0)[0])
    p[[row, other]] = p[[other, row]]                 # still a permutation, but row `row` no longer holds its seed
    out = qap.two_opt(dense01([A]), dense01([B]), torch.from_numpy(np.pad(p, (0, PAD), constant_values=-1))[None],
                      nvalid=torch.tensor([n]), seeds=seeds_tensor([sd], n + PAD))
    assert out['status'].tolist() == [2] and out['qap'].tolist() == [-1] and out['nit'].tolist() == [0] and out['swaps'].tolist() == [0]
    assert out['perm'][0, :n].tolist() == p.tolist()


def test_invalid_seeds_and_trivial_pairs():
    n, N = 12, 12 + PAD
    A, B = R.zero_one_pair(n, 0)
    good = S.seed_vector(n, 4, 0)
    shared = good.copy()
    rows = np.flatnonzero(good >= 0)
    shared[rows[1]] = shared[rows[0]]                 # two rows, one target
    outside = good.copy()
    outside[rows[0]] = n                              # inside [0, N) but beyond n_b
    everything = np.random.default_rng(0).permutation(n)
    sds = [good, shared, outside, everything]
    out = qap.faq(dense01([A] * 4), dense01([B] * 4), nvalid=torch.full((4,), n), seeds=seeds_tensor(sds, N))
    assert out['status'].tolist()[1:] == [2, 2, 0] and int(out['status'][0]) in (0, 1)
    assert out['nit'].tolist()[1:] == [0, 0, 0] and int(out['nit'][0]) >= 1
    assert out['qap'].tolist()[1:3] == [-1, -1]
    assert bool((out['perm'][1:3] == -1).all())
    assert out['perm'][3, :n].tolist() == everything.tolist()
    assert int(out['qap'][3]) == int((A * B[np.ix_(everything, everything)]).sum())
    assert out['seeded'].tolist() == [4, 4, 4, n]
    # a matching start against a seed: status 2, perm = the start
    p = S.completed(good, 1)
    other = int(np.flatnonzero(good < 0)[0])
    p[[rows[0], other]] = p[[other, rows[0]]]
    P0 = torch.from_numpy(np.pad(p, (0, PAD), constant_values=-1))[None]
    out = qap.faq(dense01([A]), dense01([B]), nvalid=torch.tensor([n]), P0=P0, seeds=seeds_tensor([good], N))
    assert out['status'].tolist() == [2] and out['nit'].tolist() == [0] and out['perm'][0, :n].tolist() == p.tolist()


def test_seeds_from_partial_match():
    pm = [np.array([[3, 1], [0, 4]]), None, np.zeros((0, 2), dtype=np.int64), torch.tensor([[2, 2]])]
    t = qap.seeds_from_partial_match(pm, 4, 5)
    assert t.dtype == torch.int32 and tuple(t.shape) == (4, 5)
    assert t.tolist() == [[4, -1, -1, 1, -1], [-1] * 5, [-1] * 5, [-1, -1, 2, -1, -1]]
    sd = S.seed_vector(12, 4, 3)
    assert qap.seeds_from_partial_match([S.partial_match_of(sd)], 1, 12)[0].tolist() == sd.tolist()
    assert qap.seeds_from_partial_match([S.partial_match_of(sd)[::-1].copy()], 1, 12)[0].tolist() == sd.tolist()   # any order
    for bad in ([np.array([[0, 5]])], [np.array([[-1, 0]])], [np.array([[1, 0], [1, 2]])], [np.array([0, 1])], [np.array([[0.0, 1.0]])]):
        with pytest.raises(ValueError):
            qap.seeds_from_partial_match(bad, 1, 5)
    with pytest.raises(ValueError):
        qap.seeds_from_partial_match(pm, 3, 5)


def test_refusals():
    A, B = R.zero_one_pair(12, 0)
    x1, x2 = dense01([A]), dense01([B])
    a = torch.arange(12 + PAD)[None]
    with pytest.raises(ValueError, match='partial_match'):
        qap.faq(x1, x2, partial_match=np.array([[0, 0]]))                     # SciPy's spelling keeps raising
    for bad in (torch.zeros(1, 12), torch.zeros(2, 12 + PAD, dtype=torch.int64), torch.zeros(1, 12 + PAD), [0] * 15):
        with pytest.raises(ValueError, match='seeds'):
            qap.faq(x1, x2, seeds=bad)
        with pytest.raises(ValueError, match='seeds'):
            qap.two_opt(x1, x2, a, seeds=bad)
    with pytest.raises(TypeError):
        qap.two_opt_weighted(padded([A], 12), padded([B], 12), a[:, :12], seeds=torch.full((1, 12), -1))
    assert 'seeds' in qap.two_opt_weighted.__doc__


def test_c_interface_is_declared_and_bound():
    with open(HEADER) as f:
        text = f.read()
    for name in SYMBOLS:
        assert re.search(r'\b%s\(' % name, text), name
        assert name in _lib.EXPORTS
    assert '#define FGNN_SEEDS_STREAM 8' in text and '#define FGNN_SEED_MAX_N 256' in text
    assert _lib.FGNN_SEED_MAX_N == 256
