"""Host: the random restarts of qap.faq on CPU tensors -- qap.random_starts against tests/restarts_ref.py bit for bit (and that
against SciPy's private _doubly_stochastic where it can be imported), every restart of qap.faq(restarts=) against
scipy.optimize.quadratic_assignment with that P0, the best-of rule with a constructed tie, the refusals, and the C ABI's entries."""
import os
import re

import numpy as np
import pytest
import torch

import faq_ref as F
import restarts_ref as RR
from graph_neural_net_amd import _lib, qap, synthetic

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'fgnn_hip.h')
SEED = 11


def test_host_philox_is_the_reference_philox():
    pos = np.array([0, 1, 7, 8, (3 << 32) | (5 << 16) | 9, (63 << 32) | (255 << 16) | 255], dtype=np.int64)
    for seed, pair in ((0, 0), (SEED, 5), (2 ** 64 - 1, 2 ** 40 + 3)):
        assert qap.pair_stream_draws(seed, pair, 9, pos).tolist() == RR.pairgen_ref.draws(seed, pair, 9, pos).tolist()


@pytest.mark.parametrize('n', [0, 1, 2, 3, 16, 37, 50])
def test_host_starts_equal_the_restatement(n):
    N, R = max(n, 1) + 2, 4
    nv = torch.tensor([n, n], dtype=torch.int32)
    idx = torch.tensor([5, 0])
    out = qap.random_starts(nv, N, R, seed=SEED, pair_index=idx)
    assert out.shape == (2, R, N, N) and out.dtype == torch.float64
    for b, p in enumerate(idx.tolist()):
        assert np.array_equal(out[b].numpy(), RR.starts(SEED, p, R, n, N))
    if n > 1:
        K = 2 * out[0, 1:, :n, :n].numpy() - 1.0 / n
        assert np.abs(K.sum(1) - 1).max() < 2e-3 and np.abs(K.sum(2) - 1).max() < 2e-3 and (K > 0).all()
    # a start depends on (seed, p, k, n) only: not on the batch, the number of restarts or the padding
    one = qap.random_starts(torch.tensor([n], dtype=torch.int32), N + 5, 2, seed=SEED, pair_index=torch.tensor([5]))
    assert np.array_equal(one[0, :, :N, :N].numpy(), out[0, :2].numpy()) and not one[0, :, N:].any() and not one[0, :, :, N:].any()
    # a float base: restart 0 is the base, the others its mean with K
    if n > 0:
        base = torch.zeros(2, N, N, dtype=torch.float64)
        base[:, :n, :n] = torch.from_numpy(F.interior_start(n, 3))
        withb = qap.random_starts(nv, N, R, seed=SEED, base=base, pair_index=idx)
        assert np.array_equal(withb[1].numpy(), RR.starts(SEED, 0, R, n, N, base[1, :n, :n].numpy()))
        assert torch.equal(withb[:, 0], base)


def test_batch_size_instead_of_counts():
    a = qap.random_starts(2, 6, 3, seed=4)
    assert np.array_equal(a[1].numpy(), RR.starts(4, 1, 3, 6, 6))


@pytest.mark.parametrize('n', [2, 3, 16, 37, 64])
def test_restatement_equals_scipy(n):
    try:
        from scipy.optimize._qap import _doubly_stochastic
    except ImportError:
        pytest.skip('scipy.optimize._qap._doubly_stochastic is not importable')
    for p, k in ((0, 1), (1, 2), (5, 7)):
        U = RR.uniform(SEED, p, k, n)
        assert U.min() > 0 and U.max() <= 1 and np.array_equal(U.astype(np.float32).astype(np.float64), U)
        K, rounds = RR.doubly_stochastic(U)
        assert rounds <= 21 and np.array_equal(K, _doubly_stochastic(U))
        assert np.array_equal(qap._doubly_stochastic(U), K)


def _cpu_inputs(pairs, N, weighted):
    if weighted:
        x = [torch.zeros(len(pairs), N, N, dtype=torch.float64) for _ in (0, 1)]
        for b, p in enumerate(pairs):
            for side in (0, 1):
                x[side][b, :len(p[side]), :len(p[side])] = torch.from_numpy(p[side])
        return x
    out = []
    for side in (0, 1):
        dense = np.zeros((len(pairs), N, N))
        for b, p in enumerate(pairs):
            dense[b, :len(p[side]), :len(p[side])] = p[side]
        out.append(torch.from_numpy(synthetic.pack_adjacency(dense).view(np.int32)))
    return out


@pytest.mark.parametrize('weighted', [False, True])
def test_every_restart_equals_scipy_and_the_winner_obeys_the_rule(weighted):
    sizes, N, R = (12, 16), 16, 3
    pairs = [(F.real_pair if weighted else F.zero_one_pair)(n, 2) for n in sizes]
    x1, x2 = _cpu_inputs(pairs, N, weighted)
    nv = torch.tensor(sizes, dtype=torch.int32)
    out = qap.faq(x1, x2, nvalid=nv, weighted=weighted, restarts=R, seed=SEED, return_all=True)
    assert out['restart'].dtype == torch.int64 and out['all_qap'].shape == (2, R) and out['all_perm'].shape == (2, R, N)
    for b, n in enumerate(sizes):
        for k in range(R):
            col, fun, nit = RR.scipy_restart(*pairs[b], SEED, b, k)
            assert out['all_perm'][b, k, :n].tolist() == col.tolist(), (b, k)
            assert int(out['all_nit'][b, k]) == nit and float(out['all_qap'][b, k]) == fun
        w = RR.best_of(out['all_qap'][b].tolist(), out['all_status'][b].tolist())
        assert int(out['restart'][b]) == w
        assert torch.equal(out['perm'][b], out['all_perm'][b, w]) and out['qap'][b] == out['all_qap'][b, w]
        assert out['nit'][b] == out['all_nit'][b, w] and out['status'][b] == out['all_status'][b, w]
        assert out['qap'][b] >= out['all_qap'][b, 0]
    single = qap.faq(x1, x2, nvalid=nv, weighted=weighted)
    assert set(single) == {'perm', 'qap', 'acc', 'nit', 'status'}              # restarts=1: the keys of always
    for key in ('perm', 'qap', 'nit', 'status'):
        assert torch.equal(single[key], out['all_' + key][:, 0]), key
    # polish: the exchange search on every restart, the choice by the polished objective
    pol = qap.faq(x1, x2, nvalid=nv, weighted=weighted, restarts=R, seed=SEED, polish=True, return_all=True)
    for b in range(2):
        w = int(pol['restart'][b])
        two = (qap.two_opt_weighted if weighted else qap.two_opt)(x1[b:b + 1], x2[b:b + 1], out['all_perm'][b, w:w + 1], nvalid=nv[b:b + 1])
        assert pol['qap'][b] == two['qap'][0] and torch.equal(pol['perm'][b], two['perm'][0]) and pol['swaps'][b] == two['swaps'][0]
        assert pol['status_2opt'][b] == two['status'][0] and pol['qap'][b] == pol['all_qap'][b].max()
        assert (pol['all_qap'][b] >= out['all_qap'][b]).all()


def test_seeded_restarts_on_the_host():
    n, R = 12, 3
    A, B = F.zero_one_pair(n, 4)
    x1, x2 = _cpu_inputs([(A, B)], n, False)
    seeds = torch.full((1, n), -1, dtype=torch.int64)
    seeds[0, 2], seeds[0, 7] = 5, 0
    out = qap.faq(x1, x2, seeds=seeds, restarts=R, seed=SEED, pair_index=torch.tensor([3]), return_all=True)
    free_a = [i for i in range(n) if i not in (2, 7)]
    free_b = [j for j in range(n) if j not in (5, 0)]
    P = RR.starts(SEED, 3, R, n - 2, n - 2)
    for k in range(R):
        full = torch.zeros(1, n, n, dtype=torch.float64)
        full[0][np.ix_(free_a, free_b)] = torch.from_numpy(P[k])
        one = qap.faq(x1, x2, seeds=seeds, P0=full)
        assert torch.equal(one['perm'][0], out['all_perm'][0, k]) and one['qap'][0] == out['all_qap'][0, k]
        assert out['all_perm'][0, k, 2] == 5 and out['all_perm'][0, k, 7] == 0
    assert int(out['seeded'][0]) == 2 and int(out['restart'][0]) == RR.best_of(out['all_qap'][0].tolist(), out['all_status'][0].tolist())


def test_best_of_rule():
    nan = float('nan')
    assert RR.best_of([3, 7, 7, 5], [0, 0, 1, 0]) == 1                      # a tie: the smaller k
    assert RR.best_of([nan, 2.0, nan], [0, 0, 0]) == 1                      # a NaN never wins
    assert RR.best_of([nan, nan], [0, 1]) == 0
    assert RR.best_of([9, 8], [2, 0]) == 1 and RR.best_of([9, 8], [2, 2]) == 0
    assert RR.best_of([1, 2, 3], [0, 0, 0]) == 2 and RR.best_of([9, 8], [0, 0], veto=[2, 0]) == 1
    q = np.array([[3, 7, 7, 5], [9, 8, 1, 1]], dtype=np.int64)
    st = np.array([[0, 0, 1, 0], [2, 2, 2, 2]])
    assert qap._best_of_host(q, st).tolist() == [1, 0]
    assert qap._best_of_host(np.array([[nan, 2.0, nan]]), np.zeros((1, 3), dtype=np.int64)).tolist() == [1]


def test_a_tie_goes_to_the_smaller_restart():
    # the complete graph against itself: every matching has the same objective, so every restart ties
    n = 6
    A = np.ones((n, n)) - np.eye(n)
    x1, x2 = _cpu_inputs([(A, A)], n, False)
    out = qap.faq(x1, x2, restarts=4, seed=1, return_all=True)
    assert out['all_qap'][0].tolist() == [n * (n - 1)] * 4 and int(out['restart'][0]) == 0


def test_refusals():
    n = 8
    A, B = F.zero_one_pair(n, 0)
    x1, x2 = _cpu_inputs([(A, B)], n, False)
    for bad in (0, 65, 2.5, True, -1):
        with pytest.raises(ValueError, match='restarts'):
            qap.faq(x1, x2, restarts=bad)
        with pytest.raises(ValueError, match='restarts'):
            qap.random_starts(1, n, bad)
    with pytest.raises(ValueError, match='seed'):
        qap.faq(x1, x2, restarts=2, seed=-1)
    with pytest.raises(ValueError, match='matching'):
        qap.faq(x1, x2, restarts=2, P0=torch.arange(n)[None])
    with pytest.raises(ValueError, match='return_P'):
        qap.faq(x1, x2, restarts=2, return_P=True)
    w1, w2 = _cpu_inputs([(A, B)], n, True)
    with pytest.raises(ValueError, match='two_opt_weighted takes no seeds'):
        qap.faq(w1, w2, weighted=True, restarts=2, polish=True, seeds=torch.full((1, n), -1))
    with pytest.raises(ValueError):
        qap.faq(x1, x2, restarts=2, P0='randomized')
    with pytest.raises(ValueError):
        qap.faq(x1, x2, restarts=2, rng=0)
    with pytest.raises(ValueError, match='pair_index'):
        qap.faq(x1, x2, restarts=2, pair_index=torch.zeros(3, dtype=torch.int64))


def test_header_and_bindings():
    text = open(HEADER).read()
    for name, nargs in (('fgnn_faq_restart_starts', 9), ('fgnn_qap_best_of_i64', 14), ('fgnn_qap_best_of_f32', 14)):
        decl = re.search(r'int %s\(([^;]*)\);' % name, text)
        assert decl, name
        params = re.sub(r'/\*.*?\*/', '', decl.group(1), flags=re.S)
        assert len(params.split(',')) == nargs == len(_lib._SIGNATURES[name]), name
    for macro, value in (('FGNN_RESTART_STREAM', 9), ('FGNN_RESTART_MAX_R', 64), ('FGNN_RESTART_MAX_STARTS', 65535)):
        assert re.search(r'#define %s %d\b' % (macro, value), text) and getattr(_lib, macro) == value
