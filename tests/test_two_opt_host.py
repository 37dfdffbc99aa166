"""Host: the pairwise-exchange search -- tests/two_opt_ref.py and the host route of qap.two_opt (CPU tensors) -- against
scipy.optimize.quadratic_assignment(method='2opt', maximize=True, partial_guess=the whole start): col_ind, fun and nit, exactly.
SciPy evaluates the whole objective per candidate, so its legs stay at n <= 40."""
import numpy as np
import pytest
import torch
from scipy.optimize import quadratic_assignment

import qap_ref
import two_opt_ref as R
from graph_neural_net_amd import qap

SIZES = (1, 2, 3, 7, 12, 33, 40)


def starts_of(n, q, seed):
    out = [R.transposed(q, k, seed + k) for k in (1, 2, 3) if n >= 2]
    if n <= 12:
        out.append(np.random.default_rng(seed).permutation(n))
    return out or [q.copy()]


def scipy_2opt(A, B, start):
    n = len(start)
    res = quadratic_assignment(A, B, method='2opt', options={'maximize': True, 'partial_guess': np.stack([np.arange(n), start], 1)})
    return res.col_ind.tolist(), int(res.fun), int(res.nit)


def words(mats, N):
    return torch.from_numpy(np.stack([qap_ref.pack_bits(m, N) for m in mats]).view(np.int32))


def run_host(As, Bs, starts, N, **kw):
    """qap.two_opt on CPU bit words, the pairs zero-padded to N"""
    assign = np.full((len(As), N), -1, dtype=np.int64)
    for b, s in enumerate(starts):
        assign[b, :len(s)] = s
    nv = torch.tensor([len(s) for s in starts], dtype=torch.int32)
    return qap.two_opt(words(As, N), words(Bs, N), torch.from_numpy(assign), nvalid=nv, **kw)


@pytest.mark.parametrize('symmetric', [True, False])
@pytest.mark.parametrize('n', SIZES)
def test_reference_and_host_route_equal_scipy(n, symmetric):
    As, Bs, starts = [], [], []
    for seed in (0, 1):
        A, B, q = R.make_pair(n, seed, symmetric)
        assert symmetric == (np.array_equal(A, A.T) and not A.diagonal().any()) or n < 3
        for s in starts_of(n, q, seed):
            As.append(A), Bs.append(B), starts.append(s)
    got = run_host(As, Bs, starts, n)
    assert set(got) == {'perm', 'qap', 'qap0', 'acc', 'swaps', 'nit', 'status'}
    total = 0
    for b, (A, B, s) in enumerate(zip(As, Bs, starts)):
        col, fun, nit = scipy_2opt(A, B, s)
        ref = R.two_opt(A, B, s)
        assert (ref['perm'].tolist(), ref['qap'], ref['nit'], ref['status']) == (col, fun, nit, R.OPTIMUM)
        assert ref['qap'] == R.objective(A, B, ref['perm']) and fun == R.objective(A, B, np.array(col))
        assert got['perm'][b].tolist() == col and got['perm'].dtype == torch.int32
        assert (int(got['qap'][b]), int(got['nit'][b]), int(got['status'][b])) == (fun, nit, 0)
        assert int(got['swaps'][b]) == ref['swaps'] and int(got['qap0'][b]) == R.objective(A, B, s)
        assert int(got['acc'][b]) == int((np.array(col) == np.arange(n)).sum())
        assert fun >= int(got['qap0'][b]) + ref['swaps']                # every exchange raises the objective
        total += ref['swaps']
    assert n < 7 or total > 0                                       # the starts are not all local optima


@pytest.mark.parametrize('symmetric', [True, False])
def test_identity_on_an_isomorphic_pair_makes_no_exchange(symmetric):
    for n in SIZES:
        A = R.make_pair(n, 3, symmetric)[0]
        ident = np.arange(n)
        col, fun, nit = scipy_2opt(A, A, ident)
        ref = R.two_opt(A, A, ident)
        got = run_host([A], [A], [ident], n)
        assert col == ident.tolist() and fun == int(A.sum()) and nit == n * (n + 1) // 2
        assert (ref['perm'].tolist(), ref['qap'], ref['swaps'], ref['nit']) == (col, fun, 0, nit)
        assert (got['perm'][0].tolist(), int(got['qap'][0]), int(got['swaps'][0]), int(got['nit'][0])) == (col, fun, 0, nit)
        assert int(got['acc'][0]) == n and int(got['qap0'][0]) == fun


def test_ragged_batch_dense_input_and_labels():
    """pairs of 0, 1, 7 and 33 vertices in one batch of N = 33; the dense tensor representation gives what the bit words give"""
    N, sizes = 33, (0, 1, 7, 33)
    pairs = [R.make_pair(n, 5, True) for n in sizes]
    As, Bs = [p[0] for p in pairs], [p[1] for p in pairs]
    starts = [R.transposed(p[2], min(2, len(p[2]) // 2), 9) for p in pairs]
    labels = np.full((len(sizes), N), -1, dtype=np.int64)
    for b, p in enumerate(pairs):
        labels[b, :len(p[2])] = p[2]
    got = run_host(As, Bs, starts, N, labels=torch.from_numpy(labels))
    for b, (A, B, s) in enumerate(zip(As, Bs, starts)):
        ref = R.two_opt(A, B, s)
        n = len(s)
        assert got['perm'][b].tolist() == ref['perm'].tolist() + [-1] * (N - n)
        assert [int(got[k][b]) for k in ('qap', 'swaps', 'nit', 'status')] == [ref[k] for k in ('qap', 'swaps', 'nit', 'status')]
        assert int(got['acc'][b]) == int((ref['perm'] == pairs[b][2]).sum())
    assert got['nit'][:2].tolist() == [0, 1] and got['nit'].dtype == torch.int64
    dense = []
    for mats in (As, Bs):
        x = torch.zeros(len(sizes), 2, N, N)
        for b, m in enumerate(mats):
            n = len(m)
            x[b, 0, :n, :n] = torch.from_numpy(m).float()
            x[b, 1, :n, :n] = torch.diag(torch.from_numpy(m.sum(1)).float())
        dense.append(x)
    assign = np.full((len(sizes), N), -1, dtype=np.int64)
    for b, s in enumerate(starts):
        assign[b, :len(s)] = s
    again = qap.two_opt(dense[0], dense[1], torch.from_numpy(assign), nvalid=torch.tensor(sizes), labels=torch.from_numpy(labels))
    assert all(torch.equal(again[k], got[k]) for k in got)


@pytest.mark.parametrize('symmetric', [True, False])
def test_max_swaps_stops_after_that_many_exchanges(symmetric):
    n = 12
    A, B, q = R.make_pair(n, 2, symmetric)
    start = np.random.default_rng(4).permutation(n)
    full = R.two_opt(A, B, start)
    assert full['swaps'] >= 3
    # the serial algorithm, stopped by hand after k accepted exchanges
    p, nit, trail = start.copy(), 0, []
    best = R.objective(A, B, p)
    for _ in range(3):
        pos = 0
        for i in range(n):
            for j in range(i, n):
                pos += 1
                p[[i, j]] = p[[j, i]]
                if R.objective(A, B, p) > best:
                    break
                p[[i, j]] = p[[j, i]]
            else:
                continue
            break
        best, nit = R.objective(A, B, p), nit + pos
        trail.append((p.tolist(), best, nit))
    for k in (0, 1, 2, 3):
        want = (start.tolist(), R.objective(A, B, start), 0) if k == 0 else trail[k - 1]
        ref = R.two_opt(A, B, start, max_swaps=k)
        got = run_host([A], [B], [start], n, max_swaps=k)
        assert (ref['perm'].tolist(), ref['qap'], ref['nit'], ref['swaps'], ref['status']) == want + (k, R.STOPPED)
        assert (got['perm'][0].tolist(), int(got['qap'][0]), int(got['nit'][0]), int(got['swaps'][0]), int(got['status'][0])) == want + (k, 1)
    ample = run_host([A], [B], [start], n, max_swaps=full['swaps'] + 1)
    assert int(ample['status'][0]) == 0 and int(ample['nit'][0]) == full['nit'] and ample['perm'][0].tolist() == full['perm'].tolist()
    with pytest.raises(ValueError, match='max_swaps'):
        run_host([A], [B], [start], n, max_swaps=-1)


def test_an_invalid_start_is_reported_and_handed_back():
    n = 7
    A, B, q = R.make_pair(n, 1, True)
    bad = [np.array([0, 1, 2, -1, 4, 5, 6]), np.array([0, 1, 2, 7, 4, 5, 6]), np.array([0, 1, 2, 2, 4, 5, 6])]
    starts = [bad[0], q, bad[1], bad[2]]
    got = run_host([A] * 4, [B] * 4, starts, n)
    for b, s in enumerate(starts):
        if b == 1:
            ref = R.two_opt(A, B, q)
            assert (got['perm'][b].tolist(), int(got['qap'][b]), int(got['nit'][b]), int(got['status'][b])) \
                == (ref['perm'].tolist(), ref['qap'], ref['nit'], 0)
            continue
        assert R.two_opt(A, B, s)['status'] == R.NO_PERMUTATION
        assert got['perm'][b].tolist() == s.tolist()
        assert [int(got[k][b]) for k in ('qap', 'swaps', 'nit', 'status')] == [-1, 0, 0, 2]


def test_weighted_is_refused():
    x = torch.zeros(1, 4, 4)
    with pytest.raises(NotImplementedError, match='weighted'):
        qap.two_opt(x, x, torch.arange(4)[None], weighted=True)
