"""Host: the pairwise-exchange search on real-weighted pairs -- tests/two_opt_weighted_ref.py and the host route of
qap.two_opt_weighted (CPU tensors) -- against scipy.optimize.quadratic_assignment(method='2opt', maximize=True, partial_guess=the
whole start): col_ind, fun and nit, exactly, on integer weights in [-3, 3] and dyadic weights k/8, symmetric pairs and directed
pairs with non-zero diagonals.  Also: the C interface is declared and bound, and every exact case of the GPU test is a search the
reference ends as a local optimum."""
import os
import re

import numpy as np
import pytest
import torch
from scipy.optimize import quadratic_assignment

import two_opt_weighted_ref as R
from graph_neural_net_amd import _lib, qap

SIZES = (1, 2, 3, 7, 12, 33)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'fgnn_hip.h')


def starts_of(n, q, seed):
    out = [R.transposed(q, k, seed + k) for k in (1, 3) if n >= 2]
    if n <= 12:
        out.append(np.random.default_rng(seed).permutation(n))
    return out or [q.copy()]


def scipy_2opt(A, B, start):
    n = len(start)
    res = quadratic_assignment(A, B, method='2opt', options={'maximize': True, 'partial_guess': np.stack([np.arange(n), start], 1)})
    return res.col_ind.tolist(), float(res.fun), int(res.nit)


def padded(mats, N, fill=float('nan')):
    """pairs' matrices -> (B, N, N) float32 CPU tensor, `fill` outside each corner"""
    x = torch.full((len(mats), N, N), fill, dtype=torch.float32)
    for b, m in enumerate(mats):
        x[b, :len(m), :len(m)] = torch.from_numpy(m).float()
    return x


def run_host(As, Bs, starts, N, **kw):
    """qap.two_opt_weighted on CPU tensors, NaN outside the corners"""
    assign = np.full((len(As), N), -1, dtype=np.int64)
    for b, s in enumerate(starts):
        assign[b, :len(s)] = s
    nv = torch.tensor([len(s) for s in starts], dtype=torch.int32)
    return qap.two_opt_weighted(padded(As, N), padded(Bs, N), torch.from_numpy(assign), nvalid=nv, **kw)


@pytest.mark.parametrize('kind', ['int', 'dyadic'])
@pytest.mark.parametrize('symmetric', [True, False])
@pytest.mark.parametrize('n', SIZES)
def test_reference_and_host_route_equal_scipy(n, symmetric, kind):
    As, Bs, starts = [], [], []
    for seed in (0, 1):
        A, B, q = R.make_pair(n, seed, symmetric, kind)
        if n >= 7:
            assert symmetric == (np.array_equal(A, A.T) and not A.diagonal().any())
            assert symmetric or (A.diagonal().any() and B.diagonal().any())
            assert kind == 'int' or (np.array_equal(A * 8, np.round(A * 8)) and not np.array_equal(A, np.round(A)))
        for s in starts_of(n, q, seed):
            As.append(A), Bs.append(B), starts.append(s)
    got = run_host(As, Bs, starts, n)
    assert set(got) == {'perm', 'qap', 'qap0', 'acc', 'swaps', 'nit', 'status'}
    assert got['perm'].dtype == torch.int32 and got['qap'].dtype == got['qap0'].dtype == torch.float64
    assert all(got[k].dtype == torch.int64 for k in ('acc', 'swaps', 'nit', 'status'))
    total = 0
    for b, (A, B, s) in enumerate(zip(As, Bs, starts)):
        col, fun, nit = scipy_2opt(A, B, s)
        ref = R.two_opt(A, B, s)
        assert (ref['perm'].tolist(), ref['qap'], ref['nit'], ref['status']) == (col, fun, nit, R.OPTIMUM)
        assert ref['qap'] == R.objective(A, B, ref['perm'])
        assert got['perm'][b].tolist() == col
        assert (float(got['qap'][b]), int(got['nit'][b]), int(got['status'][b])) == (fun, nit, 0)
        assert int(got['swaps'][b]) == ref['swaps'] and float(got['qap0'][b]) == R.objective(A, B, s)
        assert int(got['acc'][b]) == int((np.array(col) == np.arange(n)).sum())
        assert fun > float(got['qap0'][b]) or ref['swaps'] == 0
        total += ref['swaps']
    assert n < 7 or total > 0                                       # the starts are not all local optima


def test_ragged_batch_with_nan_outside_the_corners_and_labels():
    N, sizes = 33, (0, 1, 7, 33, 12)
    pairs = [R.make_pair(n, 5, b % 2 == 0, 'dyadic' if b % 2 else 'int') for b, n in enumerate(sizes)]
    As, Bs = [p[0] for p in pairs], [p[1] for p in pairs]
    starts = [R.transposed(p[2], min(3, len(p[2]) // 2), 9) for p in pairs]
    labels = np.full((len(sizes), N), -1, dtype=np.int64)
    for b, p in enumerate(pairs):
        labels[b, :len(p[2])] = p[2]
    got = run_host(As, Bs, starts, N, labels=torch.from_numpy(labels))
    for b, (A, B, s) in enumerate(zip(As, Bs, starts)):
        ref = R.two_opt(A, B, s)
        n = len(s)
        assert got['perm'][b].tolist() == ref['perm'].tolist() + [-1] * (N - n)
        assert [got[k][b].item() for k in ('qap', 'swaps', 'nit', 'status')] == [ref[k] for k in ('qap', 'swaps', 'nit', 'status')]
        assert int(got['acc'][b]) == int((ref['perm'] == pairs[b][2]).sum())
    assert got['nit'][:2].tolist() == [0, 1] and int(got['swaps'].sum()) > 0
    # channel 0 of a (B, C, N, N) batch is what the (B, N, N) matrices are
    x1, x2 = (torch.stack([padded(m, N), torch.full((len(sizes), N, N), 7.0)], 1) for m in (As, Bs))
    assign = np.full((len(sizes), N), -1, dtype=np.int64)
    for b, s in enumerate(starts):
        assign[b, :len(s)] = s
    again = qap.two_opt_weighted(x1, x2, torch.from_numpy(assign), nvalid=torch.tensor(sizes), labels=torch.from_numpy(labels))
    assert all(torch.equal(again[k], got[k]) for k in got)


@pytest.mark.parametrize('symmetric', [True, False])
def test_max_swaps_stops_after_that_many_exchanges(symmetric):
    n = 12
    A, B, q = R.make_pair(n, 2, symmetric, 'dyadic')
    start = np.random.default_rng(4).permutation(n)
    full = R.two_opt(A, B, start)
    assert full['swaps'] >= 3 and full['status'] == R.OPTIMUM
    # the serial algorithm with whole objectives, stopped by hand after k accepted exchanges
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
        assert (got['perm'][0].tolist(), float(got['qap'][0]), int(got['nit'][0]), int(got['swaps'][0]), int(got['status'][0])) \
            == want + (k, 1)
    ample = run_host([A], [B], [start], n, max_swaps=full['swaps'] + 1)
    assert int(ample['status'][0]) == 0 and int(ample['nit'][0]) == full['nit'] and ample['perm'][0].tolist() == full['perm'].tolist()
    with pytest.raises(ValueError, match='max_swaps'):
        run_host([A], [B], [start], n, max_swaps=-1)


def test_an_invalid_start_is_reported_and_handed_back():
    n = 7
    A, B, q = R.make_pair(n, 1, False, 'int')
    bad = [np.array([0, 1, 2, -1, 4, 5, 6]), np.array([0, 1, 2, 7, 4, 5, 6]), np.array([0, 1, 2, 2, 4, 5, 6])]
    starts = [bad[0], q, bad[1], bad[2]]
    got = run_host([A] * 4, [B] * 4, starts, n)
    for b, s in enumerate(starts):
        if b == 1:
            ref = R.two_opt(A, B, q)
            assert (got['perm'][b].tolist(), float(got['qap'][b]), int(got['nit'][b]), int(got['status'][b])) \
                == (ref['perm'].tolist(), ref['qap'], ref['nit'], 0)
            continue
        assert R.two_opt(A, B, s)['status'] == R.NO_PERMUTATION
        assert got['perm'][b].tolist() == s.tolist()
        assert [got[k][b].item() for k in ('qap', 'swaps', 'nit', 'status')] == [-1.0, 0, 0, 2]
    assert got['qap0'].tolist()[::2] == [-1.0, -1.0] and float(got['qap0'][3]) == R.objective(A, B, bad[2])


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: '%d-%d-%s-%s' % (c[0], c[1], 'sym' if c[2] else 'dir', c[3]))
def test_every_exact_gpu_case_ends_as_a_local_optimum_within_the_bound(case):
    N, B, symmetric, kind = case
    refs = R.reference(*case)
    starts = R.batch_of(*case)[2]
    assert len(refs) == B
    for ref, s in zip(refs, starts):
        n = len(s)
        assert ref['status'] == R.OPTIMUM and ref['swaps'] < max(n * n, 1)
        assert abs(ref['qap']) * 64 < 2 ** 24                        # fp32 holds the objective exactly
    assert N < 3 or sum(r['swaps'] for r in refs) > 0


def test_the_interface_is_declared_and_bound():
    text = open(HEADER).read()
    assert re.search(r'\bint\s+fgnn_qapw_2opt\s*\(', text) and re.search(r'\blong long\s+fgnn_qapw_2opt_ws_bytes\s*\(\s*int B,\s*int N\)', text)
    assert 'fgnn_qapw_2opt' in _lib.EXPORTS and 'fgnn_qapw_2opt_ws_bytes' in _lib.EXPORTS
    lib = _lib.load()
    assert lib.fgnn_qapw_2opt_ws_bytes(0, 5) == 0 and lib.fgnn_qapw_2opt_ws_bytes(3, 128) >= 0
    for B, N in ((1, 129), (5, 200), (70, 256), (65535, 256)):
        assert lib.fgnn_qapw_2opt_ws_bytes(B, N) >= B * N * N * 4
