"""Host: the numpy float64 route of qap.faq (CPU tensors) against scipy.optimize.quadratic_assignment(method='faq',
options={'maximize': True, ...}): col_ind, nit and fun, exactly -- the route restates SciPy's loop operation for operation -- on
seeded 0/1 pairs (Regular and ErdosRenyi parents, noise 0.1; directed pairs with loops) and on real-weighted pairs, from the
barycenter, from a permutation and from a doubly stochastic matrix, with maxiter 1, 3 and 30.  Also: the argument refusals, the
padding contract (ragged corners, NaN around them in A, B and P0), status, and that the C interface is declared and bound."""
import os
import re

import numpy as np
import pytest
import torch

import faq_ref as R
from graph_neural_net_amd import _lib, qap, synthetic

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'fgnn_hip.h')
KEYS = {'perm', 'qap', 'acc', 'nit', 'status'}


def padded(mats, N, fill=float('nan'), dtype=torch.float64):
    """pairs' matrices -> (B, N, N) CPU tensor, `fill` outside each corner"""
    x = torch.full((len(mats), N, N), fill, dtype=dtype)
    for b, m in enumerate(mats):
        x[b, :len(m), :len(m)] = torch.from_numpy(np.asarray(m)).to(dtype)
    return x


def pairs_of(kind, n):
    if kind in ('Regular', 'ErdosRenyi'):
        return [R.zero_one_pair(n, s, kind) for s in (0, 1)]
    if kind == 'directed':
        return [R.directed_pair(n, s) for s in (0, 1)]
    return [R.real_pair(n, s, symmetric=kind == 'real') for s in (0, 1)]


def start_of(start, n, seed):
    if start == 'barycenter':
        return 'barycenter', 'barycenter'
    if start == 'perm':
        p = np.random.default_rng(seed).permutation(n)
        return np.eye(n)[p], p
    P = R.interior_start(n, seed)
    return P, P


@pytest.mark.parametrize('maxiter', [1, 3, 30])
@pytest.mark.parametrize('start', ['barycenter', 'perm', 'matrix'])
@pytest.mark.parametrize('kind', ['Regular', 'ErdosRenyi', 'directed', 'real', 'real-directed'])
@pytest.mark.parametrize('n', [5, 16, 33])
def test_host_route_equals_scipy(n, kind, start, maxiter):
    weighted = kind.startswith('real')
    N = n + 3
    pairs = pairs_of(kind, n)
    starts = [start_of(start, n, s) for s in range(len(pairs))]
    want = [R.scipy_faq(A, B, P0=s[0], maxiter=maxiter) for (A, B), s in zip(pairs, starts)]
    if start == 'barycenter':
        P0 = 'barycenter'
    elif start == 'perm':
        P0 = torch.full((len(pairs), N), -1, dtype=torch.int64)
        for b, s in enumerate(starts):
            P0[b, :n] = torch.from_numpy(s[1])
    else:
        P0 = padded([s[1] for s in starts], N)
    nv = torch.full((len(pairs),), n, dtype=torch.int32)
    if weighted:
        x1, x2 = padded([p[0] for p in pairs], N), padded([p[1] for p in pairs], N)
    else:                                            # dense tensor representations; garbage (not NaN: channel 1 is checked on the corner only)
        x1, x2 = (torch.stack([torch.from_numpy(np.pad(synthetic.tensor_representation(p[side].astype(np.float32)),
                                                       ((0, 0), (0, 3), (0, 3)), constant_values=7.0)) for p in pairs]) for side in (0, 1))
    out = qap.faq(x1, x2, nvalid=nv, P0=P0, maxiter=maxiter, weighted=weighted)
    assert set(out) == KEYS
    assert out['nit'].dtype == out['status'].dtype == out['acc'].dtype == torch.int64 and out['perm'].dtype == torch.int32
    for b, (col, fun, nit) in enumerate(want):
        assert out['perm'][b].tolist() == col.tolist() + [-1] * 3, (b, nit)
        assert int(out['nit'][b]) == nit and float(out['qap'][b]) == fun
        assert int(out['status'][b]) in ((R.STOPPED_ON_TOL, R.MAXITER) if nit == maxiter else (R.STOPPED_ON_TOL,))
        assert int(out['acc'][b]) == int((col == np.arange(n)).sum())
    if maxiter == 30 and start == 'barycenter' and n > 5:
        assert any(w[2] > 1 for w in want)           # the loop ran


def test_bit_words_and_dense_input_agree():
    n = 16
    pairs = [R.zero_one_pair(n, s) for s in range(3)]
    bits = [torch.from_numpy(synthetic.pack_adjacency(np.stack([p[side] for p in pairs])).view(np.int32)) for side in (0, 1)]
    dense = [torch.stack([torch.from_numpy(synthetic.tensor_representation(p[side].astype(np.float32))) for p in pairs]) for side in (0, 1)]
    a, b = qap.faq(bits[0], bits[1]), qap.faq(dense[0], dense[1])
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    assert a['qap'].dtype == torch.int64
    assert a['qap'].tolist() == [R.scipy_faq(A, B)[1] for A, B in pairs]
    w = qap.faq(torch.from_numpy(np.stack([p[0] for p in pairs])), torch.from_numpy(np.stack([p[1] for p in pairs])), weighted=True)
    assert w['qap'].dtype == torch.float64 and torch.equal(w['perm'], a['perm']) and w['qap'].tolist() == a['qap'].tolist()
    with pytest.raises(RuntimeError, match='tensor representation'):
        qap.faq(dense[0] * 0.5, dense[1])


def test_padding_contract_labels_status_and_return_P():
    """ragged corners with NaN around them in A, B and P0: every pair gives what it gives alone; n_b = 0, n_b = 1, and a matching
    P0 that is no permutation are status 2 / trivial; labels are counted; P is the last iterate, zero around the corner"""
    N, sizes = 12, [0, 1, 2, 5, 12, 7]
    pairs = [R.real_pair(n, 3 + n) for n in sizes]
    x1, x2 = padded([p[0] for p in pairs], N), padded([p[1] for p in pairs], N)
    nv = torch.tensor(sizes)
    labels = torch.stack([torch.roll(torch.arange(N), 1) for _ in sizes])
    out = qap.faq(x1, x2, nvalid=nv, labels=labels, weighted=True, return_P=True)
    assert set(out) == KEYS | {'P'}
    for b, n in enumerate(sizes):
        if n == 0:
            assert int(out['status'][b]) == R.FAILED and int(out['nit'][b]) == 0 and float(out['qap'][b]) == -1
            assert out['perm'][b].tolist() == [-1] * N
            continue
        col, fun, nit = R.scipy_faq(*pairs[b])
        assert out['perm'][b].tolist() == col.tolist() + [-1] * (N - n) and int(out['nit'][b]) == nit and float(out['qap'][b]) == fun
        assert int(out['acc'][b]) == int((col == np.roll(np.arange(N), 1)[:n]).sum())
        P = out['P'][b].numpy()
        assert np.isfinite(P).all() and not P[n:].any() and not P[:, n:].any()
        assert np.allclose(P[:n, :n].sum(0), 1) and np.allclose(P[:n, :n].sum(1), 1)
    assert int(out['nit'][1]) == 1 and int(out['status'][1]) == R.STOPPED_ON_TOL and out['perm'][1, 0] == 0
    # a matrix P0 with NaN around its corners
    starts = [R.interior_start(n, b) for b, n in enumerate(sizes)]
    out = qap.faq(x1, x2, nvalid=nv, P0=padded(starts, N), weighted=True, maxiter=3)
    for b, n in enumerate(sizes):
        if n:
            col, fun, nit = R.scipy_faq(*pairs[b], P0=starts[b], maxiter=3)
            assert out['perm'][b, :n].tolist() == col.tolist() and int(out['nit'][b]) == nit and float(out['qap'][b]) == fun
    # a matching that is no permutation of its corner: status 2, perm = the matching, qap -1, nit 0
    P0 = torch.stack([torch.arange(N) for _ in sizes])
    P0[3, :5] = torch.tensor([0, 1, 1, 3, 4])
    P0[4, 2] = 12
    out = qap.faq(x1, x2, nvalid=nv, P0=P0, weighted=True)
    assert out['status'].tolist()[3:5] == [R.FAILED] * 2 and out['nit'].tolist()[3:5] == [0, 0] and out['qap'].tolist()[3:5] == [-1, -1]
    assert out['perm'][3].tolist() == [0, 1, 1, 3, 4] + [-1] * 7 and out['perm'][4].tolist() == P0[4].tolist()
    assert int(out['status'][5]) in (R.STOPPED_ON_TOL, R.MAXITER) and int(out['nit'][5]) >= 1


def test_stop_rule():
    A, B = R.real_pair(16, 0)
    x1, x2 = torch.from_numpy(A)[None], torch.from_numpy(B)[None]
    out = qap.faq(x1, x2, weighted=True, tol=1e9)
    assert out['nit'].tolist() == [1] and out['status'].tolist() == [R.STOPPED_ON_TOL]
    out = qap.faq(x1, x2, weighted=True, maxiter=1)
    assert out['nit'].tolist() == [1] and out['status'].tolist() == [R.MAXITER]


@pytest.mark.parametrize('kw', [{'P0': 'randomized'}, {'P0': 'identity'}, {'partial_match': [[0, 0]]}, {'shuffle_input': True},
                                {'rng': 0}, {'maxiter': 0}, {'maxiter': -3}, {'maxiter': 2.5}, {'tol': 0}, {'tol': -0.1},
                                {'P0': torch.zeros(2, 5)}, {'P0': torch.zeros(2, 5, 4)}, {'P0': torch.zeros(2, 4, dtype=torch.int64)},
                                {'P0': torch.zeros(2, 5, dtype=torch.bool)}],
                         ids=lambda kw: '-'.join('%s' % k for k in kw))
def test_bad_arguments_are_refused(kw):
    x = torch.zeros(2, 5, 5)
    with pytest.raises(ValueError):
        qap.faq(x, x, weighted=True, **kw)


def test_interface_is_declared_and_bound():
    hdr = open(HEADER).read()
    for name in ('fgnn_qapw_faq_ws_bytes', 'fgnn_qapw_faq'):
        assert re.search(r'\b%s\s*\(' % name, hdr) and name in _lib.EXPORTS
    assert _lib._RESTYPES['fgnn_qapw_faq_ws_bytes'] is _lib.C.c_longlong
    assert len(_lib._SIGNATURES['fgnn_qapw_faq']) == 18
