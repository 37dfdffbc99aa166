"""CPU: the host route of qap.degree_profile (numpy float64) against tests/degree_profile_ref.py, the integer-grid W1 against a
brute-force integral, the statuses, the argument errors and the declarations of the two new entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import degree_profile_ref as D
import pairgen_ref as PR
import planted_ref as PL
import wigner_ref as W
from graph_neural_net_amd import _lib, evaluation, qap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {'X', 'perm', 'qap', 'acc', 'status'}


def _wigner(N=20, count=3, noise=0.1, vertex_proba=1.0):
    labs = []
    for k in range(count):
        n = W.pair(9, k, N, noise, vertex_proba=vertex_proba)[2]
        labs.append(np.concatenate([PL.planted_perm(9, k, n), np.full(N - n, -1)]))
    A, B, n = W.pairs(9, range(count), N, noise, vertex_proba=vertex_proba, labels=labs)
    return A, B, n, np.stack(labs)


def _er(N=24, count=3, noise=0.02, vertex_proba=1.0, p=0.3):
    M1, M2, n = PR.generate(4, 0, count, N, 'ErdosRenyi', 'ErdosRenyi', p, noise, vertex_proba)
    return M1.astype(np.uint8), M2.astype(np.uint8), n


def _bits(M):
    return torch.from_numpy(PL.pack_bits(M).view(np.int32))


def _check_pair(out, b, A, B, weighted, lab=None):
    """every key of pair b against the restatement on the corners A, B (exact)"""
    n = len(A)
    Z, status, sides = D.pair(A, B, weighted)
    assert out['status'][b].item() == status
    X = out['X'][b].numpy()
    assert not X[n:].any() and not X[:, n:].any()
    if status:
        assert not X.any() and (out['perm'][b] == -1).all() and out['qap'][b].item() == -1
        return
    assert np.array_equal(X[:n, :n], -Z)
    pi = D.matching(Z)
    assert out['perm'][b, :n].tolist() == pi.tolist() and (out['perm'][b, n:] == -1).all()
    assert out['qap'][b].item() == (A * B[pi][:, pi]).sum()
    assert out['acc'][b].item() == int((pi == (np.arange(n) if lab is None else lab[:n])).sum())
    if 'profiles' in out:
        for side, rows in enumerate(sides):
            slab, cnt = out['profiles'][side][b].numpy(), out['counts'][b, side].numpy()
            assert cnt[:n].tolist() == [len(r) for r in rows] and not cnt[n:].any()
            for i, r in enumerate(rows):
                assert np.array_equal(slab[i, :len(r)], r) and np.isposinf(slab[i, len(r):]).all()
            assert np.isposinf(slab[n:]).all()


def test_cpu_weighted_equals_the_restatement_exactly():
    A, B, n, labs = _wigner(vertex_proba=0.8)
    A4 = np.stack([A, np.full_like(A, np.nan)], 1)                        # channel 0 of a (B, 2, N, N) batch
    out = qap.degree_profile(torch.from_numpy(A4), torch.from_numpy(B), nvalid=torch.from_numpy(n), labels=torch.from_numpy(labs),
                             weighted=True, return_profiles=True)
    assert set(out) == KEYS | {'profiles', 'counts'}
    assert out['X'].dtype == torch.float64 and out['perm'].dtype == torch.int32 and out['counts'].dtype == torch.int32
    assert out['status'].dtype == torch.int64 and out['acc'].dtype == torch.int64
    for b, m in enumerate(n):
        _check_pair(out, b, A[b, :m, :m], B[b, :m, :m], True, labs[b])
    plain = qap.degree_profile(torch.from_numpy(A), torch.from_numpy(B), nvalid=torch.from_numpy(n), weighted=True)
    assert set(plain) == KEYS and torch.equal(plain['X'], out['X'])


def test_cpu_bit_words_and_dense_input_equal_the_restatement_exactly():
    M1, M2, n = _er(vertex_proba=0.9)
    out = qap.degree_profile(_bits(M1), _bits(M2), nvalid=torch.from_numpy(n), return_profiles=True)
    assert out['qap'].dtype == torch.int64
    for b, m in enumerate(n):
        _check_pair(out, b, M1[b, :m, :m].astype(np.int64), M2[b, :m, :m].astype(np.int64), False)
    dense = [torch.from_numpy(np.stack([M.astype(np.float32), np.stack([np.diag(x.sum(1)) for x in M]).astype(np.float32)], 1))
             for M in (M1, M2)]
    again = qap.degree_profile(dense[0], dense[1], nvalid=torch.from_numpy(n))
    assert torch.equal(again['X'], out['X']) and torch.equal(again['perm'], out['perm'])


def test_host_route_beyond_256_vertices_takes_any_device_tensor():
    """N > 256 goes to the host whatever the device: here a CPU batch of N = 258 with a small corner"""
    A, B, n, _ = _wigner(N=12, count=1)
    big1, big2 = np.full((1, 258, 258), np.nan), np.full((1, 258, 258), np.nan)
    big1[0, :12, :12], big2[0, :12, :12] = A[0], B[0]
    out = qap.degree_profile(torch.from_numpy(big1), torch.from_numpy(big2), nvalid=torch.tensor([12]), weighted=True)
    _check_pair(out, 0, A[0], B[0], True)


def test_grid_w1_equals_the_brute_force_integral():
    """random lists of unequal lengths 1 .. 9 with repeated values: the loop, the blocked sums and int |F - G| agree"""
    rng = np.random.default_rng(0)
    for _ in range(300):
        a = np.sort(rng.integers(-3, 4, rng.integers(1, 10)) * 0.37)
        b = np.sort(rng.integers(-3, 4, rng.integers(1, 10)) * 0.37 + rng.integers(0, 2) * 0.11)
        z = D.w1_grid(a, b)
        assert abs(z - D.w1_brute(a, b)) <= 1e-13
        assert D.w1_matrix([a], [b])[0, 0] == z == qap._profile_distances([a], [b])[0, 0]
        if len(a) == len(b):
            assert abs(z - np.abs(a - b).mean()) <= 1e-13


def test_empty_profiles_and_full_rows():
    """an isolated vertex has the point mass at 0 for a profile; a vertex adjacent to all others has r = 0 and the values 0"""
    n = 9
    M = np.zeros((n, n), dtype=np.int64)
    M[0, 1:8] = M[1:8, 0] = 1                                              # vertex 0: adjacent to all but the isolated vertex 8
    M[1, 2] = M[2, 1] = M[3, 4] = M[4, 3] = 1
    M2 = M.copy()
    M2[0, 8] = M2[8, 0] = 1                                                # side 2: vertex 0 adjacent to ALL others, r = 0
    M2[5, 5] = 1                                                           # a self-loop: ignored
    out = qap.degree_profile(_bits(M[None].astype(np.uint8)), _bits(M2[None].astype(np.uint8)), return_profiles=True)
    assert out['status'].tolist() == [0]
    assert out['counts'][0, 0].tolist() == [7, 2, 2, 2, 2, 1, 1, 1, 0] and out['counts'][0, 1].tolist() == [8, 2, 2, 2, 2, 1, 1, 1, 1]
    assert np.isposinf(out['profiles'][0][0, 8].numpy()).all()
    assert not out['profiles'][1][0, 0, :8].any()                          # r = 0: eight zeros
    P1, P2 = D.bit_profiles(M), D.bit_profiles(M2)
    assert len(P1[8]) == 0
    Z = -out['X'][0].numpy()
    assert Z[8, 0] == 0.0                                                  # point mass at 0 against eight zeros
    for j in range(n):
        assert Z[8, j] == D.w1_grid([], P2[j]) == np.abs(P2[j]).mean()
    M2[5, 5] = 0
    _check_pair(out, 0, M, M2, False)


def test_status_2_and_3():
    A, B, n, _ = _wigner(count=3)
    A[1, 2, 3] = np.inf
    out = qap.degree_profile(torch.from_numpy(A), torch.from_numpy(B), nvalid=torch.tensor([20, 20, 1]), weighted=True,
                             return_profiles=True)
    assert out['status'].tolist() == [0, 3, 2]
    assert not out['X'][1:].any() and (out['perm'][1:] == -1).all() and out['qap'][1:].tolist() == [-1, -1]
    assert torch.isposinf(out['profiles'][0][1:]).all() and not out['counts'][1:].any()
    B[0, 4, 4] = np.nan                                                    # the diagonal lies inside the corner
    assert qap.degree_profile(torch.from_numpy(A), torch.from_numpy(B), weighted=True)['status'].tolist() == [3, 3, 0]
    M1, M2, _ = _er(count=4)
    M1[1] = 0                                                              # an empty graph
    M2[2] = 1 - np.eye(24, dtype=np.uint8)                                 # a complete graph
    out = qap.degree_profile(_bits(M1), _bits(M2), nvalid=torch.tensor([24, 24, 24, 0]))
    assert out['status'].tolist() == [0, 2, 2, 2] and out['qap'].tolist()[1:] == [-1, -1, -1]
    assert not out['X'][1:].any() and (out['perm'][1:] == -1).all() and sorted(out['perm'][0].tolist()) == list(range(24))


@pytest.mark.parametrize('kw', [{'weighted': 1}, {'weighted': None}, {'return_profiles': 1}, {'return_profiles': 'yes'}])
def test_argument_errors_raise_value_error(kw):
    A, B, _, _ = _wigner(count=1)
    kw = dict({'weighted': True}, **kw)
    with pytest.raises(ValueError):
        qap.degree_profile(torch.from_numpy(A), torch.from_numpy(B), **kw)


def test_empty_batch_and_too_many_pairs_raise_value_error():
    with pytest.raises(ValueError, match='empty batch'):
        qap.degree_profile(torch.zeros(0, 5, 5), torch.zeros(0, 5, 5), weighted=True)
    with pytest.raises(ValueError, match='empty batch'):
        qap.degree_profile(torch.zeros(2, 0, 0), torch.zeros(2, 0, 0), weighted=True)

    class OnDevice:                                                        # the limit is checked before anything is launched
        is_cuda, shape, device = True, (qap.DEGREE_PROFILE_MAX_B + 1, 4, 4), torch.device('cpu')

    with pytest.raises(ValueError, match='at most 65535 pairs'):
        qap.degree_profile(OnDevice(), OnDevice(), weighted=True)


def test_new_declarations_have_signatures():
    hdr = open(os.path.join(ROOT, 'include', 'fgnn_hip.h')).read()
    lib = _lib.load()
    ctype = {'const float *': ctypes.c_void_p, 'const unsigned *': ctypes.c_void_p, 'const int *': ctypes.c_void_p,
             'float *': ctypes.c_void_p, 'int *': ctypes.c_void_p, 'void *': ctypes.c_void_p, 'long long': ctypes.c_longlong,
             'int': ctypes.c_int}
    for name, ret in (('fgnn_degree_profile_ws_bytes', 'long long'), ('fgnn_degree_profile', 'int')):
        m = re.search(r'\b(int|long long)\s+%s\s*\(([^;]*)\);' % name, hdr)
        assert m and m.group(1) == ret, '%s is not declared in include/fgnn_hip.h' % name
        params = [re.sub(r'/\*.*?\*/', '', p).strip() for p in m.group(2).split(',')]
        types = [re.match(r'(.*?)\s*\w+$', p).group(1).strip() for p in params]
        assert name in _lib._SIGNATURES and name in _lib.EXPORTS and hasattr(lib, name)
        assert [ctype[t] for t in types] == _lib._SIGNATURES[name], (name, types)         # one ctypes type per C parameter
        assert (_lib._RESTYPES.get(name) is not None) == (ret == 'long long')
    assert lib.fgnn_degree_profile_ws_bytes(0, 5) == 0 and lib.fgnn_degree_profile_ws_bytes(5, 0) == 0
    assert lib.fgnn_degree_profile_ws_bytes(8, 256) >= 3 * 8 * 256 * 256 * 4 + 2 * 8 * 2 * 256 * 4
    assert qap.DEGREE_PROFILE_MAX_B == 65535


def test_baseline_curve_refuses_an_unknown_method_and_a_stray_keyword():
    class NeverCalled:
        def __getattr__(self, name):
            raise AssertionError('baseline_curve touched the generator (%s) before refusing its arguments' % name)

    assert evaluation.BASELINE_METHODS == ('grampa', 'degree_profile')
    with pytest.raises(ValueError, match="'grampa' or 'degree_profile'"):
        evaluation.baseline_curve(NeverCalled(), (0.0,), 4, 2, method='nope')
    with pytest.raises(ValueError, match="'eta'"):
        evaluation.baseline_curve(NeverCalled(), (0.0,), 4, 2, method='degree_profile', eta=0.2)
    with pytest.raises(ValueError, match="'return_profile'"):
        evaluation.baseline_curve(NeverCalled(), (0.0,), 4, 2, method='degree_profile', return_profile=True)
    with pytest.raises(ValueError, match="'bandwidth'"):
        evaluation.baseline_curve(NeverCalled(), (0.0,), 4, 2, method='grampa', bandwidth=0.2)
