"""CPU: the host route of qap.grampa (numpy float64, the eigen formula itself) and its argument errors."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import grampa_ref as G
import planted_ref as PL
import wigner_ref as W
from graph_neural_net_amd import qap

KEYS = {'X', 'perm', 'qap', 'acc', 'nit', 'res', 'status'}


def _pairs(N=24, count=3, noise=0.1, vertex_proba=1.0):
    labs = []
    for k in range(count):
        n = W.pair(9, k, N, noise, vertex_proba=vertex_proba)[2]
        labs.append(np.concatenate([PL.planted_perm(9, k, n), np.full(N - n, -1)]))
    A, B, n = W.pairs(9, range(count), N, noise, vertex_proba=vertex_proba, labels=labs)
    return A, B, n, np.stack(labs)


def test_cpu_tensors_equal_the_eigen_formula_exactly():
    A, B, n, labs = _pairs(vertex_proba=0.8)
    A4 = np.stack([A, np.full_like(A, np.nan)], 1)                        # channel 0 of a (B, 2, N, N) batch
    out = qap.grampa(torch.from_numpy(A4), torch.from_numpy(B), nvalid=torch.from_numpy(n), labels=torch.from_numpy(labs),
                     weighted=True)
    assert set(out) == KEYS and out['X'].dtype == torch.float64 and out['perm'].dtype == torch.int32
    assert out['nit'].tolist() == [0] * 3 and out['status'].tolist() == [0] * 3
    for b, m in enumerate(n):
        Xa = G.eig(A[b, :m, :m], B[b, :m, :m])
        assert np.array_equal(out['X'][b, :m, :m].numpy(), Xa)
        assert not out['X'][b, m:].any() and not out['X'][b, :, m:].any()
        pi = linear_sum_assignment(-Xa)[1]
        assert out['perm'][b, :m].tolist() == pi.tolist() and (out['perm'][b, m:] == -1).all()
        assert out['res'][b].item() == G.true_residual(A[b, :m, :m], B[b, :m, :m], Xa) < 1e-12
        assert out['acc'][b].item() == int((pi == labs[b, :m]).sum()) == m
        assert out['qap'][b].item() == (A[b, :m, :m] * B[b, :m, :m][pi][:, pi]).sum()


def test_rhs_standardize_and_bit_words_on_the_host():
    A, B, n, _ = _pairs(count=2)
    H = np.random.default_rng(0).random((2, 24, 24)) + 0.5
    out = qap.grampa(torch.from_numpy(A), torch.from_numpy(B), weighted=True, rhs=torch.from_numpy(H), eta=0.3, standardize=True)
    for b in range(2):
        assert np.array_equal(out['X'][b].numpy(), G.eig(G.standardize64(A[b]), G.standardize64(B[b]), eta=0.3, H=H[b]))
    rng = np.random.default_rng(1)
    M = np.triu(rng.random((3, 20, 20)) < 0.3, 1)
    M = (M | M.transpose(0, 2, 1)).astype(np.uint8)
    M[2] = 0                                                              # an empty graph: no variance
    bits = torch.from_numpy(PL.pack_bits(M).view(np.int32))
    out = qap.grampa(bits, bits)                                          # standardize defaults to True on 0/1 input
    assert out['status'].tolist() == [0, 0, 2] and out['qap'].dtype == torch.int64 and out['qap'][2].item() == -1
    assert (out['perm'][2] == -1).all() and not out['X'][2].any()
    for b in range(2):
        S = G.standardize64(M[b])
        assert np.array_equal(out['X'][b].numpy(), G.eig(S, S))
    empty = qap.grampa(torch.from_numpy(A), torch.from_numpy(B), nvalid=torch.tensor([0, 24]), weighted=True)
    assert empty['status'].tolist() == [2, 0]


def test_a_non_symmetric_cpu_input_raises():
    A, B, _, _ = _pairs(count=1)
    with pytest.raises(ValueError, match='not symmetric'):
        qap.grampa(torch.from_numpy(np.triu(A)), torch.from_numpy(B), weighted=True)
    with pytest.raises(ValueError, match='not symmetric'):
        qap.grampa(torch.from_numpy(A), torch.from_numpy(np.tril(B)), weighted=True)


@pytest.mark.parametrize('kw', [{'eta': 0.0}, {'eta': -1.0}, {'eta': float('nan')}, {'eta': float('inf')}, {'tol': 0.0}, {'tol': -1e-3},
                                {'maxiter': 0}, {'maxiter': 1025}, {'maxiter': 2.5}, {'maxiter': True}, {'standardize': 1},
                                {'weighted': 1}, {'rhs': torch.ones(1, 5, 5)}, {'rhs': torch.ones(1, 24, 24, dtype=torch.int64)}])
def test_argument_errors_raise_value_error(kw):
    A, B, _, _ = _pairs(count=1)
    kw = dict({'weighted': True}, **kw)
    with pytest.raises(ValueError):
        qap.grampa(torch.from_numpy(A), torch.from_numpy(B), **kw)


def test_the_three_restatements_agree():
    """(a) and (b) on a symmetric pair, and (c) within fp32 of them"""
    A, B, _, _ = _pairs(N=8, count=1)
    Xa, Xb = G.eig(A[0], B[0]), G.kron_solve(A[0], B[0])
    assert G.rel_err(Xb, Xa) < 1e-10
    Xc, nit, res, status = G.cg32(A[0], B[0], maxiter=256, tol=1e-6)
    assert status == 0 and res < 1e-6 and G.rel_err(Xc, Xa) < 1e-5
