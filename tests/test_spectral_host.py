"""Host: tests/spectral_ref.py (the restatement of loaders/data_generator.py:221-232 the GPU tests compare against) held to the
reference's own recorded output (tests/golden/spectral_features.npz) and, where the reference is present, to the imported
reference; plus the one convention it adds (an isolated vertex gives zeros where the reference gives NaN)."""
import os
import sys

import numpy as np
import pytest
import torch

import spectral_ref as R

GROUPS = R.fixture_groups()
# ref_err is a difference against an fp64 chain, which has rounding of its own: entries <= 1 carry <= a few 1e-16 per operation, and
# the last bits of an fp64 1 / sqrt differ between hosts' vector kernels.  Against ref_err >= 1.5e-9 that is below 1e-6 of it.
FP64_NOISE = 1e-6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _make_golden():
    sys.path.insert(0, GOLDEN)
    try:
        import make_golden
    finally:
        sys.path.remove(GOLDEN)
    return make_golden


def _graphs(g):
    for b, n in enumerate(g['nvalid']):
        yield b, R.unpack_bits(g['bits'][b], int(n))


def test_fixture_holds_the_cases_and_no_isolated_vertex():
    assert {g['bits'].shape[1] for k, g in GROUPS.items() if k.startswith('er')} == {7, 33, 50, 64, 65, 120, 200, 256}
    assert {'reg50', 'ragged120', 'directed'} <= set(GROUPS)
    for name, g in GROUPS.items():
        assert ('ref32' in g) == (g['bits'].shape[1] <= 64), name
        assert g['ref_err'].shape == (len(g['nvalid']), R.FIXTURE_POWERS) and (g['ref_err'] < 1e-6).all(), name
        for b, W in _graphs(g):
            assert W.sum(1).min() >= 1, (name, b)                      # the reference is NaN otherwise
            assert np.array_equal(R.pack_bits(W, g['bits'].shape[1]), g['bits'][b]), (name, b)
    W = R.unpack_bits(GROUPS['directed']['bits'][0])
    assert not np.array_equal(W, W.T)
    n = GROUPS['ragged120']['nvalid']
    assert n.min() >= 30 and n.max() <= 120 and len(set(n.tolist())) > 1


@pytest.mark.parametrize('name', sorted(k for k, g in GROUPS.items() if 'ref32' in g))
def test_restatement_equals_the_recorded_reference_bit_for_bit(name):
    g = GROUPS[name]
    for b, W in _graphs(g):
        assert torch.equal(torch.from_numpy(R.features(W, 4, torch.float32)), torch.from_numpy(g['ref32'][b])), (name, b)


@pytest.mark.parametrize('name', sorted(GROUPS))
def test_restatement_reproduces_the_reference_error(name):
    g = GROUPS[name]
    for b, W in _graphs(g):
        err = np.abs(R.features(W, R.FIXTURE_POWERS, torch.float32).astype(np.float64)
                     - R.features(W, R.FIXTURE_POWERS, torch.float64)).max(axis=(1, 2))
        assert np.allclose(err, g['ref_err'][b], rtol=FP64_NOISE, atol=0), (name, b, err, g['ref_err'][b])
    own, _ = R.own_error(g['bits'], g['nvalid'], R.FIXTURE_POWERS)
    assert np.allclose(own, g['ref_err'].max(0), rtol=FP64_NOISE, atol=0)


@pytest.mark.skipif(not os.path.isdir(_make_golden().REF), reason='the reference is not on this machine')
def test_restatement_equals_the_reference_live():
    before = list(sys.path)
    _make_golden().import_reference()
    try:
        from loaders.data_generator import make_laplacian, make_spectral_feature
    finally:
        sys.path[:] = before
    rng = np.random.default_rng(77)
    for n, p in ((5, 0.6), (20, 0.3), (47, 0.2), (90, 0.15)):
        while True:
            A = np.triu(rng.random((n, n)) < p, 1)
            W = (A | A.T).astype(np.float32)
            if W.sum(1).min() >= 1:
                break
        D = (W * (1 - np.triu(rng.random((n, n)) < 0.3, 1))).astype(np.float32)            # directed: some i < j arcs dropped
        for M in (W, D):
            if M.sum(1).min() < 1:
                continue
            want = make_spectral_feature(make_laplacian(torch.from_numpy(M)), 6)
            assert torch.equal(torch.from_numpy(R.features(M, 6, torch.float32)), want), n


def test_isolated_vertex_gives_a_zero_row_and_column_and_finite_values():
    rng = np.random.default_rng(3)
    n = 12
    A = np.triu(rng.random((n, n)) < 0.4, 1)
    W = (A | A.T).astype(np.float64)
    W[5, :] = W[:, 5] = 0
    keep = [i for i in range(n) if i != 5]
    assert W[np.ix_(keep, keep)].sum(1).min() >= 1
    for dtype in (torch.float32, torch.float64):
        F = R.features(W, 4, dtype)
        assert np.isfinite(F).all() and (F[:, 5, :] == 0).all() and (F[:, :, 5] == 0).all()
        # the rest is the graph without that vertex
        assert np.allclose(F[:, keep][:, :, keep], R.features(W[np.ix_(keep, keep)], 4, dtype), rtol=0, atol=1e-6)
    assert (R.features(np.zeros((6, 6)), 4) == 0).all()
    pad = R.padded_features(np.stack([R.pack_bits(W, 40)]), np.array([n]), 4, n_out=20)
    assert pad.shape == (1, 4, 20, 20) and (pad[:, :, n:] == 0).all() and (pad[:, :, :, n:] == 0).all()
    assert np.array_equal(pad[0, :, :n, :n], R.features(W, 4))
