"""CPU: the numpy restatement of the epoch permutation (tests/epoch_ref.py) -- a bijection at every size class, independent of how
an epoch is cut, wrapping past M, different per epoch and seed, uniform in its margins -- and the host arithmetic of
graph_neural_net_amd.sampler.EpochSampler (which positions a rank takes at a step), with the restatement standing in for the kernel."""
import numpy as np
import pytest
import torch

import epoch_ref as E
from graph_neural_net_amd.sampler import EpochSampler, epoch_index

SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 255, 256, 257, 1000, 20000]


def test_half_bits():
    assert [E.half_bits(M) for M in (1, 2, 3, 4, 5, 16, 17, 64, 65, 256, 257, 20000, 1 << 40)] == [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 8, 20]


@pytest.mark.parametrize('M', SIZES)
def test_bijection(M):
    for seed, epoch in ((0, 0), (7, 3)):
        p = E.epoch_index(seed, epoch, M, 0, M)
        assert p.dtype == np.int64 and np.array_equal(np.sort(p), np.arange(M))
    if M == 1:
        assert E.epoch_index(5, 9, 1, 3, 4).tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize('M', [5, 33, 1000])
def test_independent_of_the_cut_and_wrap(M):
    whole = E.epoch_index(2, 5, M, 0, M)
    for a, c in ((0, 1), (M // 3, M // 2), (M - 1, 1), (M // 2, M - M // 2)):
        assert np.array_equal(E.epoch_index(2, 5, M, a, c), whole[a:a + c])
    # positions >= M are positions mod M of the same epoch: a window that crosses M, and one far beyond it
    assert np.array_equal(E.epoch_index(2, 5, M, M - 2, 5), np.concatenate([whole[M - 2:], whole[:3]]))
    assert np.array_equal(E.epoch_index(2, 5, M, 7 * M + 1, 3), np.resize(whole, 2 * M + 4)[1:4])


def test_epochs_and_seeds_differ():
    a, b, c = (E.epoch_index(s, e, 1000, 0, 1000) for s, e in ((0, 0), (0, 1), (1, 0)))
    assert (a == b).sum() < 20 and (a == c).sum() < 20          # 1 expected
    assert not np.array_equal(a, np.arange(1000))


def test_marginal_uniformity():
    """M = 8, epochs 0 .. 4095: every value at position 0 between 400 and 624 times (512 +- 5 sigma, sigma = sqrt(4096 * 7 / 64) = 21.2)."""
    v = E.permute(0, range(4096), 8, [0] * 4096)
    counts = np.bincount(v, minlength=8)
    print('counts at position 0:', counts.tolist())
    assert counts.sum() == 4096 and counts.min() >= 400 and counts.max() <= 624, counts


def _epoch_of(sampler, epoch, B):
    """every rank's indices of one epoch, the restatement standing in for the kernel: (ranks, steps * B)"""
    out = []
    for r in range(sampler.world_size):
        s = EpochSampler(sampler.num_examples, sampler.seed, sampler.shuffle, r, sampler.world_size, sampler.drop_last)
        out.append(np.concatenate([E.epoch_index(s.seed, epoch, s.num_examples, *s.window(step, B))
                                   for step in range(s.steps_per_epoch(B))] or [np.zeros(0, dtype=np.int64)]))
    return np.stack(out)


@pytest.mark.parametrize('w', [1, 2, 3])
def test_sampler_arithmetic(w):
    M, B = 50, 4
    s = EpochSampler(M, seed=3, world_size=w)
    steps = s.steps_per_epoch(B)
    assert steps == -(-M // (B * w))
    idx = _epoch_of(s, 2, B)
    assert idx.shape == (w, steps * B)
    counts = np.bincount(idx.reshape(-1), minlength=M)
    assert len(counts) == M and counts.min() >= 1 and counts.max() <= 2           # padded by wrapping: nothing missing, nothing thrice
    # the ranks' slices interleave into the epoch order: global step s = positions [s B w, (s + 1) B w)
    order = idx.reshape(w, steps, B).transpose(1, 0, 2).reshape(-1)
    assert np.array_equal(order, E.epoch_index(3, 2, M, 0, steps * B * w))
    d = EpochSampler(M, seed=3, world_size=w, drop_last=True)
    assert d.steps_per_epoch(B) == M // (B * w)
    idx = _epoch_of(d, 2, B)
    assert idx.size == d.steps_per_epoch(B) * B * w and np.bincount(idx.reshape(-1), minlength=M).max() <= 1
    with pytest.raises(ValueError, match='step'):
        d.window(d.steps_per_epoch(B), B)


def test_unshuffled_order_is_arange():
    s = EpochSampler(50, shuffle=False, device='cpu')
    got = torch.cat([s.batch_index(4, step, 4) for step in range(s.steps_per_epoch(4))])
    assert got.dtype == torch.int64 and torch.equal(got, torch.arange(52) % 50)
    r1 = EpochSampler(50, shuffle=False, rank=1, world_size=2, device='cpu')
    assert r1.batch_index(0, 1, 4).tolist() == [12, 13, 14, 15] and r1.batch_index(0, 6, 4).tolist() == [2, 3, 4, 5]
    assert EpochSampler(50, shuffle=False, drop_last=True, device='cpu').steps_per_epoch(4) == 12


def test_host_validation():
    for kw in (dict(num_examples=0), dict(num_examples=(1 << 40) + 1), dict(num_examples=5, rank=2, world_size=2),
               dict(num_examples=5, world_size=0), dict(num_examples=5, seed=-1)):
        with pytest.raises(ValueError):
            EpochSampler(**kw)
    with pytest.raises(ValueError, match='batch_size'):
        EpochSampler(5).steps_per_epoch(0)
    cfg = dict(num_examples_train=20000, num_examples_val=1000, n_vertices=50)
    assert EpochSampler.from_config(cfg).num_examples == 20000
    assert EpochSampler.from_config(cfg, split='val', shuffle=False).num_examples == 1000
    with pytest.raises(KeyError):
        EpochSampler.from_config(cfg, split='test')
    with pytest.raises(ValueError, match='split'):
        EpochSampler.from_config(cfg, split='dev')
    with pytest.raises(RuntimeError, match='no CPU path'):
        EpochSampler(5, device='cpu').batch_index(0, 0, 2)
    with pytest.raises(ValueError, match='num_examples'):
        epoch_index(0, 0, 0, 0, 4, device='cpu')


def test_library_refuses_bad_arguments():
    """fgnn_epoch_index checks M and count before it launches anything (no GPU needed to be refused)."""
    from graph_neural_net_amd import _lib
    lib = _lib.load()
    for M, first, count in ((0, 0, 4), ((1 << 40) + 1, 0, 4), (8, 0, -1), (8, 0, 1 << 31), (8, -1, 4)):
        assert lib.fgnn_epoch_index(0, 0, M, first, count, None, None) == 1
        assert b'fgnn_epoch_index' in lib.fgnn_last_error()
    assert lib.fgnn_epoch_index(0, 0, 8, 0, 0, None, None) == 0           # an empty window is no launch
    args = _lib.PairgenArgs()
    args.N, args.B, args.bits1, args.bits2, args.thr_vertex, args.first = 20, 4, 8, 8, 1 << 32, -5
    assert lib.fgnn_pairgen_indexed(args, None, None) == 1 and b'NULL index' in lib.fgnn_last_error()
    assert lib.fgnn_pairgen(args, None) == 1 and b'bad arguments' in lib.fgnn_last_error()
