"""GPU: pairs by index list (fgnn_pairgen_indexed, PairGenerator.bits / dense / spectral (index=)), the epoch permutation
(fgnn_epoch_index) bit for bit against its numpy restatement (tests/epoch_ref.py), both under graph capture, and
FgnnTrainer.train_epoch on an EpochSampler."""
import ctypes as C

import numpy as np
import pytest
import torch

import epoch_ref as E
from graph_neural_net_amd import _lib
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.sampler import EpochSampler, epoch_index

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 255, 256, 257, 1000, 20000]
SEEDS = (0, 0xFEDCBA9876543210)
EPOCHS = (0, 1, 1 << 31)

K = 24
_perm = np.random.RandomState(0).permutation(K)
# a shuffled arrangement of [0, K), one index once more, and a stretch in descending order
IDX = np.concatenate([_perm, _perm[5:6], np.arange(15, 7, -1)]).astype(np.int64)


def dev_index():
    return torch.from_numpy(IDX).to(DEV)


@pytest.mark.parametrize('M', SIZES)
def test_epoch_index_equals_restatement(M):
    # the whole epoch once, then windows from the middle of the epoch, across M and far beyond it
    windows = [(0, M), (M // 2, min(M, 70)), (max(M - 3, 0), 10), (5 * M + 1, 9)]
    for seed in SEEDS:
        for epoch in EPOCHS:
            for first, count in (windows if (seed, epoch) == (SEEDS[0], 0) else windows[1:]):
                got = epoch_index(seed, epoch, M, first, count, device=DEV)
                assert got.dtype == torch.int64 and got.shape == (count,)
                ref = torch.from_numpy(E.epoch_index(seed, epoch, M, first, count))
                assert torch.equal(got.cpu(), ref), (seed, epoch, first, count)
    if M == 1:
        assert not epoch_index(3, 4, 1, 0, 5, device=DEV).any()
    out = torch.full((7,), -1, dtype=torch.int64, device=DEV)              # into a caller's buffer, and nothing past the count
    epoch_index(1, 2, M, 3, 5, out=out[:5])
    assert torch.equal(out.cpu(), torch.cat([torch.from_numpy(E.epoch_index(1, 2, M, 3, 5)), torch.tensor([-1, -1])]))


def test_sampler_on_the_device():
    M, B = 50, 4
    for w in (1, 3):
        samplers = [EpochSampler(M, seed=9, rank=r, world_size=w, device=DEV) for r in range(w)]
        steps = samplers[0].steps_per_epoch(B)
        got = torch.stack([torch.stack([s.batch_index(6, step, B) for s in samplers]) for step in range(steps)])    # (steps, w, B)
        assert torch.equal(got.reshape(-1).cpu(), torch.from_numpy(E.epoch_index(9, 6, M, 0, steps * B * w)))
    s = EpochSampler(M, shuffle=False, rank=1, world_size=2, device=DEV)
    assert s.batch_index(3, 6, B).tolist() == [2, 3, 4, 5] and s.batch_index(3, 0, B).device == DEV


CONSTANT = [(f, m, N, 1.0) for f in ('ErdosRenyi', 'Regular', 'BarabasiAlbert') for m in ('ErdosRenyi', 'EdgeSwap') for N in (20, 33)]
CONSTANT += [('Regular', m, 64, 1.0) for m in ('ErdosRenyi', 'EdgeSwap')]
RAGGED = [(f, m, N, 0.8) for f in ('ErdosRenyi', 'Regular') for m in ('ErdosRenyi', 'EdgeSwap') for N in (20, 33)]


@pytest.mark.parametrize('family,noise_model,N,vertex_proba', CONSTANT + RAGGED)
def test_indexed_equals_contiguous(family, noise_model, N, vertex_proba):
    gen = PairGenerator(N, family, noise_model, vertex_proba=vertex_proba, seed=13, device=DEV)
    whole = gen.bits(0, K)
    idx = dev_index()
    got = gen.bits(index=idx)
    assert got[0].shape == (len(IDX), N, (N + 31) // 32) and got[0].dtype == torch.int32
    assert whole[0].any() and not torch.equal(whole[0], whole[1])
    for a, b in zip(got[:2], whole[:2]):
        assert torch.equal(a, torch.index_select(b, 0, idx))
    if vertex_proba == 1.0:
        assert got[2] is None
    else:
        assert got[2].dtype == torch.int32 and torch.equal(got[2], torch.index_select(whole[2], 0, idx))
        assert len(set(whole[2].tolist())) > 1
    # a list and a CPU tensor are moved to the device
    few = gen.bits(index=IDX[:3].tolist())
    assert torch.equal(few[0], got[0][:3]) and torch.equal(gen.bits(index=torch.from_numpy(IDX[:3]))[1], got[1][:3])


def test_arange_index_equals_range():
    for vp in (1.0, 0.8):
        gen = PairGenerator(33, 'Regular', 'ErdosRenyi', vertex_proba=vp, seed=2, device=DEV)
        first, count = (1 << 33) + 5, 7                        # indices beyond 32 bits
        a = gen.bits(first, count)
        b = gen.bits(index=torch.arange(first, first + count, device=DEV))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert (a[2] is None and b[2] is None) if vp == 1.0 else torch.equal(a[2], b[2])
    e = gen.bits(index=torch.zeros(0, dtype=torch.int64, device=DEV))
    assert e[0].shape == (0, 33, 2) and e[2].shape == (0,)


def test_dense_and_spectral_by_index():
    idx = dev_index()
    gen = PairGenerator(20, 'Regular', 'ErdosRenyi', seed=3, device=DEV)
    for whole, got in ((gen.dense(0, K), gen.dense(index=idx)), (gen.spectral(0, K), gen.spectral(index=idx)),
                       (gen.spectral(0, K, n_powers=2), gen.spectral(n_powers=2, index=idx))):
        for w, g in zip(whole, got):
            assert g['input'].shape[0] == len(IDX) and torch.equal(g['input'], torch.index_select(w['input'], 0, idx))
    rg = PairGenerator(20, 'ErdosRenyi', 'ErdosRenyi', vertex_proba=0.7, seed=3, device=DEV)
    for whole, got in ((rg.dense(0, K), rg.dense(index=idx)), (rg.spectral(0, K), rg.spectral(index=idx))):
        for w, g in zip(whole, got):                              # IDX holds every pair of [0, K): both are padded to the same largest n
            assert g.tensor.shape[1:] == w.tensor.shape[1:] and torch.equal(g.tensor, torch.index_select(w.tensor, 0, idx))
            assert torch.equal(g.nvalid, torch.index_select(w.nvalid, 0, idx))


def test_argument_errors_and_negative_index():
    gen = PairGenerator(20, 'Regular', 'EdgeSwap', seed=1, device=DEV)
    idx = torch.tensor([3, -1, 5, -(1 << 40)], dtype=torch.int64, device=DEV)
    for call in (lambda: gen.bits(0, 4, index=idx), lambda: gen.bits(), lambda: gen.bits(4), lambda: gen.dense(0, 4, idx),
                 lambda: gen.spectral(0, 4, index=idx), lambda: gen.spectral(), lambda: gen.bits(index=idx.reshape(2, 2)),
                 lambda: gen.bits(index=idx.to(torch.int32))):
        with pytest.raises(ValueError):
            call()
    # a negative index: the documented empty graph, read from the outputs
    for g in (gen, PairGenerator(33, 'ErdosRenyi', 'ErdosRenyi', vertex_proba=0.8, seed=1, device=DEV)):
        b1, b2, nv = g.bits(index=idx)
        torch.cuda.synchronize()
        for b in (b1, b2):
            assert not b[1].any() and not b[3].any() and b[0].any() and b[2].any()
        assert torch.equal(b1[0], g.bits(3, 1)[0][0]) and torch.equal(b2[2], g.bits(5, 1)[1][0])
        if nv is not None:
            v = nv.tolist()
            assert v[1] == 0 and v[3] == 0 and v[0] >= 2 and v[2] >= 2


def test_capture_epoch_index_then_pairgen_indexed():
    M, B, N, seed = 1000, 8, 33, 5
    gen = PairGenerator(N, 'Regular', 'ErdosRenyi', vertex_proba=0.8, seed=seed, device=DEV)
    eager_idx = epoch_index(seed, 3, M, 17, B, device=DEV)
    eager = gen.bits(index=eager_idx)                         # (also the first launch of both kernels, before any capture)
    buf = torch.zeros(B, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        epoch_index(seed, 3, M, 17, B, out=buf)
        out = gen.bits(index=buf)
    for rep in range(2):                                      # the replay rewrites the index buffer and everything after it
        buf.fill_(-1)
        for t in out:
            t.fill_(-1)
        g.replay()
        assert torch.equal(buf, eager_idx)
        assert all(torch.equal(a, b) for a, b in zip(out, eager))
    # the generator launch alone, replayed on an index buffer that another epoch's order has been written into
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        out2 = gen.bits(index=buf)
    for epoch in (4, 1 << 31):
        epoch_index(seed, epoch, M, 990, B, out=buf)          # a window that crosses M
        g2.replay()
        want = gen.bits(index=torch.from_numpy(E.epoch_index(seed, epoch, M, 990, B)).to(DEV))
        assert all(torch.equal(a, b) for a, b in zip(out2, want))
    args = _lib.PairgenArgs()                                 # the raw entry point takes the same struct as fgnn_pairgen; first is ignored
    args.seed, args.first, args.B, args.N, args.family, args.noise_model = seed, -99, B, N, 1, 0
    args.edge_density, args.swaps_per_edge = gen.edge_density, gen.swaps_per_edge
    args.thr_edge, args.thr_noise1, args.thr_noise2, args.thr_vertex = gen._thr
    raw = [torch.empty_like(t) for t in eager]
    args.bits1, args.bits2, args.nvalid = (t.data_ptr() for t in raw)
    _lib.call('fgnn_pairgen_indexed', C.byref(args), _lib.ptr(eager_idx), _lib.stream_ptr())
    assert all(torch.equal(a, b) for a, b in zip(raw, eager))


def test_train_epoch():
    from graph_neural_net_amd.engine import ParamLayout
    from graph_neural_net_amd.trainer import FgnnTrainer
    lay = ParamLayout(2, 1, 32, 32, 3)
    p0 = lay.init_flat(5, DEV)
    gen = PairGenerator(16, 'Regular', 'ErdosRenyi', edge_density=0.25, noise=0.05, seed=4, device=DEV)
    M, B = 12, 4

    def epoch(shuffle, seed=7):
        tr = FgnnTrainer(lay, p0.clone(), lr=2e-3)
        losses = tr.train_epoch(gen, EpochSampler(M, seed=seed, shuffle=shuffle, device=DEV), 1, B)
        assert losses.shape == (3,) and losses.is_cuda and bool(torch.isfinite(losses).all())
        return tr.params.clone(), losses

    by_hand = FgnnTrainer(lay, p0.clone(), lr=2e-3)
    hand_losses = [by_hand.train_step_bits(*gen.bits(B * s, B))[0] for s in range(3)]
    plain, plain_losses = epoch(False)
    assert torch.equal(plain, by_hand.params) and torch.equal(plain_losses, torch.stack(hand_losses))
    a, la = epoch(True)
    b, lb = epoch(True)
    assert torch.equal(a, b) and torch.equal(la, lb)
    assert not torch.equal(a, plain) and not torch.equal(a, p0)
