"""CPU: the numpy restatement of the on-device QAP pair generator (tests/pairgen_ref.py) -- its Philox stream against numpy's own
Philox4x64-10, the invariants of each family and noise model, its distribution against the reference's generators
(tests/golden/pairgen_stats.npz) -- and the host-side validation of graph_neural_net_amd.pairgen.PairGenerator."""
import numpy as np
import pytest
import torch

import pairgen_ref as R
from pairgen_stats import CONFIGS, gate_failures, statistics
from graph_neural_net_amd.pairgen import PairGenerator, threshold


@pytest.mark.parametrize('key,counter', [(0, 0), (5, 1), (2 ** 64 - 1, 7), (0x0123456789ABCDEF, 2 ** 64 - 2), (99, 3 << 130)])
def test_philox_equals_numpy(key, counter):
    """numpy.random.Philox(key, counter).random_raw() yields the blocks at counter + 1, counter + 2, ... (it steps before it draws)."""
    raw = np.random.Philox(key=key, counter=counter).random_raw(12)
    got = []
    for b in range(3):
        c = (counter + 1 + b) % (1 << 256)
        out = R.philox4x64([np.array([(c >> (64 * i)) & (2 ** 64 - 1)], dtype=np.uint64) for i in range(4)], (key, 0))
        got += [int(x) for x in out[:, 0]]
    assert [int(x) for x in raw] == got


def test_draw_addressing():
    """Draw t is 32-bit word t & 7 (low half first) of the block at counter (t >> 3, pair, stream, 0)."""
    u = R.draws(17, 5, 3, np.arange(16))
    for q in range(2):
        blk = R.philox4x64([np.array([v], dtype=np.uint64) for v in (q, 5, 3, 0)], (17, 0))[:, 0]
        words = [int(b) >> s & 0xFFFFFFFF for b in blk for s in (0, 32)]
        assert u[8 * q:8 * q + 8].tolist() == words
    assert threshold(1.0) == 1 << 32 and threshold(0.5) == 1 << 31 and threshold(0.0) == 0 and threshold(1.5) == 1 << 32


def _check_graph(w, n):
    assert (w == w.T).all() and not w.diagonal().any()
    assert not w[n:].any() and not w[:, n:].any()


@pytest.mark.parametrize('family,noise_model', [(f, m) for f in R.FAMILIES for m in R.NOISE_MODELS])
def test_invariants(family, noise_model):
    N, p = 40, 0.25
    vp = 0.8 if family != 'BarabasiAlbert' else 1.0
    W1, W2, n = R.generate(12, 3, 6, N, family, noise_model, p, 0.2, vp)
    for w1, w2, nk in zip(W1, W2, n.tolist()):
        _check_graph(w1, nk)
        _check_graph(w2, nk)
        deg = w1.sum(1)[:nk]
        if family == 'Regular':
            assert (deg == R.regular_degree(nk, p)).all()
        if family == 'BarabasiAlbert':
            m = R.ba_attachments(nk, p)
            assert w1.sum() // 2 == m * (nk - m)
        if noise_model == 'EdgeSwap':
            assert (w2.sum(1) == w1.sum(1)).all()
    if noise_model == 'EdgeSwap':
        assert (W1 != W2).any()          # the noise does something
    if vp < 1:
        assert len(set(n.tolist())) > 1 and (n >= 2).all()


def test_chunks_give_the_same_pairs():
    for family in ('Regular', 'BarabasiAlbert', 'ErdosRenyi'):
        whole = R.generate(4, 10, 6, 30, family, 'EdgeSwap', 0.3, 0.2)
        parts = [R.generate(4, 10, 2, 30, family, 'EdgeSwap', 0.3, 0.2), R.generate(4, 12, 4, 30, family, 'EdgeSwap', 0.3, 0.2)]
        for i in range(3):
            assert np.array_equal(whole[i], np.concatenate([parts[0][i], parts[1][i]]))


def test_small_and_degenerate_sizes():
    for N in (1, 2, 3):
        for family in ('ErdosRenyi', 'Regular'):
            W1, W2, n = R.generate(0, 0, 3, N, family, 'ErdosRenyi', 0.5, 0.5)
            assert W1.shape == (3, N, N) and (n == N).all()
            for w in W1:
                _check_graph(w, N)
    # a binomial count below 2 is redrawn
    _, _, n = R.generate(0, 0, 20, 2, 'ErdosRenyi', 'ErdosRenyi', 0.5, 0.1, vertex_proba=0.3)
    assert (n == 2).all()


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_statistics_match_the_reference_generators(name, golden_dir):
    """Small K on the host: gate |dmean| <= 4 sqrt(s_ref^2 / K_ref + s^2 / K) against the reference's recorded statistics."""
    cfg = CONFIGS[name]
    fx = np.load('%s/pairgen_stats.npz' % golden_dir)
    K = 150 if cfg['n_vertices'] <= 50 else 6
    W1, W2, n = R.generate(2024, 0, K, cfg['n_vertices'], cfg['generative_model'], cfg['noise_model'], cfg['edge_density'],
                           cfg['noise'], cfg['vertex_proba'])
    st = statistics(torch.from_numpy(W1).double(), torch.from_numpy(W2).double(),
                    None if cfg['vertex_proba'] == 1 else torch.from_numpy(n).double())
    bad = gate_failures(fx, name, {k: v.numpy() for k, v in st.items()})
    assert not bad, bad


def test_host_validation():
    with pytest.raises(ValueError, match='n_vertices'):
        PairGenerator(257, device='cpu')
    with pytest.raises(ValueError, match='n_vertices'):
        PairGenerator(0, device='cpu')
    with pytest.raises(ValueError, match='edge_density'):
        PairGenerator(50, edge_density=1.0, device='cpu')
    with pytest.raises(ValueError, match='noise'):
        PairGenerator(50, noise=1.5, device='cpu')
    with pytest.raises(ValueError, match='Barabasi-Albert'):
        PairGenerator(10, 'BarabasiAlbert', edge_density=0.2, device='cpu')          # m = int(0.2 * 9 / 2) = 0
    with pytest.raises(ValueError, match='constant vertex count'):
        PairGenerator(50, 'BarabasiAlbert', vertex_proba=0.8, device='cpu')
    with pytest.raises(ValueError, match='unknown graph family'):
        PairGenerator(50, 'Grid', device='cpu')
    with pytest.raises(ValueError, match='unknown noise model'):
        PairGenerator(50, noise_model='Flip', device='cpu')
    with pytest.raises(ValueError, match='vertex_proba'):
        PairGenerator(50, vertex_proba=0.0, device='cpu')
    g = PairGenerator.from_config(dict(CONFIGS['regular_er_n50'], num_examples_train=20000, sparsify=None), seed=3, device='cpu')
    assert (g.n_vertices, g.generative_model, g.noise_model, g.edge_density, g.noise, g.seed) == (50, 'Regular', 'ErdosRenyi', 0.2, 0.1, 3)
    assert g.constant_n_vertices
    with pytest.raises(RuntimeError, match='no CPU path'):
        g.bits(0, 4)


def test_library_declares_the_generator():
    from graph_neural_net_amd import _lib
    lib = _lib.load()
    assert lib.fgnn_pairgen_supported(256, 1, 1) == 1 and lib.fgnn_pairgen_supported(257, 0, 0) == 0
    assert lib.fgnn_pairgen_supported(50, 3, 0) == 0 and lib.fgnn_pairgen_supported(50, 0, 2) == 0
