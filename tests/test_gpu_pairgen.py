"""GPU: the on-device QAP pair generator (csrc/pairgen.hip, graph_neural_net_amd/pairgen.py) -- bit for bit against the numpy
restatement (tests/pairgen_ref.py), independent of how a range is split, distributed like the reference's generators
(tests/golden/pairgen_stats.npz), consistent with the existing input path, and good training data."""
import numpy as np
import pytest
import torch

import pairgen_ref as R
from pairgen_stats import CONFIGS, STATS, gate_failures, statistics
from graph_neural_net_amd import synthetic
from graph_neural_net_amd.inputs import expand_adjacency, pack_tensor_representation
from graph_neural_net_amd.pairgen import PairGenerator

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def packed(w):
    return torch.from_numpy(synthetic.pack_adjacency(w).view(np.int32)).to(DEV)


def check_equal(gen, first, count):
    b1, b2, nv = gen.bits(first, count)
    W1, W2, n = R.generate(gen.seed, first, count, gen.n_vertices, gen.generative_model, gen.noise_model, gen.edge_density,
                           gen.noise, gen.vertex_proba, gen.swaps_per_edge)
    assert torch.equal(b1, packed(W1)), 'parent graphs differ'
    assert torch.equal(b2, packed(W2)), 'noisy graphs differ'
    if gen.constant_n_vertices:
        assert nv is None
    else:
        assert nv.cpu().tolist() == n.tolist()
    return b1, b2, nv, n


CASES = [(f, m, N) for f in ('ErdosRenyi', 'Regular', 'BarabasiAlbert') for m in ('ErdosRenyi', 'EdgeSwap')
         for N in (2, 17, 50, 64, 65, 200, 256) if not (f == 'BarabasiAlbert' and N < 17)]


@pytest.mark.parametrize('family,noise_model,N', CASES)
def test_device_equals_restatement(family, noise_model, N):
    count = 3 if N <= 65 else 1
    seed = 11 if N % 2 else 0xFEDCBA9876543210
    gen = PairGenerator(N, family, noise_model, seed=seed, device=DEV)
    b1, b2, _, _ = check_equal(gen, 1000 + N, count)
    words = (N + 31) // 32
    if N % 32:                                     # the padding bits of the last word are zero
        pad = torch.tensor(-(1 << (N % 32)), dtype=torch.int32, device=DEV)
        assert not (b1[:, :, words - 1] & pad).any() and not (b2[:, :, words - 1] & pad).any()


@pytest.mark.parametrize('family', ['ErdosRenyi', 'Regular', 'BarabasiAlbert'])
def test_two_seeds_and_noise_levels(family):
    for seed, noise, p in ((3, 0.3, 0.25), (2 ** 40 + 7, 0.05, 0.15)):
        gen = PairGenerator(50, family, 'ErdosRenyi' if seed == 3 else 'EdgeSwap', edge_density=p, noise=noise, seed=seed, device=DEV)
        check_equal(gen, 7, 4)


@pytest.mark.parametrize('family,noise_model', [(f, m) for f in ('ErdosRenyi', 'Regular') for m in ('ErdosRenyi', 'EdgeSwap')])
def test_ragged_equals_restatement(family, noise_model):
    gen = PairGenerator(120, family, noise_model, vertex_proba=0.8, seed=5, device=DEV)
    b1, b2, nv, n = check_equal(gen, 40, 3)
    for k, nk in enumerate(n.tolist()):            # rows / columns >= n_k are empty
        assert 2 <= nk <= 120 and not b1[k, nk:].any() and not b2[k, nk:].any()
    assert nv.dtype == torch.int32


def test_chunks_and_generators_are_independent():
    for family, vp in (('Regular', 1.0), ('ErdosRenyi', 0.8)):
        g = PairGenerator(50, family, 'ErdosRenyi', vertex_proba=vp, seed=21, device=DEV)
        whole = g.bits(0, 64)
        parts = [g.bits(0, 40), PairGenerator(50, family, 'ErdosRenyi', vertex_proba=vp, seed=21, device=DEV).bits(40, 24)]
        for i in range(2):
            assert torch.equal(whole[i], torch.cat([parts[0][i], parts[1][i]]))
        if vp < 1:
            assert torch.equal(whole[2], torch.cat([parts[0][2], parts[1][2]]))
        other = PairGenerator(50, family, 'ErdosRenyi', vertex_proba=vp, seed=22, device=DEV).bits(0, 64)
        assert not torch.equal(whole[0], other[0])


def test_consistent_with_the_input_path():
    gen = PairGenerator(50, 'Regular', 'ErdosRenyi', seed=9, device=DEV)
    b1, b2, _ = gen.bits(3, 4)
    W1, W2, _ = R.generate(9, 3, 4, 50)
    x1 = expand_adjacency(b1, 50)
    ref = torch.from_numpy(np.stack([synthetic.tensor_representation(w.astype(np.float32)) for w in W1])).to(DEV)
    assert torch.equal(x1, ref)
    assert torch.equal(pack_tensor_representation(x1), b1)
    assert torch.equal(pack_tensor_representation(expand_adjacency(b2, 50)), b2)
    d1, d2 = gen.dense(3, 4)
    assert torch.equal(d1['input'], x1) and torch.equal(d2['input'], expand_adjacency(b2, 50))
    rg = PairGenerator(60, 'ErdosRenyi', 'ErdosRenyi', vertex_proba=0.7, seed=9, device=DEV)
    m1, m2 = rg.dense(0, 5)
    c1, c2, nv = rg.bits(0, 5)
    n = int(nv.max())
    assert m1.tensor.shape == (5, 2, n, n) and torch.equal(m1.nvalid.cpu(), nv.cpu())
    assert torch.equal(m2.tensor, expand_adjacency(c2, 60, nv)[:, :, :n, :n])


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_statistics_match_the_reference_generators(name, golden_dir):
    """Thousands of pairs per config, statistics on the device, gate |dmean| <= 4 sqrt(s_ref^2 / K_ref + s^2 / K) against the
    fixture recorded from the reference's own generators."""
    cfg = CONFIGS[name]
    fx = np.load('%s/pairgen_stats.npz' % golden_dir)
    K = 4000 if cfg['n_vertices'] <= 120 else 1000
    gen = PairGenerator.from_config(cfg, seed=77, device=DEV)
    b1, b2, nv = gen.bits(0, K)
    N = cfg['n_vertices']
    x1 = expand_adjacency(b1, N, nv)[:, 0].double()
    x2 = expand_adjacency(b2, N, nv)[:, 0].double()
    st = statistics(x1, x2, None if nv is None else nv.double())
    bad = gate_failures(fx, name, {k: v.cpu().numpy() for k, v in st.items()})
    assert not bad, bad


def test_training_on_generated_pairs():
    from graph_neural_net_amd.engine import ParamLayout
    from graph_neural_net_amd.trainer import FgnnTrainer
    # bits path == dense path on the same generated pairs (the structured block 1's rounding class, tests/test_gpu_struct.py)
    lay = ParamLayout(2, 2, 32, 32, 3)
    p0 = lay.init_flat(5, DEV)
    gen = PairGenerator(24, 'Regular', 'ErdosRenyi', edge_density=0.25, noise=0.05, seed=4, device=DEV)
    losses = {}
    for mode in ('bits', 'dense'):
        tr = FgnnTrainer(lay, p0.clone(), lr=2e-3, precision='fp32', block1='structured')
        out = []
        for s in range(3):
            if mode == 'bits':
                b1, b2, _ = gen.bits(4 * s, 4)
                loss, _ = tr.train_step_bits(b1, b2)
            else:
                d1, d2 = gen.dense(4 * s, 4)
                loss, _ = tr.train_step(d1['input'], d2['input'])
            out.append(loss.item())
        losses[mode] = out
    for a, b in zip(losses['bits'], losses['dense']):
        assert abs(a - b) <= 2e-4 * abs(b)
    # 300 steps on fresh pairs every step (B = 32, N = 50): the loss comes down
    lay = ParamLayout(2, 4, 32, 32, 3)
    tr = FgnnTrainer(lay, lay.init_flat(0, DEV), lr=1e-3, capture=True)
    gen = PairGenerator.from_config(CONFIGS['regular_er_n50'], seed=1, device=DEV)
    hist = []
    for s in range(300):
        b1, b2, _ = gen.bits(32 * s, 32)
        loss, _ = tr.train_step_bits(b1, b2)
        hist.append(loss.item())
    hist = np.array(hist)
    assert hist[-25:].mean() < hist[:25].mean(), (hist[:25].mean(), hist[-25:].mean())
