"""GPU: pairs from stored graphs (fgnn_pairstore_gather, PairStore.bits / dense / spectral).  A store filled with a generator's
parents must return that generator's pairs bit for bit; on parents no generator makes the noisy copy is compared with the numpy
restatement of both noise functions (tests/pairgen_ref.py); then the stored second side, caller errors on the device, noise
levels, planted permutations, graph capture, and the epoch loops of FgnnTrainer with a store in the generator's place."""
import os

import numpy as np
import pytest
import torch

import pairgen_ref as R
from graph_neural_net_amd.inputs import expand_adjacency
from graph_neural_net_amd.pairgen import PairGenerator, threshold
from graph_neural_net_amd.pairstore import PairStore
from graph_neural_net_amd.planted import planted_permutation, relabel_bits
from graph_neural_net_amd.sampler import EpochSampler
from graph_neural_net_amd.spectral import spectral_features
from graph_neural_net_amd.synthetic import pack_adjacency

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

K = 24
_perm = np.random.RandomState(0).permutation(K)
# a shuffled arrangement of [0, K), one index once more, and a stretch in descending order (the IDX of test_gpu_pairgen_indexed.py)
IDX = np.concatenate([_perm, _perm[5:6], np.arange(15, 7, -1)]).astype(np.int64)
NOISES = ('ErdosRenyi', 'EdgeSwap')


def dev_index():
    return torch.from_numpy(IDX).to(DEV)


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None and w is None) or (g.dtype == w.dtype and torch.equal(g, w))


def filled_from(gen, M=K, **kw):
    """a store of the generator's first M parents with its settings, and those pairs"""
    whole = gen.bits(0, M)
    kw = dict(dict(noise_model=gen.noise_model, noise=gen.noise, seed=gen.seed, edge_density=gen.edge_density), **kw)
    return PairStore.from_bits(whole[0], sizes=whole[2], **kw), whole


# every family x both noise models at one row block with and without a word boundary inside the row; the 64-lane stride of
# edge_list at N = 64; the smallest graphs and the full word at N = 2 and 32; constant and binomial vertex counts
CASES = [(f, m, N, 1.0) for f in ('ErdosRenyi', 'Regular', 'BarabasiAlbert') for m in NOISES for N in (20, 33)]
CASES += [(f, m, N, 0.8) for f in ('ErdosRenyi', 'Regular') for m in NOISES for N in (20, 33)]
CASES += [('ErdosRenyi', m, N, vp) for m in NOISES for N in (2, 32, 64) for vp in (1.0, 0.8)]
CASES += [('Regular', m, 64, 1.0) for m in NOISES]


@pytest.mark.parametrize('family,noise_model,N,vertex_proba', CASES)
def test_store_of_a_generators_parents_returns_its_pairs(family, noise_model, N, vertex_proba):
    p = 0.5 if N == 2 else 0.2
    gen = PairGenerator(N, family, noise_model, edge_density=p, noise=0.15, vertex_proba=vertex_proba, seed=13, device=DEV)
    store, whole = filled_from(gen)
    assert store.num_examples == K and store.device == DEV and store.constant_n_vertices == (vertex_proba == 1.0) and not store.paired
    assert whole[0].any() and (N == 2 or not torch.equal(whole[0], whole[1]))
    idx = dev_index()
    got = store.bits(index=idx)
    assert got[0].shape == (len(IDX), N, (N + 31) // 32) and got[0].dtype == torch.int32
    same(got, gen.bits(index=idx))
    same(store.bits(0, K), whole)
    same(store.bits(5, 9), gen.bits(5, 9))
    same(store.bits(index=IDX[:3].tolist()), gen.bits(index=IDX[:3].tolist()))          # a list is moved to the device
    if N >= 20:
        store.seed = 14                                                  # a plain attribute: other noise on the same parents
        again = store.bits(index=idx)
        assert torch.equal(again[0], got[0]) and not torch.equal(again[1], got[1])


# ---------------------------------------------------------------------------------------------------------- numpy equality
def _parents():
    """graphs no generator makes, at ragged sizes inside N = 33: (name, (n, n) bool)"""
    def sym(n, edges):
        w = np.zeros((n, n), dtype=bool)
        for u, v in edges:
            w[u, v] = w[v, u] = True
        return w
    cliques = [(u, v) for base in (0, 6) for u in range(base, base + 6) for v in range(u + 1, base + 6)]
    return [('empty', sym(5, [])), ('complete33', sym(33, [(u, v) for u in range(33) for v in range(u + 1, 33)])),
            ('path', sym(20, [(u, u + 1) for u in range(19)])), ('star', sym(32, [(0, v) for v in range(1, 32)])),
            ('cliques', sym(12, cliques)), ('edge', sym(2, [(0, 1)])), ('cycle', sym(9, [(u, (u + 1) % 9) for u in range(9)]))]


def _unpack(bits, N):
    b = bits.cpu().numpy().view(np.uint32)
    return ((b[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(b.shape[0], N, -1)[:, :, :N]


@pytest.fixture(scope='module')
def noise_reference():
    """the numpy copies of every parent, per (noise model, seed): computed once, shared, never changed"""
    graphs = [w for _, w in _parents()]
    edges = sum(int(w.sum()) // 2 for w in graphs)
    slots = sum(len(w) * (len(w) - 1) // 2 for w in graphs)
    p, noise, N = edges / slots, 0.3, 33
    thr1, thr2 = threshold(noise), threshold(p * noise / (1 - p))
    ref = {}
    for seed in (7, (1 << 63) + 11):
        ref['ErdosRenyi', seed] = [R.noise_erdos_renyi(seed, k, w, N, thr1, thr2) for k, w in enumerate(graphs)]
        ref['EdgeSwap', seed] = [R.noise_edge_swap(seed, k, w, thr1) for k, w in enumerate(graphs)]
    return graphs, noise, p, ref


@pytest.mark.parametrize('noise_model', NOISES)
def test_noisy_copies_equal_the_numpy_restatement(noise_model, noise_reference):
    graphs, noise, p, ref = noise_reference
    N, M = 33, len(graphs)
    for seed in (7, (1 << 63) + 11):
        store = PairStore.from_list(graphs, noise_model=noise_model, noise=noise, seed=seed, device=DEV)
        assert store.n_vertices == N and store.edge_density == p and store.max_edges == 33 * 32 // 2
        b1, b2, nv = store.bits(0, M)
        assert nv.tolist() == [len(w) for w in graphs]
        w1, w2 = _unpack(b1, N), _unpack(b2, N)
        changed = 0
        for k, w in enumerate(graphs):
            n = len(w)
            want = ref[noise_model, seed][k]
            assert np.array_equal(w1[k, :n, :n], w) and np.array_equal(w2[k, :n, :n], want), (seed, k)
            assert not w1[k, n:].any() and not w1[k, :, n:].any() and not w2[k, n:].any() and not w2[k, :, n:].any()
            assert (b2[k].cpu().numpy().view(np.uint32) == pack_adjacency(np.pad(want, (0, N - n))[None])[0]).all()      # padding bits too
            changed += int((want != w).any())
        assert changed >= 2                                                # the noise does something on these parents
        rev = torch.arange(M - 1, -1, -1, device=DEV)
        same(store.bits(index=rev), (b1.flip(0), b2.flip(0), nv.flip(0)))


# ------------------------------------------------------------------------------------------- stored second side, caller errors
def _paired_store(N=33, M=K, ragged=True, seed=3):
    rng = np.random.default_rng(seed)
    sizes = [int(rng.integers(4, N + 1)) if ragged else N for _ in range(M)]

    def graph(n):
        w = np.triu(rng.random((n, n)) < 0.3, 1)
        w[0, 1] = True                                                    # no empty graph
        return (w | w.T).astype(np.float32)

    return PairStore.from_list([graph(n) for n in sizes], seconds=[graph(n) for n in sizes], n_vertices=N, seed=seed, device=DEV)


@pytest.mark.parametrize('ragged', (True, False))
def test_paired_store_returns_its_second_side(ragged):
    store = _paired_store(ragged=ragged)
    idx = dev_index()
    assert store.paired and store.parents.any() and not torch.equal(store.parents, store.seconds)
    b1, b2, nv = store.bits(index=idx)
    assert torch.equal(b1, store.parents[idx]) and torch.equal(b2, store.seconds[idx])
    assert (nv is None and store.sizes is None) if not ragged else (nv.dtype == torch.int32 and torch.equal(nv, store.sizes[idx]))
    same(store.bits(4, 7), (store.parents[4:11], store.seconds[4:11], None if not ragged else store.sizes[4:11]))
    p1, p2, pnv, labels = store.bits(index=idx, permute=True)
    want = planted_permutation(store.seed, store.n_vertices, index=idx, nvalid=nv, device=DEV)
    assert torch.equal(labels, want) and torch.equal(p1, b1) and torch.equal(p2, relabel_bits(b2, want, nv))


@pytest.mark.parametrize('vertex_proba', (1.0, 0.8))
def test_from_dense_packs_device_batches(vertex_proba):
    gen = PairGenerator(33, 'Regular', 'ErdosRenyi', vertex_proba=vertex_proba, seed=6, device=DEV)
    b1, b2, nv = gen.bits(0, K)
    x1, x2 = expand_adjacency(b1, 33, nv), expand_adjacency(b2, 33, nv)
    store = PairStore.from_dense(x1, x2, nvalid=nv)
    assert store.paired and store.device == DEV and torch.equal(store.parents, b1) and torch.equal(store.seconds, b2)
    assert (store.sizes is None and nv is None) or torch.equal(store.sizes, nv)
    same(store.bits(0, K), (b1, b2, nv))
    bad = x1.clone()
    bad[3, 0, 1, 2] += 1.0
    with pytest.raises(ValueError):
        PairStore.from_dense(bad, nvalid=nv)
    own = PairStore.from_dense(x1, nvalid=nv, noise_model='EdgeSwap', seed=6)
    assert not own.paired and own.edge_density == own.total_edges / own.total_slots and own.max_edges == int(x1[:, 0].sum((1, 2)).max()) // 2


@pytest.mark.parametrize('kind', NOISES + ('paired',))
@pytest.mark.parametrize('vertex_proba', (1.0, 0.8))
def test_an_index_outside_the_store_gives_the_empty_graph(kind, vertex_proba):
    if kind == 'paired':
        store = _paired_store(N=20, ragged=vertex_proba < 1.0)
    else:
        store, _ = filled_from(PairGenerator(20, 'Regular', kind, vertex_proba=vertex_proba, seed=1, device=DEV))
    M = store.num_examples
    idx = torch.tensor([3, -1, 5, M, 1 << 40, M - 1, -(1 << 40)], dtype=torch.int64, device=DEV)
    b1, b2, nv = store.bits(index=idx)
    torch.cuda.synchronize()                                              # no error: the rows are the documented empty graph
    for b in (b1, b2):
        assert not b[[1, 3, 4, 6]].any() and b[0].any() and b[2].any() and b[5].any()
    same((b1[[0, 2, 5]], b2[[0, 2, 5]]), store.bits(index=[3, 5, M - 1])[:2])
    if nv is not None:
        assert nv[[1, 3, 4, 6]].tolist() == [0, 0, 0, 0] and nv[[0, 2, 5]].tolist() == store.sizes[[3, 5, M - 1]].tolist()


# ------------------------------------------------------------------------------------------------------------------ levels
@pytest.mark.parametrize('noise_model', NOISES)
@pytest.mark.parametrize('vertex_proba', (1.0, 0.8))
def test_levels_equal_a_store_of_that_single_noise(noise_model, vertex_proba):
    noises = (0.0, 0.1, 0.5, 1.0)
    gen = PairGenerator(33, 'ErdosRenyi', noise_model, noise=0.2, vertex_proba=vertex_proba, seed=21, device=DEV)
    store, _ = filled_from(gen)
    idx = dev_index()
    lv = store.levels(noises)
    assert lv.edge_density == store.edge_density and lv.table.device == DEV
    level = torch.arange(len(IDX), device=DEV) % 4
    got = store.bits(index=idx, levels=lv, level=level)
    same(got, gen.bits(index=idx, levels=gen.levels(noises), level=level))
    for j, v in enumerate(noises):
        store.noise = v                                                   # a plain attribute
        single = store.bits(index=idx)
        rows = level == j
        for g, s in zip(got[:2], single[:2]):
            assert torch.equal(g[rows], s[rows])
    assert torch.equal(got[1][level == 0], got[0][level == 0])            # noise 0 is the parent itself
    store.noise = 0.2
    same(store.bits(2, 6, levels=lv, level=[1] * 6), store.bits(index=torch.arange(2, 8), levels=lv, level=[1] * 6))
    # a level outside the table: the empty graph
    bad = level.clone()
    bad[1], bad[4] = 4, -1
    b1, b2, nv = store.bits(index=idx, levels=lv, level=bad)
    keep = torch.ones(len(IDX), dtype=torch.bool, device=DEV)
    keep[1] = keep[4] = False
    assert not b1[~keep].any() and not b2[~keep].any() and torch.equal(b1[keep], got[0][keep]) and torch.equal(b2[keep], got[1][keep])
    assert nv is None or nv[~keep].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------ permute, dense, spectral, capture
@pytest.mark.parametrize('vertex_proba', (1.0, 0.8))
def test_permute_returns_the_planted_labels_and_the_relabelled_second_side(vertex_proba):
    gen = PairGenerator(33, 'Regular', 'ErdosRenyi', vertex_proba=vertex_proba, seed=(1 << 63) + 2, device=DEV)
    store, _ = filled_from(gen)
    idx = dev_index()
    for sel in ({'index': idx}, {'first': 3, 'count': 8}):
        b1, b2, nv = store.bits(**sel)
        p1, p2, pnv, labels = store.bits(permute=True, **sel)
        want = planted_permutation(store.seed, 33, nvalid=nv, device=DEV, **sel)
        assert labels.dtype == torch.int32 and torch.equal(labels, want)
        assert torch.equal(p1, b1) and torch.equal(p2, relabel_bits(b2, want, nv)) and not torch.equal(p2, b2)
        same((p1, p2, pnv, labels), gen.bits(permute=True, **sel))


def test_dense_and_spectral_are_built_from_bits():
    idx = dev_index()
    store, _ = filled_from(PairGenerator(20, 'Regular', 'ErdosRenyi', seed=3, device=DEV))
    b1, b2, nv = store.bits(index=idx)
    x1, x2 = store.dense(index=idx)
    assert torch.equal(x1['input'], expand_adjacency(b1, 20)) and torch.equal(x2['input'], expand_adjacency(b2, 20))
    for kw in ({}, {'n_powers': 2}):
        f1, f2 = store.spectral(index=idx, **kw)
        assert torch.equal(f1['input'], spectral_features(b1, None, kw.get('n_powers', 4)))
        assert torch.equal(f2['input'], spectral_features(b2, None, kw.get('n_powers', 4)))
    *_, labels = store.dense(2, 5, permute=True)
    assert torch.equal(labels, planted_permutation(3, 20, 2, 5, device=DEV))
    gen = PairGenerator(20, 'ErdosRenyi', 'ErdosRenyi', vertex_proba=0.7, seed=3, device=DEV)
    ragged, _ = filled_from(gen)
    b1, b2, nv = ragged.bits(index=idx)
    n = int(nv.max())
    m1, m2 = ragged.dense(index=idx)
    for m, b, name in ((m1, b1, 'N'), (m2, b2, 'M')):
        assert m.tensor.shape == (len(IDX), 2, n, n) and torch.equal(m.tensor, expand_adjacency(b, 20, nv)[:, :, :n, :n])
        assert torch.equal(m.nvalid, nv)
    s1, s2 = ragged.spectral(index=idx)
    assert torch.equal(s1.tensor, spectral_features(b1, nv, 4, n_out=n)) and torch.equal(s2.tensor, spectral_features(b2, nv, 4, n_out=n))
    for mine, theirs in zip(ragged.dense(index=idx) + ragged.spectral(index=idx), gen.dense(index=idx) + gen.spectral(index=idx)):
        assert torch.equal(mine.tensor, theirs.tensor) and torch.equal(mine.nvalid, theirs.nvalid)


@pytest.mark.parametrize('noise_model', NOISES)
def test_a_captured_gather_replays_to_the_same_words(noise_model):
    store, _ = filled_from(PairGenerator(33, 'Regular', noise_model, vertex_proba=0.8, seed=5, device=DEV))
    buf = dev_index()[:8].clone()
    eager = store.bits(index=buf)                                         # (also the kernel's first launch, before any capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = store.bits(index=buf)
    for rep in range(2):
        for t in out:
            t.fill_(-1)
        g.replay()
        same(out, eager)
    buf.copy_(dev_index()[8:16])                                          # the replay reads the index buffer again
    g.replay()
    same(out, store.bits(index=dev_index()[8:16]))


# ------------------------------------------------------------------------------------------------------- through the loops
@pytest.fixture(scope='module')
def model():
    from graph_neural_net_amd.engine import ParamLayout
    lay = ParamLayout(2, 1, 32, 32, 3)
    return lay, lay.init_flat(5, DEV)


@pytest.mark.parametrize('vertex_proba', (1.0, 0.8))
def test_the_epoch_loops_take_a_store_for_a_generator(model, vertex_proba):
    from graph_neural_net_amd.trainer import FgnnTrainer
    lay, p0 = model
    M, B = 8, 4
    gen = PairGenerator(12, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.05, vertex_proba=vertex_proba, seed=4, device=DEV)
    store, _ = filled_from(gen, M)
    shuffled = EpochSampler(M, seed=7, device=DEV)
    plain = EpochSampler(M, shuffle=False, device=DEV)
    noises = (0.0, 0.1, 0.3)
    out = {}
    for name, src in (('generator', gen), ('store', store)):
        tr = FgnnTrainer(lay, p0.clone(), lr=2e-3)
        losses = tr.train_epoch(src, shuffled, 1, B)
        assert losses.shape == (2,) and bool(torch.isfinite(losses).all()) and not torch.equal(tr.params, p0)
        trained = tr.params.clone()
        record = tr.evaluate(src, plain, B).buf.clone()
        curve = tr.noise_curve(src, noises, M, B)
        history = tr.fit(src, shuffled, src, plain, 1, B)
        out[name] = (losses, trained, record, curve.buf.clone(), curve.result(), history, tr.params.clone())
    a, b = out['generator'], out['store']
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])             # train_epoch: losses, then parameters bit for bit
    assert a[2].any() and torch.equal(a[2], b[2])                          # evaluate: the record's bytes
    assert torch.equal(a[3], b[3]) and a[4] == b[4] and len(a[4]) == 3     # noise_curve: one record per level
    (ha,), (hb,) = a[5], b[5]                                              # fit: one epoch's history
    assert torch.equal(ha.pop('train_losses'), hb.pop('train_losses')) and ha == hb and torch.equal(a[6], b[6])


def test_train_epoch_on_the_reference_dataset_fixture(model, golden_dir):
    from graph_neural_net_amd.trainer import FgnnTrainer
    lay, p0 = model
    store = PairStore.from_reference_dataset(os.path.join(golden_dir, 'pairstore_dataset.pt'), device=DEV)
    assert store.paired and store.device == DEV and not store.constant_n_vertices
    for src in (store, PairStore.from_reference_dataset(os.path.join(golden_dir, 'pairstore_dataset.pt'), noisy=True, device=DEV)):
        tr = FgnnTrainer(lay, p0.clone(), lr=2e-3)
        losses = tr.train_epoch(src, EpochSampler(src.num_examples, seed=1, device=DEV), 0, 3)
        assert losses.shape == (2,) and bool(torch.isfinite(losses).all()) and not torch.equal(tr.params, p0)
