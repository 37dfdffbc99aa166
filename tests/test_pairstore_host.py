"""Host side of the stored-graph source (graph_neural_net_amd/pairstore.py, csrc/pairstore.hip): the C interface and its ctypes
mirror, the constructors' validation and packing against synthetic.pack_adjacency, argument checks that run without a GPU, the
density arithmetic, save / load, and the reference's dataset fixture."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from graph_neural_net_amd import _lib
from graph_neural_net_amd.pairgen import NoiseLevels, threshold
from graph_neural_net_amd.pairstore import PairStore
from graph_neural_net_amd.synthetic import pack_adjacency

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {'unsigned long long': C.c_ulonglong, 'long long': C.c_longlong, 'int': C.c_int}


def random_graph(rng, n, p=0.4):
    w = np.triu(rng.random((n, n)) < p, 1)
    return (w | w.T).astype(np.float32)


def words_of(graphs, N):
    pad = np.zeros((len(graphs), N, N), dtype=np.float32)
    for k, g in enumerate(graphs):
        pad[k, :len(g), :len(g)] = g
    return torch.from_numpy(pack_adjacency(pad).view(np.int32))


def test_header_binding_and_library_agree():
    hdr = open(os.path.join(ROOT, 'include', 'fgnn_hip.h')).read()
    lib = _lib.load()
    for name in ('fgnn_pairstore_gather', 'fgnn_pairstore_supported'):
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, '%s is not declared in include/fgnn_hip.h' % name
        params = [p.strip() for p in m.group(1).split(',')]
        sig = _lib._SIGNATURES[name]
        assert len(sig) == len(params), name
        for p, t in zip(params, sig):               # argument by argument: pointers travel as void *, the struct by its mirror
            if 'fgnn_pairstore_args' in p:
                assert t is C.POINTER(_lib.PairstoreArgs), p
            elif '*' in p:
                assert t is C.c_void_p, p
            else:
                assert t is CTYPES[p.rsplit(' ', 1)[0]], p
        assert hasattr(lib, name), 'libfgnn_hip.so does not export %s' % name
    assert lib.fgnn_pairstore_supported(256, 1) == 1 and lib.fgnn_pairstore_supported(1, 0) == 1
    assert lib.fgnn_pairstore_supported(257, 0) == 0 and lib.fgnn_pairstore_supported(0, 0) == 0 and lib.fgnn_pairstore_supported(50, 2) == 0


def test_struct_has_the_headers_fields_in_order():
    hdr = open(os.path.join(ROOT, 'include', 'fgnn_hip.h')).read()
    body = re.search(r'typedef struct \{([^}]*)\} fgnn_pairstore_args;', hdr).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        if decl.strip():
            m = re.fullmatch(r'(?:const )?([a-z ]+?) ?((?:\*?\w+(?:, )?)+)', decl.strip())
            for name in m.group(2).split(', '):
                fields.append((name.lstrip('*'), C.c_void_p if name.startswith('*') else CTYPES[m.group(1)]))
    assert len(fields) == 19
    assert [(n, t) for n, t in _lib.PairstoreArgs._fields_] == fields


def test_library_refuses_bad_arguments():
    lib = _lib.load()
    a = _lib.PairstoreArgs()
    a.M, a.B, a.N, a.parents, a.bits1, a.bits2 = 4, 0, 20, 8, 8, 8          # B = 0: checked, nothing launched, no pointer read
    assert lib.fgnn_pairstore_gather(C.byref(a), None) == 0
    assert lib.fgnn_pairstore_gather(None, None) != 0
    for field, value, word in (('N', 257, 'unsupported'), ('noise_model', 2, 'unsupported'), ('M', 0, 'bad arguments'),
                               ('first', -1, 'bad arguments'), ('thr_noise1', (1 << 32) + 1, 'thresholds'), ('K', 65, 'levels'),
                               ('noise_model', 1, None), ('emax', 191, 'emax')):
        b = _lib.PairstoreArgs.from_buffer_copy(a)
        if field == 'emax':
            b.noise_model = 1
        if field == 'K':
            b.level_thr = b.level = 8
        setattr(b, field, value)
        rc = lib.fgnn_pairstore_gather(C.byref(b), None)
        assert (rc == 0) if word is None else (rc != 0 and word in _lib.last_error()), (field, _lib.last_error())
    b = _lib.PairstoreArgs.from_buffer_copy(a)                              # levels together with a stored second side
    b.seconds = b.level_thr = b.level = 8
    b.K = 2
    assert lib.fgnn_pairstore_gather(C.byref(b), None) != 0 and 'second side' in _lib.last_error()


def test_constructors_refuse_what_is_not_an_adjacency():
    rng = np.random.default_rng(0)
    good = random_graph(rng, 7)
    asym, frac, diag = good.copy(), good.copy(), good.copy()
    asym[1, 2], asym[2, 1] = 1.0, 0.0
    frac[3, 4] = frac[4, 3] = 0.5
    diag[2, 2] = 1.0
    for bad in (asym, frac, diag):
        with pytest.raises(ValueError):
            PairStore.from_list([good, bad])
        with pytest.raises(ValueError):
            PairStore.from_list([good, good], seconds=[good, bad])
        x = torch.zeros(1, 2, 7, 7)
        x[0, 0] = torch.from_numpy(bad)
        with pytest.raises(ValueError):
            PairStore.from_dense(x)
    for bad in (asym, diag):
        with pytest.raises(ValueError):
            PairStore.from_bits(words_of([bad], 7))
    w = words_of([good], 7)
    dirty = w.clone()
    dirty[0, 0, 0] |= 1 << 9                                            # a bit past column N
    with pytest.raises(ValueError):
        PairStore.from_bits(dirty)
    with pytest.raises(ValueError):                                    # an edge past the vertex count
        PairStore.from_bits(words_of([np.ones((7, 7), dtype=np.float32) - np.eye(7, dtype=np.float32)], 7), sizes=[5])
    for sizes in ([8], [-1], [3, 3], [2.0]):
        with pytest.raises(ValueError):
            PairStore.from_bits(w, sizes=sizes)
    with pytest.raises(ValueError):
        PairStore.from_bits(w, seconds=words_of([good, good], 7))
    with pytest.raises(ValueError):
        PairStore.from_bits(w.to(torch.int64))
    with pytest.raises(ValueError):
        PairStore.from_list([])
    with pytest.raises(ValueError):
        PairStore.from_list([good], n_vertices=6)
    with pytest.raises(ValueError):
        PairStore.from_list([good], seconds=[random_graph(rng, 6)])
    for kw in ({'noise_model': 'Flip'}, {'noise': 1.5}, {'edge_density': 1.0}, {'seed': -1}):
        with pytest.raises(ValueError):
            PairStore.from_bits(w, **kw)
    # outside the corner of a padded dense batch nothing is read, and what is there is not stored
    x = torch.full((1, 2, 9, 9), 7.0)
    x[0, 0, :7, :7] = torch.from_numpy(good)
    s = PairStore.from_dense(x, nvalid=[7])
    assert torch.equal(s.parents, words_of([good], 9)) and s.sizes.tolist() == [7]


def test_from_list_packs_the_words_of_pack_adjacency():
    rng = np.random.default_rng(1)
    sizes = (5, 7, 6, 33)
    graphs = [random_graph(rng, n) for n in sizes]
    seconds = [random_graph(rng, n) for n in sizes]
    s = PairStore.from_list(graphs, seconds=seconds)
    assert (s.num_examples, s.n_vertices, s.paired, s.constant_n_vertices) == (4, 33, True, False)
    assert s.parents.dtype == torch.int32 and s.parents.shape == (4, 33, 2) and s.device.type == 'cpu'
    assert torch.equal(s.parents, words_of(graphs, 33)) and torch.equal(s.seconds, words_of(seconds, 33))
    assert s.sizes.dtype == torch.int32 and s.sizes.tolist() == list(sizes)
    for k, n in enumerate(sizes):                                       # zero padding: rows and word bits past n
        u = ((s.parents[k].unsqueeze(-1) >> torch.arange(32, dtype=torch.int32)) & 1).reshape(33, -1)
        assert u.any() and not u[n:].any() and not u[:, n:].any()
    # tensor representations (channel 0 is read), tensors, a wider padding; equal sizes make a constant-size store
    reps = [torch.stack([torch.from_numpy(g), torch.diag(torch.from_numpy(g).sum(1))]) for g in graphs[:3]]
    t = PairStore.from_list(reps, n_vertices=40)
    assert t.n_vertices == 40 and torch.equal(t.parents, words_of(graphs[:3], 40)) and not t.paired
    c = PairStore.from_list([graphs[1], seconds[1]])
    assert c.constant_n_vertices and c.sizes is None and c.n_vertices == 7
    # the chunks of a long list meet without a seam
    many = [random_graph(rng, 3 + k % 5) for k in range(2048 + 5)]
    m = PairStore.from_list(many)
    assert m.num_examples == 2053 and torch.equal(m.parents, words_of(many, 7)) and m.sizes.tolist() == [3 + k % 5 for k in range(2053)]
    # from_dense on CPU tensors is the same packer
    x = torch.zeros(4, 2, 33, 33)
    for k, g in enumerate(graphs):
        x[k, 0, :len(g), :len(g)] = torch.from_numpy(g)
    d = PairStore.from_dense(x, nvalid=torch.tensor(sizes))
    assert torch.equal(d.parents, s.parents) and torch.equal(d.sizes, s.sizes)


def test_edge_density_none_is_the_stores_own():
    rng = np.random.default_rng(2)
    sizes = (5, 7, 6, 12)
    graphs = [random_graph(rng, n) for n in sizes]
    edges = sum(int(g.sum()) // 2 for g in graphs)
    slots = sum(n * (n - 1) // 2 for n in sizes)
    s = PairStore.from_list(graphs, n_vertices=16)
    assert (s.total_edges, s.total_slots) == (edges, slots) and s.edge_density == edges / slots
    assert s.max_edges == max(int(g.sum()) // 2 for g in graphs)
    c = PairStore.from_list([graphs[1]] * 3, n_vertices=7)              # constant size: M N (N - 1) / 2 slots
    assert c.total_slots == 3 * 21 and c.edge_density == 3 * (int(graphs[1].sum()) // 2) / 63
    assert PairStore.from_list(graphs, edge_density=0.25).edge_density == 0.25
    assert PairStore.from_list([np.zeros((4, 4))]).edge_density == 0.0 and PairStore.from_list([np.zeros((1, 1))]).edge_density == 0.0
    with pytest.raises(ValueError, match='complete'):
        PairStore.from_list([np.ones((4, 4)) - np.eye(4)])
    assert PairStore.from_list([np.ones((4, 4)) - np.eye(4)], edge_density=0.5).max_edges == 6
    lv = s.levels([0.0, 0.1])
    assert isinstance(lv, NoiseLevels) and lv.edge_density == s.edge_density
    assert lv.thresholds[1] == (threshold(0.1), threshold(s.edge_density * 0.1 / (1 - s.edge_density)))


def test_bits_checks_every_argument_before_the_device():
    rng = np.random.default_rng(3)
    graphs = [random_graph(rng, 9) for _ in range(6)]
    s = PairStore.from_list(graphs)
    p = PairStore.from_list(graphs, seconds=graphs)
    idx = torch.arange(4)
    for call in (lambda: s.bits(0, 4, index=idx), lambda: s.bits(), lambda: s.bits(2), lambda: s.dense(0, 4, idx),
                 lambda: s.spectral(0, 4, index=idx), lambda: s.bits(index=idx.reshape(2, 2)), lambda: s.bits(index=idx.to(torch.int32)),
                 lambda: s.bits(-1, 2)):
        with pytest.raises(ValueError, match='first|index'):
            call()
    with pytest.raises(ValueError, match='outside the store'):
        s.bits(3, 4)
    lv = s.levels([0.0, 0.2])
    with pytest.raises(ValueError, match='paired'):                    # levels on a paired store
        p.bits(index=idx, levels=p.levels([0.1]), level=[0, 0, 0, 0])
    with pytest.raises(ValueError, match='paired'):
        p.dense(0, 4, levels=p.levels([0.1]), level=[0, 0, 0, 0])
    other = PairStore.from_list(graphs, edge_density=0.123)
    with pytest.raises(ValueError, match='this generator'):            # levels from another density
        s.bits(index=idx, levels=other.levels([0.0, 0.2]), level=[0, 1, 0, 1])
    with pytest.raises(ValueError, match='go together'):
        s.bits(index=idx, levels=lv)
    with pytest.raises(ValueError, match='level must be'):
        s.bits(index=idx, levels=lv, level=[0, 1])
    s.noise = 2.0
    with pytest.raises(ValueError, match='noise'):
        s.bits(0, 4)
    s.noise = 0.1
    for call in (lambda: s.bits(0, 4), lambda: s.bits(index=idx, levels=lv, level=[0, 1, 1, 0]), lambda: p.bits(index=idx, permute=True),
                 lambda: s.dense(0, 2), lambda: s.spectral(index=idx)):
        with pytest.raises(RuntimeError, match='no CPU path'):          # everything valid: only the device is missing
            call()


def test_save_and_load_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    sizes = (5, 7, 6, 33)
    graphs = [random_graph(rng, n) for n in sizes]
    seconds = [random_graph(rng, n) for n in sizes]
    for kw in ({'seconds': seconds}, {}):
        s = PairStore.from_list(graphs, noise_model='EdgeSwap', noise=0.07, seed=(1 << 63) + 5, **kw)
        path = str(tmp_path / 'store.pt')
        s.save(path)
        assert isinstance(torch.load(path, weights_only=True), dict)       # plain tensors and settings: no pickled code
        t = PairStore.load(path)
        assert t.device.type == 'cpu' and torch.equal(t.parents, s.parents) and torch.equal(t.sizes, s.sizes)
        assert (t.seconds is None) == (s.seconds is None) and (t.seconds is None or torch.equal(t.seconds, s.seconds))
        for name in ('n_vertices', 'num_examples', 'paired', 'constant_n_vertices', 'noise_model', 'noise', 'seed', 'edge_density',
                     'max_edges', 'total_edges', 'total_slots'):
            assert getattr(t, name) == getattr(s, name), name
    torch.save({'format': 'something else'}, path)
    with pytest.raises(ValueError, match='not a saved PairStore'):
        PairStore.load(path)
    c = PairStore.from_list([graphs[0]] * 2)
    c.save(path)
    assert PairStore.load(path).sizes is None and PairStore.load(path).to('cpu').constant_n_vertices


def test_reference_dataset_fixture(golden_dir):
    path = os.path.join(golden_dir, 'pairstore_dataset.pt')
    assert os.path.getsize(path) < 64 * 1024
    data = torch.load(path, weights_only=True)
    sizes = [b.shape[-1] for b, _ in data]
    N = max(sizes)
    assert len(data) >= 4 and len(set(sizes)) > 1 and N <= 12
    s = PairStore.from_reference_dataset(path)
    assert (s.paired, s.num_examples, s.n_vertices, s.constant_n_vertices) == (True, len(data), N, False)
    assert s.sizes.tolist() == sizes
    assert torch.equal(s.parents, words_of([b[0].numpy() for b, _ in data], N))
    assert torch.equal(s.seconds, words_of([bn[0].numpy() for _, bn in data], N))
    assert not torch.equal(s.parents, s.seconds)
    n = PairStore.from_reference_dataset(data, noisy=True, noise=0.05, n_vertices=16)
    assert not n.paired and n.n_vertices == 16 and n.seconds is None and n.noise == 0.05
    assert torch.equal(n.parents, words_of([b[0].numpy() for b, _ in data], 16))
    assert n.edge_density == sum(int(b[0].sum()) // 2 for b, _ in data) / sum(k * (k - 1) // 2 for k in sizes)
    with pytest.raises(ValueError):
        PairStore.from_reference_dataset([data[0][0]])
