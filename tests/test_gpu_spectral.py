"""GPU: the spectral input features on the device (csrc/spectral.hip, graph_neural_net_amd/spectral.py, PairGenerator.spectral)
against tests/spectral_ref.py and the reference's recorded output and error (tests/golden/spectral_features.npz).

Gates.  Power 1 is one chain of correctly rounded operations per entry: torch.equal to the fp32 restatement.  Powers >= 2: max-abs
distance from the fp64 restatement <= ERR_GATE x the reference's own fp32 distance from fp64 for that case and power (`ref_err` of
the fixture; for shapes beyond it the fp32 restatement's own distance, computed here) -- the project's per-tensor bar for "within
the reference's own fp32 error" (the gradient gates of tests/test_gpu_parity.py).  Ratios measured on an MI355X (this file run
with -s prints them; profiles/spectral_parity.txt keeps them): median 1.00, at most 2.59 (N = 7, one graph, power 8).
"""
import functools

import numpy as np
import pytest
import torch

import spectral_ref as R
from graph_neural_net_amd import _lib, spectral, synthetic
from graph_neural_net_amd.masked import MaskedTensor
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.siamese import Siamese_Node_Exp
from util import is_zero_grad, rel

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ERR_GATE = 4.0
GROUPS = R.fixture_groups()
# fused_step against the eager module path on models that run zero-padded on the engine:
# tests/test_gpu_widths.py::test_fused_step_on_models_that_run_zero_padded_on_the_engine -- scores and gradients bit for bit, loss to
ZERO_PADDED_LOSS_RTOL = 1e-6
# ... and on MaskedTensor batches (the fused step scales by a device reciprocal of sum(n), the module path divides on the host; the
# padded geometries differ): tests/test_gpu_module_surface.py::test_bf16_fused_step_on_masked_tensor_batches_equals_the_eager_module_path
MASKED_LOSS_SCORE_RTOL, MASKED_GRAD_RTOL = 1e-5, 1e-4


def _dev(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int32)).to(DEV)


def _nv(nvalid):
    return None if nvalid is None else torch.from_numpy(np.asarray(nvalid, dtype=np.int32)).to(DEV)


def _er(rng, n, p):
    A = np.triu(rng.random((n, n)) < p, 1)
    return (A | A.T).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _shape_case(N, G):
    """seeded ER graphs (isolated vertices allowed: the restatement has the device's convention) -> bits, and once for all powers:
    the fp32 restatement, its own distance from fp64 per power, the fp64 restatement"""
    rng = np.random.default_rng(100 * N + G)
    bits = np.stack([R.pack_bits(_er(rng, N, 0.5 if N < 10 else 0.25)) for _ in range(G)])
    own, f64 = R.own_error(bits, None, R.FIXTURE_POWERS)
    f32 = R.padded_features(bits, None, R.FIXTURE_POWERS)
    return bits, f32, own, f64


def _check(tag, got, f32, f64, yard):
    """got (G, P, n, n) device tensor; f32 / f64 restatements with >= P powers; yard: per-power yard-stick"""
    got = got.cpu()
    P = got.shape[1]
    assert torch.isfinite(got).all()
    assert torch.equal(got[:, 0], torch.from_numpy(f32[:, 0])), tag
    err = (got.double() - torch.from_numpy(f64[:, :P])).abs().amax((0, 2, 3)).numpy()
    ratios = [e / y if y > 0 else (0.0 if e == 0 else float('inf')) for e, y in zip(err, yard[:P])]
    print('spectral parity %-22s max|dev - fp64| / yard-stick per power: %s' % (tag, ' '.join('%.2f' % r for r in ratios)))
    assert all(e <= ERR_GATE * y for e, y in zip(err[1:], yard[1:P])), (tag, err, yard[:P])


@pytest.mark.parametrize('n_powers', [1, 4, 8])
@pytest.mark.parametrize('G', [1, 3])
@pytest.mark.parametrize('N', [1, 2, 7, 31, 32, 33, 50, 64, 65, 200, 256])
def test_features_at_panel_and_word_edges(N, G, n_powers):
    bits, f32, own, f64 = _shape_case(N, G)
    got = spectral.spectral_features(_dev(bits), n_powers=n_powers)
    assert got.shape == (G, n_powers, N, N) and got.dtype == torch.float32 and got.is_cuda
    _check('N=%d G=%d P=%d' % (N, G, n_powers), got, f32, f64, own)


@pytest.mark.parametrize('name', sorted(GROUPS))
def test_features_on_the_fixture_within_the_reference_error(name):
    g = GROUPS[name]
    bits, nvalid = g['bits'], g['nvalid']
    N = bits.shape[1]
    ragged = bool((nvalid != N).any())
    got = spectral.spectral_features(_dev(bits), _nv(nvalid) if ragged else None, n_powers=R.FIXTURE_POWERS)
    f32 = R.padded_features(bits, nvalid, R.FIXTURE_POWERS)
    f64 = R.padded_features(bits, nvalid, R.FIXTURE_POWERS, dtype=torch.float64)
    _check(name, got, f32, f64, g['ref_err'].max(0))
    if 'ref32' in g:                            # the reference's own first power, bit for bit
        assert torch.equal(got[:, 0].cpu(), torch.from_numpy(g['ref32'][:, 0]))
    if ragged:
        for b, n in enumerate(nvalid):
            assert (got[b, :, n:, :] == 0).all() and (got[b, :, :, n:] == 0).all()


def test_directed_graph_uses_rows_for_degrees_and_is_not_its_transpose():
    g = GROUPS['directed']
    W = R.unpack_bits(g['bits'][0])
    got = spectral.spectral_features(_dev(g['bits']), n_powers=4).cpu()
    wrong = R.features(W.T, 4, torch.float64)                         # (what reading W by columns would give)
    right = R.features(W, 4, torch.float64)
    assert (got[0].double() - torch.from_numpy(right)).abs().max() < 1e-6
    assert (got[0].double() - torch.from_numpy(wrong)).abs().max() > 1e-3


def test_ragged_batch_and_smaller_n_out_leave_exact_zeros_outside_every_corner():
    rng = np.random.default_rng(12)
    N, sizes = 70, [70, 0, 33, 64, 1, 40]
    bits = np.stack([R.pack_bits(_er(rng, n, 0.3), N) if n else np.zeros((N, 3), dtype=np.uint32) for n in sizes])
    want = R.padded_features(bits, sizes, 4)
    own, f64 = R.own_error(bits, sizes, 4)
    for n_out in (None, 70, 65, 64, 40, 33, 7):                       # 40 / 33 / 7 crop some graphs: the top-left corner of the planes
        m = N if n_out is None else n_out
        out = torch.full((len(sizes), 4, m, m), float('nan'), device=DEV)
        got = spectral.spectral_features(_dev(bits), _nv(sizes), 4, n_out=n_out, out=out)
        assert got is out
        _check('ragged n_out=%s' % n_out, got, want[:, :, :m, :m], f64[:, :, :m, :m], own)
        for b, n in enumerate(sizes):
            assert (got[b, :, n:, :] == 0).all() and (got[b, :, :, n:] == 0).all()
    # the largest n of a batch as n_out: what PairGenerator.spectral writes
    sub = [2, 3, 4]
    got = spectral.spectral_features(_dev(bits[sub]), _nv([sizes[i] for i in sub]), 4, n_out=64)
    clean = spectral.spectral_features(_dev(bits[sub]), _nv([sizes[i] for i in sub]), 4)
    assert torch.equal(got, clean[:, :, :64, :64])


def test_garbage_bits_outside_the_corner_do_not_change_the_result():
    rng = np.random.default_rng(13)
    N, sizes = 100, [100, 37, 64, 65, 0, 96]
    clean = np.stack([R.pack_bits(_er(rng, n, 0.3), N) if n else np.zeros((N, 4), dtype=np.uint32) for n in sizes])
    dirty = clean.copy()
    for b, n in enumerate(sizes):
        junk = rng.integers(0, 1 << 32, size=(N, 4), dtype=np.uint64).astype(np.uint32)
        full = np.unpackbits(junk.view(np.uint8).reshape(N, -1), axis=-1, bitorder='little')      # (N, 128): also bits >= N of a word
        keep = np.unpackbits(clean[b].view(np.uint8).reshape(N, -1), axis=-1, bitorder='little')
        full[:n, :n] = keep[:n, :n]
        dirty[b] = np.packbits(full, axis=-1, bitorder='little').view(np.uint32).reshape(N, 4)
    assert not np.array_equal(dirty, clean)
    a = spectral.spectral_features(_dev(clean), _nv(sizes), 5)
    b = spectral.spectral_features(_dev(dirty), _nv(sizes), 5)
    assert torch.equal(a, b)
    assert torch.equal(a[:, 0].cpu(), torch.from_numpy(R.padded_features(clean, sizes, 1)[:, 0]))
    # counts outside [0, N] are clamped
    c = spectral.spectral_features(_dev(clean[:2]), _nv([1000, -5]), 2)
    assert torch.equal(c[0], spectral.spectral_features(_dev(clean[:1]), None, 2)[0]) and (c[1] == 0).all()


def test_isolated_vertex_and_empty_graph_give_zeros_not_nan():
    rng = np.random.default_rng(14)
    n = 45
    W = _er(rng, n, 0.3)
    W[17, :] = W[:, 17] = 0
    W[40, :] = W[:, 40] = 0
    bits = np.stack([R.pack_bits(W), np.zeros((n, 2), dtype=np.uint32)])
    got = spectral.spectral_features(_dev(bits), n_powers=8)
    own, f64 = R.own_error(bits, None, 8)
    _check('isolated', got, R.padded_features(bits, None, 8), f64, own)
    assert (got[0, :, [17, 40], :] == 0).all() and (got[0, :, :, [17, 40]] == 0).all() and got[0].abs().max() > 0
    assert (got[1] == 0).all()


def test_spectral_from_dense_packs_verifies_and_equals_the_bit_route():
    rng = np.random.default_rng(15)
    N, sizes = 52, [52, 30, 47]
    Ws = np.zeros((3, N, N), dtype=np.float32)
    for b, n in enumerate(sizes):
        Ws[b, :n, :n] = _er(rng, n, 0.3)
    bits = np.stack([R.pack_bits(Ws[b]) for b in range(3)])
    want = spectral.spectral_features(_dev(bits), _nv(sizes), 4)
    adj = torch.from_numpy(Ws).to(DEV)
    rep = torch.from_numpy(np.stack([synthetic.tensor_representation(w) for w in Ws])).to(DEV)
    assert torch.equal(spectral.spectral_from_dense(adj, _nv(sizes)), want)
    assert torch.equal(spectral.spectral_from_dense(rep, _nv(sizes)), want)
    assert torch.equal(spectral.spectral_from_dense(adj[:1]), spectral.spectral_features(_dev(bits[:1])))
    assert torch.equal(spectral.spectral_from_dense(rep[:1], n_powers=2), want[:1, :2])
    # a directed adjacency goes through as it is
    D = Ws[:1] * (1 - np.triu(rng.random((N, N)) < 0.4, 1)).astype(np.float32)
    assert torch.equal(spectral.spectral_from_dense(torch.from_numpy(D).to(DEV)),
                       spectral.spectral_features(_dev(np.stack([R.pack_bits(D[0])]))))
    bad = adj.clone()
    bad[1, 3, 4] = 0.5
    with pytest.raises(RuntimeError, match='NOT the tensor representation'):
        spectral.spectral_from_dense(bad, _nv(sizes))
    bad = rep.clone()
    bad[0, 0, 2, 3] = 2.0
    with pytest.raises(RuntimeError, match='NOT the tensor representation'):
        spectral.spectral_from_dense(bad, _nv(sizes))
    with pytest.raises(RuntimeError):
        spectral.spectral_from_dense(adj.cpu())
    with pytest.raises(RuntimeError):
        spectral.spectral_from_dense(torch.zeros(2, 3, 8, 8, device=DEV))


def test_bad_arguments_raise():
    z = torch.zeros(2, 40, 2, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match='no CPU'):
        spectral.spectral_features(z.cpu())
    with pytest.raises(RuntimeError):
        spectral.spectral_features(z.float())
    with pytest.raises(RuntimeError):
        spectral.spectral_features(z[:, :, :1])
    with pytest.raises(RuntimeError, match='256'):
        spectral.spectral_features(torch.zeros(1, 257, 9, dtype=torch.int32, device=DEV))
    for p in (0, 9):
        with pytest.raises(ValueError):
            spectral.spectral_features(z, n_powers=p)
    for m in (0, 41):
        with pytest.raises(ValueError):
            spectral.spectral_features(z, n_out=m)
    with pytest.raises(RuntimeError):
        spectral.spectral_features(z, nvalid=torch.zeros(3, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError):
        spectral.spectral_features(z, out=torch.zeros(2, 4, 40, 41, device=DEV))
    lib, st = _lib.load(), _lib.stream_ptr()
    p, o = _lib.ptr(z), _lib.ptr(torch.zeros(2 * 8 * 40 * 40, device=DEV))
    assert lib.fgnn_spectral_features(p, None, 2, 257, 4, o, 40, st) == 1
    assert lib.fgnn_spectral_features(p, None, 2, 40, 9, o, 40, st) == 1 and 'powers' in _lib.last_error()
    assert lib.fgnn_spectral_features(p, None, 2, 40, 4, o, 41, st) == 1
    assert lib.fgnn_spectral_features(p, None, 2, 40, 4, None, 40, st) == 1
    assert lib.fgnn_spectral_features(p, None, 0, 40, 4, o, 40, st) == 1


@pytest.mark.parametrize('vp', [1.0, 0.7])
def test_pair_generator_spectral_is_bits_then_the_kernel_with_the_structures_of_dense(vp):
    gen = PairGenerator(40, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.25, noise=0.1, vertex_proba=vp, seed=5, device=DEV)
    first, count = 7, 6
    b1, b2, nv = gen.bits(first, count)
    s1, s2 = gen.spectral(first, count)
    d1, d2 = gen.dense(first, count)
    if vp == 1.0:
        assert nv is None and isinstance(s1, dict) and isinstance(s2, dict) and list(s1) == list(d1) == ['input']
        t1, t2 = s1['input'], s2['input']
        assert t1.shape == (count, 4, 40, 40) and d1['input'].shape == (count, 2, 40, 40)
        n_out = None
    else:
        assert isinstance(s1, MaskedTensor) and isinstance(s2, MaskedTensor)
        for s, d in ((s1, d1), (s2, d2)):
            assert s.names == d.names and s.masked_dims == d.masked_dims and s.base_name == d.base_name
            assert torch.equal(s.nvalid, d.nvalid) and torch.equal(s.nvalid, nv)
        t1, t2 = s1.tensor.rename(None), s2.tensor.rename(None)
        n_out = int(nv.max())
        assert 1 < n_out < 40                                           # (the crop is exercised)
        assert t1.shape == (count, 4, n_out, n_out) and d1.tensor.shape[-2:] == t1.shape[-2:]
    assert torch.equal(t1, spectral.spectral_features(b1, nv, 4, n_out=n_out))
    assert torch.equal(t2, spectral.spectral_features(b2, nv, 4, n_out=n_out))
    p1 = gen.spectral(first, count, n_powers=2)[0]
    p1 = p1['input'] if vp == 1.0 else p1.tensor.rename(None)
    assert torch.equal(p1, t1[:, :2])
    # pair k depends on (seed, k) only: a range split into two calls equals one call
    a1, a2 = gen.spectral(first, 2)
    c1, c2 = gen.spectral(first + 2, count - 2)
    for whole, parts in ((t1, (a1, c1)), (t2, (a2, c2))):
        lo = 0
        for part in parts:
            pt = part['input'] if vp == 1.0 else part.tensor.rename(None)
            m = pt.shape[-1]
            assert torch.equal(pt, whole[lo:lo + pt.shape[0], :, :m, :m])
            assert (whole[lo:lo + pt.shape[0], :, m:, :] == 0).all() and (whole[lo:lo + pt.shape[0], :, :, m:] == 0).all()
            lo += pt.shape[0]


def test_spectral_features_is_capturable_and_replays_on_new_inputs():
    N, G = 90, 4
    g1 = PairGenerator(N, 'ErdosRenyi', seed=1, device=DEV, edge_density=0.2)
    g2 = PairGenerator(N, 'ErdosRenyi', seed=2, device=DEV, edge_density=0.1, vertex_proba=0.8)
    ba, _, _ = g1.bits(0, G)
    bb, _, nvb = g2.bits(0, G)
    eager_a = spectral.spectral_features(ba, torch.full((G,), N, dtype=torch.int32, device=DEV))
    eager_b = spectral.spectral_features(bb, nvb)
    bits, nv = ba.clone(), torch.full((G,), N, dtype=torch.int32, device=DEV)
    out = torch.empty(G, 4, N, N, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        spectral.spectral_features(bits, nv, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        spectral.spectral_features(bits, nv, out=out)
    out.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_a)
    bits.copy_(bb)
    nv.copy_(nvb)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_b) and not torch.equal(eager_a, eager_b)


def _ne(blocks, ragged=False):
    ne = dict(type='node_embedding', block_init='block_emb', block_inside='block', num_blocks=blocks, in_features=32,
              out_features=32, depth_of_mlp=3)
    if ragged:
        ne['constant_n_vertices'] = False
    return ne


def test_end_to_end_constant_size_fused_step_equals_the_eager_module_path():
    """a 4-channel model fed by PairGenerator.spectral: the captured fused step (zero-padded parameters) and the eager module
    path agree as tests/test_gpu_widths.py::test_fused_step_on_models_that_run_zero_padded_on_the_engine asks"""
    torch.manual_seed(21)
    model = Siamese_Node_Exp(4, _ne(2), metric='max').to(DEV)
    x1, x2 = PairGenerator(20, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.1, seed=3, device=DEV).spectral(0, 2)
    assert x1['input'].shape == (2, 4, 20, 20)
    scores = model(x1, x2)
    loss = model.loss(scores)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(scores).all()
    eager = {n: p.grad.clone() for n, p in model.named_parameters()}
    for cap in (False, True, True):
        for p in model.parameters():
            p.grad = None
        l2, s2 = model.fused_step(x1, x2, capture=cap)
        assert torch.isfinite(l2)
        assert torch.equal(s2, scores.detach()) and abs(l2.item() - loss.item()) <= ZERO_PADDED_LOSS_RTOL * abs(loss.item())
        for n, p in model.named_parameters():
            assert torch.equal(p.grad, eager[n]), (cap, n)


def test_end_to_end_ragged_fused_step_equals_the_eager_module_path():
    torch.manual_seed(22)
    model = Siamese_Node_Exp(4, _ne(2, ragged=True), metric='max').to(DEV)
    gen = PairGenerator(24, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.1, vertex_proba=0.8, seed=4, device=DEV)
    m1, m2 = gen.spectral(0, 2)
    sizes = m1.nvalid.tolist()
    assert isinstance(m1, MaskedTensor) and m1.tensor.shape[1] == 4 and len(set(sizes)) == 2
    scores = model(m1, m2)
    loss = model.loss(scores)
    loss.backward()
    assert torch.isfinite(loss)
    eager = {n: p.grad.clone() for n, p in model.named_parameters()}
    for cap in (False, True, True):
        for p in model.parameters():
            p.grad = None
        l2, s2 = model.fused_step(m1, m2, capture=cap)
        assert torch.isfinite(l2) and abs(l2.item() - loss.item()) <= MASKED_LOSS_SCORE_RTOL * abs(loss.item())
        for i, n in enumerate(sizes):
            assert rel(s2.tensor.rename(None)[i, :n, :n], scores.tensor.rename(None)[i, :n, :n].detach()) < MASKED_LOSS_SCORE_RTOL
        for name, p in model.named_parameters():
            if not is_zero_grad(name):
                assert rel(p.grad, eager[name]) < MASKED_GRAD_RTOL, (cap, name, rel(p.grad, eager[name]))
