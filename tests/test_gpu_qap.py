"""GPU: the matching decode on the device (csrc/qap.hip, graph_neural_net_amd/qap.py, Siamese_Node_Exp.match) against numpy, the
reference's recorded results (tests/golden/qap_decode.npz) and tests/qap_ref.py.  The quantities are integers or halves: every
comparison is exact."""
import numpy as np
import pytest
import torch

import qap_ref as R
from graph_neural_net_amd import _lib, qap, synthetic
from graph_neural_net_amd.masked import MaskedTensor, from_list
from graph_neural_net_amd.metrics import accuracy_linear_assignment
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.siamese import Siamese_Node_Exp

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TS, GREEDY_KEYS = R.TS, R.GREEDY_KEYS
GROUPS = R.fixture_groups()


def _dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _cost_dev(bits1, bits2, assign, nvalid=None, ld=None, bstride=None, fill=-777.0):
    B, N, _ = bits1.shape
    ld = N if ld is None else ld
    bstride = N * ld if bstride is None else bstride
    buf = torch.full((B * bstride,), fill, dtype=torch.float32, device=DEV)
    nv = _dev_i32(nvalid) if nvalid is not None else None
    b1, b2, a = _dev_i32(bits1), _dev_i32(bits2), _dev_i32(assign)          # (kept alive: a freed tensor's block is handed out again)
    _lib.call('fgnn_qap_improve_cost', _lib.ptr(b1), _lib.ptr(b2), _lib.ptr(a), _lib.ptr(nv), B, N, _lib.ptr(buf), bstride, ld,
              _lib.stream_ptr())
    return buf.cpu().numpy()


def _check_cost(bits1, bits2, assign, nvalid=None, ld=None, bstride=None):
    """the device cost against -(A @ P @ B) on every corner; everything outside the corners keeps the fill value"""
    B, N, _ = bits1.shape
    ld_, bs_ = (N if ld is None else ld), None
    bs_ = N * ld_ if bstride is None else bstride
    got = _cost_dev(bits1, bits2, assign, nvalid, ld, bstride)
    untouched = np.ones(got.shape, dtype=bool)
    for b in range(B):
        n = N if nvalid is None else int(nvalid[b])
        A, Bm = R.unpack_bits(bits1[b], n), R.unpack_bits(bits2[b], n)
        want = -(A @ R.perm_matrix(np.arange(n), assign[b, :n]) @ Bm) if n else np.zeros((0, 0))
        rows = (b * bs_ + np.arange(n)[:, None] * ld_ + np.arange(n)[None, :]).reshape(n, n)
        assert np.array_equal(got[rows], want.astype(np.float32)), b
        untouched[rows] = False
    assert (got[untouched] == -777.0).all()


@pytest.mark.parametrize('name', sorted(GROUPS))
def test_improve_cost_on_every_fixture_pair(name):
    g = GROUPS[name]
    _check_cost(g['bits1'], g['bits2'], g['assign0'], g['nvalid'])


@pytest.mark.parametrize('N', [1, 31, 32, 33, 65])
def test_improve_cost_at_word_edges(N):
    rng = np.random.default_rng(N)
    B = 3
    W1 = (rng.random((B, N, N)) < 0.4)
    W2 = (rng.random((B, N, N)) < 0.4)                     # directed: neither matrix is symmetric
    assign = np.stack([rng.permutation(N) for _ in range(B)]).astype(np.int32)
    _check_cost(synthetic.pack_adjacency(W1), synthetic.pack_adjacency(W2), assign)


def test_improve_cost_ragged_garbage_outside_the_corner_and_strides():
    rng = np.random.default_rng(5)
    B, N = 4, 70
    nvalid = np.array([70, 0, 33, 64], dtype=np.int32)
    W1, W2 = rng.random((B, N, N)) < 0.3, rng.random((B, N, N)) < 0.3          # bits everywhere, also outside the corners
    assign = np.full((B, N), -1, dtype=np.int32)
    for b, n in enumerate(nvalid):
        assign[b, :n] = rng.permutation(n)
    b1, b2 = synthetic.pack_adjacency(W1), synthetic.pack_adjacency(W2)
    _check_cost(b1, b2, assign, nvalid)
    _check_cost(b1, b2, assign, nvalid, ld=N + 7, bstride=N * (N + 7) + 13)
    # the objective ignores the same garbage
    obj = qap.objective_bits(_dev_i32(b1), _dev_i32(b2), _dev_i32(assign), _dev_i32(nvalid))
    for b, n in enumerate(nvalid):
        A, Bm, pi = W1[b, :n, :n].astype(np.int64), W2[b, :n, :n].astype(np.int64), assign[b, :n]
        want = (int((A * Bm[np.ix_(pi, pi)]).sum()), int((A * Bm).sum()), int(A.sum()), int(Bm.sum()))
        assert tuple(int(obj[k][b]) for k in ('qap', 'planted', 'na', 'nb')) == want


def test_improve_cost_on_the_non_symmetric_pair_differs_from_its_transpose():
    g = GROUPS['nonsym']
    A, Bm = R.unpack_bits(g['bits1'][0]), R.unpack_bits(g['bits2'][0])
    n = A.shape[0]
    P = R.perm_matrix(np.arange(n), g['assign0'][0])
    got = _cost_dev(g['bits1'], g['bits2'], g['assign0']).reshape(n, n)
    assert np.array_equal(got, (-(A @ P @ Bm)).astype(np.float32))
    assert not np.array_equal(got, (-(A @ P @ Bm.T)).astype(np.float32))       # (what using B's rows as its columns would give)


@pytest.mark.parametrize('name', sorted(GROUPS))
def test_objective_equals_numpy(name):
    g = GROUPS[name]
    b1, b2, nv = _dev_i32(g['bits1']), _dev_i32(g['bits2']), _dev_i32(g['nvalid'])
    obj = qap.qap_objective(b1, b2, _dev_i32(g['assign0']), nv)
    assert all(v.is_cuda and v.dtype == torch.int64 for v in obj.values())
    assert np.array_equal(obj['qap'].cpu().numpy(), g['qap']) and np.array_equal(obj['planted'].cpu().numpy(), g['planted'])
    assert np.array_equal(obj['na'].cpu().numpy(), 2 * g['T0/na']) and np.array_equal(obj['nb'].cpu().numpy(), 2 * g['T0/nb'])
    B, N = g['assign0'].shape
    ident = np.where(np.arange(N)[None, :] < g['nvalid'][:, None], np.arange(N)[None, :], -1).astype(np.int32)
    oi = qap.qap_objective(b1, b2, _dev_i32(ident), nv)
    assert torch.equal(oi['qap'], oi['planted'])
    holed = g['assign0'].copy()
    holed[0, 0] = -1                                        # inside the corner: the solver found no finite matching
    oh = qap.qap_objective(b1, b2, _dev_i32(holed), nv)
    assert int(oh['qap'][0]) == -1 and torch.equal(oh['qap'][1:], obj['qap'][1:]) and torch.equal(oh['planted'], obj['planted'])


def _check_perm(out, b1, b2, nv, nvalid):
    again = qap.qap_objective(b1, b2, out['perm'], nv)
    assert torch.equal(again['qap'].double(), 2 * out['s_best'])
    perm = out['perm'].cpu().numpy()
    for b, n in enumerate(nvalid):
        assert sorted(perm[b, :n].tolist()) == list(range(n)) and (perm[b, n:] == -1).all()


@pytest.mark.parametrize('name', sorted(GROUPS))
def test_greedy_equals_fixture(name):
    g = GROUPS[name]
    b1, b2, nv, a0 = _dev_i32(g['bits1']), _dev_i32(g['bits2']), _dev_i32(g['nvalid']), _dev_i32(g['assign0'])
    for T in TS:
        out = qap.greedy_qap(b1, b2, a0, T, nv)
        for k in GREEDY_KEYS:
            want = g['T%d/%s' % (T, k)]
            assert out[k].is_cuda and out[k].dtype == (torch.float64 if want.dtype == np.float64 else torch.int64)
            assert np.array_equal(out[k].cpu().numpy(), want), (name, T, k)
        _check_perm(out, b1, b2, nv, g['nvalid'])
        again = qap.greedy_qap(b1, b2, a0, T, nv)
        assert all(torch.equal(out[k], again[k]) for k in out)


@pytest.mark.parametrize('family,N,vp', [('Regular', 50, 1.0), ('ErdosRenyi', 50, 0.8), ('Regular', 200, 1.0), ('ErdosRenyi', 200, 1.0),
                                         ('ErdosRenyi', 256, 0.9)])
def test_greedy_on_generated_pairs_equals_the_restatement(family, N, vp):
    B, T = 4, 10
    b1, b2, nv = PairGenerator(N, family, 'ErdosRenyi', edge_density=0.2, noise=0.1, vertex_proba=vp, seed=N, device=DEV).bits(3, B)
    nvalid = nv.cpu().numpy() if nv is not None else np.full(B, N)
    rng = np.random.default_rng(N)
    a0 = np.full((B, N), -1, dtype=np.int32)
    for b, n in enumerate(nvalid):                          # noisy starts: the identity with a shuffled share of the vertices
        pi = np.arange(n)
        idx = rng.choice(n, size=int(n * (0.2, 0.5, 0.8, 1.0)[b]), replace=False)
        pi[idx] = pi[rng.permutation(idx)]
        a0[b, :n] = pi
    out = qap.greedy_qap(b1, b2, _dev_i32(a0), T, nv)
    w1, w2 = b1.cpu().numpy(), b2.cpu().numpy()
    for b, n in enumerate(nvalid):
        n = int(n)
        want = R.greedy_qap(R.unpack_bits(w1[b], n), R.unpack_bits(w2[b], n), R.perm_matrix(np.arange(n), a0[b, :n]), T)
        got = tuple(out[k][b].item() for k in GREEDY_KEYS)
        assert got == tuple(want[:5]), (b, got, want[:5])
    _check_perm(out, b1, b2, nv, nvalid)


def test_greedy_is_capturable_and_replays_on_new_inputs():
    """one stream, a linear chain of launches: no host round trip inside"""
    g = GROUPS['er50']
    B, N = g['assign0'].shape
    T = 10
    other = PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.15, seed=9, device=DEV).bits(0, B)
    rng = np.random.default_rng(2)
    a_other = _dev_i32(np.stack([rng.permutation(N) for _ in range(B)]))
    b1, b2, a0 = _dev_i32(g['bits1']).clone(), _dev_i32(g['bits2']).clone(), _dev_i32(g['assign0']).clone()
    eager_other = qap.greedy_qap(other[0], other[1], a_other, T)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        qap.greedy_qap(b1, b2, a0, T)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = qap.greedy_qap(b1, b2, a0, T)
    graph.replay()
    torch.cuda.synchronize()
    for k in GREEDY_KEYS:
        assert np.array_equal(out[k].cpu().numpy(), g['T%d/%s' % (T, k)]), k
    b1.copy_(other[0])
    b2.copy_(other[1])
    a0.copy_(a_other)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], eager_other[k]) for k in out)


def test_bad_arguments_return_the_error_code_without_launching():
    lib = _lib.load()
    z = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = _lib.ptr(z)
    st = _lib.stream_ptr()
    assert lib.fgnn_qap_objective(p, p, p, None, 1, _lib.FGNN_QAP_MAX_N + 1, p, None, None, None, st) == 1
    assert lib.fgnn_qap_improve_cost(p, p, p, None, 1, 4, p, 16, 3, st) == 1                 # ld < N
    assert lib.fgnn_qap_improve_cost(p, p, p, None, 1, 4, None, 16, 4, st) == 1
    assert lib.fgnn_greedy_qap(p, p, p, None, 1, 4, 10, p, 8, p, p, p, None, st) == 1         # workspace too small
    assert 'workspace' in _lib.last_error()
    assert lib.fgnn_greedy_qap(p, p, p, None, 1, 4, -1, p, 1 << 20, p, p, p, None, st) == 1
    with pytest.raises(ValueError):
        qap.greedy_qap(z.view(1, 64, 1)[:, :4], z.view(1, 64, 1)[:, :4], z[:4].view(1, 4), T=-1)


def test_dense_input_is_packed_and_verified_on_the_device():
    g = GROUPS['er33']
    x1 = torch.from_numpy(np.stack([synthetic.tensor_representation(R.unpack_bits(w).astype(np.float32)) for w in g['bits1']])).to(DEV)
    x2 = torch.from_numpy(np.stack([synthetic.tensor_representation(R.unpack_bits(w).astype(np.float32)) for w in g['bits2']])).to(DEV)
    out = qap.greedy_qap(x1, x2, _dev_i32(g['assign0']), 10)
    assert np.array_equal(out['s_best'].cpu().numpy(), g['T10/s_best']) and np.array_equal(out['T_best'].cpu().numpy(), g['T10/T_best'])
    scores = torch.from_numpy(g['scores']).to(DEV)
    acc, q, planted = qap.all_acc_qap(scores, x1, x2)
    assert np.array_equal(planted.cpu().numpy(), g['planted'])
    # the matching is the device solver's on the device's log_softmax: compared through the solver's own output
    N = scores.shape[-1]
    cost = (-torch.log_softmax(scores, -1)).contiguous()
    correct = torch.empty(len(scores), dtype=torch.int32, device=DEV)
    assign = torch.empty(len(scores), N, dtype=torch.int32, device=DEV)
    _lib.call('fgnn_lsap_accuracy', _lib.ptr(cost), N * N, N, None, len(scores), N, _lib.ptr(correct), _lib.ptr(assign), _lib.stream_ptr())
    assert torch.equal(acc, correct.long())
    for b, pi in enumerate(assign.cpu().numpy()):
        A, Bm = R.unpack_bits(g['bits1'][b]), R.unpack_bits(g['bits2'][b])
        assert int(q[b]) == int((A * Bm[pi, :][:, pi]).sum())
    bad = x1.clone()
    bad[1, 0, 2, 3] = 2.0
    with pytest.raises(RuntimeError, match='NOT the tensor representation'):
        qap.qap_objective(bad, x2, _dev_i32(g['assign0']))


def _ne(blocks, ragged=False):
    ne = dict(type='node_embedding', block_init='block_emb', block_inside='block', num_blocks=blocks, in_features=32,
              out_features=32, depth_of_mlp=3)
    if ragged:
        ne['constant_n_vertices'] = False
    return ne


def _check_match(model, out, x1t, x2t, sizes, refine):
    """out of model.match against the pieces it is made of; x1t / x2t: dense (B, 2, n, n) host tensors, sizes: vertex counts"""
    scores = out['scores']
    s = scores.tensor.rename(None) if isinstance(scores, MaskedTensor) else scores
    B, N, _ = s.shape
    ragged = isinstance(scores, MaskedTensor)
    sm = s
    nvd = None
    if ragged:
        nvd = torch.tensor(sizes, dtype=torch.int32, device=DEV)
        col = torch.arange(N, device=DEV)[None, None, :] < nvd[:, None, None]
        sm = s.masked_fill(~col, float('-inf'))
    cost = (-torch.log_softmax(sm.float(), -1)).contiguous()
    correct = torch.empty(B, dtype=torch.int32, device=DEV)
    assign = torch.empty(B, N, dtype=torch.int32, device=DEV)
    _lib.call('fgnn_lsap_accuracy', _lib.ptr(cost), N * N, N, _lib.ptr(nvd), B, N, _lib.ptr(correct), _lib.ptr(assign), _lib.stream_ptr())
    assert torch.equal(out['assign'], assign)
    per = accuracy_linear_assignment(scores, aggregate_score=False)
    assert [a / n for a, n in zip(out['acc'].tolist(), sizes)] == per
    pis = assign.cpu().numpy()
    for b, n in enumerate(sizes):
        g1, g2, col = x1t[b, 0, :n, :n].numpy(), x2t[b, 0, :n, :n].numpy(), pis[b, :n]
        assert int(out['qap'][b]) == int((g1 * (g2[col, :][:, col])).sum())
        assert int(out['planted'][b]) == int((g1 * g2).sum())
    if refine:
        for b, n in enumerate(sizes):
            want = R.greedy_qap(x1t[b, 0, :n, :n].double().numpy(), x2t[b, 0, :n, :n].double().numpy(),
                                R.perm_matrix(np.arange(n), pis[b, :n]), refine)
            assert tuple(out[k][b].item() for k in GREEDY_KEYS) == tuple(want[:5])
    else:
        assert 's_best' not in out


def test_module_match_dense_dict_and_refine():
    torch.manual_seed(3)
    model = Siamese_Node_Exp(2, _ne(2)).to(DEV)
    x1, x2 = synthetic.make_batch(11, 4, 40, 'ErdosRenyi', 0.2, 0.1)
    loss = model.loss(model(x1.to(DEV), x2.to(DEV)))
    loss.backward()
    grads = [p.grad.clone() for p in model.parameters()]
    sizes = [40] * 4
    out = model.match(x1.to(DEV), x2.to(DEV))
    _check_match(model, out, x1, x2, sizes, 0)
    out_d = model.match({'input': x1.to(DEV)}, {'input': x2.to(DEV)}, refine=10)
    _check_match(model, out_d, x1, x2, sizes, 10)
    assert torch.equal(out_d['scores'], out['scores']) and torch.equal(out_d['assign'], out['assign'])
    assert not out['scores'].requires_grad
    assert all(torch.equal(p.grad, g) for p, g in zip(model.parameters(), grads))
    bad = x1.clone()
    bad[0, 0, 3, 4] = 0.25
    with pytest.raises(RuntimeError, match='NOT the tensor'):
        model.match(bad.to(DEV), x2.to(DEV))
    with pytest.raises(RuntimeError, match='NOT the tensor'):
        qap.to_bits(torch.zeros(2, 3, 12, 12, device=DEV))                          # three channels: no tensor representation


def test_module_match_masked_batch():
    torch.manual_seed(4)
    model = Siamese_Node_Exp(2, _ne(2, ragged=True)).to(DEV)
    sizes = [30, 17, 24]
    rng = np.random.default_rng(8)
    xs, ys = [], []
    for n in sizes:
        a, b = synthetic.make_pair(rng, n, 'ErdosRenyi', 0.3, 0.1)
        xs.append(torch.from_numpy(a))
        ys.append(torch.from_numpy(b))
    m1 = from_list([x.to(DEV) for x in xs], dims=(1, 2), base_name='N')
    m2 = from_list([y.to(DEV) for y in ys], dims=(1, 2), base_name='M')
    nmax = max(sizes)
    x1t, x2t = torch.zeros(3, 2, nmax, nmax), torch.zeros(3, 2, nmax, nmax)
    for b, n in enumerate(sizes):
        x1t[b, :, :n, :n], x2t[b, :, :n, :n] = xs[b], ys[b]
    out = model.match(m1, m2, refine=10)
    assert isinstance(out['scores'], MaskedTensor)
    _check_match(model, out, x1t, x2t, sizes, 10)
    assert all(p.grad is None for p in model.parameters())
