"""GPU: the matching decode on real-weighted pairs (csrc/qap_weighted.hip, graph_neural_net_amd/qap.py with weighted=True,
Siamese_Node_Exp.match(weighted=True)) against numpy float64, the reference's recorded results (tests/golden/qap_weighted.npz) and
tests/qap_weighted_ref.py.

Exact inputs (integer weights 0 .. 15, dyadic k / 8: every product and partial sum is representable in fp32, all sums < 2^24 units for
N <= 256) are compared EXACTLY.  Real inputs are held to the any-order summation bound computed from the inputs: a sum of m fp32
terms lies within gamma_m sum |terms| of its exact value, gamma_m = m u / (1 - m u), u = 2^-24 (R.gamma; m = n^2 for the objective
sums, m = n for one cost entry)."""
import numpy as np
import pytest
import torch

import qap_weighted_ref as R
from graph_neural_net_amd import _lib, qap, synthetic
from graph_neural_net_amd.masked import MaskedTensor
from graph_neural_net_amd.metrics import lsap_device
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.siamese import Siamese_Node_Exp

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TS, GREEDY_KEYS = R.TS, R.GREEDY_KEYS
GROUPS = R.fixture_groups()
FILL = -777.0


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _int_pairs(seed, B, N, sym=False):
    """(a1, a2) (B, N, N) float32 with integer weights 0 .. 15 (about 40 % non-zero); not symmetric unless asked"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        w = rng.integers(1, 16, size=(B, N, N)) * (rng.random((B, N, N)) < 0.4)
        if sym:
            w = np.triu(w, 1) + np.triu(w, 1).transpose(0, 2, 1)
        out.append(w.astype(np.float32))
    return out


def _perms(seed, B, N, nvalid=None):
    rng = np.random.default_rng(seed)
    a = np.full((B, N), -1, dtype=np.int32)
    for b in range(B):
        n = N if nvalid is None else int(nvalid[b])
        a[b, :n] = rng.permutation(n)
    return a


def _cost_dev(x1, x2, gstride, ld, assign, nvalid, B, N, cost_ld=None, bstride=None):
    """fgnn_qapw_improve_cost on device tensors x1 / x2 (data_ptr = channel 0 of pair 0) -> the whole cost buffer, pre-filled with FILL"""
    cost_ld = N if cost_ld is None else cost_ld
    bstride = N * cost_ld if bstride is None else bstride
    buf = torch.full((B * bstride,), FILL, dtype=torch.float32, device=DEV)
    nv = _dev(nvalid, np.int32) if nvalid is not None else None
    a = _dev(assign, np.int32)                               # (kept alive: a freed tensor's block is handed out again)
    _lib.call('fgnn_qapw_improve_cost', _lib.ptr(x1), _lib.ptr(x2), gstride, ld, _lib.ptr(a), _lib.ptr(nv), B, N, _lib.ptr(buf), bstride,
              cost_ld, _lib.stream_ptr())
    return buf.cpu().numpy()


def _check_cost(a1, a2, assign, nvalid=None, cost_ld=None, bstride=None, dev_inputs=None, exact=True):
    """the device cost against -(A @ P @ B) in float64 on every corner (a1 / a2: clean host matrices); everything outside the corners
    keeps the fill value.  dev_inputs = (x1, x2, gstride, ld) overrides how the matrices reach the device."""
    B, N, _ = a1.shape
    ld_ = N if cost_ld is None else cost_ld
    bs_ = N * ld_ if bstride is None else bstride
    x1, x2, gs, ld = dev_inputs if dev_inputs is not None else (_dev(a1), _dev(a2), N * N, N)
    got = _cost_dev(x1, x2, gs, ld, assign, nvalid, B, N, cost_ld, bstride)
    untouched = np.ones(got.shape, dtype=bool)
    for b in range(B):
        n = N if nvalid is None else int(nvalid[b])
        A, Bm = a1[b, :n, :n].astype(np.float64), a2[b, :n, :n].astype(np.float64)
        P = R.perm_matrix(np.arange(n), assign[b, :n])
        rows = (b * bs_ + np.arange(n)[:, None] * ld_ + np.arange(n)[None, :]).reshape(n, n)
        want = -(A @ P @ Bm)
        if exact:
            assert np.array_equal(got[rows], want.astype(np.float32)), b
        else:
            bound = R.gamma(n) * (np.abs(A) @ P @ np.abs(Bm))
            assert np.isfinite(got[rows]).all() and (np.abs(got[rows] - want) <= bound).all(), (b, np.abs(got[rows] - want).max())
        untouched[rows] = False
    assert (got[untouched] == FILL).all()


def _objective_dev(a1, a2, assign, nvalid=None):
    nv = _dev(nvalid, np.int32) if nvalid is not None else None
    out = qap.objective_weighted(_dev(a1), _dev(a2), _dev(assign, np.int32), nv)
    assert all(v.is_cuda and v.dtype == torch.float32 for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


KEYS5 = ('qap', 'trace', 'planted', 'na', 'nb')


def _check_objective(a1, a2, assign, nvalid=None, exact=True):
    B, N, _ = a1.shape
    got = _objective_dev(a1, a2, assign, nvalid)
    for b in range(B):
        n = N if nvalid is None else int(nvalid[b])
        A, Bm, pi = a1[b, :n, :n].astype(np.float64), a2[b, :n, :n].astype(np.float64), assign[b, :n]
        want, bound = R.objective(A, Bm, pi), R.objective_bounds(A, Bm, pi)
        for k, w, e in zip(KEYS5, want, bound):
            if exact:
                assert got[k][b] == w, (b, k, got[k][b], w)
            else:
                assert np.isfinite(got[k][b]) and abs(float(got[k][b]) - w) <= e, (b, k, got[k][b], w, e)
    return got


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('N', [1, 2, 15, 16, 17, 31, 32, 33, 64, 65])
def test_cost_and_objective_at_tile_edges_are_exact(N, B):
    a1, a2 = _int_pairs(100 * N + B, B, N)
    assign = _perms(N + B, B, N)
    _check_cost(a1, a2, assign)
    _check_objective(a1, a2, assign)


def test_cost_and_objective_at_the_largest_graph():
    N = _lib.FGNN_QAPW_MAX_N
    a1, a2 = _int_pairs(7, 2, N)
    a1[0], a2[0] = 15.0, 15.0                                # the largest sums the exact contract covers: 225 * 256^2 < 2^24
    assign = _perms(8, 2, N)
    _check_cost(a1, a2, assign)
    _check_objective(a1, a2, assign)


@pytest.mark.parametrize('N', [50, 130, 256])
def test_real_weights_lie_within_the_summation_bound(N):
    rng = np.random.default_rng(N)
    a1 = (rng.random((2, N, N)) - 0.3).astype(np.float32)              # mixed signs: cancellation, the bound is on sum |a||b|
    a2 = (rng.random((2, N, N)) - 0.3).astype(np.float32)
    assign = _perms(N, 2, N)
    _check_cost(a1, a2, assign, exact=False)
    got = _check_objective(a1, a2, assign, exact=False)
    again = _objective_dev(a1, a2, assign)
    assert all(np.array_equal(got[k], again[k]) for k in KEYS5)        # fixed order: bit-identical from run to run


def test_ragged_batch_ignores_nan_outside_the_corners_and_writes_only_the_corners():
    B, N = 5, 70
    nvalid = np.array([70, 0, 1, 33, 64], dtype=np.int32)
    a1, a2 = _int_pairs(5, B, N)
    assign = _perms(6, B, N, nvalid)
    n1, n2 = a1.copy(), a2.copy()
    for b, n in enumerate(nvalid):
        for m in (n1, n2):
            m[b, n:, :] = np.nan
            m[b, :, n:] = np.nan
    _check_cost(a1, a2, assign, nvalid, dev_inputs=(_dev(n1), _dev(n2), N * N, N))
    _check_cost(a1, a2, assign, nvalid, cost_ld=N + 7, bstride=N * (N + 7) + 13, dev_inputs=(_dev(n1), _dev(n2), N * N, N))
    clean, dirty = _check_objective(a1, a2, assign, nvalid), _objective_dev(n1, n2, assign, nvalid)
    assert all(np.isfinite(dirty[k]).all() and np.array_equal(clean[k], dirty[k]) for k in KEYS5)
    assert all(clean[k][1] == 0 for k in KEYS5)                        # the empty pair
    nv, a0 = _dev(nvalid), _dev(assign)
    gc, gd = qap.greedy_qap(_dev(a1), _dev(a2), a0, 3, nv, weighted=True), qap.greedy_qap(_dev(n1), _dev(n2), a0, 3, nv, weighted=True)
    assert all(torch.equal(gc[k], gd[k]) and (gd[k].is_floating_point() is False or torch.isfinite(gd[k]).all()) for k in gc)
    assert [gc[k][1].item() for k in GREEDY_KEYS] == [0, 0, 0, 0, 0] and (gc['perm'][1] == -1).all()
    holed = assign.copy()
    holed[0, 3] = -1                                         # inside the corner: -1 is then the sentinel, not a value
    oh = _objective_dev(a1, a2, holed, nvalid)
    assert oh['qap'][0] == -1 and oh['trace'][0] == -1 and oh['planted'][0] == clean['planted'][0]
    assert np.array_equal(oh['qap'][1:], clean['qap'][1:]) and np.array_equal(oh['trace'][1:], clean['trace'][1:])


def test_input_pitch_pair_stride_and_a_four_channel_batch_in_place():
    B, N = 3, 37
    a1, a2 = _int_pairs(11, B, N)
    assign = _perms(12, B, N)
    # ld > N and gstride > N ld: the matrices sit in the corner of NaN-filled (N + 3) x (N + 5) planes
    p1, p2 = np.full((B, N + 3, N + 5), np.nan, np.float32), np.full((B, N + 3, N + 5), np.nan, np.float32)
    p1[:, :N, :N], p2[:, :N, :N] = a1, a2
    wide = (_dev(p1), _dev(p2), (N + 3) * (N + 5), N + 5)
    _check_cost(a1, a2, assign, dev_inputs=wide)
    _check_cost(a1, a2, assign, cost_ld=N + 2, bstride=N * (N + 2) + 5, dev_inputs=wide)
    # (B, 4, N, N): channel 0 in place, the other channels NaN
    c1, c2 = np.full((B, 4, N, N), np.nan, np.float32), np.full((B, 4, N, N), np.nan, np.float32)
    c1[:, 0], c2[:, 0] = a1, a2
    x1, x2 = _dev(c1), _dev(c2)
    _check_cost(a1, a2, assign, dev_inputs=(x1, x2, 4 * N * N, N))
    v1, v2, gs, ld = qap.weighted_views(x1, x2)
    assert (v1.data_ptr(), v2.data_ptr(), gs, ld) == (x1.data_ptr(), x2.data_ptr(), 4 * N * N, N)          # nothing is copied
    want = _check_objective(a1, a2, assign)
    got = qap.qap_objective(x1, x2, _dev(assign), weighted=True)
    assert set(got) == {'qap', 'planted', 'na', 'nb'}
    assert all(np.array_equal(got[k].cpu().numpy(), want[k]) for k in got)
    # the views of the padded planes pass without a copy as well
    s1, s2 = wide[0][:, :N, :N], wide[1][:, :N, :N]
    assert qap.weighted_views(s1, s2)[2:] == ((N + 3) * (N + 5), N + 5)
    got = qap.qap_objective(s1, s2, _dev(assign), weighted=True)
    assert all(np.array_equal(got[k].cpu().numpy(), want[k]) for k in got)


def test_qap_and_trace_differ_on_the_non_symmetric_pairs():
    g = GROUPS['int_nonsym']
    got = _check_objective(g['a1'], g['a2'], g['assign0'])
    assert (got['qap'] != got['trace']).any()
    assert np.array_equal(got['qap'], g['qap']) and np.array_equal(got['trace'], 2 * g['score0'])
    n = g['a1'].shape[1]
    A, Bm, P = g['a1'][1].astype(np.float64), g['a2'][1].astype(np.float64), R.perm_matrix(np.arange(n), g['assign0'][1])
    cost = _cost_dev(_dev(g['a1'][1:2]), _dev(g['a2'][1:2]), n * n, n, g['assign0'][1:2], None, 1, n).reshape(n, n)
    assert np.array_equal(cost, (-(A @ P @ Bm)).astype(np.float32))
    assert not np.array_equal(cost, (-(A @ P @ Bm.T)).astype(np.float32))       # (what using B's rows as its columns would give)


def _group_dev(g):
    ragged = bool((g['nvalid'] != g['a1'].shape[1]).any())
    return _dev(g['a1']), _dev(g['a2']), _dev(g['assign0']), _dev(g['nvalid']) if ragged else None


def _check_perm(out, a1, a2, nvalid):
    """perm is a permutation of the corner (-1 in the padding) whose trace / 2, recomputed in float64, is s_best within the bound;
    returns the bounds"""
    perm, s_best = out['perm'].cpu().numpy(), out['s_best'].cpu().numpy()
    bounds = []
    for b, n in enumerate(nvalid):
        n = int(n)
        assert sorted(perm[b, :n].tolist()) == list(range(n)) and (perm[b, n:] == -1).all()
        A, Bm = a1[b, :n, :n].astype(np.float64), a2[b, :n, :n].astype(np.float64)
        trace, bound = R.objective(A, Bm, perm[b, :n])[1], R.objective_bounds(A, Bm, perm[b, :n])[1]
        assert abs(float(s_best[b]) - trace / 2) <= bound / 2, (b, s_best[b], trace / 2, bound / 2)
        bounds.append(bound / 2)
    return bounds


@pytest.mark.parametrize('name', R.EXACT_GROUPS)
def test_greedy_equals_fixture(name):
    g = GROUPS[name]
    a1, a2, a0, nv = _group_dev(g)
    for T in TS:
        out = qap.greedy_qap(a1, a2, a0, T, nv, weighted=True)
        for k in GREEDY_KEYS:
            want = g['T%d/%s' % (T, k)]
            assert out[k].is_cuda and out[k].dtype == (torch.float32 if want.dtype == np.float64 else torch.int64), k
            assert np.array_equal(out[k].cpu().numpy(), want), (name, T, k, out[k].cpu().numpy(), want)
        assert out['perm'].dtype == torch.int32
        again = qap.objective_weighted(a1, a2, out['perm'], nv)
        assert torch.equal(again['trace'], 2 * out['s_best'])
        _check_perm(out, g['a1'], g['a2'], g['nvalid'])
        if T == 0:
            assert torch.equal(out['perm'], a0) and np.array_equal(out['s_best'].cpu().numpy(), g['score0'])
        twice = qap.greedy_qap(a1, a2, a0, T, nv, weighted=True)
        assert all(torch.equal(out[k], twice[k]) for k in out)


def test_all_acc_qap_equals_fixture():
    for name in ('int_sym', 'ragged'):
        g = GROUPS[name]
        a1, a2, _, nv = _group_dev(g)
        acc, q, planted = qap.all_acc_qap(_dev(g['scores']), a1, a2, nv, weighted=True)
        assert acc.dtype == torch.int64 and q.dtype == planted.dtype == torch.float32
        assert np.array_equal(acc.cpu().numpy(), g['acc']) and np.array_equal(q.cpu().numpy(), g['qap'])
        assert np.array_equal(planted.cpu().numpy(), g['planted'])


def test_greedy_at_n200_equals_the_restatement():
    N, B, T = 200, 2, 3
    a1, _ = _int_pairs(21, B, N, sym=True)
    rng = np.random.default_rng(22)
    a2 = a1.copy()
    for b in range(B):                                        # the second side: some edges re-weighted, symmetrically
        m = np.triu(rng.random((N, N)) < 0.1, 1)
        a2[b][m | m.T] = 0
    a0 = np.tile(np.arange(N, dtype=np.int32), (B, 1))
    for b in range(B):
        idx = rng.choice(N, size=N // 2, replace=False)
        a0[b, idx] = a0[b, rng.permutation(idx)]
    out = qap.greedy_qap(_dev(a1), _dev(a2), _dev(a0), T, weighted=True)
    for b in range(B):
        want = R.greedy_qap(a1[b].astype(np.float64), a2[b].astype(np.float64), R.perm_matrix(np.arange(N), a0[b]), T)
        assert tuple(out[k][b].item() for k in GREEDY_KEYS) == want[:5], (b, want[:5])
        assert np.array_equal(out['perm'][b].cpu().numpy(), want[5])


def test_greedy_invariants_on_the_spectral_pairs():
    g = GROUPS['spectral']
    a1, a2, a0, nv = _group_dev(g)
    B, N = g['assign0'].shape
    obj = _check_objective(g['a1'], g['a2'], g['assign0'], exact=False)
    for b in range(B):                                        # the reference's recorded values, under the same bound
        A, Bm = g['a1'][b].astype(np.float64), g['a2'][b].astype(np.float64)
        bq, bt, bp, ba, bb = R.objective_bounds(A, Bm, g['assign0'][b])
        assert abs(obj['qap'][b] - g['qap'][b]) <= bq and abs(obj['trace'][b] - 2 * g['score0'][b]) <= bt
        assert abs(obj['planted'][b] - g['planted'][b]) <= bp
        assert abs(obj['na'][b] - 2 * g['na'][b]) <= ba and abs(obj['nb'][b] - 2 * g['nb'][b]) <= bb
    t0 = qap.greedy_qap(a1, a2, a0, 0, nv, weighted=True)
    assert torch.equal(t0['perm'], a0) and torch.equal(t0['s_best'], _dev(obj['trace']) / 2)
    assert torch.equal(t0['T_best'], torch.zeros_like(t0['T_best']))
    for T in (1, 10):
        out = qap.greedy_qap(a1, a2, a0, T, nv, weighted=True)
        assert out['s_best'].dtype == out['na'].dtype == out['nb'].dtype == torch.float32
        _check_perm(out, g['a1'], g['a2'], g['nvalid'])
        s = out['s_best'].cpu().numpy()
        for b in range(B):                                    # never below the initial score (itself within ITS bound of score0)
            A, Bm = g['a1'][b].astype(np.float64), g['a2'][b].astype(np.float64)
            assert s[b] >= g['score0'][b] - R.objective_bounds(A, Bm, g['assign0'][b])[1] / 2
            assert 0 <= int(out['T_best'][b]) < T and 0 <= int(out['acc_best'][b]) <= N
        twice = qap.greedy_qap(a1, a2, a0, T, nv, weighted=True)
        assert all(torch.equal(out[k], twice[k]) for k in out)


def test_greedy_is_capturable_and_replays_on_new_inputs():
    """one stream, a linear chain of launches: no host round trip inside"""
    g = GROUPS['int_sym']
    B, N = g['assign0'].shape
    T = 10
    o1, o2 = _int_pairs(31, B, N, sym=True)
    other = (_dev(o1), _dev(o2), _dev(_perms(32, B, N)))
    a1, a2, a0 = _dev(g['a1']).clone(), _dev(g['a2']).clone(), _dev(g['assign0']).clone()
    eager_other = qap.greedy_qap(other[0], other[1], other[2], T, weighted=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        qap.greedy_qap(a1, a2, a0, T, weighted=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = qap.greedy_qap(a1, a2, a0, T, weighted=True)
    graph.replay()
    torch.cuda.synchronize()
    for k in GREEDY_KEYS:
        assert np.array_equal(out[k].cpu().numpy(), g['T%d/%s' % (T, k)]), k
    a1.copy_(other[0])
    a2.copy_(other[1])
    a0.copy_(other[2])
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], eager_other[k]) for k in out)


def test_bad_arguments_return_the_error_code_without_launching():
    lib = _lib.load()
    z = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = _lib.ptr(z)
    st = _lib.stream_ptr()
    big = _lib.FGNN_QAPW_MAX_N + 1
    assert lib.fgnn_qapw_objective(p, p, big * big, big, p, None, 1, big, p, None, None, None, None, st) == 1
    assert 'at most' in _lib.last_error()
    assert lib.fgnn_qapw_improve_cost(p, p, big * big, big, p, None, 1, big, p, big * big, big, st) == 1
    assert lib.fgnn_greedy_qapw(p, p, big * big, big, p, None, 1, big, 1, p, 1 << 30, p, p, p, None, st) == 1
    assert lib.fgnn_qapw_objective(p, p, 16, 3, p, None, 1, 4, p, None, None, None, None, st) == 1          # ld < N
    assert lib.fgnn_qapw_objective(p, p, 15, 4, p, None, 1, 4, p, None, None, None, None, st) == 1          # gstride < N ld
    assert lib.fgnn_qapw_improve_cost(p, p, 16, 3, p, None, 1, 4, p, 16, 4, st) == 1                        # ld < N
    assert lib.fgnn_qapw_improve_cost(p, p, 16, 4, p, None, 1, 4, p, 16, 3, st) == 1                        # cost_ld < N
    assert lib.fgnn_qapw_improve_cost(p, p, 16, 4, p, None, 1, 4, p, 15, 4, st) == 1                        # bstride < N cost_ld
    assert lib.fgnn_qapw_improve_cost(p, p, 16, 4, p, None, 1, 4, None, 16, 4, st) == 1                     # null pointers
    assert lib.fgnn_qapw_improve_cost(None, p, 16, 4, p, None, 1, 4, p, 16, 4, st) == 1
    assert lib.fgnn_qapw_objective(p, None, 16, 4, p, None, 1, 4, p, None, None, None, None, st) == 1
    assert lib.fgnn_qapw_objective(p, p, 16, 4, None, None, 1, 4, p, None, None, None, None, st) == 1
    assert lib.fgnn_greedy_qapw(p, p, 16, 4, p, None, 1, 4, 10, p, 1 << 20, None, p, p, None, st) == 1
    assert lib.fgnn_greedy_qapw(p, p, 16, 4, p, None, 1, 4, 10, None, 1 << 20, p, p, p, None, st) == 1
    assert lib.fgnn_greedy_qapw(p, p, 16, 4, p, None, 1, 4, 10, p, 8, p, p, p, None, st) == 1               # workspace too small
    assert 'workspace' in _lib.last_error()
    assert lib.fgnn_greedy_qapw(p, p, 16, 4, p, None, 1, 4, -1, p, 1 << 20, p, p, p, None, st) == 1
    with pytest.raises(ValueError):
        qap.greedy_qap(torch.zeros(1, 4, 4, device=DEV), torch.zeros(1, 4, 4, device=DEV), z[:4].view(1, 4), T=-1, weighted=True)
    torch.cuda.synchronize()


def _ne(blocks, ragged=False):
    ne = dict(type='node_embedding', block_init='block_emb', block_inside='block', num_blocks=blocks, in_features=32,
              out_features=32, depth_of_mlp=3)
    if ragged:
        ne['constant_n_vertices'] = False
    return ne


@pytest.mark.parametrize('vertex_proba', [1.0, 0.8])
def test_module_match_takes_spectral_pairs(vertex_proba):
    torch.manual_seed(5)
    ragged = vertex_proba < 1
    model = Siamese_Node_Exp(4, _ne(2, ragged=ragged)).to(DEV)
    gen = PairGenerator(20, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.1, vertex_proba=vertex_proba, seed=3, device=DEV)
    x1, x2 = gen.spectral(0, 4)
    out = model.match(x1, x2, refine=3, weighted=True)
    assert set(out) == {'scores', 'assign', 'acc', 'qap', 'planted', 's_best', 'na', 'nb', 'acc_best', 'T_best', 'perm'}
    assert isinstance(out['scores'], MaskedTensor) == ragged
    for k in ('qap', 'planted', 's_best', 'na', 'nb'):
        assert out[k].dtype == torch.float32 and out[k].is_cuda and out[k].shape == (4,), k
    for k in ('acc', 'acc_best', 'T_best'):
        assert out[k].dtype == torch.int64, k
    assert out['assign'].dtype == out['perm'].dtype == torch.int32
    assert all(p.grad is None for p in model.parameters())
    t1, t2 = (x1.tensor.rename(None), x2.tensor.rename(None)) if ragged else (x1['input'], x2['input'])
    s = out['scores'].tensor.rename(None) if ragged else out['scores']
    nv = x1.nvalid.to(torch.int32) if ragged else None
    correct, assign = lsap_device(s, nv, want_assign=True)
    assert torch.equal(out['assign'], assign) and torch.equal(out['acc'], correct.long())
    N = s.shape[-1]
    sizes = nv.tolist() if ragged else [N] * 4
    a1, a2, pis = t1[:, 0].cpu().numpy(), t2[:, 0].cpu().numpy(), assign.cpu().numpy()
    for b, n in enumerate(sizes):
        A, Bm = a1[b, :n, :n].astype(np.float64), a2[b, :n, :n].astype(np.float64)
        want, bound = R.objective(A, Bm, pis[b, :n]), R.objective_bounds(A, Bm, pis[b, :n])
        assert abs(out['qap'][b].item() - want[0]) <= bound[0] and abs(out['planted'][b].item() - want[2]) <= bound[2]
        assert abs(out['na'][b].item() - want[3] / 2) <= bound[3] / 2 and abs(out['nb'][b].item() - want[4] / 2) <= bound[4] / 2
        assert out['s_best'][b].item() >= want[1] / 2 - bound[1] / 2
    _check_perm(out, a1, a2, sizes)
    # the same call without the keyword still refuses the batch: channel 0 is L, no 0/1 matrix
    with pytest.raises(RuntimeError, match='NOT the tensor'):
        model.match(x1, x2, refine=3)
    with pytest.raises(RuntimeError, match='NOT the tensor'):
        qap.qap_objective(t1, t2, assign, nv)


def test_weighted_and_bit_paths_agree_on_a_zero_one_batch():
    B, N, T = 4, 40, 10
    x1, x2 = synthetic.make_batch(13, B, N, 'ErdosRenyi', 0.2, 0.1)
    x1, x2 = x1.to(DEV), x2.to(DEV)
    rng = np.random.default_rng(14)
    scores = _dev((2.0 * np.eye(N) + 1.2 * rng.standard_normal((B, N, N))).astype(np.float32))
    _, a0 = lsap_device(scores, None, want_assign=True)
    o, ow = qap.qap_objective(x1, x2, a0), qap.qap_objective(x1, x2, a0, weighted=True)
    assert set(o) == set(ow) and all(torch.equal(o[k], ow[k].to(o[k].dtype)) for k in o)
    g, gw = qap.greedy_qap(x1, x2, a0, T), qap.greedy_qap(x1, x2, a0, T, weighted=True)
    assert set(g) == set(gw) and all(torch.equal(g[k], gw[k].to(g[k].dtype)) for k in g)
    r, rw = qap.all_acc_qap(scores, x1, x2), qap.all_acc_qap(scores, x1, x2, weighted=True)
    assert all(torch.equal(u, v.to(u.dtype)) for u, v in zip(r, rw))
