"""GPU: the pairwise-exchange search on real-weighted pairs -- fgnn_qapw_2opt through qap.two_opt_weighted -- against
tests/two_opt_weighted_ref.py (held to SciPy by tests/test_two_opt_weighted_host.py).

Exact inputs (integer weights in [-3, 3], dyadic k/8; symmetric pairs and directed pairs with loops): every gain and objective is
exact in fp32, so perm, swaps, nit, status and qap equal the float64 reference exactly.  The shapes: each instantiation (N <= 32, 64,
128 in LDS; N <= 256 with Bp in the workspace) on both sides of its edge, one pair, a few, and more pairs than a wave has lanes;
corners of 0, 1 and N vertices in one batch with NaN outside the corners and arbitrary `assign` entries outside them.

Real weights (the spectral L of PairGenerator.spectral): the trajectory is the kernel's own, so the checks are properties.  With
u = 2^-24 and one fmaf chain of 2 n terms whose factors are two rounded differences, the fp32 gain g' of a pair and the float64
gain g of the same fp32 matrices obey |g' - g| <= gamma_m sum |terms|, gamma_m = m u / (1 - m u), m = 2 n + 12: a pair that was
not accepted (g' <= 0) has g <= gamma_m sum |terms|, an accepted one (g' > 0) has g >= -gamma_m sum |terms|.  For ANY pair and
matching sum |terms| <= 2 n (2 max|A|) (2 max|B|), which bounds the loss of every exchange of a trajectory."""
import numpy as np
import pytest
import torch

import two_opt_weighted_ref as R
from graph_neural_net_amd import _lib, qap
from graph_neural_net_amd.pairgen import PairGenerator

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INT_KEYS = ('swaps', 'nit', 'status')
U = 2.0 ** -24


def _dense(mats, N, seed=None):
    """pairs' matrices -> (B, N, N) float32 device tensor; outside each corner zero (seed None), else NaN and arbitrary values"""
    x = torch.zeros(len(mats), N, N)
    if seed is not None:
        x = torch.randn(len(mats), N, N, generator=torch.Generator().manual_seed(seed)) * 5
        x[:, ::2] = float('nan')
    for b, m in enumerate(mats):
        x[b, :len(m), :len(m)] = torch.from_numpy(m).float()
    return x.to(DEV)


def _assign(starts, N, junk=False):
    a = np.full((len(starts), N), -1, dtype=np.int32)
    for b, s in enumerate(starts):
        a[b, :len(s)] = s
        if junk:
            a[b, len(s):] = (b + 3) % N
    return torch.from_numpy(a).to(DEV)


def _nv(starts):
    return torch.tensor([len(s) for s in starts], dtype=torch.int32, device=DEV)


def _check(out, refs, starts, N):
    """every output against the reference's, exactly -> the exchanges of the batch"""
    got_perm = out['perm'].cpu().tolist()
    got = {k: out[k].cpu().tolist() for k in INT_KEYS + ('qap',)}
    for b, (ref, s) in enumerate(zip(refs, starts)):
        print('pair %d n %d: swaps %d nit %d status %d qap %r | reference %d %d %d %r' % (
            b, len(s), got['swaps'][b], got['nit'][b], got['status'][b], got['qap'][b], ref['swaps'], ref['nit'], ref['status'], ref['qap']))
    for b, (ref, s) in enumerate(zip(refs, starts)):
        assert got_perm[b] == ref['perm'].tolist() + [-1] * (N - len(s)), b
        assert [got[k][b] for k in INT_KEYS] == [ref[k] for k in INT_KEYS], (b, len(s))
        assert got['qap'][b] == ref['qap'], (b, len(s))
    return sum(r['swaps'] for r in refs)


def _ids(c):
    return '%d-%d-%s-%s' % (c[0], c[1], 'sym' if c[2] else 'dir', c[3])


# ------------------------------------------------------------------------------------------------------------- 1. exact cases
@pytest.mark.parametrize('case', R.CASES, ids=_ids)
def test_kernel_equals_the_reference_exactly(case):
    N, B, symmetric, kind = case
    As, Bs, starts = R.batch_of(*case)
    refs = R.reference(*case)
    ragged = B > 1
    x1, x2 = _dense(As, N, N if ragged else None), _dense(Bs, N, N + 99 if ragged else None)
    assign = _assign(starts, N, junk=ragged)
    nv = _nv(starts) if ragged else None
    out = qap.two_opt_weighted(x1, x2, assign, nvalid=nv)
    assert set(out) == {'perm', 'qap', 'qap0', 'acc', 'swaps', 'nit', 'status'} and all(t.is_cuda for t in out.values())
    assert out['perm'].dtype == torch.int32 and out['qap'].dtype == out['qap0'].dtype == torch.float32
    assert all(out[k].dtype == torch.int64 for k in ('acc', 'swaps', 'nit', 'status'))
    total = _check(out, refs, starts, N)
    assert N < 3 or total > 0
    assert out['qap0'].cpu().tolist() == [R.objective(A, Bm, s) for A, Bm, s in zip(As, Bs, starts)]
    assert out['acc'].cpu().tolist() == [int((r['perm'] == np.arange(len(s))).sum()) for r, s in zip(refs, starts)]
    if not symmetric and N > 2:
        assert any(len(A) > 2 and (not np.array_equal(A, A.T)) and A.diagonal().any() for A in As)


# ----------------------------------------------------------------------------------------------------------------- 2. layouts
@pytest.mark.parametrize('case', [(33, 5, False, 'dyadic'), (65, 5, False, 'dyadic'), (129, 5, False, 'int')], ids=_ids)
def test_channel_zero_in_place_a_wider_pitch_and_junk_outside_the_corners(case):
    N, B, symmetric, kind = case
    As, Bs, starts = R.batch_of(*case)
    refs = R.reference(*case)
    nv, assign = _nv(starts), _assign(starts, N, junk=True)
    flat = [_dense(As, N, 1), _dense(Bs, N, 2)]
    # channel 0 of a (B, 4, N, N) batch: read in place, pairs 4 N N floats apart
    four = [torch.full((B, 4, N, N), float('nan'), device=DEV) for _ in range(2)]
    for f, x in zip(four, flat):
        f[:, 0] = x
    v1, v2, gs, ld = qap.weighted_views(four[0], four[1])
    assert (gs, ld) == (4 * N * N, N) and v1.data_ptr() == four[0].data_ptr() and v2.data_ptr() == four[1].data_ptr()
    out = qap.two_opt_weighted(four[0], four[1], assign, nvalid=nv)
    _check(out, refs, starts, N)
    copy = qap.two_opt_weighted(flat[0], flat[1], assign, nvalid=nv)
    assert all(torch.equal(out[k], copy[k]) for k in out)
    # the corner of wider matrices: row pitch N + 5, pairs (N + 3) (N + 5) floats apart
    wide = [torch.full((B, N + 3, N + 5), float('nan'), device=DEV) for _ in range(2)]
    for w, x in zip(wide, flat):
        w[:, :N, :N] = x
    views = [w[:, :N, :N] for w in wide]
    assert qap.weighted_views(*views)[2:] == ((N + 3) * (N + 5), N + 5)
    pitched = qap.two_opt_weighted(views[0], views[1], assign, nvalid=nv)
    assert all(torch.equal(out[k], pitched[k]) for k in out)
    # entries of `assign` outside the corner do not matter
    plain = qap.two_opt_weighted(flat[0], flat[1], _assign(starts, N), nvalid=nv)
    assert all(torch.equal(out[k], plain[k]) for k in out)


# ------------------------------------------------------------------------------------------------------------ 3. real weights
@pytest.mark.parametrize('family', ['ErdosRenyi', 'Regular'])
@pytest.mark.parametrize('N', [33, 50, 129])
def test_real_weights_end_in_a_local_optimum_up_to_rounding(N, family):
    B = 3
    gen = PairGenerator(N, family, 'ErdosRenyi', edge_density=0.3, noise=0.1, seed=N, device=DEV)
    f1, f2 = (d['input'] for d in gen.spectral(0, B))
    assert f1.shape == (B, 4, N, N) and f1.dtype == torch.float32
    rng = np.random.default_rng(N + len(family))
    starts = [rng.permutation(N) for _ in range(B)]
    assign = _assign(starts, N)
    out = qap.two_opt_weighted(f1, f2, assign)
    again = qap.two_opt_weighted(f1, f2, assign)
    assert all(torch.equal(out[k], again[k]) for k in out)                                          # (e)
    assert torch.equal(out['qap'], qap.objective_weighted(f1, f2, out['perm'], None)['qap'])        # (d)
    assert torch.equal(out['qap0'], qap.objective_weighted(f1, f2, assign, None)['qap'])
    m = 2 * N + 12
    gamma = m * U / (1 - m * U)
    perm, status, swaps = out['perm'].cpu().numpy(), out['status'].cpu().tolist(), out['swaps'].cpu().tolist()
    upper = np.triu(np.ones((N, N), dtype=bool), 1)
    for b in range(B):
        A, Bm = f1[b, 0].double().cpu().numpy(), f2[b, 0].double().cpu().numpy()
        p = perm[b].astype(np.int64)
        assert sorted(p.tolist()) == list(range(N))                                                 # (a)
        g, s = R.gains(A, Bm[np.ix_(p, p)])
        worst = float((g - gamma * s)[upper].max())
        any_pair = gamma * 2 * N * (2 * np.abs(A).max()) * (2 * np.abs(Bm).max())
        assert float(s.max()) <= 2 * N * (2 * np.abs(A).max()) * (2 * np.abs(Bm).max())
        gain = R.objective(A, Bm, p) - R.objective(A, Bm, starts[b])
        print('N %d %s pair %d: status %d swaps %d nit %d qap0 %.6f qap %.6f; largest (gain - bound) of a pair %.3e; '
              'float64 gain of the search %.6f, allowed loss %.3e' % (N, family, b, status[b], swaps[b], int(out['nit'][b]),
                                                                       float(out['qap0'][b]), float(out['qap'][b]), worst, gain,
                                                                       swaps[b] * any_pair))
        assert status[b] in (0, 1) and (status[b] == 0 or swaps[b] == N * N)
        if status[b] == 0:
            assert worst <= 0.0                                                                     # (b)
        assert gain >= -swaps[b] * any_pair                                                         # (c)
    assert sum(swaps) > 0


# ----------------------------------------------------------------------------------------------------------------- 4. control
CONTROL = (50, 5, True, 'dyadic')


@pytest.mark.parametrize('max_swaps', [0, 1, 3])
def test_max_swaps_stops_the_search_in_the_references_state(max_swaps):
    N = CONTROL[0]
    As, Bs, starts = R.batch_of(*CONTROL)
    refs = R.reference(*CONTROL, max_swaps)
    x1, x2, assign, nv = _dense(As, N, 5), _dense(Bs, N, 6), _assign(starts, N), _nv(starts)
    out = qap.two_opt_weighted(x1, x2, assign, nvalid=nv, max_swaps=max_swaps)
    _check(out, refs, starts, N)
    status = out['status'].cpu().tolist()
    assert status[0] == 0 and status[2] == 1 and int(out['swaps'][2]) == max_swaps      # (the empty pair; a pair that had more to do)
    if max_swaps == 0:
        assert torch.equal(out['perm'][2], assign[2]) and out['nit'].cpu().tolist()[1:] == [0] * 4
        assert torch.equal(out['qap'], out['qap0'])
    with pytest.raises(ValueError, match='max_swaps'):
        qap.two_opt_weighted(x1, x2, assign, nvalid=nv, max_swaps=-2)


@pytest.mark.parametrize('N', [33, 129])
def test_an_invalid_start_is_reported_and_its_neighbours_are_not_touched(N):
    pairs = [R.make_pair(N, b, b % 2 == 0, 'int') for b in range(5)]
    As, Bs = [p[0] for p in pairs], [p[1] for p in pairs]
    starts = [R.transposed(p[2], 3, b) for b, p in enumerate(pairs)]
    for b, (at, value) in {0: (4, -1), 2: (N - 1, N), 4: (7, None)}.items():
        starts[b][at] = starts[b][at + 1] if value is None else value
    x1, x2, assign = _dense(As, N), _dense(Bs, N), _assign(starts, N)
    out = qap.two_opt_weighted(x1, x2, assign)
    refs = [R.two_opt(A, Bm, s) for A, Bm, s in zip(As, Bs, starts)]
    _check(out, refs, starts, N)
    assert out['status'].cpu().tolist() == [2, 0, 2, 0, 2] and out['qap'].cpu().tolist()[::2] == [-1.0, -1.0, -1.0]
    assert torch.equal(out['perm'][::2], assign[::2]) and out['nit'].cpu().tolist()[::2] == [0, 0, 0]
    assert out['swaps'].cpu().tolist()[::2] == [0, 0, 0]
    alone = qap.two_opt_weighted(x1[1:2], x2[1:2], assign[1:2])
    assert all(torch.equal(alone[k][0], out[k][1]) for k in out)


def test_bad_arguments_return_the_error_code_without_launching():
    lib = _lib.load()
    z = torch.zeros(1024, dtype=torch.int32, device=DEV)
    p, st = _lib.ptr(z), _lib.stream_ptr()
    big = _lib.FGNN_QAPW_MAX_N + 1

    def entry(a1=p, a2=p, gs=16, ld=4, assign=p, B=1, N=4, ws=None, nbytes=0, perm=p, swaps=p, nit=p, status=p):
        return lib.fgnn_qapw_2opt(a1, a2, gs, ld, assign, None, B, N, -1, ws, nbytes, perm, swaps, nit, status, st)
    assert entry(gs=big * big, ld=big, N=big, ws=p, nbytes=1 << 30) == 1 and 'at most' in _lib.last_error()
    assert entry(ld=3) == 1                                         # ld < N
    assert entry(gs=15) == 1                                        # gstride < N ld
    assert entry(B=65536) == 1
    for null in ('a1', 'a2', 'assign', 'perm', 'swaps', 'nit', 'status'):
        assert entry(**{null: None}) == 1, null
    # N = 129 needs its workspace: present, long enough, 16-byte aligned
    n = 129
    need = lib.fgnn_qapw_2opt_ws_bytes(1, n)
    assert need >= n * n * 4
    ws = torch.zeros(need + 64, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 16 == 0
    at129 = dict(gs=n * n, ld=n, N=n)
    assert entry(**at129, ws=None, nbytes=0) == 1 and 'workspace' in _lib.last_error()
    assert entry(**at129, ws=_lib.ptr(ws), nbytes=need - 1) == 1
    assert entry(**at129, ws=_lib.ptr(ws[4:]), nbytes=need) == 1    # misaligned
    assert lib.fgnn_qapw_2opt_ws_bytes(1, 128) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- 5. chain
def test_greedy_then_two_opt_equals_the_host_route_of_the_same_chain():
    N, B = 50, 3
    pairs = [R.make_pair(N, 20 + b, True, 'dyadic') for b in range(B)]
    x1, x2 = _dense([p[0] for p in pairs], N), _dense([p[1] for p in pairs], N)
    rng = np.random.default_rng(50)
    assign = _assign([rng.permutation(N) for _ in range(B)], N)
    labels = torch.from_numpy(np.stack([p[2] for p in pairs])).to(DEV)
    g = qap.greedy_weighted(x1, x2, assign, 2, None)
    out = qap.two_opt_weighted(x1, x2, g['perm'], labels=labels)
    hg = qap.greedy_qap(x1.cpu(), x2.cpu(), assign.cpu(), 2, weighted=True)
    assert torch.equal(g['perm'].cpu(), hg['perm'])
    host = qap.two_opt_weighted(x1.cpu(), x2.cpu(), hg['perm'], labels=labels.cpu())
    print('chain: greedy s_best %s -> qap0 %s -> qap %s, swaps %s' % (g['s_best'].tolist(), out['qap0'].tolist(), out['qap'].tolist(),
                                                                      out['swaps'].tolist()))
    for k in out:
        assert torch.equal(out[k].cpu().double() if k in ('qap', 'qap0') else out[k].cpu(), host[k]), k
    assert bool((out['status'] == 0).all()) and int(out['swaps'].sum()) > 0 and bool((out['qap'] >= out['qap0']).all())
