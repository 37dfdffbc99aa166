"""GPU: the seeded pairwise-exchange search on real-weighted pairs -- fgnn_qapw_2opt_seeded through qap.two_opt_weighted_seeded --
against tests/seeded_two_opt_weighted_ref.py (held to SciPy with partial_match by tests/test_seeded_two_opt_weighted_host.py).

Exact inputs (integer weights in [-3, 3], dyadic k/8; symmetric pairs and directed pairs with loops): every gain and objective is
exact in fp32, so perm, swaps, nit, status and qap equal the float64 reference exactly.  The shapes: each instantiation (N <= 32, 64,
128 in LDS; N <= 256 with Bp in the workspace) on both sides of its edge; one pair, a few, and more pairs than a wave has lanes;
corners of 0, 1 and N vertices in one batch with NaN outside the corners and arbitrary `assign` and `seeds` entries outside them.
Seed patterns: every 3rd / 4th row, all rows, all but one, all but two, none (all -1: torch.equal to the unseeded call).

Real weights (the spectral L of PairGenerator.spectral): property checks, with the bound of tests/test_gpu_two_opt_weighted.py --
the fp32 gain g' of a pair and the float64 gain g of the same fp32 matrices obey |g' - g| <= gamma_m sum |terms|, gamma_m =
m u / (1 - m u), u = 2^-24, m = 2 n + 12 (the chain runs over all n vertices with seeds as without) -- applied to the FREE pairs."""
import numpy as np
import pytest
import torch

import seeded_two_opt_weighted_ref as S
import two_opt_weighted_ref as R
from graph_neural_net_amd import _lib, qap
from graph_neural_net_amd.pairgen import PairGenerator

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INT_KEYS = ('swaps', 'nit', 'status')
ALL_KEYS = {'perm', 'qap', 'qap0', 'acc', 'swaps', 'nit', 'status'}
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


def _rows(vectors, N, junk=None):
    """per-pair vectors -> (B, N) int32 device tensor, -1 past each pair's length (junk: arbitrary values there, some >= 0)"""
    a = np.full((len(vectors), N), -1, dtype=np.int32)
    for b, s in enumerate(vectors):
        a[b, :len(s)] = s
        if junk is not None:
            a[b, len(s):] = (b + junk) % N
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
    return '%d-%d-%s-%s-%s' % (c[0], c[1], 'sym' if c[2] else 'dir', c[3], c[4])


# ------------------------------------------------------------------------------------------------------------- 1. exact cases
@pytest.mark.parametrize('case', S.CASES, ids=_ids)
def test_kernel_equals_the_reference_exactly(case):
    N, B, symmetric, kind, pattern = case
    As, Bs, starts, seeds = S.batch_of(*case)
    refs = S.reference(*case)
    ragged = B > 1
    x1, x2 = _dense(As, N, N if ragged else None), _dense(Bs, N, N + 99 if ragged else None)
    assign = _rows(starts, N, junk=3 if ragged else None)
    sd = _rows(seeds, N, junk=5 if ragged else None)
    nv = _nv(starts) if ragged else None
    out = qap.two_opt_weighted_seeded(x1, x2, assign, sd, nvalid=nv)
    assert set(out) == ALL_KEYS and all(t.is_cuda for t in out.values())
    assert out['perm'].dtype == torch.int32 and out['qap'].dtype == out['qap0'].dtype == torch.float32
    assert all(out[k].dtype == torch.int64 for k in ('acc', 'swaps', 'nit', 'status'))
    total = _check(out, refs, starts, N)
    free = max(int((s < 0).sum()) for s in seeds)
    assert free <= 2 or total > 0                                   # not an idle search
    perm = out['perm'].cpu().numpy()
    for b, s in enumerate(seeds):
        assert (perm[b, :len(s)][s >= 0] == s[s >= 0]).all(), b     # the seeds hold
        f = int((s < 0).sum())
        if f <= 1:                                                  # nothing to exchange: the start, one fruitless scan
            assert perm[b, :len(s)].tolist() == starts[b].tolist() and int(out['status'][b]) == 0
            assert int(out['swaps'][b]) == 0 and int(out['nit'][b]) == f * (f + 1) // 2
    assert out['qap0'].cpu().tolist() == [R.objective(A, Bm, s) for A, Bm, s in zip(As, Bs, starts)]
    assert out['acc'].cpu().tolist() == [int((r['perm'] == np.arange(len(s))).sum()) for r, s in zip(refs, starts)]
    if pattern == 'none':                                           # all -1: the unseeded search, key for key
        plain = qap.two_opt_weighted(x1, x2, assign, nvalid=nv)
        assert all(torch.equal(out[k], plain[k]) for k in ALL_KEYS)


@pytest.mark.parametrize('case', [(31, 5, False, 'int'), (64, 5, True, 'dyadic'), (129, 5, False, 'int'), (256, 1, True, 'dyadic')],
                         ids=lambda c: '%d-%d' % c[:2])
def test_seeds_of_minus_one_equal_the_unseeded_launch_on_every_key(case):
    N, B = case[:2]
    As, Bs, starts = R.batch_of(*case)
    ragged = B > 1
    x1, x2 = _dense(As, N, 7 if ragged else None), _dense(Bs, N, 8 if ragged else None)
    assign, nv = _rows(starts, N, junk=3 if ragged else None), _nv(starts) if ragged else None
    plain = qap.two_opt_weighted(x1, x2, assign, nvalid=nv)
    seeded = qap.two_opt_weighted_seeded(x1, x2, assign, torch.full((B, N), -1, dtype=torch.int32, device=DEV), nvalid=nv)
    assert set(plain) == set(seeded) == ALL_KEYS and all(torch.equal(plain[k], seeded[k]) for k in ALL_KEYS)
    _check(seeded, R.reference(*case), starts, N)
    assert int(plain['swaps'].sum()) > 0


# --------------------------------------------------------------------------------------------------------------- 2. refusals
@pytest.mark.parametrize('N', [33, 129])
def test_bad_seeds_are_refused_and_their_neighbours_are_not_touched(N):
    B = 6
    pairs = [R.make_pair(N, b, b % 2 == 0, 'int') for b in range(B)]
    As, Bs = [p[0] for p in pairs], [p[1] for p in pairs]
    masks = [S.seeded_rows(N, 'fourth', b) for b in range(B)]
    starts = [S.start_on_free_rows(p[2], m, 3, 50 + b) for b, (p, m) in enumerate(zip(pairs, masks))]
    seeds = [np.where(m, p[2], -1).astype(np.int64) for p, m in zip(pairs, masks)]
    free = [np.flatnonzero(~m) for m in masks]
    seeds[0][free[0][2]] = N                                         # a target outside the corner
    seeds[2][free[2][1]] = seeds[2][np.flatnonzero(masks[2])[0]]     # one target for two rows
    seeds[4][free[4][0]] = starts[4][free[4][3]]                     # the start holds another column on that row
    x1, x2, assign, sd = _dense(As, N), _dense(Bs, N), _rows(starts, N), _rows(seeds, N)
    out = qap.two_opt_weighted_seeded(x1, x2, assign, sd)
    refs = [S.two_opt_seeded(A, Bm, s, d) for A, Bm, s, d in zip(As, Bs, starts, seeds)]
    _check(out, refs, starts, N)
    assert out['status'].cpu().tolist() == [2, 0, 2, 0, 2, 0] and out['qap'].cpu().tolist()[::2] == [-1.0, -1.0, -1.0]
    assert torch.equal(out['perm'][::2], assign[::2]) and out['nit'].cpu().tolist()[::2] == [0, 0, 0]
    assert out['swaps'].cpu().tolist()[::2] == [0, 0, 0] and int(out['swaps'][1::2].sum()) > 0
    alone = qap.two_opt_weighted_seeded(x1[1:2], x2[1:2], assign[1:2], sd[1:2])
    assert all(torch.equal(alone[k][0], out[k][1]) for k in out)
    # a start that is no permutation is refused with seeds as without
    broken = assign.clone()
    broken[3, 0] = broken[3, 1]
    again = qap.two_opt_weighted_seeded(x1, x2, broken, sd)
    assert again['status'].cpu().tolist() == [2, 0, 2, 2, 2, 0] and torch.equal(again['perm'][3], broken[3])
    assert all(torch.equal(again[k][5], out[k][5]) for k in out)


def test_bad_arguments_return_the_error_code_without_launching():
    lib = _lib.load()
    z = torch.zeros(1024, dtype=torch.int32, device=DEV)
    p, st = _lib.ptr(z), _lib.stream_ptr()

    def entry(a1=p, a2=p, gs=16, ld=4, assign=p, seeds=p, B=1, N=4, ws=None, nbytes=0, perm=p, swaps=p, nit=p, status=p):
        return lib.fgnn_qapw_2opt_seeded(a1, a2, gs, ld, assign, seeds, None, B, N, -1, ws, nbytes, perm, swaps, nit, status, st)
    big = _lib.FGNN_QAPW_MAX_N + 1
    assert entry(gs=big * big, ld=big, N=big, ws=p, nbytes=1 << 30) == 1 and 'fgnn_qapw_2opt_seeded: at most' in _lib.last_error()
    assert entry(ld=3) == 1 and entry(gs=15) == 1 and entry(B=65536) == 1
    for null in ('a1', 'a2', 'assign', 'seeds', 'perm', 'swaps', 'nit', 'status'):
        assert entry(**{null: None}) == 1, null
    n = 129
    need = lib.fgnn_qapw_2opt_ws_bytes(1, n)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device=DEV)
    at129 = dict(gs=n * n, ld=n, N=n)
    assert entry(**at129, ws=None, nbytes=0) == 1 and 'workspace' in _lib.last_error()
    assert entry(**at129, ws=_lib.ptr(ws), nbytes=need - 1) == 1
    assert entry(**at129, ws=_lib.ptr(ws[4:]), nbytes=need) == 1    # misaligned
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match='two_opt_weighted_seeded: seeds must be'):
        qap.two_opt_weighted_seeded(torch.zeros(1, 4, 4, device=DEV), torch.zeros(1, 4, 4, device=DEV),
                             torch.arange(4, device=DEV)[None], torch.zeros(1, 5, dtype=torch.int32))


# ----------------------------------------------------------------------------------------------------------------- 3. layouts
@pytest.mark.parametrize('case', [(33, 5, False, 'dyadic', 'third'), (65, 5, False, 'dyadic', 'third'), (129, 5, False, 'int', 'third')],
                         ids=_ids)
def test_channel_zero_in_place_and_a_wider_pitch_equal_the_contiguous_run(case):
    N, B = case[:2]
    As, Bs, starts, seeds = S.batch_of(*case)
    refs = S.reference(*case)
    nv, assign, sd = _nv(starts), _rows(starts, N, junk=3), _rows(seeds, N, junk=5)
    flat = [_dense(As, N, 1), _dense(Bs, N, 2)]
    copy = qap.two_opt_weighted_seeded(flat[0], flat[1], assign, sd, nvalid=nv)
    _check(copy, refs, starts, N)
    four = [torch.full((B, 4, N, N), float('nan'), device=DEV) for _ in range(2)]
    for f, x in zip(four, flat):
        f[:, 0] = x
    v1, v2, gs, ld = qap.weighted_views(four[0], four[1])
    assert (gs, ld) == (4 * N * N, N) and v1.data_ptr() == four[0].data_ptr() and v2.data_ptr() == four[1].data_ptr()
    out = qap.two_opt_weighted_seeded(four[0], four[1], assign, sd, nvalid=nv)
    assert all(torch.equal(out[k], copy[k]) for k in out)
    wide = [torch.full((B, N + 3, N + 5), float('nan'), device=DEV) for _ in range(2)]
    for w, x in zip(wide, flat):
        w[:, :N, :N] = x
    views = [w[:, :N, :N] for w in wide]
    assert qap.weighted_views(*views)[2:] == ((N + 3) * (N + 5), N + 5)
    pitched = qap.two_opt_weighted_seeded(views[0], views[1], assign, sd, nvalid=nv)
    assert all(torch.equal(pitched[k], copy[k]) for k in out)
    # entries of `assign` and `seeds` outside the corner do not matter
    plain = qap.two_opt_weighted_seeded(flat[0], flat[1], _rows(starts, N), _rows(seeds, N), nvalid=nv)
    assert all(torch.equal(plain[k], copy[k]) for k in out)


# ------------------------------------------------------------------------------------------------------------ 4. real weights
@pytest.mark.parametrize('N', [50, 130])
def test_real_weights_hold_the_seeds_and_end_in_a_local_optimum_of_the_free_pairs(N):
    B = 3
    gen = PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.1, seed=N, device=DEV)
    f1, f2 = (d['input'] for d in gen.spectral(0, B))
    assert f1.shape == (B, 4, N, N) and f1.dtype == torch.float32
    rng = np.random.default_rng(N)
    masks = [S.seeded_rows(N, 'third' if b % 2 == 0 else 'fourth', b) for b in range(B)]
    truth = [rng.permutation(N) for _ in range(B)]                  # any permutation is a legal set of seed targets
    starts = [S.start_on_free_rows(t, m, None, N + b) for b, (t, m) in enumerate(zip(truth, masks))]
    seeds = [np.where(m, t, -1).astype(np.int64) for t, m in zip(truth, masks)]
    assign, sd = _rows(starts, N), _rows(seeds, N)
    out = qap.two_opt_weighted_seeded(f1, f2, assign, sd)
    again = qap.two_opt_weighted_seeded(f1, f2, assign, sd)
    assert all(torch.equal(out[k], again[k]) for k in out)                                          # two runs, the same bits
    assert torch.equal(out['qap'], qap.objective_weighted(f1, f2, out['perm'], None)['qap'])
    assert torch.equal(out['qap0'], qap.objective_weighted(f1, f2, assign, None)['qap'])
    m = 2 * N + 12
    gamma = m * U / (1 - m * U)
    perm, status, swaps = out['perm'].cpu().numpy(), out['status'].cpu().tolist(), out['swaps'].cpu().tolist()
    for b in range(B):
        A, Bm = f1[b, 0].double().cpu().numpy(), f2[b, 0].double().cpu().numpy()
        p = perm[b].astype(np.int64)
        assert sorted(p.tolist()) == list(range(N))
        assert (p[masks[b]] == seeds[b][masks[b]]).all()
        free_pairs = np.triu(np.ones((N, N), dtype=bool), 1) & ~masks[b][:, None] & ~masks[b][None, :]
        g, s = R.gains(A, Bm[np.ix_(p, p)])
        worst = float((g - gamma * s)[free_pairs].max())
        print('N %d pair %d: status %d swaps %d nit %d qap0 %.6f qap %.6f; largest (gain - bound) of a free pair %.3e' % (
            N, b, status[b], swaps[b], int(out['nit'][b]), float(out['qap0'][b]), float(out['qap'][b]), worst))
        assert status[b] in (0, 1) and (status[b] == 0 or swaps[b] == N * N)
        if status[b] == 0:
            assert worst <= 0.0
    assert bool((out['qap'] >= out['qap0']).all()) and sum(swaps) > 0
