"""GPU: seeds for the QAP solvers -- fgnn_seed_index / fgnn_seed_gather / fgnn_seed_const, fgnn_qapw_faq_seeded through
qap.faq(seeds=), fgnn_qap_2opt_seeded through qap.two_opt(seeds=), fgnn_reveal_seeds and the seeded decode -- against
tests/seeds_ref.py (float64), the host routes and SciPy with partial_match.

Shapes: B <= 16, N <= 80.  (n, m) = (24, 8) and (40, 8) make u = 16 and 32, where 1 / u and every entry of G are exact; (5, 2), (33, 1),
(50, 10), (65, 31) give u = 3, 32, 40, 34: either side of the 32-wide MFMA tile edge, u no multiple of 4, ragged corners inside a
padded N.  The bounds are seeds_ref's: an any-order summation bound over the 2 u + 2 m products of an entry of G."""
import ctypes

import numpy as np
import pytest
import torch

import faq_ref as R
import seeds_ref as S
from graph_neural_net_amd import _lib, evaluation, planted, qap, synthetic
from graph_neural_net_amd.pairgen import PairGenerator

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dense(mats, N, seed):
    x = torch.randn(len(mats), N, N, generator=torch.Generator().manual_seed(seed)) * 5
    x[:, ::2] = float('nan')
    for b, m in enumerate(mats):
        x[b, :len(m), :len(m)] = torch.from_numpy(np.asarray(m)).float()
    return x.to(DEV)


def _nv(mats):
    return torch.tensor([len(m) for m in mats], dtype=torch.int32, device=DEV)


def _bits(mats, N=None):
    N = N or len(mats[0])
    full = np.zeros((len(mats), N, N))
    for b, m in enumerate(mats):
        full[b, :len(m), :len(m)] = m
    return torch.from_numpy(synthetic.pack_adjacency(full).view(np.int32)).to(DEV)


def _seeds(sds, N, junk=True):
    t = torch.full((len(sds), N), -1, dtype=torch.int32)
    for b, sd in enumerate(sds):
        t[b, :len(sd)] = torch.from_numpy(np.asarray(sd)).int()
        if junk and len(sd) < N:
            t[b, len(sd):] = 3                       # rows at or beyond n_b are ignored
    return t.to(DEV)


def _rows(vecs, N, fill=-1):
    t = torch.full((len(vecs), N), fill, dtype=torch.int32)
    for b, v in enumerate(vecs):
        t[b, :len(v)] = torch.from_numpy(np.asarray(v)).int()
    return t.to(DEV)


def _holds(perm, sds):
    for b, sd in enumerate(sds):
        held = np.asarray(sd) >= 0
        got = perm[b, :len(sd)].cpu().numpy()
        assert np.array_equal(got[held], np.asarray(sd)[held]), b


# ---------------------------------------------------------------------------------------------------- 1. exact first iteration
@pytest.mark.parametrize('n', [24, 40])
@pytest.mark.parametrize('kind', ['Regular', 'ErdosRenyi', 'directed'])
def test_first_iteration_equals_scipy_exactly(n, kind):
    make = R.directed_pair if kind == 'directed' else (lambda n, s: R.zero_one_pair(n, s, kind))
    pairs = [make(n, s) for s in range(4)]
    sds = [S.seed_vector(n, 8, s) for s in range(4)]
    want = [S.scipy_faq(A, B, sd, maxiter=1) for (A, B), sd in zip(pairs, sds)]
    As, Bs = [p[0] for p in pairs], [p[1] for p in pairs]
    outs = {'weighted': qap.faq(_dense(As, n, 1), _dense(Bs, n, 2), weighted=True, maxiter=1, seeds=_seeds(sds, n)),
            'ragged': qap.faq(_dense(As, 64, 3), _dense(Bs, 64, 4), nvalid=_nv(As), weighted=True, maxiter=1, seeds=_seeds(sds, 64)),
            'bits': qap.faq(_bits(As), _bits(Bs), maxiter=1, seeds=_seeds(sds, n))}
    for name, out in outs.items():
        assert set(out) == {'perm', 'qap', 'acc', 'nit', 'status', 'seeded'} and all(t.is_cuda for t in out.values())
        assert out['seeded'].dtype == torch.int64 and out['seeded'].cpu().tolist() == [8] * 4
        for b, (col, fun, nit) in enumerate(want):
            assert out['perm'][b, :n].cpu().tolist() == col.tolist(), (name, b)
            assert float(out['qap'][b]) == fun
        assert out['nit'].cpu().tolist() == [1] * 4
        assert bool((out['perm'][:, n:] == -1).all())
        _holds(out['perm'], sds)


# ------------------------------------------------------------------------------------------- 2. one round from a known P
CASES = ((5, 2), (33, 1), (50, 10), (65, 31))
# u = 132 > FQ_COLS = 128: the seeded gradient and step across the second column block.  (n, m, the pair's generator seed): the cap
# tol < 1e-3 |best| at the end of the test binds at this size (the tolerance grows with gamma_(3 u)), and these seeds are the ones
# of 0 .. 119 that keep the most room under it, evaluated in float64 with P1 from the host update: 0.945 / 0.960 (sym / dir) of
# the cap for (136, 4, 20), 0.959 / 0.983 for (133, 1, 89)
WIDE = ((136, 4, 20), (133, 1, 89))


@pytest.mark.parametrize('symmetric', [True, False], ids=['sym', 'dir'])
def test_one_round_from_a_known_P(symmetric):
    for N, cases in ((72, [(n, m, b) for b, (n, m) in enumerate(CASES)]), (136, WIDE)):
        _one_round_from_a_known_P(N, cases, symmetric)


def _one_round_from_a_known_P(N, cases, symmetric):
    pairs = [R.real_pair(n, s, symmetric) for n, m, s in cases]
    As, Bs = [p[0] for p in pairs], [p[1] for p in pairs]
    sds = [S.seed_vector(n, m, s) for n, m, s in cases]
    starts, P0 = [], torch.full((len(cases), N, N), float('nan'))
    for b, (n, m, s) in enumerate(cases):
        free_a, free_b, _, _ = S.lists_of(sds[b], n)
        starts.append(R.interior_start(n - m, s))
        P0[b][np.ix_(free_a, free_b)] = torch.from_numpy(starts[b]).float()
    out = qap.faq(_dense(As, N, 5), _dense(Bs, N, 6), nvalid=_nv(As), P0=P0.to(DEV), weighted=True, maxiter=1, return_P=True,
                  seeds=_seeds(sds, N))
    assert out['nit'].cpu().tolist() == [1] * len(cases) and out['seeded'].cpu().tolist() == [m for _, m, _ in cases]
    _holds(out['perm'], sds)
    for b, (n, m, _) in enumerate(cases):
        u = n - m
        A22, B22, C, Cabs = S.blocks(As[b], Bs[b], sds[b])
        P = starts[b]
        full = out['P'][b].cpu().numpy()
        assert np.isfinite(full).all() and not full[u:].any() and not full[:, u:].any()
        P1 = full[:u, :u].astype(np.float64)
        G, d = S.gradient(A22, B22, C, P), S.gradient_bound(A22, B22, Cabs, P, m)
        q_host = R.direction(G)
        D = P1 - P
        q = D.argmax(1)
        if not ((D[np.arange(u), q] > 0).all() and sorted(q.tolist()) == list(range(u))):        # x = 1: P' = P says nothing about q
            assert np.array_equal(P1, P)
            q = q_host
        rows = np.arange(u)
        slack = 2 * d.max(1).sum()
        print('pair %d u %d m %d: <G,Q_dev> %.9g <G,Q_host> %.9g slack %.3g' % (b, u, m, G[rows, q].sum(), G[rows, q_host].sum(), slack))
        assert G[rows, q].sum() >= G[rows, q_host].sum() - slack, (b, n, m)
        Q = np.eye(u)[q]
        Rm = P - Q
        if np.abs(Rm).max() > 0:
            at = np.unravel_index(np.abs(Rm).argmax(), Rm.shape)
            x = (P1 - Q)[at] / Rm[at]
            assert -4 * R.U <= x <= 1 + 4 * R.U and np.abs(P1 - (Q + x * Rm)).max() <= 4 * R.U, (b, x)
        best, x_best = S.segment_maximum(A22, B22, C, P, q)
        tol = S.line_search_tolerance(A22, B22, C, Cabs, P, q, P1, m)
        got = S.objective(A22, B22, C, P1)
        print('          f(P\') %.12g max on the segment %.12g (x %.6f) tolerance %.3g' % (got, best, x_best, tol))
        assert abs(got - best) <= tol, (b, n, m)
        assert tol < 1e-3 * abs(best)


# ----------------------------------------------------------------------------------------------------------------- 3. full runs
@pytest.mark.parametrize('kind', ['int', 'dyadic'])
@pytest.mark.parametrize('symmetric', [True, False], ids=['sym', 'dir'])
def test_lock_step_with_the_host_route(symmetric, kind):
    """integer / dyadic weights from a permutation that holds the seeds: G, C, a and b are exact, and while the host's iterates are
    fp32 numbers the device follows it bit for bit.  m_b is mixed within the batch, 0 and n_b included."""
    N, shape = 64, ((50, 10), (33, 0), (32, 32), (16, 5), (5, 2), (40, 1), (24, 23))
    pairs = [R.exact_pair(n, b, symmetric, kind) for b, (n, m) in enumerate(shape)]
    As, Bs = [p[0] for p in pairs], [p[1] for p in pairs]
    sds = [S.seed_vector(n, m, b) for b, (n, m) in enumerate(shape)]
    P0 = _rows([S.completed(sd, b) for b, sd in enumerate(sds)], N)
    x1, x2, nv, seeds = _dense(As, N, 8), _dense(Bs, N, 9), _nv(As), _seeds(sds, N)
    compared, alive = 0, list(range(len(shape)))
    for k in range(1, 5):
        host = qap.faq(x1.cpu().double(), x2.cpu().double(), nvalid=nv.cpu(), P0=P0.cpu(), weighted=True, maxiter=k, return_P=True,
                       seeds=seeds.cpu())
        alive = [b for b in alive if torch.equal(host['P'][b].float().double(), host['P'][b])]
        dev = qap.faq(x1, x2, nvalid=nv, P0=P0, weighted=True, maxiter=k, return_P=True, seeds=seeds)
        _holds(dev['perm'], sds)
        assert dev['seeded'].cpu().tolist() == host['seeded'].tolist() == [m for _, m in shape]
        for b in alive:
            assert dev['perm'][b].cpu().tolist() == host['perm'][b].tolist(), (k, b)
            assert int(dev['nit'][b]) == int(host['nit'][b]) and int(dev['status'][b]) == int(host['status'][b]), (k, b)
            assert torch.equal(dev['P'][b].cpu().double(), host['P'][b]), (k, b)
            assert float(dev['qap'][b]) == float(host['qap'][b])
            compared += 1
    print('lock-step comparisons: %d' % compared)
    assert compared >= 10
    assert int(dev['status'][2]) == 0 and int(dev['nit'][2]) == 0                 # m_b = n_b: perm = seeds


def test_statuses_on_the_device():
    n, N = 12, 16
    A, B = R.zero_one_pair(n, 0)
    good = S.seed_vector(n, 4, 0)
    rows = np.flatnonzero(good >= 0)
    shared, outside = good.copy(), good.copy()
    shared[rows[1]] = shared[rows[0]]
    outside[rows[0]] = n
    sds = [good, shared, outside, np.random.default_rng(0).permutation(n)]
    x1, x2, nv = _bits([A] * 4, N), _bits([B] * 4, N), torch.full((4,), n, dtype=torch.int32, device=DEV)
    dev = qap.faq(x1, x2, nvalid=nv, seeds=_seeds(sds, N))
    host = qap.faq(x1.cpu(), x2.cpu(), nvalid=nv.cpu(), seeds=_seeds(sds, N).cpu())
    for k in ('perm', 'nit', 'status', 'qap', 'seeded', 'acc'):
        assert dev[k].cpu().tolist() == host[k].tolist(), k
    assert dev['status'].cpu().tolist()[1:] == [2, 2, 0]
    p = S.completed(good, 1)
    other = int(np.flatnonzero(good < 0)[0])
    p[[rows[0], other]] = p[[other, rows[0]]]
    out = qap.faq(x1[:1], x2[:1], nvalid=nv[:1], P0=_rows([p], N), seeds=_seeds([good], N))
    assert out['status'].cpu().tolist() == [2] and out['nit'].cpu().tolist() == [0] and out['perm'][0, :n].cpu().tolist() == p.tolist()


# ------------------------------------------------------------------------------------------------- 4. the set-up kernels
def _call_index(seeds, nv):
    ix = qap.seed_index_device(seeds, nv)
    return {k: v.cpu().numpy() for k, v in ix.items()}


def test_index_gather_and_const_kernels():
    N, shape = 80, ((65, 31), (50, 10), (33, 0), (32, 32), (5, 2), (0, 0), (80, 79))
    rng = np.random.default_rng(3)
    sds = [S.seed_vector(n, m, b) for b, (n, m) in enumerate(shape)]
    bad = [S.seed_vector(40, 6, 0), S.seed_vector(40, 6, 1)]
    r0, r1 = np.flatnonzero(bad[0] >= 0)[:2]
    bad[0][r1] = bad[0][r0]                               # shared target
    bad[1][np.flatnonzero(bad[1] >= 0)[0]] = 40           # beyond n_b
    allsd = sds + bad
    sizes = [n for n, _ in shape] + [40, 40]
    seeds = _seeds(allsd, N)
    nv = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    ix = _call_index(seeds, nv)
    assert ix['valid'].tolist() == [1] * len(shape) + [0, 0]
    for b, (n, m) in enumerate(shape):
        free_a, free_b, seed_a, seed_b = S.lists_of(allsd[b], n)
        assert ix['nfree'][b] == n - m and ix['nseed'][b] == m
        for name, want in (('free_a', free_a), ('free_b', free_b), ('seed_a', seed_a), ('seed_b', seed_b)):
            assert ix[name][b].tolist() == want.tolist() + [-1] * (N - len(want)), (name, b)
    for b in (len(shape), len(shape) + 1):
        assert ix['nseed'][b] == 6 and ix['nfree'][b] == 34
        assert all((ix[name][b] == -1).all() for name in ('free_a', 'free_b', 'seed_a', 'seed_b'))
    again = _call_index(seeds, nv)
    assert all(np.array_equal(ix[k], again[k]) for k in ix)
    # gather: bit-exact against fancy indexing, on a pitched view, NaN outside the corners never read into the block
    B = len(shape)
    big = torch.randn(B, 2, N, N + 8, generator=torch.Generator().manual_seed(1)).to(DEV)
    x = big[:, 1, :, :N]
    dix = qap.seed_index_device(seeds[:B], nv[:B])
    got = qap.seed_gather_device(x, dix['free_a'], dix['free_b'], dix['nfree']).cpu().numpy()
    xs = x.cpu().numpy()
    for b, (n, m) in enumerate(shape):
        free_a, free_b, _, _ = S.lists_of(allsd[b], n)
        want = np.zeros((N, N), dtype=np.float32)
        want[:n - m, :n - m] = xs[b][np.ix_(free_a, free_b)]
        assert np.array_equal(got[b].view(np.uint32), want.view(np.uint32)), b
    # const: exact on integer data, against float64
    A = rng.integers(-3, 4, size=(B, N, N)).astype(np.float32)
    Bm = rng.integers(-3, 4, size=(B, N, N)).astype(np.float32)
    a, bm = torch.from_numpy(A).to(DEV), torch.from_numpy(Bm).to(DEV)
    C = torch.full((B, N, N), float('nan'), device=DEV)
    _lib.call('fgnn_seed_const', _lib.ptr(a), _lib.ptr(bm), N * N, N, _lib.ptr(dix['free_a']), _lib.ptr(dix['free_b']),
              _lib.ptr(dix['seed_a']), _lib.ptr(dix['seed_b']), _lib.ptr(dix['nfree']), _lib.ptr(dix['nseed']), B, N, _lib.ptr(C),
              _lib.stream_ptr())
    C = C.cpu().numpy()
    for b, (n, m) in enumerate(shape):
        _, _, want, _ = S.blocks(A[b, :n, :n].astype(np.float64), Bm[b, :n, :n].astype(np.float64), allsd[b])
        full = np.zeros((N, N))
        full[:n - m, :n - m] = want
        assert np.array_equal(C[b].astype(np.float64), full), b


# ------------------------------------------------------------------------------------------------------------- 5. 2-opt seeded
@pytest.mark.parametrize('n', [7, 33, 64])
def test_two_opt_seeded_equals_host_and_scipy(n):
    ms = (0, 3, n - 1)
    pairs = [R.zero_one_pair(n, s, 'ErdosRenyi' if s == 1 else 'Regular') for s in range(2)] + [R.directed_pair(n, 0)]
    As, Bs = [p[0] for p in pairs], [p[1] for p in pairs]
    sds = [S.seed_vector(n, m, 30 + b) for b, m in enumerate(ms)]
    starts = [S.completed(sd, 40 + b) for b, sd in enumerate(sds)]
    for N in (n, n + 5):
        x1, x2, nv = _bits(As, N), _bits(Bs, N), torch.full((3,), n, dtype=torch.int32, device=DEV)
        dev = qap.two_opt(x1, x2, _rows(starts, N), nvalid=nv, seeds=_seeds(sds, N))
        host = qap.two_opt(x1.cpu(), x2.cpu(), _rows(starts, N).cpu(), nvalid=nv.cpu(), seeds=_seeds(sds, N).cpu())
        for k in ('perm', 'qap', 'qap0', 'acc', 'swaps', 'nit', 'status'):
            assert dev[k].cpu().tolist() == host[k].tolist(), (k, N)
        for b in range(3):
            col, fun, nit = S.scipy_2opt(As[b], Bs[b], sds[b], starts[b])
            assert dev['perm'][b, :n].cpu().tolist() == col.tolist() and int(dev['qap'][b]) == fun and int(dev['nit'][b]) == nit, b
        _holds(dev['perm'], sds)
    assert int(dev['swaps'][0]) > 0 and int(dev['swaps'][2]) == 0 and int(dev['nit'][2]) == 1
    # all -1 seeds: the unseeded search, bit for bit
    free = qap.two_opt(x1, x2, _rows(starts, N), nvalid=nv, seeds=torch.full((3, N), -1, dtype=torch.int32, device=DEV))
    plain = qap.two_opt(x1, x2, _rows(starts, N), nvalid=nv)
    assert set(free) == set(plain) and all(torch.equal(free[k], plain[k]) for k in plain)
    # a start against a seed: status 2
    p = starts[1].copy()
    row, other = int(np.flatnonzero(sds[1] >= 0)[0]), int(np.flatnonzero(sds[1] < 0)[0])
    p[[row, other]] = p[[other, row]]
    out = qap.two_opt(x1[1:2], x2[1:2], _rows([p], N), nvalid=nv[1:2], seeds=_seeds(sds[1:2], N))
    assert out['status'].cpu().tolist() == [2] and out['qap'].cpu().tolist() == [-1] and out['nit'].cpu().tolist() == [0]
    assert out['perm'][0, :n].cpu().tolist() == p.tolist()


def _planted_pair(n, b):
    """-> (A, B, q): pair b of the batches below relabelled by a known q, B[q(i), q(k)] = (the noisy copy of A)[i, k]; b = 2 is
    directed with loops"""
    rng = np.random.default_rng(500 * n + b)
    if b < 2:
        A, M = R.zero_one_pair(n, b, 'ErdosRenyi' if b == 1 else 'Regular')
    else:
        A = (rng.random((n, n)) < 0.3).astype(np.float64)
        M = np.where(rng.random((n, n)) < 0.1, (rng.random((n, n)) < 0.3).astype(np.float64), A)
    q = rng.permutation(n)
    B = np.zeros_like(A)
    B[np.ix_(q, q)] = M
    return A, B, q


@pytest.mark.parametrize('n', [65, 129])
def test_two_opt_seeded_across_waves_equals_host(n):
    """n > 64: the rank table's prefix crosses waves (and, with N > 128, the NW = 8 form; n = 65 runs NW = 4).  m = 0, 3, n - 1 seeds
    on the planted matching; seeded and free rows at index >= 64, and at n = 129 at index 128: pair 0 has every row free, pair 1 seeds
    rows 2, 70 (n = 65: 40) and n - 1, pair 2 leaves only row n - 1 free.  The starts are the planted matching with three
    transpositions of free rows (none in pair 2), so the host route ends after a few rounds.  Host route only: SciPy is compared
    at the sizes of the test above."""
    trio = [_planted_pair(n, b) for b in range(3)]
    As, Bs = [t[0] for t in trio], [t[1] for t in trio]
    held = ([], [2, 70 if n > 70 else 40, n - 1], list(range(n - 1)))
    sds, starts = [], []
    for (_, _, q), rows in zip(trio, held):
        sd = np.full(n, -1, dtype=np.int64)
        sd[rows] = q[rows]
        fr = np.flatnonzero(sd < 0)
        p = q.copy()
        if len(fr) > 1:
            for i, j in ((fr[0], fr[-1]), (fr[1], fr[len(fr) // 2]), (fr[5], fr[6])):
                p[[i, j]] = p[[j, i]]
        sds.append(sd)
        starts.append(p)
    assert sds[0][n - 1] < 0 and sds[1][n - 1] >= 0 and sds[2][n - 1] < 0 and sds[1][n - 2] < 0
    for N in (n, n + 5):
        x1, x2, nv = _bits(As, N), _bits(Bs, N), torch.full((3,), n, dtype=torch.int32, device=DEV)
        dev = qap.two_opt(x1, x2, _rows(starts, N), nvalid=nv, seeds=_seeds(sds, N))
        host = qap.two_opt(x1.cpu(), x2.cpu(), _rows(starts, N).cpu(), nvalid=nv.cpu(), seeds=_seeds(sds, N).cpu())
        for k in ('perm', 'qap', 'qap0', 'acc', 'swaps', 'nit', 'status'):
            assert dev[k].cpu().tolist() == host[k].tolist(), (k, N)
        _holds(dev['perm'], sds)
        assert dev['status'].cpu().tolist() == [0] * 3
        assert int(dev['swaps'][0]) > 0 and int(dev['swaps'][1]) > 0 and int(dev['swaps'][2]) == 0 and int(dev['nit'][2]) == 1
        # all -1 seeds: the unseeded search, bit for bit
        free = qap.two_opt(x1, x2, _rows(starts, N), nvalid=nv, seeds=torch.full((3, N), -1, dtype=torch.int32, device=DEV))
        plain = qap.two_opt(x1, x2, _rows(starts, N), nvalid=nv)
        assert set(free) == set(plain) and all(torch.equal(free[k], plain[k]) for k in plain)
        assert int(plain['swaps'].max()) > 0


# --------------------------------------------------------------------------------------------- 7. the unseeded path, bit for bit
def _free_seeds_are_the_unseeded_chain(N, sizes):
    """plain, seeds=None and all -1 seeds: equal bytes on every key -> (x1, x2, nv) of the batch"""
    pairs = [R.real_pair(n, 40 + b) for b, n in enumerate(sizes)]
    As, Bs = [p[0] for p in pairs], [p[1] for p in pairs]
    x1, x2, nv = _dense(As, N, 10), _dense(Bs, N, 11), _nv(As)
    free = torch.full((len(sizes), N), -1, dtype=torch.int32, device=DEV)
    plain = qap.faq(x1, x2, nvalid=nv, weighted=True, return_P=True)
    none = qap.faq(x1, x2, nvalid=nv, weighted=True, return_P=True, seeds=None)
    seeded = qap.faq(x1, x2, nvalid=nv, weighted=True, return_P=True, seeds=free)
    again = qap.faq(x1, x2, nvalid=nv, weighted=True, return_P=True, seeds=free)
    assert set(plain) == set(none) == {'perm', 'qap', 'acc', 'nit', 'status', 'P'}
    for k in plain:
        assert torch.equal(plain[k], none[k]), k
        assert torch.equal(plain[k], seeded[k]), k
    assert all(torch.equal(seeded[k], again[k]) for k in seeded)
    assert int(plain['nit'].max()) > 1 and seeded['seeded'].cpu().tolist() == [0] * len(sizes)
    return x1, x2, nv


def test_free_seeds_are_the_unseeded_chain_bit_for_bit():
    _free_seeds_are_the_unseeded_chain(136, (136, 130, 129))          # n > FQ_COLS = 128: the second column block
    N, sizes = 64, (50, 33, 32, 16, 5, 2, 1)
    x1, x2, nv = _free_seeds_are_the_unseeded_chain(N, sizes)
    # with seeds: run to run, and a pair's result does not depend on the batch around it
    sds = [S.seed_vector(n, n // 4, b) for b, n in enumerate(sizes)]
    seeds = _seeds(sds, N)
    out = qap.faq(x1, x2, nvalid=nv, weighted=True, return_P=True, seeds=seeds)
    again = qap.faq(x1, x2, nvalid=nv, weighted=True, return_P=True, seeds=seeds)
    _holds(out['perm'], sds)
    for b in range(len(sizes)):
        alone = qap.faq(x1[b:b + 1], x2[b:b + 1], nvalid=nv[b:b + 1], weighted=True, return_P=True, seeds=seeds[b:b + 1])
        for k in out:
            assert torch.equal(out[k], again[k]) and torch.equal(out[k][b:b + 1], alone[k]), (k, b)


def test_seeded_chain_is_capturable():
    n = 24
    pairs = [R.zero_one_pair(n, s) for s in range(2)]
    As, Bs = [p[0] for p in pairs], [p[1] for p in pairs]
    x1, x2 = _dense(As, n, 1), _dense(Bs, n, 2)
    seeds = _seeds([S.seed_vector(n, 8, s) for s in range(2)], n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = qap.faq_weighted(x1, x2, None, seeds=seeds, maxiter=3)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = qap.faq_weighted(x1, x2, None, seeds=seeds, maxiter=3)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(eager[k], cap[k]) for k in eager)


# ------------------------------------------------------------------------------------------------------------- 8. reveal_seeds
def test_reveal_seeds():
    N, B = 48, 16
    nv = torch.tensor([48, 30, 5, 0, 1, 48, 17, 33] * 2, dtype=torch.int32, device=DEV)
    labels = planted.planted_permutation(5, N, first=0, count=B, nvalid=nv)
    for count in (0, 8, 100):
        sd = planted.reveal_seeds(labels, nv, count, seed=11)
        assert sd.dtype == torch.int32 and tuple(sd.shape) == (B, N)
        held = sd >= 0
        assert held.sum(1).cpu().tolist() == [min(count, int(n)) for n in nv.cpu()]
        assert torch.equal(sd[held], labels[held]) and bool((sd[~held] == -1).all())
        assert torch.equal(sd, planted.reveal_seeds(labels, nv, count, seed=11))
    sd = planted.reveal_seeds(labels, nv, 8, seed=11)
    # (seed, pair index) only: a window of the batch, and index=, give the same rows
    part = planted.reveal_seeds(labels[4:9], nv[4:9], 8, seed=11, first=4)
    assert torch.equal(part, sd[4:9])
    idx = torch.tensor([7, 0, 7], dtype=torch.int64)
    pick = planted.reveal_seeds(labels[idx.to(DEV)], nv[idx.to(DEV)], 8, seed=11, index=idx)
    assert torch.equal(pick, sd[idx.to(DEV)])
    other = planted.reveal_seeds(labels, nv, 8, seed=12)
    assert not torch.equal(other, sd)
    assert not torch.equal((sd[0] >= 0), (sd[5] >= 0))                           # two pairs of 48: different rows
    # every row is revealed about equally often over many pairs (8 of 48: p = 1/6; 600 pairs, sd of a count ~ 9.1)
    lab = torch.arange(N, dtype=torch.int32, device=DEV).expand(600, N).contiguous()
    hits = (planted.reveal_seeds(lab, None, 8, seed=3) >= 0).sum(0).cpu().numpy()
    assert hits.sum() == 4800 and np.abs(hits - 100).max() < 46                   # 5 sd


# ------------------------------------------------------------------------------------------------------------ 9. decode chain
def test_decode_chain_keeps_the_seeds():
    B, N = 4, 24
    sizes = (24, 17, 9, 24)
    pairs = [R.zero_one_pair(n, s) for s, n in enumerate(sizes)]
    As, Bs = [p[0] for p in pairs], [p[1] for p in pairs]
    b1, b2, nv = _bits(As, N), _bits(Bs, N), _nv(As)
    scores = torch.randn(B, N, N, generator=torch.Generator().manual_seed(4)).to(DEV)
    sds = [S.seed_vector(n, m, b, truth=np.arange(n)) for b, (n, m) in enumerate(zip(sizes, (6, 4, 9, 0)))]
    seeds = _seeds(sds, N)
    for faq in ({'P0': 'scores'}, {'P0': 'barycenter'}):
        out = evaluation.decode_scores(scores, b1, b2, nvalid=nv, faq=faq, two_opt=True, seeds=seeds)
        assert out['seeded'].cpu().tolist() == [6, 4, 9, 0]
        _holds(out['faq_perm'], sds)
        _holds(out['perm'], sds)
        assert out['status'].cpu().tolist() == [0] * B and bool((out['faq_status'] != 2).all())
        for b, n in enumerate(sizes):
            assert sorted(out['perm'][b, :n].cpu().tolist()) == list(range(n))
        want = qap.objective_bits(b1, b2, out['perm'], nv)['qap']
        assert torch.equal(out['refined'].to(torch.int64), want)
    assert out['faq_nit'].cpu().tolist()[2] == 0                                    # u_b = 0
    for kw in ({'two_opt': True}, {'faq': True, 'refine': 2}, {'refine': 1}):
        with pytest.raises(ValueError, match='seeds'):
            evaluation.decode_scores(scores, b1, b2, nvalid=nv, seeds=seeds, **kw)
    with pytest.raises(ValueError, match='seeds'):
        evaluation.decode_scores(scores, b1, b2, nvalid=nv, faq=True, seeds=seeds[:, :-1])
    plain = evaluation.decode_scores(scores, b1, b2, nvalid=nv, faq={'P0': 'scores'}, two_opt=True)
    none = evaluation.decode_scores(scores, b1, b2, nvalid=nv, faq={'P0': 'scores'}, two_opt=True, seeds=None)
    assert set(plain) == set(none) and 'seeded' not in plain
    for k, v in plain.items():
        if torch.is_tensor(v):
            assert torch.equal(v, none[k]), k


# ---------------------------------------------------------------------------------------------------------------- 10. recovery
RECOVERY_SEEDS = 8


def test_recovery_with_seeds_matches_scipy():
    """16 relabelled generator pairs (Regular of degree 10 on 48 vertices, ErdosRenyi noise 0.1), 8 seeds revealed, FAQ from the
    barycenter: the device recovers at least as many free vertices as float64 SciPy on the same pairs and seeds, less 2 % of them."""
    B, N = 16, 48
    gen = PairGenerator(N, 'Regular', 'ErdosRenyi', edge_density=0.21, noise=0.1, seed=17, device=DEV)     # degree int(0.21 * 48) = 10
    b1, b2, nv, labels = gen.bits(0, B, permute=True)
    assert nv is None
    seeds = planted.reveal_seeds(labels, None, RECOVERY_SEEDS, seed=17)
    out = qap.faq(b1, b2, labels=labels, seeds=seeds)
    A = np.unpackbits(b1.cpu().numpy().view(np.uint8), axis=-1, bitorder='little')[:, :, :N].astype(np.float64)
    Bm = np.unpackbits(b2.cpu().numpy().view(np.uint8), axis=-1, bitorder='little')[:, :, :N].astype(np.float64)
    lab, sd = labels.cpu().numpy(), seeds.cpu().numpy()
    assert int(A[0].sum(1)[0]) == 10
    free = sd < 0
    total = int(free.sum())
    assert total == B * (N - RECOVERY_SEEDS)
    ref = sum(int(((S.scipy_faq(A[b], Bm[b], sd[b])[0] == lab[b]) & free[b]).sum()) for b in range(B))
    got = int(((out['perm'].cpu().numpy() == lab) & free).sum())
    print('free vertices recovered: SciPy %d / %d (%.3f), device %d (%.3f)' % (ref, total, ref / total, got, got / total))
    assert ref >= 0.9 * total
    assert got >= ref - 0.02 * total
    _holds(out['perm'], list(sd))
    assert int(out['acc'].sum()) == got + B * RECOVERY_SEEDS
