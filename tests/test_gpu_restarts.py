"""GPU: random restarts for FAQ -- fgnn_faq_restart_starts through qap.random_starts against tests/restarts_ref.py (float64),
fgnn_qap_best_of against its rule on hand-made results, qap.faq(restarts=) against single-start calls, and the decode's keys.

Starts: (B, N, R) = (3, 16, 1); (4, 50, 3) with corners 0, 1, 50, 37; (2, 200, 2); (1, 256, 2) -- one and several column slices
(n <= 64: 16 slices of a column, 200 and 256: 4), the corner edge, the padded N -- a seeded case on nfree, and a float base.
The bounds: K's own tolerance on its sums is 1e-3, the halving with an exactly stochastic base brings it to 5e-4, fp32 rounding of
n <= 256 terms of about 1 / n adds about 256 * 2^-25 / 1 = 1.5e-5 at the most: 1e-3 holds.  Against the restatement every entry
may differ by one fp32 ulp: the fp64 sums differ in order only (about 1e-13 relative), so nothing but a rounding boundary of the
final conversion can be crossed."""
import numpy as np
import pytest
import torch

import faq_ref as F
import restarts_ref as RR
from graph_neural_net_amd import _lib, qap, synthetic
from graph_neural_net_amd.evaluation import QapMeter, decode_scores
from graph_neural_net_amd.pairgen import PairGenerator

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = 11


def _ulps(got, want64):
    """got fp32, want float64 -> the largest distance in fp32 ulps between got and float32(want)"""
    want = want64.astype(np.float32)
    assert ((got == 0) == (want == 0)).all()
    return int(np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max()) if got.size else 0


def _check_starts(out, sizes, pidx, base=None):
    B, R, N, _ = out.shape
    got = out.cpu().numpy()
    for b, n in enumerate(sizes):
        bb = base[b, :n, :n].double().cpu().numpy() if base is not None else None
        want = RR.starts(SEED, pidx[b], R, n, N, bb)
        assert _ulps(got[b], want) <= 1, (b, n)
        assert not got[b, :, n:].any() and not got[b, :, :, n:].any()
        if n > 0:
            first = base[b, :n, :n].cpu().numpy() if base is not None else np.full((n, n), np.float32(1.0 / n), dtype=np.float32)
            assert np.array_equal(got[b, 0, :n, :n], first)
            sums = got[b, :, :n, :n].astype(np.float64)
            assert np.abs(sums.sum(1) - 1).max() < 1e-3 and np.abs(sums.sum(2) - 1).max() < 1e-3, (b, n)
        if n == 1:
            assert (got[b, :, 0, 0] == 1).all()


# ------------------------------------------------------------------------------------------------------------------ the starts
@pytest.mark.parametrize('B,N,R,sizes', [(3, 16, 1, None), (4, 50, 3, (0, 1, 50, 37)), (2, 200, 2, None), (1, 256, 2, None)])
def test_starts_equal_the_restatement(B, N, R, sizes):
    nv = torch.tensor(sizes, dtype=torch.int32, device=DEV) if sizes else None
    out = qap.random_starts(nv if sizes else B, N, R, seed=SEED, device=DEV)
    assert out.shape == (B, R, N, N) and out.dtype == torch.float32 and out.is_cuda
    _check_starts(out, sizes or (N,) * B, list(range(B)))
    again = qap.random_starts(nv if sizes else B, N, R, seed=SEED, device=DEV)
    assert torch.equal(out, again)                                  # two runs: identical bytes
    if R > 1:
        other = qap.random_starts(nv if sizes else B, N, R, seed=SEED + 1, device=DEV)
        assert torch.equal(other[:, 0], out[:, 0]) and not torch.equal(other[:, 1:], out[:, 1:])


def test_a_float_base_and_pair_indices():
    sizes, N, R = (37, 16, 5), 40, 3
    base = torch.full((3, N, N), float('nan'))
    for b, n in enumerate(sizes):
        base[b, :n, :n] = torch.from_numpy(F.interior_start(n, b)).float()
    base = base.to(DEV)
    nv = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    idx = torch.tensor([5, 2 ** 40, 0], device=DEV)
    out = qap.random_starts(nv, N, R, seed=SEED, base=base, pair_index=idx)
    _check_starts(out, sizes, idx.tolist(), base)


def test_a_start_depends_on_seed_pair_restart_and_corner_only():
    nv4 = torch.tensor([50, 37, 50, 16], dtype=torch.int32, device=DEV)
    idx4 = torch.tensor([3, 1, 7, 0], device=DEV)
    a = qap.random_starts(nv4, 50, 4, seed=SEED, pair_index=idx4)
    wide = qap.random_starts(nv4, 64, 2, seed=SEED, pair_index=idx4)          # the same corners inside N = 64, fewer restarts
    assert torch.equal(wide[:, :, :50, :50], a[:, :2]) and not wide[:, :, 50:].any() and not wide[:, :, :, 50:].any()
    for b in range(4):                                                          # B = 1 against B = 4
        one = qap.random_starts(nv4[b:b + 1], 50, 4, seed=SEED, pair_index=idx4[b:b + 1])
        assert torch.equal(one[0], a[b]), b
    # the batch position is the pair index when none is given
    plain = qap.random_starts(nv4, 50, 4, seed=SEED)
    assert torch.equal(plain, qap.random_starts(nv4, 50, 4, seed=SEED, pair_index=torch.arange(4, device=DEV)))
    assert torch.equal(plain[1], a[1]) and not torch.equal(plain[0, 1:], a[0, 1:])      # (pair 1 sits at position 1 in both)


def test_starts_on_the_free_block_of_seeds():
    n, N, R = 20, 24, 3
    seeds = torch.full((2, N), -1, dtype=torch.int32, device=DEV)
    seeds[0, 3], seeds[0, 11], seeds[1, 0] = 7, 0, 19
    nv = torch.tensor([n, n], dtype=torch.int32, device=DEV)
    ix = qap.seed_index_device(seeds, nv)
    assert ix['nfree'].tolist() == [18, 19]
    out = qap.random_starts(ix['nfree'], N, R, seed=SEED)
    _check_starts(out, (18, 19), [0, 1])


def test_limits():
    for kw in ({'B': 1, 'N': 257, 'R': 2}, {'B': 1, 'N': 8, 'R': 65}, {'B': 1024, 'N': 2, 'R': 64}):
        starts = torch.empty(1, device=DEV)
        with pytest.raises(RuntimeError, match='fgnn_faq_restart_starts'):
            _lib.call('fgnn_faq_restart_starts', None, None, None, 0, kw['B'], kw['N'], kw['R'], _lib.ptr(starts), _lib.stream_ptr())


# ------------------------------------------------------------------------------------------------------------------- the choice
@pytest.mark.parametrize('dtype', [torch.int64, torch.float32])
def test_best_of_on_hand_made_results(dtype):
    nan = float('nan')
    R, N = 4, 70
    cases = [([3, 7, 7, 5], [0, 1, 0, 0], None),                # a tie: the smaller k
             ([9, 8, 1, 1], [2, 2, 2, 2], None),                # no candidate: restart 0 as it is
             ([1, 2, 3, 4], [0, 0, 1, 1], None),                # a winner in the last slot
             ([9, 8, 7, 6], [2, 0, 0, 0], None),                # status 2 holds the largest objective
             ([9, 8, 7, 6], [0, 0, 0, 0], [2, 2, 0, 0]),        # a veto
             ([-5, -3, -4, -3], [1, 1, 1, 1], None)]
    if dtype == torch.float32:
        cases += [([nan, 2.5, nan, 2.5], [0, 0, 0, 0], None), ([nan, nan, nan, nan], [0, 1, 0, 1], None),
                  ([0.5, nan, float('inf'), 1.0], [0, 0, 0, 0], None)]
    B = len(cases)
    q = torch.tensor([c[0] for c in cases], dtype=dtype, device=DEV).view(-1)
    status = torch.tensor([c[1] for c in cases], dtype=torch.int32, device=DEV).view(-1)
    veto = torch.tensor([c[2] or [0] * R for c in cases], dtype=torch.int32, device=DEV).view(-1)
    nit = torch.arange(B * R, dtype=torch.int32, device=DEV) + 100
    perm = torch.randint(-1, N, (B * R, N), dtype=torch.int32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    for v in (veto, None):
        out = qap.best_of_device(q, status, nit, perm, R, v)
        for b, (qs, st, vt) in enumerate(cases):
            w = RR.best_of(qs, st, vt if v is not None else None)
            assert int(out['restart'][b]) == w, (b, v is None)
            assert torch.equal(out['perm'][b], perm[b * R + w]) and int(out['nit'][b]) == 100 + b * R + w and int(out['status'][b]) == st[w]
            got, want = out['qap'][b:b + 1], q[b * R + w:b * R + w + 1]
            assert got.dtype == dtype and torch.equal(got.view(torch.int32 if dtype == torch.float32 else dtype),
                                                      want.view(torch.int32 if dtype == torch.float32 else dtype))
    assert out['restart'].dtype == torch.int32


# -------------------------------------------------------------------------------------------------------- qap.faq(restarts=R)
def _bits(mats, N):
    dense = np.zeros((len(mats), N, N))
    for b, m in enumerate(mats):
        dense[b, :len(m), :len(m)] = m
    return torch.from_numpy(synthetic.pack_adjacency(dense).view(np.int32)).to(DEV)


def _dense(mats, N):
    x = torch.full((len(mats), N, N), float('nan'))
    for b, m in enumerate(mats):
        x[b, :len(m), :len(m)] = torch.from_numpy(np.asarray(m)).float()
    return x.to(DEV)


CASES = {'bits16': (16, (16, 16, 16), False), 'bits32': (32, (32, 32), False), 'bits48': (48, (48, 33, 17, 1, 0), False),
         'real48': (48, (48, 20, 5), True)}


def _inputs(case):
    N, sizes, weighted = CASES[case]
    pairs = [(F.real_pair if weighted else F.zero_one_pair)(n, b) if n > 1 else (np.zeros((n, n)), np.zeros((n, n)))
             for b, n in enumerate(sizes)]
    make = _dense if weighted else _bits
    return make([p[0] for p in pairs], N), make([p[1] for p in pairs], N), torch.tensor(sizes, dtype=torch.int32, device=DEV), weighted


@pytest.mark.parametrize('case', sorted(CASES))
def test_restarted_faq_equals_single_starts_and_keeps_the_best(case):
    x1, x2, nv, weighted = _inputs(case)
    B, N, R = x1.shape[0], x1.shape[1], 4
    idx = torch.arange(B, device=DEV) + 9
    out = qap.faq(x1, x2, nvalid=nv, weighted=weighted, restarts=R, seed=SEED, pair_index=idx, return_all=True)
    assert all(t.is_cuda for t in out.values()) and out['restart'].dtype == torch.int64 and out['all_perm'].shape == (B, R, N)
    starts = qap.random_starts(nv, N, R, seed=SEED, pair_index=idx)
    plain = qap.faq(x1, x2, nvalid=nv, weighted=weighted)
    assert set(plain) == {'perm', 'qap', 'acc', 'nit', 'status'}
    for k in range(R):
        one = plain if k == 0 else qap.faq(x1, x2, nvalid=nv, weighted=weighted, P0=starts[:, k])
        for key in ('perm', 'nit', 'status', 'qap'):
            assert torch.equal(one[key], out['all_' + key][:, k]), (k, key)
    print(case, 'all_qap', out['all_qap'].cpu().tolist(), 'restart', out['restart'].cpu().tolist())
    for b in range(B):
        w = RR.best_of(out['all_qap'][b].cpu().tolist(), out['all_status'][b].cpu().tolist())
        assert int(out['restart'][b]) == w
        for key in ('perm', 'nit', 'status', 'qap'):
            assert torch.equal(out[key][b], out['all_' + key][b, w]), (b, key)
    assert bool((out['qap'] >= plain['qap']).all())
    obj = qap.objective_weighted(x1, x2, out['perm'], nv)['qap'] if weighted else qap.objective_bits(x1, x2, out['perm'], nv)['qap']
    live = out['status'] != 2
    assert torch.equal(obj[live], out['qap'][live]) and bool((out['qap'][~live] == -1).all())
    # polish: the exchange search on every restart's matching, the choice by the polished objective
    pol = qap.faq(x1, x2, nvalid=nv, weighted=weighted, restarts=R, seed=SEED, pair_index=idx, polish=True, return_all=True)
    flat = out['all_perm'].reshape(B * R, N)
    rep = [t.repeat_interleave(R, 0) for t in (x1, x2, nv)]
    two = qap.two_opt_weighted(*rep[:2], flat, nvalid=rep[2]) if weighted else qap.two_opt(*rep[:2], flat, nvalid=rep[2])
    alive = out['all_status'] != 2
    assert torch.equal(pol['all_qap'][alive], two['qap'].view(B, R)[alive]) and bool((pol['all_qap'][~alive] == -1).all())
    assert torch.equal(pol['all_perm'], two['perm'].view(B, R, N)) and torch.equal(pol['all_status'], out['all_status'])
    for b in range(B):
        w = RR.best_of(two['qap'].view(B, R)[b].cpu().tolist(), out['all_status'][b].cpu().tolist(), two['status'].view(B, R)[b].cpu().tolist())
        assert int(pol['restart'][b]) == w and pol['qap'][b] == pol['all_qap'][b, w] and pol['qap'][b] == pol['all_qap'][b].max()
        assert torch.equal(pol['perm'][b], two['perm'].view(B, R, N)[b, w]) and pol['swaps'][b] == two['swaps'].view(B, R)[b, w]
        assert pol['status_2opt'][b] == two['status'].view(B, R)[b, w] and pol['nit'][b] == out['all_nit'][b, w]


def test_restarted_faq_with_seeds_keeps_every_seed():
    n, N, R = 32, 32, 4
    pairs = [F.zero_one_pair(n, s) for s in range(3)]
    b1, b2 = _bits([p[0] for p in pairs], N), _bits([p[1] for p in pairs], N)
    seeds = torch.full((3, N), -1, dtype=torch.int32, device=DEV)
    seeds[0, :4] = torch.tensor([4, 2, 9, 0], dtype=torch.int32)
    seeds[1, 30] = 1
    seeds[2, 0], seeds[2, 1] = 5, 5                                 # two rows share a target: status 2 in every restart
    out = qap.faq(b1, b2, seeds=seeds, restarts=R, seed=SEED, return_all=True, polish=True)
    assert out['status'].tolist()[2] == 2 and out['restart'].tolist()[2] == 0 and out['qap'].tolist()[2] == -1
    assert out['seeded'].tolist()[:2] == [4, 1]
    held = seeds >= 0
    for k in range(R):
        assert torch.equal(out['all_perm'][:2, k][held[:2]], seeds[:2][held[:2]])
    assert torch.equal(out['perm'][:2][held[:2]], seeds[:2][held[:2]])
    first = qap.faq(b1, b2, seeds=seeds, restarts=R, seed=SEED, return_all=True)
    plain = qap.faq(b1, b2, seeds=seeds)
    for key in ('perm', 'nit', 'status', 'qap'):
        assert torch.equal(plain[key], first['all_' + key][:, 0]), key
    assert bool((first['qap'] >= plain['qap']).all()) and bool((out['qap'] >= first['qap']).all())


def test_refusals_on_the_device():
    x1, x2, nv, _ = _inputs('bits16')
    with pytest.raises(ValueError, match='restarts'):
        qap.faq(x1, x2, restarts=65)
    with pytest.raises(ValueError, match='matching'):
        qap.faq(x1, x2, restarts=2, P0=torch.arange(16, device=DEV).expand(3, 16))
    with pytest.raises(ValueError, match='return_P'):
        qap.faq(x1, x2, restarts=2, return_P=True)
    with pytest.raises(ValueError):
        qap.faq(x1, x2, restarts=2, P0='randomized')


# ------------------------------------------------------------------------------------------------------------------- the decode
def _decode_inputs(N=24, B=4):
    gen = PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.1, seed=5, device=DEV, vertex_proba=0.8)
    b1, b2, nv, lab = gen.bits(0, B, permute=True)
    s = torch.randn(B, N, N, generator=torch.Generator(device=DEV).manual_seed(3), device=DEV)
    s.scatter_add_(2, lab.long().clamp(0, N - 1)[:, :, None], torch.full((B, N, 1), 2.0, device=DEV))
    return s, b1, b2, nv.to(torch.int32), lab


def test_decode_takes_the_restart_keys():
    s, b1, b2, nv, lab = _decode_inputs()
    B, R = s.shape[0], 3
    faq = {'restarts': R, 'seed': 5}
    eager = decode_scores(s, b1, b2, nvalid=nv, labels=lab, meter=QapMeter(DEV), faq=faq)
    assert eager['faq_restart'].dtype == torch.int32 and eager['faq_restart'].shape == (B,)
    sk = qap.sinkhorn(s, nv)
    want = qap.faq(b1, b2, nvalid=nv, P0=sk['P'], restarts=R, seed=5)
    assert torch.equal(eager['faq_perm'], want['perm']) and torch.equal(eager['faq_restart'].long(), want['restart'])
    assert torch.equal(eager['faq_qap'].long(), want['qap']) and torch.equal(eager['faq_status'].long(), want['status'])
    other = decode_scores(s, b1, b2, nvalid=nv, labels=lab, meter=QapMeter(DEV), faq=dict(faq, index=torch.arange(B, device=DEV)))
    assert torch.equal(other['faq_perm'], eager['faq_perm']) and torch.equal(other['meter'].buf, eager['meter'].buf)
    # nothing is read back: the whole decode can be captured
    torch.cuda.synchronize()
    meter, graph = QapMeter(DEV), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = decode_scores(s, b1, b2, nvalid=nv, labels=lab, meter=meter, faq=faq)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap['faq_perm'], eager['faq_perm']) and torch.equal(cap['faq_restart'], eager['faq_restart'])
    assert torch.equal(meter.buf, eager['meter'].buf) and meter.record()['pairs'] == B
    # polish, and the single start
    pol = decode_scores(s, b1, b2, nvalid=nv, labels=lab, meter=QapMeter(DEV), faq=dict(faq, polish=True))
    assert bool((pol['faq_qap'] >= eager['faq_qap']).all())
    a = decode_scores(s, b1, b2, nvalid=nv, labels=lab, meter=QapMeter(DEV), faq=True)
    b = decode_scores(s, b1, b2, nvalid=nv, labels=lab, meter=QapMeter(DEV), faq={'restarts': 1})
    assert set(a) == set(b) and a['faq_restart'] is None and b['faq_restart'] is None
    for key in a:
        if torch.is_tensor(a[key]):
            assert torch.equal(a[key], b[key]), key
    assert torch.equal(a['meter'].buf, b['meter'].buf)
    assert bool((eager['faq_qap'] >= a['faq_qap']).all())
    with pytest.raises(ValueError, match='P0'):
        decode_scores(s, b1, b2, nvalid=nv, faq={'P0': 'randomized', 'restarts': 2})
    with pytest.raises(ValueError, match='restarts'):
        decode_scores(s, b1, b2, nvalid=nv, faq={'restarts': 0})
