"""GPU: degree-profile matching -- fgnn_degree_profile through qap.degree_profile, and evaluation.baseline_curve(method=
'degree_profile') -- against tests/degree_profile_ref.py.

Bounds, none fitted to the device.  Weighted profiles are the inputs themselves: bit for bit.  A 0/1 profile value is one fp32
rounding (2^-24) of an fp64 evaluation of the formula: relative 2^-22 against the float64 restatement, its integer pre-image exact.
A distance is one fp32 rounding of an fp64 sum of non-negative terms (relative error (m + l) 2^-53 <= 2^-44): relative 2^-23 against
the float64 W1 of the DEVICE'S OWN profiles.  Everything else is exact.
Measured on the MI355X: max |X - X_ref| / |X_ref| = 2.8e-8 .. 6.0e-8 per pair over every shape and both inputs (bound 1.19e-7; half
an fp32 ulp is 6.0e-8), 0 on the pair whose profiles are all equal."""
import functools

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import degree_profile_ref as D
import pairgen_ref as PR
import planted_ref as PL
import wigner_ref as W
from test_gpu_grampa import _embed, _nv
from graph_neural_net_amd import evaluation, qap
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.wigner import WignerGenerator

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KEYS = {'X', 'perm', 'qap', 'acc', 'status'}
SHAPES = (1, 2, 5, 31, 32, 33, 63, 64, 65, 128, 129, 200, 256)
RAGGED = (33, 65, 129)                     # vertex_proba = 0.9 there
RECOVERY_SEED = 1


# --------------------------------------------------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def _weighted_case(N):
    """3 Wigner pairs of dataset 11 at s = 0 / 0.1 / 0.3, side 2 relabelled, NaN around every corner (channel 0 of a (B, 2, N, N)
    batch at even N, a pitched view at odd N) -> (fp32 corners of side 1, of side 2, labels (3, N), the device's result)"""
    As, Bs, labs = [], [], np.full((3, N), -1, dtype=np.int64)
    vp = 0.9 if N in RAGGED else 1.0
    for k, s in enumerate((0.0, 0.1, 0.3)):
        n = W.pair(11, k, N, s, vertex_proba=vp)[2]
        labs[k, :n] = PL.planted_perm(11, k, n)
        A, B, n = W.pair(11, k, N, s, vertex_proba=vp, labels=labs[k])
        As.append(A[:n, :n].astype(np.float32))
        Bs.append(B[:n, :n].astype(np.float32))
    form = 'pitched' if N % 2 else 'chan0'
    x1, x2 = _embed(As, N, form), _embed(Bs, N, form)
    out = qap.degree_profile(x1, x2, nvalid=_nv(As), labels=torch.from_numpy(labs).to(DEV), weighted=True, return_profiles=True)
    return As, Bs, labs, (x1, x2), out


@functools.lru_cache(maxsize=None)
def _bit_case(N):
    """3 Erdos-Renyi pairs (density 0.3, noise 0.05) as bit words; from N = 5 on pair 0 has an isolated vertex on side 1 and pair 1 a
    vertex adjacent to all others on side 2 -> (int64 corners of side 1, of side 2, (bits1, bits2, nv), the device's result)"""
    M1, M2, n = PR.generate(6, 0, 3, N, 'ErdosRenyi', 'ErdosRenyi', 0.3, 0.05, 0.9 if N in RAGGED else 1.0)
    M1, M2 = M1.astype(np.uint8), M2.astype(np.uint8)
    if N >= 5:
        M1[0, 1, :] = M1[0, :, 1] = 0
        M2[1, 0, 1:n[1]] = M2[1, 1:n[1], 0] = 1
    bits = [torch.from_numpy(PL.pack_bits(M).view(np.int32)).to(DEV) for M in (M1, M2)]
    nv = torch.from_numpy(n).to(device=DEV, dtype=torch.int32)
    out = qap.degree_profile(bits[0], bits[1], nvalid=nv, return_profiles=True)
    corners = [[M[b, :m, :m].astype(np.int64) for b, m in enumerate(n)] for M in (M1, M2)]
    return corners[0], corners[1], (bits[0], bits[1], nv), out


def _host(out):
    return {k: ([t.cpu().numpy() for t in v] if isinstance(v, tuple) else v.cpu().numpy()) for k, v in out.items()}


def _check_types(out, weighted):
    assert set(out) == KEYS | {'profiles', 'counts'}
    assert all(t.is_cuda for k, t in out.items() if k != 'profiles') and all(t.is_cuda for t in out['profiles'])
    assert out['X'].dtype == torch.float32 and out['perm'].dtype == torch.int32 and out['counts'].dtype == torch.int32
    assert out['status'].dtype == torch.int64 and out['acc'].dtype == torch.int64
    assert out['qap'].dtype == (torch.float32 if weighted else torch.int64)
    assert out['profiles'][0].dtype == torch.float32 and out['profiles'][0].shape == out['X'].shape == out['profiles'][1].shape


def _check_padding(slab, cnt, n):
    """+inf behind every row's m values, whole rows of +inf and counts of 0 past the corner"""
    assert not cnt[n:].any() and np.isposinf(slab[n:]).all()
    for i in range(n):
        assert np.isposinf(slab[i, cnt[i]:]).all() and np.isfinite(slab[i, :cnt[i]]).all()


def _check_distances(o, sizes, statuses):
    """X against the float64 W1 of the device's own profiles: relative 2^-23, exact zeros around the corner"""
    for b, n in enumerate(sizes):
        X = o['X'][b]
        assert not X[n:].any() and not X[:, n:].any() and not np.signbit(X[n:]).any() and not np.signbit(X[:, n:]).any()
        assert o['status'][b] == statuses[b]
        if statuses[b]:
            assert not X.any() and (o['perm'][b] == -1).all()
            continue
        Z = D.w1_matrix(D.from_slabs(o['profiles'][0][b], o['counts'][b, 0, :n]), D.from_slabs(o['profiles'][1][b], o['counts'][b, 1, :n]))
        err = np.abs(X[:n, :n].astype(np.float64) + Z)
        worst = (err / np.where(Z > 0, Z, 1.0)).max()
        print('n=%d pair %d: max |X - X_ref| / |X_ref| = %.3e (bound %.3e)' % (n, b, worst, 2.0 ** -23))
        assert (err <= 2.0 ** -23 * Z).all()


def _check_matching(o, sizes, labs):
    """perm = SciPy's assignment of the device's own X, -1 in the padding; acc counts the labels"""
    for b, n in enumerate(sizes):
        if o['status'][b]:
            assert (o['perm'][b] == -1).all() and o['acc'][b] == 0
            continue
        pi = linear_sum_assignment(-o['X'][b, :n, :n].astype(np.float64))[1]
        assert o['perm'][b, :n].tolist() == pi.tolist() and (o['perm'][b, n:] == -1).all()
        assert o['acc'][b] == int((pi == (np.arange(n) if labs is None else labs[b, :n])).sum())


# ------------------------------------------------------------------------------------------------------------------- 1. profiles
@pytest.mark.parametrize('N', SHAPES)
def test_weighted_profiles_are_the_sorted_inputs_bit_for_bit(N):
    As, Bs, _, _, out = _weighted_case(N)
    _check_types(out, True)
    o = _host(out)
    for side, mats in enumerate((As, Bs)):
        for b, A in enumerate(mats):
            n = len(A)
            slab, cnt = o['profiles'][side][b], o['counts'][b, side]
            if n < 2:
                assert o['status'][b] == 2 and np.isposinf(slab).all() and not cnt.any()
                continue
            assert cnt[:n].tolist() == [n - 1] * n
            _check_padding(slab, cnt, n)
            want = np.stack(D.weighted_profiles(A))
            assert want.dtype == np.float32 and np.array_equal(slab[:n, :n - 1].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize('N', SHAPES)
def test_bit_profiles_order_counts_and_values(N):
    """counts exact; the integer pre-image of every value is the sorted c_ik exactly; values within 2^-22 of the float64 formula"""
    M1s, M2s, _, out = _bit_case(N)
    _check_types(out, False)
    o = _host(out)
    for b in range(3):
        n = len(M1s[b])
        status = 2 if (n < 2 or D.bit_status(M1s[b]) or D.bit_status(M2s[b])) else 0
        assert o['status'][b] == status
        for side, M in enumerate((M1s[b], M2s[b])):
            slab, cnt = o['profiles'][side][b], o['counts'][b, side]
            if status:
                assert np.isposinf(slab).all() and not cnt.any()
                continue
            d, S, cs = D.bit_counts(M)
            assert cnt[:n].tolist() == d.tolist() == [len(c) for c in cs]
            _check_padding(slab, cnt, n)
            nn1, q = n * (n - 1), S / (n * (n - 1))
            for i, c in enumerate(cs):
                got, r = slab[i, :len(c)].astype(np.float64), int(n - 1 - d[i])
                want = D.bit_value(c, r, S, n)
                assert (np.abs(got - want) <= 2.0 ** -22 * np.abs(want)).all()
                if r > 0:
                    back = (got * np.sqrt(r * q * (1.0 - q)) * nn1 + r * S) / nn1
                    assert np.array_equal(np.rint(back).astype(np.int64), c) and np.abs(back - np.rint(back)).max(initial=0) < 1e-3
    if N >= 31:
        assert o['status'].tolist() == [0, 0, 0]
        assert o['counts'][0, 0, 1] == 0 and o['counts'][1, 1, 0] == len(M2s[1]) - 1        # the isolated vertex, the full row
        assert not o['profiles'][1][1][0, :len(M2s[1]) - 1].any()                           # r = 0: the values are 0


# ------------------------------------------------------------------------------------------------------------------ 2. distances
@pytest.mark.parametrize('N', SHAPES)
def test_weighted_distances_against_w1_of_the_device_profiles(N):
    As, _, _, _, out = _weighted_case(N)
    sizes = [len(A) for A in As]
    _check_distances(_host(out), sizes, [2 if n < 2 else 0 for n in sizes])


@pytest.mark.parametrize('N', SHAPES)
def test_bit_distances_against_w1_of_the_device_profiles(N):
    """unequal lengths: every pair of degrees has its own quantile grid"""
    M1s, M2s, _, out = _bit_case(N)
    statuses = [2 if (len(a) < 2 or D.bit_status(a) or D.bit_status(b)) else 0 for a, b in zip(M1s, M2s)]
    _check_distances(_host(out), [len(a) for a in M1s], statuses)


def test_regular_graphs_heavy_ties():
    """regular graphs (every d_k equal, few distinct c_ik) and a cycle, whose profiles are all the same: Z = 0 on that pair"""
    N = 40
    M1, M2, n = PR.generate(8, 0, 3, N, 'Regular', 'ErdosRenyi', 0.2, 0.03)
    M1, M2 = M1.astype(np.uint8), M2.astype(np.uint8)
    ring = np.zeros((N, N), dtype=np.uint8)
    idx = np.arange(N)
    ring[idx, (idx + 1) % N] = ring[(idx + 1) % N, idx] = 1
    M1[2], M2[2] = ring, ring[::-1, ::-1]
    bits = [torch.from_numpy(PL.pack_bits(M).view(np.int32)).to(DEV) for M in (M1, M2)]
    out = qap.degree_profile(bits[0], bits[1], return_profiles=True)
    o = _host(out)
    _check_distances(o, [N] * 3, [0] * 3)
    _check_matching(o, [N] * 3, None)
    assert not o['X'][2].any() and np.signbit(o['X'][2]).all()             # -(float)0 on the corner, which is the whole matrix
    for b in range(2):
        assert len(np.unique(o['profiles'][0][b][np.isfinite(o['profiles'][0][b])])) < N


# ------------------------------------------------------------------------------------------------------------------- 3. matching
@pytest.mark.parametrize('N', SHAPES)
def test_weighted_matching_qap_and_acc(N):
    As, _, labs, (x1, x2), out = _weighted_case(N)
    _check_matching(_host(out), [len(A) for A in As], labs)
    q = qap.objective_weighted(x1, x2, out['perm'], _nv(As))['qap']
    assert torch.equal(out['qap'], torch.where(out['status'] != 0, torch.full_like(q, -1), q))


@pytest.mark.parametrize('N', SHAPES)
def test_bit_matching_qap_and_acc(N):
    M1s, _, (b1, b2, nv), out = _bit_case(N)
    _check_matching(_host(out), [len(a) for a in M1s], None)
    q = qap.objective_bits(b1, b2, out['perm'], nv)['qap']
    assert torch.equal(out['qap'], torch.where(out['status'] != 0, torch.full_like(q, -1), q))


def test_dense_representations_equal_bit_words():
    M1s, M2s, (b1, b2, nv), out = _bit_case(33)
    dense = []
    for bits in (b1, b2):
        M = torch.from_numpy(PL.unpack_bits(bits.cpu().numpy(), 33).astype(np.float32))
        dense.append(torch.stack([M, torch.diag_embed(M.sum(-1))], 1).to(DEV))
    again = qap.degree_profile(dense[0], dense[1], nvalid=nv, return_profiles=True)
    for k in KEYS | {'counts'}:
        assert torch.equal(again[k], out[k]), k
    assert all(torch.equal(a, b) for a, b in zip(again['profiles'], out['profiles']))


# ------------------------------------------------------------------------------------------------------------------- 4. recovery
def _margin(Z, lab):
    """the least gap between a row's entry at its label and the row's best other entry"""
    n = len(Z)
    other = Z.copy()
    other[np.arange(n), lab] = np.inf
    return (other.min(1) - Z[np.arange(n), lab]).min()


@pytest.mark.parametrize('noise', [0.0, 0.1])
def test_recovery_wigner(noise):
    """WignerGenerator(32, noise=s, seed=1), pairs 0 .. 3, permute=True: the device's matching equals the restatement's on the same
    pairs, and the restatement recovers the planted labels.  Checked on the CPU with the restatement alone (wigner_ref.pair and
    planted_ref.planted_perm, seeds 1 .. 3, all fully recovered; seed 1 kept): 32 of 32 rows on all four pairs at both levels, every
    label the strict minimum of its row of Z by at least 0.017 (s = 0) and 0.0040 (s = 0.1) -- no ties."""
    x1, x2, nv, labels = WignerGenerator(32, noise=noise, seed=RECOVERY_SEED, device=DEV).weighted(0, 4, permute=True)
    out = qap.degree_profile(x1, x2, nvalid=nv, labels=labels, weighted=True)
    assert out['status'].tolist() == [0] * 4
    for b in range(4):
        lab = labels[b].cpu().numpy().astype(np.int64)
        Z = D.pair(x1[b, 0].cpu().numpy(), x2[b, 0].cpu().numpy(), True)[0]
        pi = D.matching(Z)
        assert pi.tolist() == lab.tolist() and _margin(Z, lab) > 1e-3
        assert out['perm'][b].tolist() == pi.tolist()
    assert out['acc'].tolist() == [32] * 4


def test_recovery_erdos_renyi():
    """PairGenerator(48, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0, seed=1), pairs 0 .. 3, permute=True: as above.  On the
    CPU (pairgen_ref.generate_pair, planted_ref.relabel_matrix, seeds 1 .. 3 all fully recovered; seed 1 kept): 48 of 48 rows on all
    four pairs, Z = 0 at every label and at least 0.069 elsewhere in its row -- no two vertices share a profile."""
    gen = PairGenerator(48, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.0, seed=RECOVERY_SEED, device=DEV)
    b1, b2, nv, labels = gen.bits(0, 4, permute=True)
    out = qap.degree_profile(b1, b2, nvalid=nv, labels=labels)
    assert out['status'].tolist() == [0] * 4
    M1, M2 = PL.unpack_bits(b1.cpu().numpy(), 48).astype(np.int64), PL.unpack_bits(b2.cpu().numpy(), 48).astype(np.int64)
    for b in range(4):
        lab = labels[b].cpu().numpy().astype(np.int64)
        Z = D.pair(M1[b], M2[b], False)[0]
        pi = D.matching(Z)
        assert pi.tolist() == lab.tolist() and _margin(Z, lab) > 1e-3
        assert out['perm'][b].tolist() == pi.tolist()
    assert out['acc'].tolist() == [48] * 4


# --------------------------------------------------------------------------------------------------------------------- 5. status
def test_status_of_a_mixed_batch():
    """0/1: a normal pair, an empty pair (n = 0), a complete graph, an empty graph -> 0 / 2 / 2 / 2; weighted: a normal pair and one
    with an inf in its corner -> 0 / 3; the normal pair's bits are those of the pair run alone"""
    N = 20
    M1, M2, _ = PR.generate(3, 0, 4, N, 'ErdosRenyi', 'ErdosRenyi', 0.3, 0.05)
    M1, M2 = M1.astype(np.uint8), M2.astype(np.uint8)
    M1[2] = 1 - np.eye(N, dtype=np.uint8)
    M2[3] = 0
    bits = [torch.from_numpy(PL.pack_bits(M).view(np.int32)).to(DEV) for M in (M1, M2)]
    nv = torch.tensor([N, 0, N, N], dtype=torch.int32, device=DEV)
    out = qap.degree_profile(bits[0], bits[1], nvalid=nv, return_profiles=True)
    assert out['status'].tolist() == [0, 2, 2, 2]
    assert not out['X'][1:].any() and (out['perm'][1:] == -1).all() and out['qap'][1:].tolist() == [-1] * 3
    assert torch.isposinf(out['profiles'][0][1:]).all() and torch.isposinf(out['profiles'][1][1:]).all() and not out['counts'][1:].any()
    alone = qap.degree_profile(bits[0][:1], bits[1][:1], return_profiles=True)
    for k in KEYS | {'counts'}:
        assert torch.equal(alone[k][0], out[k][0]), k
    assert torch.equal(alone['profiles'][0][0], out['profiles'][0][0]) and torch.equal(alone['profiles'][1][0], out['profiles'][1][0])

    As, Bs, _, (x1, x2), clean = _weighted_case(33)
    bad = x1.clone()
    bad[1, 2, 3] = float('inf')
    w = qap.degree_profile(bad, x2, nvalid=_nv(As), weighted=True)
    assert w['status'].tolist() == [0, 3, 0] and not w['X'][1].any() and (w['perm'][1] == -1).all() and w['qap'][1].item() == -1
    for k in ('X', 'perm', 'qap'):
        assert torch.equal(w[k][[0, 2]], clean[k][[0, 2]]), k
    nan2 = x2.clone()
    nan2[0, 4, 4] = float('nan')                                           # the diagonal lies inside the corner
    assert qap.degree_profile(x1, nan2, nvalid=_nv(As), weighted=True)['status'].tolist() == [3, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- 6. determinism
def test_determinism_and_batch_independence():
    """twice the same bits; pair k of a batch of 5 at N = 65 equals pair k alone at the smaller padded N = its own vertex count"""
    gen = WignerGenerator(65, noise=0.2, vertex_proba=0.9, seed=4, device=DEV)
    x1, x2, nv = gen.weighted(0, 5)
    a, b = (qap.degree_profile(x1, x2, nvalid=nv, weighted=True, return_profiles=True) for _ in range(2))
    for k in KEYS | {'counts'}:
        assert torch.equal(a[k], b[k]), k
    assert all(torch.equal(p, r) for p, r in zip(a['profiles'], b['profiles']))
    for k in (0, 3):
        n = int(nv[k])
        one = qap.degree_profile(x1[k:k + 1, :, :n, :n].contiguous(), x2[k:k + 1, :, :n, :n].contiguous(), weighted=True)
        assert 2 <= n <= 65 and one['X'].shape == (1, n, n)
        assert torch.equal(one['X'][0], a['X'][k, :n, :n]) and torch.equal(one['perm'][0], a['perm'][k, :n])
        assert one['status'][0] == a['status'][k] == 0
    pg = PairGenerator(65, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.05, vertex_proba=0.9, seed=4, device=DEV)
    b1, b2, bn = pg.bits(0, 5)
    c, d = qap.degree_profile(b1, b2, nvalid=bn), qap.degree_profile(b1, b2, nvalid=bn)
    for k in KEYS:
        assert torch.equal(c[k], d[k]), k
    M1, M2 = PL.unpack_bits(b1.cpu().numpy(), 65), PL.unpack_bits(b2.cpu().numpy(), 65)
    for k in (1, 4):
        n = int(bn[k])
        small = [torch.from_numpy(PL.pack_bits(M[k:k + 1, :n, :n]).view(np.int32)).to(DEV) for M in (M1, M2)]
        one = qap.degree_profile(small[0], small[1])
        assert torch.equal(one['X'][0], c['X'][k, :n, :n]) and torch.equal(one['perm'][0], c['perm'][k, :n])
        assert torch.equal(one['qap'][0], c['qap'][k])


# ----------------------------------------------------------------------------------------------------------------- 7. capturable
@pytest.mark.parametrize('weighted', [True, False])
def test_capturable(weighted):
    if weighted:
        x1, x2, nv, labels = WignerGenerator(48, noise=0.1, seed=RECOVERY_SEED, device=DEV).weighted(0, 8, permute=True)
    else:
        gen = PairGenerator(48, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.02, seed=RECOVERY_SEED, device=DEV)
        x1, x2, nv, labels = gen.bits(0, 8, permute=True)
    kw = dict(nvalid=nv, labels=labels, weighted=weighted, return_profiles=True)
    eager = qap.degree_profile(x1, x2, **kw)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        qap.degree_profile(x1, x2, **kw)                       # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = qap.degree_profile(x1, x2, **kw)
    flat = lambda o: {**{k: v for k, v in o.items() if k != 'profiles'}, 'profiles1': o['profiles'][0], 'profiles2': o['profiles'][1]}
    for _ in range(2):
        for t in flat(out).values():
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, t in flat(out).items():
            assert torch.equal(t, flat(eager)[k]), k


# ---------------------------------------------------------------------------------------------------------------------- 8. chain
def test_decode_chain_takes_X_as_scores():
    gen = PairGenerator(48, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.0, seed=RECOVERY_SEED, device=DEV)
    b1, b2, nv, labels = gen.bits(0, 4, permute=True)
    X = qap.degree_profile(b1, b2, nvalid=nv, labels=labels)['X']
    meter, ranks = evaluation.QapMeter(DEV), evaluation.RankMeter(DEV)
    evaluation.decode_scores(X, b1, b2, nvalid=nv, labels=labels, two_opt=True, seeds='scores', faq={'P0': 'scores'}, meter=meter)
    assert meter.result()['refined_acc'] == 1.0
    evaluation.evaluate_scores(X, nvalid=nv, labels=labels, rank_meter=ranks)
    assert ranks.result()['hits@1'] == 1.0


# ------------------------------------------------------------------------------------------------------------- 9. baseline_curve
@pytest.mark.parametrize('features', [None, 'weighted'])
def test_baseline_curve_equals_the_hand_loop(features):
    """K = 3 levels x 8 examples, batch 6: the records are bit for bit those of the loop over the public functions"""
    from graph_neural_net_amd.sampler import EpochSampler
    import graph_neural_net_amd
    weighted = features == 'weighted'
    if weighted:
        gen, noises = WignerGenerator(32, seed=RECOVERY_SEED, device=DEV), (0.0, 0.2, 0.6)
        qcls = evaluation.BinnedWeightedQapMeter
    else:
        gen, noises = PairGenerator(32, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, seed=2, device=DEV), (0.0, 0.05, 0.2)
        qcls = evaluation.BinnedQapMeter
    K, M, B = 3, 8, 6
    gq, gr = qcls(DEV, K), evaluation.BinnedRankMeter(DEV, K)
    got = graph_neural_net_amd.baseline_curve(gen, noises, M, B, method='degree_profile', features=features, qap_meter=gq, two_opt=True,
                                              rank_meter=gr)
    levels = gen.levels(noises)
    meter, qm, rm = evaluation.BinnedEvalMeter(DEV, K, values=levels.noises), qcls(DEV, K), evaluation.BinnedRankMeter(DEV, K)
    sampler = EpochSampler(K * M, shuffle=False, rank=0, world_size=1, drop_last=False, device=DEV)
    for step in range(sampler.steps_per_epoch(B)):
        e = sampler.batch_index(0, step, B)
        kw = dict(index=e % M, levels=levels, level=e // M, permute=True)
        x1, x2, nv, labels = gen.weighted(**kw) if weighted else gen.bits(**kw)
        X = qap.degree_profile(x1, x2, nvalid=nv, labels=labels, weighted=weighted)['X']
        evaluation.evaluate_scores(X, nvalid=nv, labels=labels, meter=meter, live=sampler.live_count(step, B), bins=e // M,
                                   rank_meter=rm, qap_meter=qm, two_opt=True, **({'adj': (x1, x2)} if weighted else {'bits': (x1, x2)}))
    assert torch.equal(got['meter'].buf, meter.buf) and torch.equal(gq.buf, qm.buf) and torch.equal(gr.buf, rm.buf)
    assert repr(got['records']) == repr(meter.result()) and repr(got['qap_records']) == repr(qm.result())
    assert repr(got['rank_records']) == repr(rm.result())
    assert [r['pairs'] for r in got['records']] == [M] * K and [r['noise'] for r in got['records']] == list(noises)
    if weighted:
        assert got['records'][0]['acc'] == 1.0
