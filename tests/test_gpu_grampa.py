"""GPU: the GRAMPA chain -- fgnn_grampa through qap.grampa, and evaluation.baseline_curve -- against tests/grampa_ref.py.

The value bound is not fitted to the device: a pair's max|X - X_ref| / max|X_ref| (X_ref the float64 eigen formula (a), or the
Kronecker solve (b) for directed inputs) must stay within MARGIN = 4 times the error the numpy recurrence (c) has on the SAME
inputs; the margin is there because the matrix cores' chain order is not numpy's.  The same rule holds for the true float64
residual of the returned X, and the reported `res` must lie within that bound of the true residual."""
import functools

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import grampa_ref as G
import planted_ref as PL
import wigner_ref as W
from graph_neural_net_amd import evaluation, qap
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.wigner import WignerGenerator

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KEYS = {'X', 'perm', 'qap', 'acc', 'nit', 'res', 'status'}
MARGIN = 4.0
SHAPES = (1, 2, 5, 31, 32, 33, 64, 65, 128, 129, 200)
RAGGED = (33, 65, 129)                     # vertex_proba = 0.9 there
NOISES = (0.0, 0.1, 0.3)
TIGHT = dict(tol=1e-6, maxiter=256)
RECOVERY_SEED = 1


@functools.lru_cache(maxsize=None)
def _wigner_case(N):
    """3 pairs of dataset 11 at s = 0 / 0.1 / 0.3, side 2 relabelled; -> per pair (A32, B32 corners, X_a, X_c, err_c, true_c)"""
    out = []
    for k, s in enumerate(NOISES):
        vp = 0.9 if N in RAGGED else 1.0
        n = W.pair(11, k, N, s, vertex_proba=vp)[2]
        A, B, n = W.pair(11, k, N, s, vertex_proba=vp, labels=PL.planted_perm(11, k, n))
        A, B = A[:n, :n].astype(np.float32), B[:n, :n].astype(np.float32)
        Xa = G.eig(A, B)
        Xc, _, _, st = G.cg32(A, B, **TIGHT)
        assert st == 0
        out.append((A, B, Xa, Xc, G.rel_err(Xc, Xa), G.true_residual(A, B, Xc)))
    return out


def _embed(mats, N, form):
    """corners -> a device batch with NaN around every corner: 'chan0' a (B, 2, N, N) batch whose channel 0 is read in place,
    'pitched' the [:, :N, :N] view of a NaN-filled (B, N + 3, N + 5) tensor"""
    B = len(mats)
    if form == 'chan0':
        x = torch.full((B, 2, N, N), float('nan'))
        view = x[:, 0]
    else:
        x = torch.full((B, N + 3, N + 5), float('nan'))
        view = x[:, :N, :N]
    for b, m in enumerate(mats):
        view[b, :len(m), :len(m)] = torch.from_numpy(np.asarray(m, dtype=np.float32))
    x = x.to(DEV)
    return x if form == 'chan0' else x[:, :N, :N]


def _nv(mats):
    return torch.tensor([len(m) for m in mats], dtype=torch.int32, device=DEV)


def _check_against(out, refs, H=None):
    """the three bounds of the module docstring for every pair; refs: (A, B, X_ref, X_c, err_c, true_c) per pair"""
    X, res = out['X'].double().cpu().numpy(), out['res'].double().cpu().numpy()
    for b, (A, B, Xr, _, err_c, true_c) in enumerate(refs):
        n = len(A)
        Xd = X[b, :n, :n]
        h = None if H is None else H[b]
        err_d, true_d = G.rel_err(Xd, Xr), G.true_residual(A, B, Xd, H=h)
        print('n=%d pair %d: err yardstick %.3e device %.3e | true residual yardstick %.3e device %.3e | res reported %.3e'
              % (n, b, err_c, err_d, true_c, true_d, res[b]))
        assert err_d <= MARGIN * err_c
        assert true_d <= MARGIN * true_c
        assert abs(res[b] - true_d) <= MARGIN * true_c
        assert not X[b, n:].any() and not X[b, :, n:].any()


# -------------------------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize('N', SHAPES)
def test_values_at_the_tile_edges(N):
    """Wigner pairs at every tile edge, B = 3, NaN around every corner, channel 0 of a (B, 2, N, N) batch read in place (even N) or
    a pitched view (odd N), ragged at N = 33 / 65 / 129.
    Measured, yardstick (c) in numpy: max|X - X_a| / max|X_a| = 7.1e-8 .. 8.1e-8 (N = 1, 2), 2.1e-7 .. 4.5e-7 (N = 5), 3.9e-7 ..
    1.2e-6 (N >= 31, the largest at N = 200); true residual 7.1e-8 .. 8.1e-8 (N = 1, 2), 2.8e-6 .. 8.8e-6 above.  Device (MI355X):
    the same figures to every printed digit at every shape -- the host's fp32 matmul walks k in ascending order with fused
    multiply-adds, as the matrix cores do -- so error and true residual are 1.0 times the yardstick's; the reported res is 5.5e-9 ..
    9.9e-7 and lies within 8.0e-6 of the true residual (bound: 4 times 6.1e-6 .. 8.8e-6 at N >= 31)."""
    refs = _wigner_case(N)
    form = 'pitched' if N % 2 else 'chan0'
    x1, x2 = _embed([r[0] for r in refs], N, form), _embed([r[1] for r in refs], N, form)
    out = qap.grampa(x1, x2, nvalid=_nv([r[0] for r in refs]), weighted=True, **TIGHT)
    assert set(out) == KEYS and all(t.is_cuda for t in out.values())
    assert out['X'].dtype == torch.float32 and out['perm'].dtype == torch.int32 and out['res'].dtype == torch.float32
    assert out['status'].tolist() == [0, 0, 0] and (out['nit'] > 0).all()
    _check_against(out, refs)
    for b, r in enumerate(refs):
        n = len(r[0])
        assert out['perm'][b, :n].tolist() == linear_sum_assignment(-r[2])[1].tolist()
        assert (out['perm'][b, n:] == -1).all()


# --------------------------------------------------------------------------------------------------------------------- 2. directed
def test_directed_inputs_against_the_kronecker_solve():
    """n = 8, non-symmetric A and B: nothing in the chain assumes symmetry.  Reference (b).
    Measured: yardstick error 3.1e-7 .. 6.7e-7, true residual 3.5e-6 .. 6.6e-6; device (MI355X): the same figures."""
    rng = np.random.default_rng(5)
    refs = []
    for _ in range(3):
        A = (rng.standard_normal((8, 8)) / np.sqrt(8)).astype(np.float32)
        B = (0.9 * A + 0.3 * rng.standard_normal((8, 8)) / np.sqrt(8)).astype(np.float32)
        Xb = G.kron_solve(A, B)
        Xc = G.cg32(A, B, **TIGHT)[0]
        refs.append((A, B, Xb, Xc, G.rel_err(Xc, Xb), G.true_residual(A, B, Xc)))
    out = qap.grampa(_embed([r[0] for r in refs], 8, 'chan0'), _embed([r[1] for r in refs], 8, 'chan0'), weighted=True, **TIGHT)
    assert out['status'].tolist() == [0, 0, 0]
    _check_against(out, refs)


# -------------------------------------------------------------------------------------------------------------------------- 3. rhs
def test_rhs_prior_similarity():
    """a random positive (B, N, N) prior in place of the all-ones H, N = 33 (its corner read: NaN around the ragged one).
    Measured: yardstick error 5.4e-7 .. 8.4e-7, true residual 7.4e-6 .. 8.3e-6; device (MI355X): the same figures."""
    rng = np.random.default_rng(7)
    refs, Hs = [], []
    for k, n in enumerate((33, 33, 20)):
        A, B, _ = W.pair(5, k, n, 0.1)
        A, B = A.astype(np.float32), B.astype(np.float32)
        H = (rng.random((n, n)) + 0.5).astype(np.float32)
        Xa = G.eig(A, B, H=H)
        Xc = G.cg32(A, B, H=H, **TIGHT)[0]
        refs.append((A, B, Xa, Xc, G.rel_err(Xc, Xa), G.true_residual(A, B, Xc, H=H)))
        Hs.append(H)
    rhs = _embed(Hs, 33, 'pitched').contiguous()
    out = qap.grampa(_embed([r[0] for r in refs], 33, 'pitched'), _embed([r[1] for r in refs], 33, 'pitched'), nvalid=_nv(Hs),
                     weighted=True, rhs=rhs, **TIGHT)
    assert out['status'].tolist() == [0, 0, 0]
    _check_against(out, refs, H=Hs)


# ------------------------------------------------------------------------------------------------------------------ 4. standardize
def test_standardize_on_bit_words():
    """bit words of ragged Erdos-Renyi pairs (N = 40): standardize defaults to True there; reference (a) on the float64-standardised
    matrices, yardstick (c) on their fp32 images.  Measured: yardstick error 4.3e-7 .. 7.8e-7, true residual 6.7e-6 .. 7.6e-6; device (MI355X): error 4.2e-7 .. 7.1e-7 (0.87 .. 1.18
    times the yardstick's per pair), true residual 7.0e-6 .. 7.8e-6 (0.91 .. 1.10 times)."""
    gen = PairGenerator(40, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.2, noise=0.05, vertex_proba=0.9, seed=3, device=DEV)
    b1, b2, nv = gen.bits(0, 4)
    M1, M2 = PL.unpack_bits(b1.cpu().numpy(), 40), PL.unpack_bits(b2.cpu().numpy(), 40)
    refs = []
    for b, n in enumerate(nv.tolist()):
        A, B = G.standardize64(M1[b, :n, :n]), G.standardize64(M2[b, :n, :n])
        Xa = G.eig(A, B)
        Xc = G.cg32(A, B, **TIGHT)[0]
        A32, B32 = A.astype(np.float32), B.astype(np.float32)
        refs.append((A32, B32, Xa, Xc, G.rel_err(Xc, Xa), G.true_residual(A32, B32, Xc)))
    out = qap.grampa(b1, b2, nvalid=nv, **TIGHT)
    assert out['status'].tolist() == [0] * 4 and out['qap'].dtype == torch.int64
    _check_against(out, refs)
    assert torch.equal(out['qap'], qap.objective_bits(b1, b2, out['perm'], nv)['qap'])


def test_standardize_flat_graphs_are_status_2():
    """an empty and a complete graph have no variance: status 2, perm = -1, X = 0, qap = -1; the pair between them is solved"""
    n = 12
    rng = np.random.default_rng(0)
    M = np.triu(rng.random((n, n)) < 0.4, 1)
    mats = np.stack([np.zeros((n, n)), (M | M.T).astype(np.float64), 1.0 - np.eye(n)]).astype(np.uint8)
    bits = torch.from_numpy(PL.pack_bits(mats).view(np.int32)).to(DEV)
    out = qap.grampa(bits, bits)
    assert out['status'].tolist() == [2, 0, 2]
    assert (out['perm'][[0, 2]] == -1).all() and not out['X'][[0, 2]].any() and out['qap'][[0, 2]].tolist() == [-1, -1]
    assert sorted(out['perm'][1].tolist()) == list(range(n))


# ------------------------------------------------------------------------------------------------------------ 5. status and freezing
def test_status_nit_and_freezing():
    refs = _wigner_case(32)
    A, B = [r[0] for r in refs], [r[1] for r in refs]
    x1, x2 = _embed(A, 32, 'chan0'), _embed(B, 32, 'chan0')
    short = qap.grampa(x1, x2, weighted=True, maxiter=3)
    assert short['status'].tolist() == [1, 1, 1] and short['nit'].tolist() == [3, 3, 3]
    empty = qap.grampa(x1, x2, nvalid=torch.tensor([32, 0, 32], device=DEV), weighted=True, maxiter=3)
    assert empty['status'].tolist() == [1, 2, 1] and (empty['perm'][1] == -1).all() and not empty['X'][1].any()
    assert empty['qap'][1].item() == -1 and empty['nit'][1].item() == 0
    # a pair that met tol keeps the X it had at round nit
    base = qap.grampa(x1, x2, weighted=True)
    assert base['status'].tolist() == [0, 0, 0]
    for b, nit in enumerate(base['nit'].tolist()):
        at = qap.grampa(x1[b:b + 1], x2[b:b + 1], weighted=True, maxiter=nit)
        later = qap.grampa(x1[b:b + 1], x2[b:b + 1], weighted=True, maxiter=nit + 40)
        assert at['status'].item() == 0 and at['nit'].item() == nit == later['nit'].item()
        assert torch.equal(at['X'], later['X']) and torch.equal(at['X'][0], base['X'][b])


def test_inf_in_a_corner_is_status_3_and_leaves_the_others_alone():
    refs = _wigner_case(33)
    x1, x2 = _embed([r[0] for r in refs], 33, 'pitched'), _embed([r[1] for r in refs], 33, 'pitched')
    nv = _nv([r[0] for r in refs])
    clean = qap.grampa(x1, x2, nvalid=nv, weighted=True)
    bad1 = x1.clone()
    bad1[1, 2, 3] = float('inf')
    out = qap.grampa(bad1, x2, nvalid=nv, weighted=True)
    assert out['status'].tolist() == [0, 3, 0]
    assert torch.isfinite(out['X']).all()
    for k in ('X', 'perm', 'nit', 'res', 'qap'):
        assert torch.equal(out[k][[0, 2]], clean[k][[0, 2]]), k


# ---------------------------------------------------------------------------------------------------------------- 6. determinism
def test_determinism_and_batch_independence():
    gen = WignerGenerator(65, noise=0.2, vertex_proba=0.9, seed=4, device=DEV)
    x1, x2, nv = gen.weighted(0, 5)
    a, b = qap.grampa(x1, x2, nvalid=nv, weighted=True), qap.grampa(x1, x2, nvalid=nv, weighted=True)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    for k in (0, 3):
        one = qap.grampa(x1[k:k + 1], x2[k:k + 1], nvalid=nv[k:k + 1], weighted=True)
        for key in ('X', 'perm', 'nit', 'res'):
            assert torch.equal(one[key][0], a[key][k]), key


# -------------------------------------------------------------------------------------------------------------------- 7. recovery
def _recovery_pairs():
    gen = WignerGenerator(48, noise=0.1, seed=RECOVERY_SEED, device=DEV)
    return gen.weighted(0, 8, permute=True)


def test_recovery_of_the_planted_matching():
    """WignerGenerator(48, noise=0.1, seed=1), 8 pairs, permute=True: perm == labels on every row of every pair, and perm == SciPy's
    assignment of (a).  The seed's check: on the CPU, through wigner_ref.pair and planted_ref.planted_perm, (a) recovers all 8
    pairs for every seed 1 .. 7 tried (and (c) at the defaults converges in 84 .. 99 rounds on such inputs); asserted again here."""
    for k in range(8):
        lab = PL.planted_perm(RECOVERY_SEED, k, 48)
        A, B, _ = W.pair(RECOVERY_SEED, k, 48, 0.1, labels=lab)
        assert linear_sum_assignment(-G.eig(A.astype(np.float32), B.astype(np.float32)))[1].tolist() == lab.tolist()
    x1, x2, nv, labels = _recovery_pairs()
    out = qap.grampa(x1, x2, labels=labels, weighted=True)
    assert out['status'].tolist() == [0] * 8
    assert torch.equal(out['perm'], labels) and out['acc'].tolist() == [48] * 8
    for b in range(8):
        Xa = G.eig(x1[b, 0].cpu().numpy(), x2[b, 0].cpu().numpy())
        assert out['perm'][b].tolist() == linear_sum_assignment(-Xa)[1].tolist()
    assert torch.equal(out['qap'], qap.objective_weighted(x1, x2, out['perm'], None)['qap'])


def test_recovery_at_noise_zero():
    """s = 0, N = 65, side 2 a relabelled copy: the same (checked on the CPU: (a) recovers pairs 0 .. 2 of seeds 1 and 2)"""
    x1, x2, nv, labels = WignerGenerator(65, noise=0.0, seed=2, device=DEV).weighted(0, 3, permute=True)
    out = qap.grampa(x1, x2, labels=labels, weighted=True)
    assert torch.equal(out['perm'], labels)
    for b in range(3):
        Xa = G.eig(x1[b, 0].cpu().numpy(), x2[b, 0].cpu().numpy())
        assert out['perm'][b].tolist() == linear_sum_assignment(-Xa)[1].tolist()


# ----------------------------------------------------------------------------------------------------------------------- 8. chain
def test_decode_chain_takes_X_as_scores():
    x1, x2, nv, labels = _recovery_pairs()
    X = qap.grampa(x1, x2, labels=labels, weighted=True)['X']
    meter = evaluation.WeightedQapMeter(DEV)
    evaluation.decode_scores_weighted(X, x1, x2, labels=labels, faq={'P0': 'scores'}, two_opt=True, meter=meter)
    assert meter.result()['refined_acc'] == 1.0


def test_capturable():
    x1, x2, nv, labels = _recovery_pairs()
    eager = qap.grampa(x1, x2, labels=labels, weighted=True)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        qap.grampa(x1, x2, labels=labels, weighted=True)       # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = qap.grampa(x1, x2, labels=labels, weighted=True)
    for _ in range(2):
        for t in out.values():
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, t in out.items():
            assert torch.equal(t, eager[k]), k


# -------------------------------------------------------------------------------------------------------------- 9. baseline_curve
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
    got = graph_neural_net_amd.baseline_curve(gen, noises, M, B, features=features, qap_meter=gq, two_opt=True, rank_meter=gr)
    levels = gen.levels(noises)
    meter, qm, rm = evaluation.BinnedEvalMeter(DEV, K, values=levels.noises), qcls(DEV, K), evaluation.BinnedRankMeter(DEV, K)
    sampler = EpochSampler(K * M, shuffle=False, rank=0, world_size=1, drop_last=False, device=DEV)
    for step in range(sampler.steps_per_epoch(B)):
        e = sampler.batch_index(0, step, B)
        kw = dict(index=e % M, levels=levels, level=e // M, permute=True)
        x1, x2, nv, labels = gen.weighted(**kw) if weighted else gen.bits(**kw)
        X = qap.grampa(x1, x2, nvalid=nv, labels=labels, weighted=weighted)['X']
        evaluation.evaluate_scores(X, nvalid=nv, labels=labels, meter=meter, live=sampler.live_count(step, B), bins=e // M,
                                   rank_meter=rm, qap_meter=qm, two_opt=True, **({'adj': (x1, x2)} if weighted else {'bits': (x1, x2)}))
    assert torch.equal(got['meter'].buf, meter.buf) and torch.equal(gq.buf, qm.buf) and torch.equal(gr.buf, rm.buf)
    assert repr(got['records']) == repr(meter.result()) and repr(got['qap_records']) == repr(qm.result())
    assert repr(got['rank_records']) == repr(rm.result())
    assert [r['pairs'] for r in got['records']] == [M] * K and [r['noise'] for r in got['records']] == list(noises)
    if weighted:
        assert got['records'][0]['acc'] == 1.0
