"""GPU: seeds from the model's scores -- fgnn_confident_seeds through qap.confident_seeds, fgnn_seed_fold(_bins) through SeedMeter /
BinnedSeedMeter, the seeds= spec and seed_meter= of decode_scores / evaluate_scores / match / evaluate / noise_curve / fit -- against
the plain loops of confident_ref.  Everything compared is an integer or one float32 subtraction: tensors with torch.equal, records
as bytes."""
import math

import numpy as np
import pytest
import torch

import confident_ref as R
from graph_neural_net_amd import evaluation, planted, qap
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.evaluation import (BinnedEvalMeter, BinnedQapMeter, BinnedSeedMeter, EvalMeter, QapMeter, SeedMeter, decode_scores,
                                             evaluate_scores)
from graph_neural_net_amd.masked import MaskedTensor
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.sampler import EpochSampler
from graph_neural_net_amd.trainer import FgnnTrainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LAY = ParamLayout(2, 2, 32, 32, 3)


def _scores(kind, B, n, seed):
    g = np.random.default_rng(seed)
    if kind == 'ties':                                   # {0, 1, 2}: ties in both arg-maxes, equal margins across rows
        return g.integers(0, 3, size=(B, n, n)).astype(np.float32)
    S = g.standard_normal((B, n, n)).astype(np.float32)  # 'peaked': a permutation stands out, with distinct margins
    for b in range(B):
        S[b, np.arange(n), g.permutation(n)] += g.uniform(0, 4, size=n).astype(np.float32)
    return S


def _padded(S, N, nv):
    """(B, n, n) -> (B, N, N) with NaN around every pair's corner"""
    out = np.full((S.shape[0], N, N), np.nan, dtype=np.float32)
    for b, k in enumerate(nv):
        out[b, :k, :k] = S[b, :k, :k]
    return out


def _check(out, S, nv, count=None, min_margin=0.0):
    """the device result equals the plain loops, and fgnn_seed_index finds it valid"""
    seeds, nseeds, margin = R.confident_batch(S, nv, count, min_margin)
    assert out['seeds'].dtype == torch.int32 and out['nseeds'].dtype == torch.int32
    assert torch.equal(out['seeds'].cpu(), torch.from_numpy(seeds))
    assert torch.equal(out['nseeds'].cpu(), torch.from_numpy(nseeds))
    if 'margin' in out:
        assert out['margin'].dtype == torch.float32 and torch.equal(out['margin'].cpu(), torch.from_numpy(margin))
    nvt = None if nv is None else torch.as_tensor(np.asarray(nv), dtype=torch.int32, device=DEV)
    ix = qap.seed_index_device(out['seeds'], nvt)
    assert bool((ix['valid'] == 1).all()) and torch.equal(ix['nseed'], out['nseeds'])
    sd = out['seeds'].cpu().numpy()
    for b in range(sd.shape[0]):
        tg = sd[b][sd[b] >= 0].tolist()
        n = sd.shape[1] if nv is None else int(nv[b])
        assert len(set(tg)) == len(tg) and all(0 <= j < n for j in tg)
        assert (sd[b, n:] == -1).all()
    return seeds, nseeds, margin


# --------------------------------------------------------------------------------------------------------------- 1. exactness
@pytest.mark.parametrize('n', [1, 2, 31, 32, 33, 63, 64, 65, 80])
def test_equals_the_plain_loops(n):
    nv = [n, 0, max(n - 1, 1), (n + 1) // 2, n]
    for N in (n, 96):
        for kind, seed in (('ties', n), ('peaked', 100 + n)):
            S = _padded(_scores(kind, len(nv), n, seed), N, nv)
            out = qap.confident_seeds(torch.from_numpy(S).to(DEV), torch.tensor(nv, device=DEV), return_margin=True)
            _, nseeds, _ = _check(out, S, nv)
            if kind == 'peaked' and n >= 31:
                assert nseeds[0] > 0
    S = _scores('ties', 1, n, 7)                        # no nvalid: the whole matrix
    _check(qap.confident_seeds(torch.from_numpy(S).to(DEV), return_margin=True), S, None)


def test_the_largest_graph():
    N = 256
    S = _scores('peaked', 2, N, 9)
    S[1] = _scores('ties', 1, N, 10)[0]
    out = qap.confident_seeds(torch.from_numpy(S).to(DEV), return_margin=True)
    _, nseeds, _ = _check(out, S, None)
    assert nseeds[0] > 0
    with pytest.raises(RuntimeError, match='at most 256'):
        qap.confident_seeds_device(torch.zeros(1, 257, 257, device=DEV), None)
    host = qap.confident_seeds(torch.zeros(1, 257, 257, device=DEV), count=2)                   # above the limit: the host route
    assert host['seeds'].device.type == 'cuda' and host['seeds'][0, :3].tolist() == [0, -1, -1] and int(host['nseeds']) == 1


def test_non_finite_scores():
    n = 6
    S = np.arange(n * n, dtype=np.float32).reshape(n, n) % 7
    S[np.arange(n), [3, 0, 4, 1, 5, 2]] = 9.0
    S[0, 1] = np.nan                                     # strikes row 0 and column 1 (row 3's choice)
    S[2, 4] = np.inf                                     # row 2's maximum is not finite
    S[4, :] = -np.inf                                    # a row of -inf
    S[5, 0] = -np.inf
    T = np.stack([S, S.T.copy(), np.full((n, n), -np.inf, dtype=np.float32), np.full((n, n), np.nan, dtype=np.float32)])
    T = np.concatenate([T, _scores('peaked', 1, n, 1)])
    T[4, 2, 3] = -np.inf
    out = qap.confident_seeds(torch.from_numpy(T).to(DEV), return_margin=True)
    _check(out, T, None)
    assert out['seeds'][0].tolist() == [-1, 0, -1, -1, -1, 2]
    assert out['margin'][0, [0, 2, 4]].tolist() == [-math.inf] * 3 and out['nseeds'].tolist()[2:4] == [0, 0]
    one = qap.confident_seeds(torch.tensor([[[2.0]], [[math.nan]], [[-math.inf]]], device=DEV), return_margin=True)
    assert one['seeds'].flatten().tolist() == [0, -1, -1] and one['margin'].flatten().tolist() == [math.inf, -math.inf, -math.inf]


def test_strided_views_are_read_in_place():
    B, n, N = 3, 33, 40
    nv = [33, 20, 7]
    S = _padded(_scores('peaked', B, n, 4), N, nv)
    nvt = torch.tensor(nv, device=DEV)
    want = R.confident_batch(S, nv)
    for out in (qap.confident_seeds(MaskedTensor(torch.from_numpy(S).to(DEV), nvt, (1, 2)), return_margin=True),):
        assert torch.equal(out['seeds'].cpu(), torch.from_numpy(want[0])) and torch.equal(out['margin'].cpu(), torch.from_numpy(want[2]))
    big = torch.full((B + 1, N + 3, N + 8), math.nan, device=DEV)
    view = big[1:, 2:N + 2, 4:N + 4]
    view.copy_(torch.from_numpy(S))
    assert not view.is_contiguous()
    out = qap.confident_seeds(view, nvt, return_margin=True)
    _check(out, S, nv)
    t = view.transpose(1, 2)                             # rows not contiguous: copied, the same rule on the transposed scores
    _check(qap.confident_seeds(t, nvt, return_margin=True), np.ascontiguousarray(S.transpose(0, 2, 1)), nv)


# ---------------------------------------------------------------------------------------------------- 2. count and min_margin
@pytest.mark.parametrize('kind', ['ties', 'peaked'])
def test_count_and_min_margin(kind):
    n, N = 33, 40
    nv = [33, 12, 33, 0]
    S = _padded(_scores(kind, len(nv), n, 21), N, nv)
    dev_s, nvt = torch.from_numpy(S).to(DEV), torch.tensor(nv, device=DEV)
    for mm in (0, 1, 2.5):
        full, _, margin = _check(qap.confident_seeds(dev_s, nvt, min_margin=mm, return_margin=True), S, nv, None, mm)
        for count in (0, 1, 3, n, n + 5, None):
            out = qap.confident_seeds(dev_s, nvt, count=count, min_margin=mm)
            _check(out, S, nv, count, mm)
            kept = out['seeds'].cpu().numpy()
            for b in range(len(nv)):                     # a prefix of the count=None set in (margin descending, row ascending) order
                order = R.order_of(full[b], margin[b])
                want = sorted(order if count is None else order[:count])
                assert np.nonzero(kept[b] >= 0)[0].tolist() == want
                assert (kept[b][want] == full[b][want]).all()


# ------------------------------------------------------------------------------------------------------------- 3. determinism
def test_batch_independence_run_to_run_and_capture():
    n, N = 65, 96
    nv = [65, 40, 1, 0, 64, 33]
    S = _padded(_scores('ties', len(nv), n, 31), N, nv)
    S[4] = _padded(_scores('peaked', 1, n, 32), N, [64])[0]
    dev_s, nvt = torch.from_numpy(S).to(DEV), torch.tensor(nv, device=DEV, dtype=torch.int32)
    out = qap.confident_seeds(dev_s, nvt, count=9, return_margin=True)
    again = qap.confident_seeds(dev_s, nvt, count=9, return_margin=True)
    for k in out:
        assert torch.equal(out[k], again[k])
    for b in range(len(nv)):
        alone = qap.confident_seeds(dev_s[b:b + 1], nvt[b:b + 1], count=9, return_margin=True)
        for k in out:
            assert torch.equal(out[k][b:b + 1], alone[k]), (k, b)
    static = dev_s.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        qap.confident_seeds_device(static, nvt, 9, 0.0, True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = qap.confident_seeds_device(static, nvt, 9, 0.0, True)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(cap[k], out[k]) for k in out)
    T = _padded(_scores('peaked', len(nv), n, 33), N, nv)
    static.copy_(torch.from_numpy(T))
    graph.replay()
    torch.cuda.synchronize()
    _check(cap, T, nv, 9)
    assert not torch.equal(cap['seeds'], out['seeds'])


# ------------------------------------------------------------------------------------------ 4. equivalence with revealed seeds
def test_scores_that_spell_the_revealed_seeds_give_the_revealed_run():
    B, N, K = 16, 48, 8
    gen = PairGenerator(N, 'Regular', 'ErdosRenyi', edge_density=0.21, noise=0.1, seed=17, device=DEV)     # degree 10
    b1, b2, nv, labels = gen.bits(0, B, permute=True)
    revealed = planted.reveal_seeds(labels, nv, K, 17)
    scores = torch.zeros(B, N, N, device=DEV)
    scores.scatter_(2, revealed.clamp(min=0).long()[:, :, None], (revealed >= 0).float()[:, :, None] * 4.0)
    picked = qap.confident_seeds(scores, nv, min_margin=1.0)
    assert torch.equal(picked['seeds'], revealed) and picked['nseeds'].tolist() == [K] * B
    kw = dict(nvalid=nv, labels=labels, faq={'P0': 'barycenter'}, two_opt=True)
    sm, sm_ref = SeedMeter(DEV), SeedMeter(DEV)
    out = decode_scores(scores, b1, b2, seeds={'from': 'scores', 'min_margin': 1.0}, seed_meter=sm, **kw)
    ref = decode_scores(scores, b1, b2, seeds=revealed, seed_meter=sm_ref, **kw)
    for k in ('faq_perm', 'perm', 'faq_nit', 'seeded', 'seeds', 'nseeds'):
        assert torch.equal(out[k], ref[k]), k
    assert torch.equal(sm.buf, sm_ref.buf) and out['seed_meter'] is sm
    res = sm.result()
    assert res['seed_precision'] == 1.0 and res['seeds'] == B * K and res['pairs'] == B and res['clean'] == 1.0
    lab, free = labels.cpu().numpy(), revealed.cpu().numpy() < 0
    total = int(free.sum())
    assert res['free_nodes'] == total == B * (N - K)
    got = int(((out['perm'].cpu().numpy() == lab) & free).sum())
    print('free rows right: %d of %d; faq rounds %s' % (got, total, out['faq_nit'].tolist()))
    assert res['free_acc'] == got / total
    assert res['free_refined_acc'] == got / total
    stage = int(((out['faq_perm'].cpu().numpy() == lab) & free).sum())           # no status 2: the stage's matching is faq_perm
    assert bool((out['faq_status'] != 2).all()) and sm.record()['free_correct'] == stage
    # the QapMeter's count holds the seeded rows as hits; the seed meter's does not
    assert int(out['refined_correct'].sum()) == got + B * K


# ----------------------------------------------------------------------------------------------------------- 5. the seed fold
def _fold_inputs(B, N, seed):
    g = np.random.default_rng(seed)
    nv = g.integers(0, N + 1, size=B)
    nv[:3] = (N, 0, 1)
    labels = np.stack([g.permutation(N) for _ in range(B)]).astype(np.int32)
    for b in range(B):
        labels[b, nv[b]:] = g.integers(-5, 3 * N, size=N - nv[b])              # junk beyond n
    labels[g.random((B, N)) < 0.1] = -1
    assign = np.where(g.random((B, N)) < 0.5, labels, g.integers(0, N, size=(B, N))).astype(np.int32)
    perm = np.where(g.random((B, N)) < 0.8, labels, g.integers(0, N, size=(B, N))).astype(np.int32)
    seeds = np.where(g.random((B, N)) < 0.3, np.where(g.random((B, N)) < 0.85, labels, g.integers(0, N, size=(B, N))), -1).astype(np.int32)
    seeds[5] = -1                                                                # a pair without seeds
    seeds[6, :nv[6]] = labels[6, :nv[6]]                                         # and one without a free row
    return nv.astype(np.int32), labels, assign, perm, seeds


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _bytes(meter):
    return meter.buf.cpu().numpy()


def test_fold_equals_integer_sums():
    B, N = 16, 37
    nv, labels, assign, perm, seeds = _fold_inputs(B, N, 1)
    for use_perm, use_labels, use_seeds, use_nv in ((1, 1, 1, 1), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        a = [seeds if use_seeds else None, assign, perm if use_perm else None, labels if use_labels else None, nv if use_nv else None]
        if not use_nv:                                   # full corners: the junk labels are real rows now, keep seeds inside [0, N)
            a[3] = None if a[3] is None else np.clip(labels, -1, N - 1)
        d = _dev(*a)
        meter = SeedMeter(DEV)
        evaluation.seed_fold(meter, d[0], d[1], d[2], d[4], d[3], None, B, N, B)
        want = R.fold(R.empty_record(), a[0], a[1], a[2], a[3], a[4])
        assert (_bytes(meter) == R.record_bytes([want])).all(), (use_perm, use_labels, use_seeds, use_nv)
        assert meter.record() == want
        evaluation.seed_fold(meter, d[0], d[1], d[2], d[4], d[3], None, B, N, 5)          # live < B ignores the filler; a second step
        want = R.fold(want, a[0], a[1], a[2], a[3], a[4], live=5)
        assert meter.record() == want and want['steps'] == 2
        before = _bytes(meter).copy()
        evaluation.seed_fold(meter, d[0], d[1], d[2], d[4], d[3], None, B, N, 0)          # no pair: the record keeps its bytes
        assert (_bytes(meter) == before).all()
    assert math.isclose(float(meter.seed_precision), want['seed_correct'] / want['seeds'])
    assert math.isclose(float(meter.free_refined_acc), want['free_refined_correct'] / want['free_nodes'])


def test_binned_fold_and_epoch_cuts():
    B, N, K = 21, 19, 3
    nv, labels, assign, perm, seeds = _fold_inputs(B, N, 2)
    bins = np.random.default_rng(3).integers(0, K, size=B).astype(np.int32)
    bins[[2, 9]] = (-1, K)                               # outside [0, K): added nowhere
    d = _dev(seeds, assign, perm, labels, nv, bins)
    binned = BinnedSeedMeter(DEV, K, values=(0.0, 0.1, 0.2))
    evaluation.seed_fold(binned, d[0], d[1], d[2], d[4], d[3], d[5], B, N, B - 2)
    assert len(binned) == K and [r['noise'] for r in binned.result()] == [0.0, 0.1, 0.2]
    for k in range(K):                                   # record k: the bytes the plain fold gives for the bin's pairs alone
        rows = [b for b in range(B - 2) if bins[b] == k]
        plain = SeedMeter(DEV)
        sub = _dev(seeds[rows], assign[rows], perm[rows], labels[rows], nv[rows])
        evaluation.seed_fold(plain, sub[0], sub[1], sub[2], sub[4], sub[3], None, len(rows), N, len(rows))
        assert torch.equal(binned[k].buf, plain.buf), k
        assert (_bytes(plain) == R.record_bytes([R.fold(R.empty_record(), seeds, assign, perm, labels, nv, B - 2, bins, k)])).all()
    outside = BinnedSeedMeter(DEV, 1)
    evaluation.seed_fold(outside, d[0], d[1], d[2], d[4], d[3], torch.full((B,), 4, dtype=torch.int32, device=DEV), B, N, B)
    assert not outside.buf.any()
    records = []
    for cut in (3, 7):                                   # an epoch cut into batches of 3 and of 7: identical bytes but for `steps`
        m = BinnedSeedMeter(DEV, K)
        for lo in range(0, B, cut):
            hi = min(lo + cut, B)
            sub = _dev(seeds[lo:hi], assign[lo:hi], perm[lo:hi], labels[lo:hi], nv[lo:hi], bins[lo:hi])
            evaluation.seed_fold(m, sub[0], sub[1], sub[2], sub[4], sub[3], sub[5], hi - lo, N, hi - lo)
        recs = m.record()
        for r in recs:
            r.pop('steps')
        records.append(recs)
    assert records[0] == records[1]
    whole = BinnedSeedMeter(DEV, K)
    evaluation.seed_fold(whole, d[0], d[1], d[2], d[4], d[3], d[5], B, N, B)
    assert [dict(r, steps=0) for r in whole.record()] == [dict(r, steps=0) for r in records[0]]


# ------------------------------------------------------------------------------------------------------ 6. the epoch surface
N_EP, TB = 24, 16


def _gen(seed=5, **kw):
    return PairGenerator(N_EP, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.1, seed=seed, device=DEV, **kw)


@pytest.fixture(scope='module')
def trainer():
    tr = FgnnTrainer(LAY, LAY.init_flat(7, DEV), lr=2e-3)
    tr.train_step_bits(*_gen().bits(0, TB)[:2])
    return tr


def _hand_epoch(tr, gen, sampler, seeds_of):
    hq, hs, hm = QapMeter(DEV), SeedMeter(DEV), EvalMeter(DEV)
    for step in range(sampler.steps_per_epoch(TB)):
        idx, live = sampler.batch_index(0, step, TB), sampler.live_count(step, TB)
        b1, b2, nv, lab = gen.bits(index=idx, permute=True)
        tr.eval_step_bits(b1, b2, nvalid=nv, labels=lab, meter=hm, live=live, qap_meter=hq, faq=True,
                          seeds=seeds_of(b1, b2, nv, lab, idx), seed_meter=hs)
    return hq, hs, hm


def test_evaluate_with_revealed_and_with_confident_seeds(trainer):
    tr, gen = trainer, _gen(seed=3, vertex_proba=0.9)
    sampler = EpochSampler(40, shuffle=False)
    qm, sm, em = QapMeter(DEV), SeedMeter(DEV), EvalMeter(DEV)
    assert tr.evaluate(gen, sampler, TB, permute=True, meter=em, qap_meter=qm, faq=True, seeds=4, seed_meter=sm) is em
    hq, hs, hm = _hand_epoch(tr, gen, sampler, lambda b1, b2, nv, lab, idx: planted.reveal_seeds(lab, nv, 4, gen.seed, index=idx))
    assert torch.equal(qm.buf, hq.buf) and torch.equal(sm.buf, hs.buf) and torch.equal(em.buf, hm.buf)
    res = sm.result()
    assert res['pairs'] == 40 and res['seed_precision'] == 1.0 and res['clean'] == 1.0 and 0 < res['seeds'] <= 160
    print('revealed: %r' % (res,))

    def confident(b1, b2, nv, lab, idx):
        scores = tr._eval_forward(b1.shape[0], N_EP, nv, bits=torch.cat([b1, b2]).contiguous()).clone()
        return qap.confident_seeds(scores, nv)['seeds']

    qm, sm = QapMeter(DEV), SeedMeter(DEV)
    tr.evaluate(gen, sampler, TB, permute=True, qap_meter=qm, faq=True, seeds='scores', seed_meter=sm)
    hq, hs, _ = _hand_epoch(tr, gen, sampler, confident)
    assert torch.equal(qm.buf, hq.buf) and torch.equal(sm.buf, hs.buf) and sm.record()['pairs'] == 40
    print('confident: %r' % (sm.result(),))
    capped = SeedMeter(DEV)
    tr.evaluate(gen, sampler, TB, permute=True, qap_meter=QapMeter(DEV), faq=True, seeds={'from': 'scores', 'count': 2}, seed_meter=capped)
    assert capped.record()['seeds'] <= 80 and capped.record()['seeds'] <= sm.record()['seeds']


def test_refusals_of_the_epoch_surface(trainer):
    tr, gen = trainer, _gen(seed=3)
    sampler = EpochSampler(8, shuffle=False)
    with pytest.raises(ValueError, match='permute'):
        tr.evaluate(gen, sampler, 8, qap_meter=QapMeter(DEV), faq=True, seeds=4)
    with pytest.raises(ValueError, match='seeds'):
        tr.evaluate(gen, sampler, 8, permute=True, qap_meter=QapMeter(DEV), seeds='scores')                   # no faq=
    with pytest.raises(ValueError, match='seeds'):
        tr.evaluate(gen, sampler, 8, permute=True, qap_meter=QapMeter(DEV), faq=True, refine=1, seeds='scores')
    with pytest.raises(ValueError, match='qap_meter'):
        tr.evaluate(gen, sampler, 8, permute=True, seeds='scores')
    with pytest.raises(ValueError, match='seed_meter'):
        tr.evaluate(gen, sampler, 8, permute=True, qap_meter=QapMeter(DEV), faq=True, seed_meter=BinnedSeedMeter(DEV, 2))
    with pytest.raises(ValueError, match='seeds'):
        tr.evaluate(gen, sampler, 8, permute=True, qap_meter=QapMeter(DEV), faq=True, seeds={'from': 'labels'})
    with pytest.raises(ValueError, match='seeds'):
        tr.evaluate(gen, sampler, 8, permute=True, qap_meter=QapMeter(DEV), faq=True, seeds=-1)
    b1, b2, nv, lab = gen.bits(0, 8, permute=True)
    s = torch.randn(8, N_EP, N_EP, device=DEV)
    for kw in ({'two_opt': True}, {'faq': True, 'refine': 2}, {'refine': 1}):
        with pytest.raises(ValueError, match='seeds'):
            decode_scores(s, b1, b2, seeds='scores', **kw)
    with pytest.raises(ValueError, match='unknown'):
        decode_scores(s, b1, b2, faq=True, seeds={'from': 'scores', 'k': 2})
    with pytest.raises(ValueError, match='seed meter'):
        decode_scores(s, b1, b2, faq=True, seeds='scores', seed_meter=QapMeter(DEV))
    with pytest.raises(ValueError, match='qap_meter'):
        evaluate_scores(s, seeds='scores')
    with pytest.raises(ValueError, match='qap_meter'):
        evaluate_scores(s, seed_meter=SeedMeter(DEV))


def test_noise_curve_and_fit(trainer):
    tr, gen = trainer, _gen(seed=3)
    noises = (0.0, 0.1, 0.3)
    bq, bs = BinnedQapMeter(DEV, 3, values=noises), BinnedSeedMeter(DEV, 3, values=noises)
    tr.noise_curve(gen, noises, 4, 8, permute=True, qap_meter=bq, faq=True, seeds=4, seed_meter=bs)
    res = bs.result()
    assert len(bs) == 3 and [r['noise'] for r in res] == list(noises)
    assert all(r['pairs'] == 4 and r['seeds'] == 16 and r['seed_precision'] == 1.0 and r['free_nodes'] == 4 * (N_EP - 4) for r in res)
    bs2 = BinnedSeedMeter(DEV, 3)
    tr.noise_curve(gen, noises, 4, 8, permute=True, qap_meter=BinnedQapMeter(DEV, 3), faq=True, seeds='scores', seed_meter=bs2)
    assert all(r['pairs'] == 4 for r in bs2.record())
    with pytest.raises(ValueError, match='BinnedSeedMeter'):
        tr.noise_curve(gen, noises, 4, 8, permute=True, qap_meter=BinnedQapMeter(DEV, 3), faq=True, seeds=4, seed_meter=SeedMeter(DEV))
    a, b = (FgnnTrainer(LAY, LAY.init_flat(7, DEV), lr=1e-3) for _ in range(2))
    val = EpochSampler(4, shuffle=False)
    hist = a.fit(gen, EpochSampler(4, seed=1), gen, val, epochs=1, batch_size=2, decode_seeds='scores', decode_faq=True)
    plain = b.fit(gen, EpochSampler(4, seed=1), gen, val, epochs=1, batch_size=2, decode_refine=0, decode_faq=True)
    assert set(hist[0]) == set(plain[0]) | {'val_seed_precision', 'val_free_acc'}
    assert all(hist[0][k] == plain[0][k] for k in ('val_loss', 'val_acc', 'val_qap_ratio', 'val_recovered'))
    again = SeedMeter(DEV)
    a.evaluate(gen, val, 2, qap_meter=QapMeter(DEV), faq=True, seeds='scores', seed_meter=again)
    r = again.result()
    same = lambda x, y: x == y or (math.isnan(x) and math.isnan(y))
    assert same(hist[0]['val_seed_precision'], r['seed_precision']) and same(hist[0]['val_free_acc'], r['free_acc'])
    with pytest.raises(ValueError, match='decode_seeds'):
        a.fit(gen, EpochSampler(4, seed=1), gen, val, epochs=1, batch_size=2, decode_seeds='scores')


# -------------------------------------------------------------------------------------------------------- 7. unchanged paths
def _same_dict(a, b):
    assert set(a) == set(b), set(a) ^ set(b)
    for k, v in a.items():
        if torch.is_tensor(v):
            assert torch.equal(v, b[k]), k
        elif isinstance(v, dict):
            _same_dict(v, b[k])
        elif isinstance(v, MaskedTensor):
            assert torch.equal(v.tensor.rename(None), b[k].tensor.rename(None)), k
        elif v is None:
            assert b[k] is None, k


def test_defaults_change_nothing():
    B = 4
    b1, b2, nv, lab = _gen(vertex_proba=0.8).bits(0, B, permute=True)
    s = torch.randn(B, N_EP, N_EP, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV)
    s.scatter_add_(2, lab.long().clamp(0, N_EP - 1)[:, :, None], torch.full((B, N_EP, 1), 4.0, device=DEV))
    for kw in ({}, {'faq': True, 'two_opt': True}, {'refine': 2}):
        m0, m1 = QapMeter(DEV), QapMeter(DEV)
        plain = decode_scores(s, b1, b2, nvalid=nv, labels=lab, meter=m0, **kw)
        none = decode_scores(s, b1, b2, nvalid=nv, labels=lab, meter=m1, seeds=None, seed_meter=None, **kw)
        _same_dict(plain, none)
        assert torch.equal(m0.buf, m1.buf) and not {'seeds', 'nseeds', 'seeded', 'seed_meter'} & set(plain)
        e0, e1, q0, q1 = EvalMeter(DEV), EvalMeter(DEV), QapMeter(DEV), QapMeter(DEV)
        plain = evaluate_scores(s, nvalid=nv, labels=lab, meter=e0, qap_meter=q0, bits=(b1, b2), **kw)
        none = evaluate_scores(s, nvalid=nv, labels=lab, meter=e1, qap_meter=q1, bits=(b1, b2), seeds=None, seed_meter=None, **kw)
        _same_dict(plain, none)
        assert torch.equal(e0.buf, e1.buf) and torch.equal(q0.buf, q1.buf)
    from graph_neural_net_amd import synthetic
    from graph_neural_net_amd.siamese import Siamese_Node_Exp
    torch.manual_seed(3)
    ne = dict(type='node_embedding', block_init='block_emb', block_inside='block', num_blocks=2, in_features=32, out_features=32,
              depth_of_mlp=3)
    model = Siamese_Node_Exp(2, ne).to(DEV)
    x1, x2 = (x.to(DEV) for x in synthetic.make_batch(11, 4, 20, 'ErdosRenyi', 0.2, 0.1))
    for kw in ({}, {'faq': True, 'two_opt': True}):
        _same_dict(model.match(x1, x2, **kw), model.match(x1, x2, seeds=None, seed_meter=None, **kw))
    # the spec in match: the seeds qap.confident_seeds gives on the scores, held by every matching after the stage
    sm = SeedMeter(DEV)
    out = model.match(x1, x2, faq=True, two_opt=True, seeds={'from': 'scores', 'count': 3}, seed_meter=sm)
    want = qap.confident_seeds(out['scores'], count=3)
    assert torch.equal(out['seeds'], want['seeds']) and torch.equal(out['nseeds'], want['nseeds']) and torch.equal(out['seeded'], want['nseeds'])
    held = out['seeds'] >= 0
    assert torch.equal(out['perm'][held], out['seeds'][held]) and torch.equal(out['faq_perm'][held], out['seeds'][held])
    assert sm.record()['pairs'] == 4 and sm.record()['seeds'] == int(want['nseeds'].sum())
    ref = model.match(x1, x2, faq=True, two_opt=True, seeds=want['seeds'])
    assert all(torch.equal(out[k], ref[k]) for k in ('perm', 'faq_perm', 'faq_nit', 'qap_2opt', 'seeded', 'seeds', 'nseeds'))
