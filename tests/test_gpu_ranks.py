"""GPU: rank metrics on the device -- fgnn_eval_ranks / fgnn_rank_fold (csrc/rank.hip), evaluation.rank_scores / RankMeter /
BinnedRankMeter / evaluate_scores(rank_meter=), metrics.match_ranks / hits_at_k and the trainer's rank_meter= / rank_ks= -- against
the brute-force reference of tests/rank_ref.py.

The ranks are functions of comparisons on the given fp32 scores: every integer is compared for EQUALITY; the one tolerance is
1e-12 n_b on a pair's fp64 sum of 1 / rank against the correctly rounded sum.  Scores carry NaN in their padding and every output
buffer is sentinel-filled before each call, so a kernel that reads padding, writes outside the valid rows or leaves an output
unwritten fails here.

`steps` counts the fold calls that added a pair to a record, so it is the one field that depends on how an epoch was cut into
calls: the cutting tests compare the record's bytes with that word masked and assert the word separately.

Measured on the MI355X, worst over every case of test_ranks_and_fold_equal_the_reference: a pair's fp64 sum of 1 / rank lies within
1.5e-4 of its bound 1e-12 n_b."""
import ctypes

import numpy as np
import pytest
import torch

import rank_ref as RR
from graph_neural_net_amd import _lib, metrics
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.evaluation import BinnedEvalMeter, BinnedRankMeter, EvalMeter, RankMeter, evaluate_scores, rank_scores
from graph_neural_net_amd.masked import MaskedTensor
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.sampler import EpochSampler
from graph_neural_net_amd.trainer import FgnnTrainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
SENTINEL = -77
REC = ctypes.sizeof(_lib.RankRecord)
STEPS = _lib.RankRecord.steps.offset
KS = RR.KS


def _ranks(sd, nvd, labd, B, N):
    rank = torch.full((B, N), SENTINEL, dtype=torch.int32, device=DEV)
    _lib.call('fgnn_eval_ranks', _lib.ptr(sd), N * N, N, _lib.ptr(nvd), _lib.ptr(labd), B, N, _lib.ptr(rank), _lib.stream_ptr())
    return rank


def _fold(rank, nvd, live, records, bins=None, K=1, ks=KS):
    """fgnn_rank_fold of the first `live` pairs of `rank` into `records` (K x 112 bytes on the device) on sentinel-filled outputs"""
    B, N = rank.shape
    nk = len(ks)
    o = {'hits': torch.full((B, nk), SENTINEL, dtype=torch.int32, device=DEV),
         'rr': torch.full((B,), NAN, dtype=torch.float64, device=DEV),
         'rank_sum': torch.full((B,), SENTINEL, dtype=torch.int64, device=DEV),
         'targets': torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV)}
    _lib.call('fgnn_rank_fold', _lib.ptr(rank), _lib.ptr(nvd), B, N, live, (ctypes.c_int * nk)(*ks), nk, _lib.ptr(bins), K,
              _lib.ptr(o['hits']), _lib.ptr(o['rr']), _lib.ptr(o['rank_sum']), _lib.ptr(o['targets']), _lib.ptr(records),
              _lib.stream_ptr())
    return o


def _zeros(K=1):
    return torch.zeros(K * REC, dtype=torch.uint8, device=DEV)


def _record(buf, k=0):
    r = _lib.RankRecord.from_buffer_copy(buf[k * REC:(k + 1) * REC].cpu().numpy().tobytes())
    return {'rr_sum': r.rr_sum, 'rank_sum': r.rank_sum, 'targets': r.targets, 'nodes': r.nodes, 'pairs': r.pairs, 'steps': r.steps,
            'hits': list(r.hits)}


def _but_steps(buf):
    """the record's bytes with the `steps` word masked"""
    out = buf.clone().view(-1, REC)
    out[:, STEPS:STEPS + 8] = 0
    return out


def _bits(x):
    return np.float64(x).view(np.int64)


# ---------------------------------------------------------------------------------------------------------- the two kernels
@pytest.mark.parametrize('B', RR.BS)
@pytest.mark.parametrize('N', RR.NS)
def test_ranks_and_fold_equal_the_reference(N, B):
    for ragged in (False, True):
        c = RR.case(N, B, ragged)
        nv = c['nv'].tolist()
        sd = c['scores'].to(DEV)
        nvd = c['nv'].to(DEV) if ragged else None
        rows = torch.arange(N)[None, :] < c['nv'].long()[:, None]
        for name, lab in c['labels'].items():
            ref = c['ref'][name]
            labd = None if lab is None else lab.to(DEV)
            rank = _ranks(sd, nvd, labd, B, N)
            got = rank.cpu()
            assert bool((got[~rows] == SENTINEL).all()), 'a row past n_b was written'
            assert np.array_equal(got[rows].numpy(), ref['rank'][rows.numpy()]), (ragged, name)
            records = _zeros()
            o = _fold(rank, nvd, B, records)
            pairs = ref['pairs']
            assert o['hits'].cpu().tolist() == [p['hits'] for p in pairs]
            assert o['rank_sum'].cpu().tolist() == [p['rank_sum'] for p in pairs]
            assert o['targets'].cpu().tolist() == [p['targets'] for p in pairs]
            rr = o['rr'].cpu().numpy()
            worst = 0.0
            for b, p in enumerate(pairs):
                err = abs(rr[b] - p['rr'])
                worst = max(worst, err / (1e-12 * nv[b]) if nv[b] else err)
                assert err <= 1e-12 * nv[b], (b, rr[b], p['rr'])
            print('N %d B %d ragged %d %s: worst pair_rr error / (1e-12 n_b) = %.2e' % (N, B, ragged, name, worst))
            # the record: the pairs in pair order, one at a time -- rr_sum is the sequential sum of the device's own pair sums
            want = RR.fold_record(rr, o['hits'].cpu().tolist(), o['rank_sum'].cpu().tolist(), o['targets'].cpu().tolist(), nv, range(B))
            rec = _record(records)
            assert _bits(rec['rr_sum']) == _bits(want['rr_sum'])
            assert {k: v for k, v in rec.items() if k != 'rr_sum'} == {k: v for k, v in want.items() if k != 'rr_sum'}
            # the same call twice: the same bytes
            records2 = _zeros()
            assert torch.equal(_ranks(sd, nvd, labd, B, N), rank)
            o2 = _fold(rank, nvd, B, records2)
            assert torch.equal(records, records2) and all(torch.equal(o[k], o2[k]) for k in o)
            # ... and through the public functions
            if name != 'identity' or not ragged:
                mt = MaskedTensor(sd, nvd, (1, 2)) if ragged else sd
                r0 = ref['rank'].copy()
                r0[~rows.numpy()] = 0
                assert np.array_equal(metrics.match_ranks(mt, labels=labd).cpu().numpy(), r0)
                assert metrics.hits_at_k(mt, KS[2], labels=labd) == (sum(p['hits'][2] for p in pairs), sum(nv))


@pytest.mark.parametrize('N', [5, 16, 17, 64, 65, 130])
def test_adversarial_rows_hold_the_beats_rule(N):
    """small-integer scores (duplicates in every row), NaN at several columns, +-inf, a row of -inf, a constant row: the reference's
    ranks; rank == 1 is the row_hit of fgnn_eval_pairs and hits[k = 1] the count of fgnn_accuracy_max(_labels), case by case"""
    g = torch.Generator().manual_seed(N)
    s, nv = RR.adversarial(N, g)
    B = s.shape[0]
    labs = RR.label_sets(nv, N, g)
    sd, nvd = s.to(DEV), nv.to(DEV)
    rows = torch.arange(N)[None, :] < nv.long()[:, None]
    for name, lab in labs.items():
        labd = None if lab is None else lab.to(DEV)
        rank = _ranks(sd, nvd, labd, B, N)
        ref = RR.ranks(s.numpy(), nv.tolist(), None if lab is None else lab.numpy(), fill=SENTINEL)
        assert np.array_equal(rank.cpu().numpy(), ref), name
        cost = torch.empty(B, N, N, dtype=torch.float32, device=DEV)
        row_ce = torch.empty(B, N, dtype=torch.float32, device=DEV)
        row_hit = torch.full((B, N), SENTINEL, dtype=torch.int32, device=DEV)
        _lib.call('fgnn_eval_pairs', _lib.ptr(sd), _lib.ptr(nvd), _lib.ptr(labd), B, N, _lib.ptr(cost), N * N, N, _lib.ptr(row_ce),
                  _lib.ptr(row_hit), _lib.stream_ptr())
        assert torch.equal((rank == 1)[rows.to(DEV)], (row_hit == 1)[rows.to(DEV)]), name
        correct = torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV)
        if labd is None:
            _lib.call('fgnn_accuracy_max', _lib.ptr(sd), _lib.ptr(nvd), B, N, _lib.ptr(correct), _lib.stream_ptr())
        else:
            _lib.call('fgnn_accuracy_max_labels', _lib.ptr(sd), _lib.ptr(labd), _lib.ptr(nvd), B, N, _lib.ptr(correct), _lib.stream_ptr())
        o = _fold(rank, nvd, B, _zeros())
        assert KS[0] == 1 and torch.equal(o['hits'][:, 0], correct), name


@pytest.mark.parametrize('N', [16, 17, 65])
def test_the_four_arg_max_routes_agree_on_the_adversarial_rows(N):
    """one arg-max rule, four routes: fgnn_accuracy_max, fgnn_accuracy_max_labels, the row_hit of fgnn_eval_pairs and rank == 1 of
    fgnn_eval_ranks count the same rows of every pair -- against the identity written out as labels, so that all four see one target"""
    g = torch.Generator().manual_seed(N)
    s, nv = RR.adversarial(N, g)
    B = s.shape[0]
    rows = torch.arange(N)[None, :] < nv.long()[:, None]
    ident = torch.where(rows, torch.arange(N, dtype=torch.int32)[None, :], torch.full((B, N), -1, dtype=torch.int32))
    sd, nvd, labd, rows = s.to(DEV), nv.to(DEV), ident.to(DEV), rows.to(DEV)
    plain = torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV)
    labelled = torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV)
    _lib.call('fgnn_accuracy_max', _lib.ptr(sd), _lib.ptr(nvd), B, N, _lib.ptr(plain), _lib.stream_ptr())
    _lib.call('fgnn_accuracy_max_labels', _lib.ptr(sd), _lib.ptr(labd), _lib.ptr(nvd), B, N, _lib.ptr(labelled), _lib.stream_ptr())
    hits = []
    for lab in (None, labd):
        for entry in ('fgnn_eval_pairs', 'fgnn_eval_pairs_labels')[:1 if lab is None else 2]:
            cost = torch.empty(B, N, N, dtype=torch.float32, device=DEV)
            row_ce = torch.empty(B, N, dtype=torch.float32, device=DEV)
            row_hit = torch.full((B, N), SENTINEL, dtype=torch.int32, device=DEV)
            _lib.call(entry, _lib.ptr(sd), _lib.ptr(nvd), _lib.ptr(lab), B, N, _lib.ptr(cost), N * N, N, _lib.ptr(row_ce), _lib.ptr(row_hit),
                      _lib.stream_ptr())
            hits.append(row_hit == 1)
        hits.append(_ranks(sd, nvd, lab, B, N) == 1)
    for h in hits[1:]:
        assert torch.equal(h & rows, hits[0] & rows)
    count = (hits[0] & rows).sum(1).to(torch.int32)
    assert torch.equal(plain, count) and torch.equal(labelled, count) and int(count.sum()) > 0


# ---------------------------------------------------------------------------------------------------------- layout and cutting
def test_pair_alone_equals_pair_in_batch():
    N, B = 65, 9
    c = RR.case(N, B, True)
    sd, nvd, labd = c['scores'].to(DEV), c['nv'].to(DEV), c['labels']['holes'].to(DEV)
    full = _ranks(sd, nvd, labd, B, N)
    fo = _fold(full, nvd, B, _zeros())
    for b in (0, 1, 4, 8):
        one = _ranks(sd[b:b + 1].contiguous(), nvd[b:b + 1].contiguous(), labd[b:b + 1].contiguous(), 1, N)
        assert torch.equal(one[0], full[b]), b
        oo = _fold(one, nvd[b:b + 1].contiguous(), 1, _zeros())
        assert all(torch.equal(oo[k][0], fo[k][b]) for k in oo), b


def test_live_masks_the_surplus_pairs():
    N, B = 17, 9
    c = RR.case(N, B, True)
    sd, nvd = c['scores'].to(DEV), c['nv'].to(DEV)
    rank = _ranks(sd, nvd, None, B, N)
    for live in (0, 1, 5, 8, 9):
        records = _zeros()
        o = _fold(rank, nvd, live, records)
        assert bool(torch.isnan(o['rr'][live:]).all()) and bool((o['hits'][live:] == SENTINEL).all())
        assert bool((o['rank_sum'][live:] == SENTINEL).all()) and bool((o['targets'][live:] == SENTINEL).all())
        if live == 0:
            assert not bool(records.any())
            continue
        first = _zeros()
        fo = _fold(rank[:live].contiguous(), nvd[:live].contiguous(), live, first)
        assert torch.equal(records, first) and all(torch.equal(o[k][:live], fo[k]) for k in o)
        assert _record(records)['pairs'] == live and _record(records)['steps'] == 1
    # live = 0 on a record that holds something: nothing changes, the step count included
    before = records.clone()
    _fold(rank, nvd, 0, records)
    assert torch.equal(records, before)
    with pytest.raises(RuntimeError, match='fgnn_rank_fold'):
        _fold(rank, nvd, B + 1, records)
    for bad in ((), tuple(range(1, 10)), (2, 2), (0,)):
        with pytest.raises(RuntimeError, match='fgnn_rank_fold'):
            _fold(rank, nvd, B, records, ks=bad)
    with pytest.raises(RuntimeError, match='fgnn_rank_fold'):
        _fold(rank, nvd, B, records, K=2)          # more than one record goes with bins
    assert torch.equal(records, before)


def test_record_does_not_depend_on_how_the_epoch_is_cut():
    """32 examples as 32 x 1, 7 x 5 (a short last step filled with other pairs and masked by live) and 1 x 32"""
    N, M = 17, 32
    g = torch.Generator().manual_seed(5)
    nv = RR.nv_pattern(M, N, g)
    s = ((torch.randn(M, N, N, generator=g) * 8).round() / 4).masked_fill(~RR.corner(nv, N), NAN)
    lab = RR.label_sets(nv, N, g)['holes']
    bufs = []
    for B in (1, 5, 32):
        meter = RankMeter(DEV, ks=KS)
        for lo in range(0, M, B):
            live = min(B, M - lo)
            idx = list(range(lo, lo + live)) + list(range(B - live))          # (the filling: the epoch's first pairs once more)
            out = rank_scores(s[idx].to(DEV), nvalid=nv[idx].to(DEV), labels=lab[idx].to(DEV), meter=meter, live=live)
            assert out['meter'] is meter and out['rank'].shape == (B, N) and out['rr'].dtype == torch.float64
            assert not bool(out['hits'][live:].any()) and not bool(out['rr'][live:].any())
        bufs.append(meter.buf.clone())
        rec = meter.record()
        assert rec['pairs'] == M and rec['steps'] == -(-M // B) and rec['nodes'] == int(nv.sum())
    assert torch.equal(_but_steps(bufs[0]), _but_steps(bufs[1])) and torch.equal(_but_steps(bufs[0]), _but_steps(bufs[2]))
    ref = RR.ranks(s.numpy(), nv.tolist(), lab.numpy())
    sums = [RR.pair_sums(ref[b, :n], KS) for b, n in enumerate(nv.tolist())]
    assert rec['hits'] == {k: sum(p['hits'][q] for p in sums) for q, k in enumerate(KS)}
    assert rec['rank_sum'] == sum(p['rank_sum'] for p in sums) and rec['targets'] == sum(p['targets'] for p in sums)
    res = meter.result()
    assert res['mrr'] == rec['rr_sum'] / rec['targets'] == meter.mrr.item() and res['mean_rank'] == meter.mean_rank.item()
    assert all(res['hits@%d' % k] == rec['hits'][k] / rec['targets'] == meter.hits_at(k).item() for k in KS)
    assert res['targets'] == rec['targets'] < res['nodes'] == rec['nodes'] and res['pairs'] == M
    assert meter.allreduce_().record() == rec            # one rank: the sum over the ranks is the record
    assert not bool(meter.reset().buf.any())


# ---------------------------------------------------------------------------------------------------------- binned records
BINS = [2, 0, 2, 3, 0, 0, 2, -1, 2]          # K = 3: bin 1 stays empty, 3 and -1 lie outside


@pytest.mark.parametrize('N', [5, 17, 70])
def test_binned_fold_equals_plain_folds_byte_for_byte(N):
    B, K = len(BINS), 3
    c = RR.case(N, B, True) if N in RR.NS else None
    g = torch.Generator().manual_seed(N)
    nv = c['nv'] if c else RR.nv_pattern(B, N, g)
    s = c['scores'] if c else ((torch.randn(B, N, N, generator=g) * 8).round() / 4).masked_fill(~RR.corner(nv, N), NAN)
    nvd = nv.to(DEV)
    rank = _ranks(s.to(DEV), nvd, None, B, N)
    bins_d = torch.tensor(BINS, dtype=torch.int32, device=DEV)
    for live in (9, 6, 0):
        records = _zeros(K)
        for call in range(2):          # from zero records, then from what the first call left (steps and rr_sum carry over)
            start = records.clone()
            want = start.clone()
            for j in range(K):
                sel = [b for b in range(live) if BINS[b] == j]
                if sel:
                    idx = torch.tensor(sel, device=DEV)
                    _fold(rank[idx].contiguous(), nvd[idx].contiguous(), len(sel), want[j * REC:(j + 1) * REC])
            o = _fold(rank, nvd, live, records, bins=bins_d, K=K)
            assert torch.equal(records, want), (N, live, call)
            assert torch.equal(records[REC:2 * REC], start[REC:2 * REC])          # the empty bin's bytes are untouched
            plain = _fold(rank, nvd, live, _zeros())
            assert all(torch.equal(o[k], plain[k]) or k == 'rr' for k in o)
            assert torch.equal(o['rr'][:live], plain['rr'][:live]) and bool(torch.isnan(o['rr'][live:]).all())
        if live == 9:
            assert [_record(records, j)['pairs'] for j in range(K)] == [6, 0, 8] and [_record(records, j)['steps'] for j in range(K)] == [2, 0, 2]
    for bad_k in (0, _lib.FGNN_MAX_LEVELS + 1):
        with pytest.raises(RuntimeError, match='fgnn_rank_fold'):
            _fold(rank, nvd, B, records, bins=bins_d, K=bad_k)


def test_binned_meter_through_rank_scores_and_evaluate_scores():
    N, B, K = 17, len(BINS), 3
    c = RR.case(N, B, True)
    s, nv, lab = c['scores'].to(DEV), c['nv'].to(DEV), c['labels']['perm'].to(DEV)
    bins = torch.tensor(BINS, device=DEV)          # (int64: converted on the device)
    values = (0.0, 0.1, 0.2)
    meter = BinnedRankMeter(DEV, K, ks=KS, values=values)
    out = rank_scores(s, nvalid=nv, labels=lab, meter=meter, live=8, bins=bins)
    ref = rank_scores(s, nvalid=nv, labels=lab, live=8, ks=KS)
    assert out['meter'] is meter and len(meter) == K and isinstance(ref['meter'], RankMeter)
    for key in ('rank', 'hits', 'rr', 'rank_sum', 'targets'):
        assert torch.equal(out[key], ref[key]), key
    recs, res = meter.record(), meter.result()
    for j in range(K):
        sel = [b for b in range(8) if BINS[b] == j]
        want = RR.fold_record(ref['rr'].cpu().tolist(), ref['hits'].cpu().tolist(), ref['rank_sum'].cpu().tolist(),
                              ref['targets'].cpu().tolist(), c['nv'].tolist(), sel)
        want['hits'] = dict(zip(KS, want['hits']))
        assert recs[j] == dict(want, noise=values[j]) and meter[j].record() == want
        assert res[j]['noise'] == values[j] and res[j]['pairs'] == len(sel)
        if want['targets']:
            assert res[j]['mrr'] == want['rr_sum'] / want['targets'] == meter[j].mrr.item()
        else:
            assert np.isnan(res[j]['mrr']) and np.isnan(res[j]['hits@1'])
    assert meter.allreduce_().record() == recs
    # evaluate_scores(rank_meter=) with bins: the same records next to the binned EvalMeter's
    m2 = BinnedRankMeter(DEV, K, ks=KS, values=values)
    evaluate_scores(s, nvalid=nv, labels=lab, meter=BinnedEvalMeter(DEV, K), live=8, bins=bins, rank_meter=m2, hungarian=False)
    assert torch.equal(m2.buf, meter.buf)
    assert not bool(meter.reset().buf.any())


# ---------------------------------------------------------------------------------------------------------- plumbing
def test_evaluate_scores_with_a_rank_meter_changes_nothing_else():
    N, B = 17, 9
    c = RR.case(N, B, True)
    s, nv, lab = c['scores'].to(DEV), c['nv'].to(DEV), c['labels']['perm'].to(DEV)
    for kw in ({}, {'labels': lab}, {'labels': lab, 'loss_on_labels': True, 'live': 7}, {'hungarian': False}):
        plain, with_ranks = EvalMeter(DEV), EvalMeter(DEV)
        rm = RankMeter(DEV, ks=KS)
        a = evaluate_scores(s, nvalid=nv, meter=plain, **kw)
        b = evaluate_scores(s, nvalid=nv, meter=with_ranks, rank_meter=rm, **kw)
        assert torch.equal(plain.buf, with_ranks.buf)
        assert set(b) == set(a) | {'ranks'} and b['ranks']['meter'] is rm
        for key in ('ce', 'n', 'correct_max', 'correct_lsap', 'assign'):
            assert (a[key] is None and b[key] is None) or torch.equal(a[key], b[key]), key
        alone = rank_scores(s, nvalid=nv, labels=kw.get('labels'), live=kw.get('live'), ks=KS)
        assert torch.equal(alone['meter'].buf, rm.buf) and torch.equal(alone['rank'], b['ranks']['rank'])
        live = kw.get('live', B)
        assert torch.equal(b['ranks']['hits'][:live, 0], b['correct_max'][:live])          # Hits@1 is the arg-max count
        assert rm.record()['hits'][1] == with_ranks.record()['correct_max']


LAY = ParamLayout(2, 4, 32, 32, 3)
N_TR, M_TR, B_TR = 20, 40, 16


def _gen(N, seed=11, noise=0.05):
    return PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=noise, seed=seed, device=DEV)


def _state(tr):
    return [t.clone() for t in (tr.params, tr.grads, tr.opt.exp_avg, tr.opt.exp_avg_sq, tr.opt._dev_state()[1][0:1])]


def _trained(N):
    tr = FgnnTrainer(LAY, LAY.init_flat(7, DEV), lr=2e-3)
    tr.train_step_bits(*_gen(N).bits(0, 4)[:2])          # (gradients and optimizer state that are not zero)
    return tr


@pytest.mark.parametrize('permute', [False, True])
def test_evaluate_with_a_rank_meter_counts_every_example_once(permute):
    tr, gen = _trained(N_TR), _gen(N_TR, seed=3)
    before = _state(tr)
    meter, rm = EvalMeter(DEV), RankMeter(DEV, ks=(1, 5))
    assert tr.evaluate(gen, EpochSampler(M_TR, shuffle=False), B_TR, hungarian=False, permute=permute, meter=meter, rank_meter=rm) is meter
    rec, ev = rm.record(), meter.record()
    print('evaluate permute %d: %r\n  %r' % (permute, rec, ev))
    assert rec['pairs'] == M_TR and rec['steps'] == 3 and rec['targets'] == rec['nodes'] == M_TR * N_TR
    assert rec['hits'][1] == ev['correct_max'] and rec['hits'][1] <= rec['hits'][5] <= rec['targets']
    assert rec['targets'] <= rec['rank_sum'] <= rec['targets'] * N_TR and rec['hits'][1] <= rec['rr_sum'] <= rec['targets']
    # without the rank meter: the same EvalMeter record; batches of 1: the same rank record apart from its step count
    assert torch.equal(tr.evaluate(gen, EpochSampler(M_TR, shuffle=False), B_TR, hungarian=False, permute=permute).buf, meter.buf)
    one = RankMeter(DEV, ks=(1, 5))
    tr.evaluate(gen, EpochSampler(M_TR, shuffle=False), 1, hungarian=False, permute=permute, rank_meter=one)
    assert torch.equal(_but_steps(one.buf), _but_steps(rm.buf)) and one.record()['steps'] == M_TR
    assert all(torch.equal(x, y) for x, y in zip(before, _state(tr))) and tr.opt.t == 1
    with pytest.raises(ValueError, match='rank_meter'):
        tr.evaluate(gen, EpochSampler(M_TR, shuffle=False), B_TR, rank_meter=BinnedRankMeter(DEV, 2))


def test_noise_curve_with_a_binned_rank_meter_equals_separate_epochs():
    N, M, TB = 16, 5, 4
    noises = (0.0, 0.2, 0.5)
    tr, gen = _trained(N), _gen(N)
    before = _state(tr)
    rm = BinnedRankMeter(DEV, len(noises), ks=(1, 5), values=noises)
    meter = tr.noise_curve(gen, noises, M, TB, hungarian=False, rank_meter=rm)
    assert torch.equal(meter.buf, tr.noise_curve(gen, noises, M, TB, hungarian=False).buf)
    recs = rm.record()
    for j, v in enumerate(noises):
        one = RankMeter(DEV, ks=(1, 5))
        tr.evaluate(_gen(N, noise=v), EpochSampler(M, shuffle=False), TB, hungarian=False, rank_meter=one)
        want = one.record()
        print('level %d: curve %r\n         epoch %r' % (j, recs[j], want))
        assert recs[j] == dict(want, noise=v, steps=recs[j]['steps']) and recs[j]['pairs'] == M and recs[j]['targets'] == M * N
        assert torch.equal(_but_steps(rm[j].buf), _but_steps(one.buf))
    assert [r['noise'] for r in rm.result()] == list(noises)
    assert all(torch.equal(x, y) for x, y in zip(before, _state(tr)))
    with pytest.raises(ValueError, match='rank_meter'):
        tr.noise_curve(gen, noises, M, TB, rank_meter=RankMeter(DEV))


def test_fit_reports_hits_and_mrr_when_asked():
    N, B = 16, 4
    old_keys = {'epoch', 'train_losses', 'val_loss', 'val_acc', 'val_acc_max', 'lr'}
    hists = []
    for kw in ({}, {'rank_ks': (1, 5)}):
        tr = FgnnTrainer(LAY, LAY.init_flat(7, DEV), lr=1e-3)
        hists.append(tr.fit(_gen(N, seed=1), EpochSampler(8, seed=1), _gen(N, seed=2), EpochSampler(6, shuffle=False), epochs=2,
                            batch_size=B, **kw))
        assert tr.opt.t == 4
    plain, ranked = hists
    assert all(set(h) == old_keys for h in plain) and all(set(h) == old_keys | {'val_hits', 'val_mrr'} for h in ranked)
    for h, p in zip(ranked, plain):
        assert all(h[k] == p[k] for k in ('epoch', 'val_loss', 'val_acc', 'val_acc_max', 'lr')) and torch.equal(h['train_losses'], p['train_losses'])
        assert set(h['val_hits']) == {1, 5} and h['val_hits'][1] == h['val_acc_max'] <= h['val_hits'][5] <= 1.0
        assert h['val_hits'][1] <= h['val_mrr'] <= 1.0


# ---------------------------------------------------------------------------------------------------------- refusals
def test_rank_scores_refuses_what_it_cannot_run():
    s = torch.zeros(2, 4, 4, device=DEV)
    with pytest.raises(RuntimeError, match='GPU only'):
        rank_scores(torch.zeros(2, 4, 4))
    with pytest.raises(RuntimeError, match='GPU'):
        RankMeter('cpu')
    with pytest.raises(ValueError, match='rank meter'):
        rank_scores(s, meter={})
    with pytest.raises(ValueError, match='rank meter'):
        rank_scores(s, meter=EvalMeter(DEV))
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match='rank meter'):
            rank_scores(s, meter=RankMeter('cuda:1'))
    other = RankMeter(DEV)
    other.buf = other.buf.cpu()          # (a meter whose record is not on the scores' device)
    with pytest.raises(ValueError, match='rank meter'):
        rank_scores(s, meter=other)
    bins = torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match='go together'):
        rank_scores(s, bins=bins)
    with pytest.raises(ValueError, match='go together'):
        rank_scores(s, meter=RankMeter(DEV), bins=bins)
    with pytest.raises(ValueError, match='go together'):
        rank_scores(s, meter=BinnedRankMeter(DEV, 2))
    with pytest.raises(ValueError, match='go together'):
        evaluate_scores(s, rank_meter=BinnedRankMeter(DEV, 2))
    with pytest.raises(ValueError, match='differ'):
        rank_scores(s, meter=RankMeter(DEV, ks=(1, 5)), ks=(1, 3))
    with pytest.raises(ValueError, match='ks'):
        rank_scores(s, ks=(3, 1))
    with pytest.raises(ValueError, match='live'):
        rank_scores(s, live=3)
    with pytest.raises(ValueError, match='nvalid'):
        rank_scores(s, nvalid=torch.zeros(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match='bins'):
        rank_scores(s, meter=BinnedRankMeter(DEV, 2), bins=torch.zeros(3, dtype=torch.int32, device=DEV))
    out = rank_scores(s, meter=RankMeter(DEV, ks=(1, 5)), ks=(1, 5))
    assert out['rank'].tolist() == [[1, 2, 3, 4]] * 2 and out['meter'].ks == (1, 5)          # a constant row ranks by the index
    res = out['meter'].result()
    assert abs(res.pop('mrr') - (1 + 1 / 2 + 1 / 3 + 1 / 4) / 4) <= 1e-15          # (four terms in the butterfly's order)
    assert res == {'hits@1': 0.25, 'hits@5': 1.0, 'mean_rank': 2.5, 'targets': 8, 'nodes': 8, 'pairs': 2}
