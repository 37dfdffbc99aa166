"""GPU: one epoch record per bin (fgnn_eval_fold_bins, BinnedEvalMeter, evaluate_scores(bins=)) and FgnnTrainer.noise_curve.
The binned fold is defined by the plain one: record k ends with the bytes fgnn_eval_fold leaves after folding just the live pairs
of bin k, in their order, into the same starting record -- every comparison here is byte or bit equality."""
import ctypes

import pytest
import torch

import eval_ref as R
from graph_neural_net_amd import _lib
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.evaluation import BinnedEvalMeter, EvalMeter, evaluate_scores
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.sampler import EpochSampler
from graph_neural_net_amd.trainer import FgnnTrainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
SENTINEL = -77
REC = ctypes.sizeof(_lib.EvalRecord)
B, K = 9, 4
BINS = [2, 0, 2, 3, 0, 0, 2, 3, 2]          # bin 1 stays empty


def _rows(N, ragged):
    """row_ce, row_hit of one fgnn_eval_pairs launch on eval_ref scores (rows past n_b keep NaN / the sentinel), nvalid, correct"""
    g = torch.Generator().manual_seed(100 * N + ragged)
    nv = R.nv_pattern(B, N, g) if ragged else torch.full((B,), N, dtype=torch.int32)          # ragged: N, 0, 1, then random
    sd = R.make_scores(B, N, nv, g).to(DEV)
    nvd = nv.to(DEV) if ragged else None
    cost = torch.full((B, N, N), NAN, dtype=torch.float32, device=DEV)
    row_ce = torch.full((B, N), NAN, dtype=torch.float32, device=DEV)
    row_hit = torch.full((B, N), SENTINEL, dtype=torch.int32, device=DEV)
    _lib.call('fgnn_eval_pairs', _lib.ptr(sd), _lib.ptr(nvd), None, B, N, _lib.ptr(cost), N * N, N, _lib.ptr(row_ce), _lib.ptr(row_hit),
              _lib.stream_ptr())
    correct = torch.randint(0, N + 1, (B,), generator=g, dtype=torch.int32).to(DEV)
    return row_ce, row_hit, nvd, correct


def _fold(row_ce, row_hit, correct, nvd, live, record):
    """fgnn_eval_fold of the first `live` pairs into `record` (48 bytes on the device) -> pair_ce, pair_max"""
    n, N = row_ce.shape
    pair_ce = torch.full((n,), NAN, dtype=torch.float64, device=DEV)
    pair_max = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    _lib.call('fgnn_eval_fold', _lib.ptr(row_ce), _lib.ptr(row_hit), _lib.ptr(correct), _lib.ptr(nvd), n, N, live, _lib.ptr(pair_ce),
              _lib.ptr(pair_max), _lib.ptr(record), _lib.stream_ptr())
    return pair_ce, pair_max


def _fold_bins(row_ce, row_hit, correct, nvd, live, bins, k, records):
    n, N = row_ce.shape
    pair_ce = torch.full((n,), NAN, dtype=torch.float64, device=DEV)
    pair_max = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    _lib.call('fgnn_eval_fold_bins', _lib.ptr(row_ce), _lib.ptr(row_hit), _lib.ptr(correct), _lib.ptr(nvd), n, N, live, _lib.ptr(bins), k,
              _lib.ptr(pair_ce), _lib.ptr(pair_max), _lib.ptr(records), _lib.stream_ptr())
    return pair_ce, pair_max


def _expected(row_ce, row_hit, correct, nvd, live, bins, k, start):
    """the K records the defining property asks for: per bin a plain fold of its live pairs, in order, into a copy of `start`"""
    want = start.clone()
    for j in range(k):
        sel = [b for b in range(live) if bins[b] == j]
        if sel:
            idx = torch.tensor(sel, device=DEV)
            _fold(row_ce[idx].contiguous(), row_hit[idx].contiguous(), None if correct is None else correct[idx].contiguous(),
                  None if nvd is None else nvd[idx].contiguous(), len(sel), want[j * REC:(j + 1) * REC])
    return want


def _check_bins(N, ragged, bins, k):
    row_ce, row_hit, nvd, correct = _rows(N, ragged)
    bins_d = torch.tensor(bins, dtype=torch.int32, device=DEV)
    for lsap in (correct, None):
        for live in (9, 6, 0):
            records = torch.zeros(k * REC, dtype=torch.uint8, device=DEV)
            for call in range(2):          # from zero records, then from what the first call left (steps and ce_sum carry over)
                start = records.clone()
                want = _expected(row_ce, row_hit, lsap, nvd, live, bins, k, start)
                pair_ce, pair_max = _fold_bins(row_ce, row_hit, lsap, nvd, live, bins_d, k, records)
                assert torch.equal(records, want), (N, ragged, live, call, lsap is not None)
                for j in range(k):
                    if not any(bins[b] == j for b in range(live)):          # an empty bin's bytes do not change
                        assert torch.equal(records[j * REC:(j + 1) * REC], start[j * REC:(j + 1) * REC])
                ref_ce, ref_max = _fold(row_ce, row_hit, lsap, nvd, live, torch.zeros(REC, dtype=torch.uint8, device=DEV))
                assert torch.equal(pair_ce[:live], ref_ce[:live]) and torch.equal(pair_max[:live], ref_max[:live])
                assert bool(torch.isnan(pair_ce[live:]).all()) and bool((pair_max[live:] == SENTINEL).all())
            if live == 9 and k == K:
                rec = (_lib.EvalRecord * k).from_buffer_copy(records.cpu().numpy().tobytes())
                assert [r.pairs for r in rec] == [2 * bins.count(j) for j in range(k)] and [r.steps for r in rec] == [2, 0, 2, 2]
    return records


@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('N', [5, 17, 70])
def test_binned_fold_equals_plain_folds_byte_for_byte(N, ragged):
    _check_bins(N, ragged, BINS, K)


@pytest.mark.parametrize('N', [5, 70])
def test_one_bin_is_the_plain_fold(N):
    row_ce, row_hit, nvd, correct = _rows(N, True)
    zeros = torch.zeros(B, dtype=torch.int32, device=DEV)
    plain = torch.zeros(REC, dtype=torch.uint8, device=DEV)
    binned = torch.zeros(REC, dtype=torch.uint8, device=DEV)
    for live in (9, 6, 0, 9):
        p = _fold(row_ce, row_hit, correct, nvd, live, plain)
        q = _fold_bins(row_ce, row_hit, correct, nvd, live, zeros, 1, binned)
        assert torch.equal(plain, binned) and torch.equal(p[0][:live], q[0][:live]) and torch.equal(p[1][:live], q[1][:live])
    assert EvalMeter(DEV, buf=binned).record()['steps'] == 3


def _start_records(k):
    """k records that are not zero, record j = 1 the same for every k (ce_sum is not exactly representable)"""
    recs = (_lib.EvalRecord * k)()
    for j in range(k):
        q = 1 if k == 1 else j
        recs[j].ce_sum = 0.1 + q / 3.0
        recs[j].nodes, recs[j].correct_lsap, recs[j].correct_max, recs[j].pairs, recs[j].steps = 1000 + q, 500 + q, 400 + q, 30 + q, 7 + q
    return torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(DEV)


@pytest.mark.parametrize('N', [1, 64, 65])          # (a lane adds the rows l, l + 64, ...)
@pytest.mark.parametrize('nb', [1, 4, 5, 9])          # (a chunk is four pairs)
def test_the_plain_fold_is_the_binned_fold_at_the_shape_edges(nb, N):
    """fgnn_eval_fold, fgnn_eval_fold_bins with K = 1 and with K = 3 and every pair in bin 1 are one kernel: the same record bytes,
    pair_ce and pair_max from a record that is not zero; live = 0 leaves every byte, and the other bins' records always stay"""
    g = torch.Generator().manual_seed(1000 * nb + N)
    nv = torch.randint(1, N + 1, (nb,), generator=g, dtype=torch.int32)
    nv[0] = N
    nv[min(1, nb - 1)] = 0          # (ragged, one pair without vertices; with one pair, that one)
    for nvalid in ([nv] if nb > 1 else [nv, torch.tensor([N], dtype=torch.int32)]):
        inside = torch.arange(N)[None, :] < nvalid[:, None]
        row_ce = torch.where(inside, torch.rand(nb, N, generator=g) * 7.0, torch.full((nb, N), NAN)).to(DEV)
        row_hit = torch.where(inside, torch.randint(0, 2, (nb, N), generator=g, dtype=torch.int32),
                              torch.full((nb, N), SENTINEL, dtype=torch.int32)).to(DEV)
        correct = torch.randint(0, N + 1, (nb,), generator=g, dtype=torch.int32).to(DEV)
        nvd = nvalid.to(DEV)
        for live in sorted({0, nb - 1, nb}):
            plain, one, three = _start_records(1), _start_records(1), _start_records(3)
            assert torch.equal(plain, three[REC:2 * REC])
            p = _fold(row_ce, row_hit, correct, nvd, live, plain)
            q = _fold_bins(row_ce, row_hit, correct, nvd, live, torch.zeros(nb, dtype=torch.int32, device=DEV), 1, one)
            r = _fold_bins(row_ce, row_hit, correct, nvd, live, torch.ones(nb, dtype=torch.int32, device=DEV), 3, three)
            assert torch.equal(plain, one) and torch.equal(plain, three[REC:2 * REC]), (live, nvalid.tolist())
            assert torch.equal(three[:REC], _start_records(3)[:REC]) and torch.equal(three[2 * REC:], _start_records(3)[2 * REC:])
            for other in (q, r):          # (NaN / the sentinel past `live` in all three: compared as bits)
                assert torch.equal(p[0].view(torch.int64), other[0].view(torch.int64)) and torch.equal(p[1], other[1])
            assert bool(torch.isnan(p[0][live:]).all()) and bool((p[1][live:] == SENTINEL).all())
            if live == 0:
                assert torch.equal(plain, _start_records(1))
            else:
                rec = _lib.EvalRecord.from_buffer_copy(plain.cpu().numpy().tobytes())
                assert (rec.pairs, rec.steps, rec.nodes) == (31 + live, 9, 1001 + int(nvalid[:live].sum()))


@pytest.mark.parametrize('N', [17])
def test_a_bin_outside_the_records_is_ignored(N):
    bins = list(BINS)
    bins[1], bins[5] = -1, K
    _check_bins(N, True, bins, K)
    # ... which is what masking those pairs out gives: the same records as a batch without them
    row_ce, row_hit, nvd, correct = _rows(N, True)
    keep = [b for b in range(B) if 0 <= bins[b] < K]
    idx = torch.tensor(keep, device=DEV)
    a = torch.zeros(K * REC, dtype=torch.uint8, device=DEV)
    b = torch.zeros(K * REC, dtype=torch.uint8, device=DEV)
    _fold_bins(row_ce, row_hit, correct, nvd, B, torch.tensor(bins, dtype=torch.int32, device=DEV), K, a)
    _fold_bins(row_ce[idx].contiguous(), row_hit[idx].contiguous(), correct[idx].contiguous(), nvd[idx].contiguous(), len(keep),
               torch.tensor([bins[i] for i in keep], dtype=torch.int32, device=DEV), K, b)
    assert torch.equal(a, b)
    for bad_k in (0, 65):
        with pytest.raises(RuntimeError, match='fgnn_eval_fold_bins'):
            _fold_bins(row_ce, row_hit, correct, nvd, B, torch.zeros(B, dtype=torch.int32, device=DEV), bad_k, a)


def test_binned_meter_through_evaluate_scores():
    """evaluate_scores(bins=) is evaluate_scores with another fourth launch: the same per-pair tensors, the meter's views and dicts"""
    N = 17
    c = R.case(N, 32, True)
    s, nv, lab = c['scores'][:B].to(DEV), c['nv'][:B].to(DEV), c['labels'][:B].to(DEV)
    bins = torch.tensor(BINS, device=DEV)          # (int64: converted on the device)
    values = (0.0, 0.1, 0.2, 0.3)
    meter = BinnedEvalMeter(DEV, K, values=values)
    out = evaluate_scores(s, nvalid=nv, labels=lab, meter=meter, live=7, bins=bins)
    ref = evaluate_scores(s, nvalid=nv, labels=lab, live=7)
    assert out['meter'] is meter and len(meter) == K
    for key in ('ce', 'n', 'correct_max', 'correct_lsap', 'assign'):
        assert torch.equal(out[key], ref[key]), key
    recs, res = meter.record(), meter.result()
    ce, n, cmax, clsap = (ref[k].cpu().tolist() for k in ('ce', 'n', 'correct_max', 'correct_lsap'))
    for j in range(K):
        sel = [b for b in range(7) if BINS[b] == j]
        want = R.fold_record([ce[b] for b in sel], [n[b] for b in sel], [clsap[b] for b in sel], [cmax[b] for b in sel], len(sel))
        assert recs[j] == dict(want, noise=values[j]) and meter[j].record() == want
        assert res[j]['noise'] == values[j] and res[j]['pairs'] == len(sel)
        if want['nodes']:
            assert res[j]['loss'] == want['ce_sum'] / want['nodes'] == meter[j].loss.item()
            assert meter[j].acc.item() == res[j]['acc'] and meter[j].acc_max.item() == res[j]['acc_max']
    assert sum(r['pairs'] for r in recs) == 7
    assert meter.allreduce_().record() == recs          # one rank: the sum is the record
    assert not bool(meter.reset().buf.any())
    with pytest.raises(ValueError, match='bins'):
        evaluate_scores(s, meter=meter, bins=torch.zeros(B + 1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match='go together'):
        evaluate_scores(s, meter=meter)
    with pytest.raises(ValueError, match='go together'):
        evaluate_scores(s, meter=EvalMeter(DEV), bins=bins)


# ---------------------------------------------------------------------------------------------------------- noise_curve
LAY = ParamLayout(2, 2, 32, 32, 3)
NOISES = (0.0, 0.2, 0.5)
N_CURVE, M, TB = 16, 5, 4


def _trainer(precision):
    # (the 16-bit engine takes bit-packed input through the structured block 1 only; fp32 runs the generic kernels)
    tr = FgnnTrainer(LAY, LAY.init_flat(5, DEV), lr=2e-3, precision=precision, block1='structured' if precision == 'bf16' else None)
    gen = PairGenerator(N_CURVE, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.05, seed=11, device=DEV)
    tr.train_step_bits(*gen.bits(0, TB)[:2])          # (gradients and optimizer state that are not zero)
    return tr, gen


def _state(tr):
    return [t.clone() for t in (tr.params, tr.grads, tr.opt.exp_avg, tr.opt.exp_avg_sq, tr.opt._dev_state()[1][0:1])]


def _by_hand(tr, gen, rank=0, world=1, **kw):
    """the records of noise_curve from its batches made by hand: each through eval_step_bits with a fresh plain meter, the per-pair
    tensors read back and added per level in pair order on the host"""
    lv = gen.levels(NOISES)
    k = len(NOISES)
    smp = EpochSampler(k * M, shuffle=False, rank=rank, world_size=world, device=DEV)
    recs = [R.fold_record([], [], [], [], 0) for _ in range(k)]
    gkw = {'permute': True} if kw.get('permute') else {}
    for step in range(smp.steps_per_epoch(TB)):
        e = smp.batch_index(0, step, TB)
        live = smp.live_count(step, TB)
        if live == 0:
            continue
        level = e // M
        b1, b2, nv, *labels = gen.bits(index=e % M, levels=lv, level=level, **gkw)
        out = tr.eval_step_bits(b1, b2, nvalid=nv, labels=labels[0] if labels else None, meter=EvalMeter(DEV), live=live,
                                hungarian=True, loss_on_labels=bool(kw.get('loss_on_labels')))
        ce, n, cmax, clsap = (out[key].cpu().tolist() for key in ('ce', 'n', 'correct_max', 'correct_lsap'))
        lev = level.cpu().tolist()
        for j in range(k):
            sel = [b for b in range(live) if lev[b] == j]
            recs[j] = R.fold_record([ce[b] for b in sel], [n[b] for b in sel], [clsap[b] for b in sel], [cmax[b] for b in sel], len(sel),
                                    start=recs[j])
    return recs


@pytest.mark.parametrize('kw', [{}, {'permute': True, 'loss_on_labels': True}], ids=['identity', 'planted'])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_noise_curve_end_to_end(precision, kw):
    tr, gen = _trainer(precision)
    before = _state(tr)
    meter = tr.noise_curve(gen, NOISES, M, TB, hungarian=True, **kw)
    assert isinstance(meter, BinnedEvalMeter) and len(meter) == len(NOISES)
    recs = meter.record()
    want = _by_hand(tr, gen, **kw)
    print('noise_curve %s %r:\n  %r\n  by hand %r' % (precision, kw, recs, want))
    for j, v in enumerate(NOISES):
        assert recs[j] == dict(want[j], noise=v), j          # all six fields, ce_sum bit for bit
        assert recs[j]['pairs'] == M and recs[j]['nodes'] == M * N_CURVE
    # 15 examples in steps of 4: level 0 lives in steps 0, 1; level 1 in 1, 2; level 2 in 2, 3
    assert [r['steps'] for r in recs] == [2, 2, 2]
    res = meter.result()
    assert [r['noise'] for r in res] == list(NOISES) and all(r['loss'] == rec['ce_sum'] / rec['nodes'] for r, rec in zip(res, recs))
    assert all(torch.equal(x, y) for x, y in zip(before, _state(tr))) and tr.opt.t == 1
    # a meter of the caller's accumulates
    assert tr.noise_curve(gen, NOISES, M, TB, meter=meter, **kw) is meter
    again = meter.record()
    assert all(again[j][f] == 2 * recs[j][f] for j in range(len(NOISES)) for f in ('nodes', 'correct_lsap', 'correct_max', 'pairs', 'steps'))
    with pytest.raises(ValueError, match='meter'):
        tr.noise_curve(gen, NOISES, M, TB, meter=BinnedEvalMeter(DEV, 2))


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_noise_curve_equals_single_noise_epochs(precision):
    """a pair's scores do not depend on the batch around it: a level's record is the record of an
    `evaluate` epoch of a generator of that single noise value over the same pairs, ce_sum bit for bit (`steps` aside)"""
    tr, gen = _trainer(precision)
    recs = tr.noise_curve(gen, NOISES, M, TB).record()
    for j, v in enumerate(NOISES):
        one = PairGenerator(N_CURVE, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=v, seed=11, device=DEV)
        want = tr.evaluate(one, EpochSampler(M, shuffle=False), TB).record()
        print('level %d: curve %r\n         epoch %r' % (j, recs[j], want))
        assert all(recs[j][f] == want[f] for f in ('ce_sum', 'nodes', 'correct_lsap', 'correct_max', 'pairs')), j


def test_noise_curve_with_a_generator_on_the_current_device():
    tr, gen = _trainer('fp32')
    here = PairGenerator(N_CURVE, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.05, seed=11, device='cuda')
    assert tr.noise_curve(here, NOISES, M, TB).record() == tr.noise_curve(gen, NOISES, M, TB).record()


def test_noise_curve_rank_split():
    tr, gen = _trainer('fp32')
    whole = tr.noise_curve(gen, NOISES, M, TB).record()
    parts = [tr.noise_curve(gen, NOISES, M, TB, rank=r, world_size=2).record() for r in range(2)]
    for r in range(2):
        assert parts[r] == [dict(w, noise=v) for w, v in zip(_by_hand(tr, gen, rank=r, world=2), NOISES)]
    for j in range(len(NOISES)):
        for f in ('nodes', 'correct_lsap', 'correct_max', 'pairs'):
            assert parts[0][j][f] + parts[1][j][f] == whole[j][f], (j, f)
        ce, ce0, ce1 = whole[j]['ce_sum'], parts[0][j]['ce_sum'], parts[1][j]['ce_sum']
        # non-negative terms: the re-association bound of an fp64 sum of `pairs` terms
        print('level %d: ce %r, ce0 + ce1 - ce = %r' % (j, ce, ce0 + ce1 - ce))
        assert abs(ce0 + ce1 - ce) <= whole[j]['pairs'] * 2.0 ** -52 * ce
