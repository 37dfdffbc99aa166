"""Host: the rank reference of tests/rank_ref.py against np.argmax and plain counting, metrics.match_ranks / hits_at_k on CPU tensors
against the reference, the packing of the rank meters' all-reduce and the validation of the thresholds."""
import ctypes

import numpy as np
import pytest
import torch

import rank_ref as RR
from graph_neural_net_amd import _lib, metrics
from graph_neural_net_amd.evaluation import (RANK_WORDS, check_ks, pack_rank_records, pack_records, rank_record_dict, rank_result,
                                             unpack_rank_records_, unpack_records_)
from graph_neural_net_amd.masked import MaskedTensor


def test_reference_on_distinct_scores_counts_the_larger_ones():
    g = np.random.default_rng(3)
    for n in (1, 2, 7, 33):
        blk = g.permutation(n * n).reshape(n, n).astype(np.float32)          # distinct everywhere
        want = g.integers(0, n, n)
        r = RR.rank_rows(blk, want)
        assert np.array_equal(r, 1 + (blk > blk[np.arange(n), want][:, None]).sum(1))
        assert np.array_equal(r == 1, np.argmax(blk, 1) == want)
        assert np.array_equal(r, RR.rank_rows_scalar(blk, want))


@pytest.mark.parametrize('N', [5, 16, 17, 64, 65, 130])
def test_reference_rank_one_is_np_argmax_on_the_adversarial_rows(N):
    g = torch.Generator().manual_seed(N)
    s, nv = RR.adversarial(N, g)
    labs = RR.label_sets(nv, N, g)
    for name, lab in labs.items():
        for b, n in enumerate(nv.tolist()):
            blk = s[b, :n, :n].numpy()
            want = np.arange(n) if lab is None else lab[b, :n].numpy()
            r = RR.rank_rows(blk, want)
            assert np.array_equal(r == 1, np.argmax(blk, 1) == want), (name, b)
            assert np.array_equal(r == 0, (want < 0) | (want >= n))
            if N <= 17:
                assert np.array_equal(r, RR.rank_rows_scalar(blk, want)), (name, b)
    # a row of one value ranks its target by its index; a row of -inf likewise; -0.0 ties with +0.0
    assert RR.rank_rows(np.full((4, 4), 2.0, np.float32), np.arange(4)).tolist() == [1, 2, 3, 4]
    assert RR.rank_rows(np.full((3, 3), -np.inf, np.float32), [2, 0, 1]).tolist() == [3, 1, 2]
    assert RR.rank_rows(np.array([[0.0, -0.0], [-0.0, 0.0]], np.float32), [1, 0]).tolist() == [2, 1]
    # NaN above every number, the first NaN first; a number sees every NaN above it
    row = np.array([[1.0, np.nan, 5.0, np.nan]] * 4, np.float32)
    assert RR.rank_rows(row, [0, 1, 2, 3]).tolist() == [4, 1, 3, 2]


@pytest.mark.parametrize('N,B', [(5, 3), (17, 5), (65, 3)])
def test_match_ranks_and_hits_at_k_on_cpu_tensors(N, B):
    c = RR.case(N, B, True)
    nv = c['nv']
    for name, lab in c['labels'].items():
        ref = c['ref'][name]
        got = metrics.match_ranks(MaskedTensor(c['scores'], nv, (1, 2)), labels=lab)
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), ref['rank']), name
        for q, k in enumerate(RR.KS):
            hits = [p['hits'][q] for p in ref['pairs']]
            assert metrics.hits_at_k(MaskedTensor(c['scores'], nv, (1, 2)), k, labels=lab) == (sum(hits), int(nv.sum()))
            per = metrics.hits_at_k(MaskedTensor(c['scores'], nv, (1, 2)), k, labels=lab, aggregate_score=False)
            assert all((np.isnan(a) and n == 0) or a == h / n for a, h, n in zip(per, hits, nv.tolist()))
    # dense, and the reference's list of per-graph label arrays; k = 1 is accuracy_max
    d = RR.case(N, B, False)
    lab = d['labels']['perm']
    assert np.array_equal(metrics.match_ranks(d['scores'], labels=[row for row in lab]).numpy(), d['ref']['perm']['rank'])
    assert np.array_equal(metrics.match_ranks(d['scores']).numpy(), d['ref']['identity']['rank'])
    assert metrics.hits_at_k(d['scores'], 1, labels=lab) == metrics.accuracy_max(d['scores'], labels=lab)
    with pytest.raises(ValueError, match='k must be'):
        metrics.hits_at_k(d['scores'], 0)


def test_adversarial_rows_through_the_host_route():
    N = 17
    g = torch.Generator().manual_seed(N)
    s, nv = RR.adversarial(N, g)
    for lab in RR.label_sets(nv, N, g).values():
        got = metrics.match_ranks(MaskedTensor(s, nv, (1, 2)), labels=lab)
        assert np.array_equal(got.numpy(), RR.ranks(s.numpy(), nv.tolist(), None if lab is None else lab.numpy()))


def test_allreduce_packing_round_trips():
    assert ctypes.sizeof(_lib.RankRecord) == 8 * RANK_WORDS == 8 * (6 + _lib.FGNN_RANK_MAX_K)
    K = 3
    recs = (_lib.RankRecord * K)()
    for j in range(K):
        recs[j].rr_sum = 0.1 + j / 3.0          # (not exactly representable: the bits must survive)
        recs[j].rank_sum, recs[j].targets, recs[j].nodes, recs[j].pairs, recs[j].steps = 10 ** 12 + j, 2 ** 52 - j, 17 * j, j, 3
        for q in range(_lib.FGNN_RANK_MAX_K):
            recs[j].hits[q] = 1000 * j + q
    raw = bytes(recs)
    buf = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
    t = pack_rank_records(buf, K)
    assert t.shape == (K, RANK_WORDS) and t.dtype == torch.float64
    assert t[1].tolist() == [0.1 + 1 / 3.0, 10 ** 12 + 1, 2 ** 52 - 1, 17, 1, 3] + [1000 + q for q in range(8)]
    back = unpack_rank_records_(torch.zeros(K * 8 * RANK_WORDS, dtype=torch.uint8), K, t)
    assert bytes(back.numpy().tobytes()) == raw
    # two ranks: the sum of the packed vectors is the record of the sums
    both = unpack_rank_records_(torch.zeros(K * 8 * RANK_WORDS, dtype=torch.uint8), K, t + t)
    two = (_lib.RankRecord * K).from_buffer_copy(both.numpy().tobytes())
    assert two[2].rank_sum == 2 * recs[2].rank_sum and two[2].hits[7] == 2 * recs[2].hits[7] and two[2].rr_sum == 2 * recs[2].rr_sum
    rec = rank_record_dict(two[1], (1, 5))
    assert rec['hits'] == {1: 2000, 5: 2002} and rec['targets'] == 2 * (2 ** 52 - 1)
    # the rank pair is the generic one at 14 words ...
    assert torch.equal(pack_records(buf, K, RANK_WORDS), t)
    assert unpack_records_(torch.zeros(K * 8 * RANK_WORDS, dtype=torch.uint8), K, t).numpy().tobytes() == raw
    # ... which packs the evaluation record, 6 words, by the same rule
    words = ctypes.sizeof(_lib.EvalRecord) // 8
    evs = (_lib.EvalRecord * K)()
    for j in range(K):
        evs[j].ce_sum = 0.1 + j / 3.0
        evs[j].nodes, evs[j].correct_lsap, evs[j].correct_max, evs[j].pairs, evs[j].steps = 2 ** 52 - j, 2 ** 52 - 7 * j - 1, 10 ** 12 + j, j, 3
    eraw = bytes(evs)
    et = pack_records(torch.frombuffer(bytearray(eraw), dtype=torch.uint8), K, words)
    assert words == 6 and et.shape == (K, 6) and et.dtype == torch.float64
    assert et[2].tolist() == [0.1 + 2 / 3.0, 2 ** 52 - 2, 2 ** 52 - 15, 10 ** 12 + 2, 2, 3]
    assert unpack_records_(torch.zeros(K * 8 * words, dtype=torch.uint8), K, et).numpy().tobytes() == eraw
    etwo = (_lib.EvalRecord * K).from_buffer_copy(unpack_records_(torch.zeros(K * 8 * words, dtype=torch.uint8), K, et + et).numpy().tobytes())
    for j in range(K):
        assert etwo[j].ce_sum == 2 * evs[j].ce_sum
        assert all(getattr(etwo[j], n) == 2 * getattr(evs[j], n) for n in ('nodes', 'correct_lsap', 'correct_max', 'pairs', 'steps'))
    res = rank_result({'rr_sum': 3.0, 'rank_sum': 12, 'targets': 4, 'nodes': 5, 'pairs': 1, 'steps': 1, 'hits': {1: 2, 5: 4}})
    assert res == {'hits@1': 0.5, 'hits@5': 1.0, 'mrr': 0.75, 'mean_rank': 3.0, 'targets': 4, 'nodes': 5, 'pairs': 1}
    empty = rank_result({'rr_sum': 0.0, 'rank_sum': 0, 'targets': 0, 'nodes': 3, 'pairs': 1, 'steps': 1, 'hits': {1: 0}})
    assert np.isnan(empty['hits@1']) and np.isnan(empty['mrr']) and np.isnan(empty['mean_rank']) and empty['nodes'] == 3


def test_thresholds_are_validated():
    assert check_ks([1, 5, 10]) == (1, 5, 10) and check_ks((3,)) == (3,) and check_ks(range(1, 9)) == tuple(range(1, 9))
    for bad in ((), tuple(range(1, 10)), (1, 1), (5, 1), (0, 1), (-1,), (1.5,), 3):
        with pytest.raises(ValueError, match='ks'):
            check_ks(bad)
