"""GPU: the decode fold on real-weighted pairs -- fgnn_qapw_fold / fgnn_qapw_fold_bins (csrc/qap_fold_weighted.hip) -- against a
sequential Python loop over the pairs, bit for bit: the ten int64 counts and the four fp64 sums (Python floats are IEEE doubles,
float(np.float32) is exact, and the loop adds in pair order from the record's own value, as the kernel's owner thread does).

Shapes: B in {1, 3, 4, 5, 9} around the 4-pair chunk of the workgroup, N in {1, 63, 64, 65, 130} around a wave's 64 rows, live in
{0, 1, B - 1, B}, K in {1, 3, 64} with a bin that stays empty, with and without perm, with and without labels (some -1).  Every
batch of B >= 3 has one unmatched pair (an assign entry outside its corner), one pair with planted <= 0 and one negative objective."""
import ctypes

import numpy as np
import pytest
import torch

from graph_neural_net_amd import _lib
from graph_neural_net_amd.evaluation import BinnedWeightedQapMeter, WeightedQapMeter, qap_result

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZE = ctypes.sizeof(_lib.QapwRecord)
FP64 = ('ratio_sum', 'qap_sum', 'planted_sum', 'refined_sum')
INTS = ('ratio_pairs', 'correct', 'refined_correct', 'recovered', 'exact', 'improved', 'unmatched', 'nodes', 'pairs', 'steps')


def make_case(B, N, seed, with_labels):
    """-> dict of numpy arrays: nvalid, assign, perm, labels (or None), qap, planted, refined (float32)"""
    rng = np.random.default_rng(1000 * B + N + seed)
    nv = rng.integers(0, N + 1, B).astype(np.int32)
    nv[0] = N
    if B > 1:
        nv[1] = max(N - 1, 1)
    if B > 2:
        nv[2] = N
    assign = rng.integers(0, N, (B, N)).astype(np.int32)            # junk past the corners
    perm = rng.integers(0, N, (B, N)).astype(np.int32)
    labels = np.full((B, N), -1, dtype=np.int32)
    for b in range(B):
        n = int(nv[b])
        truth = rng.permutation(n)
        labels[b, :n] = truth if with_labels else np.arange(n)
        for m in (assign, perm):
            m[b, :n] = truth if with_labels else np.arange(n)
            k = rng.integers(0, n + 1)
            rows = rng.choice(n, size=k, replace=False) if n else []
            m[b, rows] = m[b, rows][rng.permutation(k)] if k else m[b, rows]
    if with_labels:
        labels[0, ::3] = -1                                          # rows without a target
        labels[B - 1, :1] = N + 5
    if B > 1:
        assign[1, 0] = nv[1]                                         # one unmatched pair: an entry just outside its corner
    qap = (rng.standard_normal(B) * 50 + 60).astype(np.float32)
    planted = (rng.standard_normal(B) * 5 + 70).astype(np.float32)
    refined = (qap + rng.standard_normal(B).astype(np.float32) * 3).astype(np.float32)
    qap[0] = np.float32(-12.625)                                     # a negative objective is a value
    if B > 2:
        planted[2] = np.float32(-3.5)                                # planted <= 0: no ratio
    if B > 3:
        planted[3] = np.float32(0.0)
        refined[3] = qap[3]                                          # not improved: r > q is strict
    return {'nvalid': nv, 'assign': assign, 'perm': perm, 'labels': labels if with_labels else None, 'qap': qap, 'planted': planted,
            'refined': refined}


def fold_ref(rec, c, lo, hi, use_perm, take=None):
    """the pairs lo <= b < hi of case c (take: only those b with take[b]) added to the record dict `rec`, in pair order
    -> (pair_correct, pair_refined_correct, pair_ratio) of those pairs (zero elsewhere)"""
    B, N = c['assign'].shape
    pc, prc, pr = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.float64)
    took = False
    for b in range(lo, hi):
        n = int(min(max(c['nvalid'][b], 0), N))
        hit = rhit = out = 0
        for i in range(n):
            t = int(c['labels'][b, i]) if c['labels'] is not None else i
            has = 0 <= t < n
            a = int(c['assign'][b, i])
            hit += has and a == t
            out += a < 0 or a >= n
            rhit += use_perm and has and int(c['perm'][b, i]) == t
        q, p, r = c['qap'][b], c['planted'][b], c['refined'][b]
        ratio = float(q) / float(p) if out == 0 and p > 0 else 0.0
        pc[b], prc[b], pr[b] = hit, rhit, ratio
        if take is not None and not take[b]:
            continue
        took = True
        rec['nodes'] += n
        rec['pairs'] += 1
        rec['correct'] += hit
        if out:
            rec['unmatched'] += 1
            continue
        rec['exact'] += hit == n
        if use_perm:
            rec['refined_correct'] += rhit
        rec['qap_sum'] += float(q)
        rec['planted_sum'] += float(p)
        rec['recovered'] += bool(q >= p)
        if p > 0:
            rec['ratio_sum'] += ratio
            rec['ratio_pairs'] += 1
        if use_perm:
            rec['refined_sum'] += float(r)
            rec['improved'] += bool(r > q)
    rec['steps'] += took
    return pc, prc, pr


def empty():
    return {**{k: 0.0 for k in FP64}, **{k: 0 for k in INTS}}


def _dev(c):
    return {k: (torch.from_numpy(v).to(DEV) if v is not None else None) for k, v in c.items()}


def _launch(d, lo, hi, use_perm, buf, bins=None, K=1, outs=True):
    """one fold call on the pairs lo .. hi of the device case d (as a batch of its own: live = hi - lo)"""
    B, N = hi - lo, d['assign'].shape[1]
    sl = lambda t: None if t is None else t[lo:hi].contiguous()
    pc, prc = torch.full((B,), -7, dtype=torch.int32, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV)
    pr = torch.full((B,), -7.0, dtype=torch.float64, device=DEV)
    pairs = (_lib.ptr(sl(d['assign'])), _lib.ptr(sl(d['perm']) if use_perm else None), _lib.ptr(sl(d['labels'])), _lib.ptr(sl(d['qap'])),
             _lib.ptr(sl(d['planted'])), _lib.ptr(sl(d['refined']) if use_perm else None), _lib.ptr(sl(d['nvalid'])), B, N, B)
    tail = ((_lib.ptr(pc), _lib.ptr(prc), _lib.ptr(pr)) if outs else (None, None, None)) + (_lib.ptr(buf), _lib.stream_ptr())
    if bins is None:
        _lib.call('fgnn_qapw_fold', *pairs, *tail)
    else:
        _lib.call('fgnn_qapw_fold_bins', *pairs, _lib.ptr(sl(bins)), K, *tail)
    return pc, prc, pr


def _records(buf, K=1):
    raw = buf.cpu().numpy().tobytes()
    recs = (_lib.QapwRecord * K).from_buffer_copy(raw)
    return [{k: getattr(r, k) for k in FP64 + INTS} for r in recs]


def _same(got, want):
    for k in FP64:
        assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (k, got[k], want[k])
    for k in INTS:
        assert got[k] == int(want[k]), (k, got[k], want[k])


def test_the_mirror_matches_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'fgnn_hip.h')).read()
    body = re.search(r'typedef struct \{([^}]*)\} fgnn_qapw_record;', hdr).group(1)
    fields = re.findall(r'(double|long long)\s+(\w+);', body)
    assert [(n, ctypes.c_double if t == 'double' else ctypes.c_longlong) for t, n in fields] == list(_lib.QapwRecord._fields_)
    assert [n for _, n in fields] == list(FP64 + INTS) and SIZE == 8 * 14


@pytest.mark.parametrize('with_labels', [False, True], ids=['identity', 'labels'])
@pytest.mark.parametrize('use_perm', [False, True], ids=['assign', 'perm'])
@pytest.mark.parametrize('B,N', [(1, 1), (3, 63), (4, 64), (5, 65), (9, 130), (9, 64)])
def test_fold_equals_the_sequential_loop_bit_for_bit(B, N, use_perm, with_labels):
    c = make_case(B, N, 1, with_labels)
    d = _dev(c)
    for live in sorted({0, 1, B - 1, B}):
        start = empty()
        start.update(ratio_sum=0.1, qap_sum=-3.3, planted_sum=1e-3, refined_sum=7.7, pairs=5, steps=2)   # a record in mid-epoch
        raw = _lib.QapwRecord(**start)
        buf = torch.from_numpy(np.frombuffer(bytes(raw), dtype=np.uint8).copy()).to(DEV)
        before = buf.clone()
        pc, prc, pr = _launch(d, 0, live, use_perm, buf) if live else (None, None, None)
        if live == 0:                                               # live = 0 of a batch of B: nothing is written
            _lib.call('fgnn_qapw_fold', _lib.ptr(d['assign']), None, _lib.ptr(d['labels']), _lib.ptr(d['qap']), _lib.ptr(d['planted']),
                      None, _lib.ptr(d['nvalid']), B, N, 0, None, None, None, _lib.ptr(buf), _lib.stream_ptr())
            assert torch.equal(buf, before)
            continue
        want = dict(start)
        rpc, rprc, rpr = fold_ref(want, c, 0, live, use_perm)
        got = _records(buf)[0]
        print('B %d N %d live %d: %s' % (B, N, live, got))
        _same(got, want)
        assert pc.cpu().tolist() == rpc[:live].tolist() and prc.cpu().tolist() == rprc[:live].tolist()
        assert pr.cpu().numpy().tobytes() == rpr[:live].tobytes()
        if not use_perm:                                            # without perm the three refinement fields are not touched
            assert (got['refined_sum'], got['refined_correct'], got['improved']) == (7.7, 0, 0)
    if B >= 3:
        assert want['unmatched'] == 1 and want['ratio_pairs'] < want['pairs'] - 5 - 1 and c['qap'][0] < 0


def test_live_below_the_batch_ignores_the_rest_and_leaves_their_outputs_alone():
    B, N = 9, 65
    c = make_case(B, N, 2, True)
    d = _dev(c)
    buf = torch.zeros(SIZE, dtype=torch.uint8, device=DEV)
    pc = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    pr = torch.full((B,), -7.0, dtype=torch.float64, device=DEV)
    _lib.call('fgnn_qapw_fold', _lib.ptr(d['assign']), _lib.ptr(d['perm']), _lib.ptr(d['labels']), _lib.ptr(d['qap']), _lib.ptr(d['planted']),
              _lib.ptr(d['refined']), _lib.ptr(d['nvalid']), B, N, 6, _lib.ptr(pc), None, _lib.ptr(pr), _lib.ptr(buf), _lib.stream_ptr())
    want = empty()
    rpc, _, rpr = fold_ref(want, c, 0, 6, True)
    _same(_records(buf)[0], want)
    assert pc.cpu().tolist() == rpc[:6].tolist() + [-7] * 3 and pr.cpu().tolist()[6:] == [-7.0] * 3


def test_one_call_of_nine_pairs_equals_calls_of_four_and_five():
    B, N = 9, 65
    c = make_case(B, N, 3, True)
    d = _dev(c)
    whole, cut = (torch.zeros(SIZE, dtype=torch.uint8, device=DEV) for _ in range(2))
    _launch(d, 0, 9, True, whole)
    _launch(d, 0, 4, True, cut)
    _launch(d, 4, 9, True, cut)
    a, b = _records(whole)[0], _records(cut)[0]
    assert b['steps'] == 2 and a['steps'] == 1
    b['steps'] = 1
    _same(a, b)
    want = empty()
    fold_ref(want, c, 0, 9, True)
    _same(a, want)
    # and the binned form cut the same way
    K = 3
    bins = torch.tensor([0, 2, 2, 0, 0, 2, 0, 2, 2], dtype=torch.int32, device=DEV)
    wb, cb = (torch.zeros(K * SIZE, dtype=torch.uint8, device=DEV) for _ in range(2))
    _launch(d, 0, 9, True, wb, bins, K)
    _launch(d, 0, 4, True, cb, bins, K)
    _launch(d, 4, 9, True, cb, bins, K)
    for k, (x, y) in enumerate(zip(_records(wb, K), _records(cb, K))):
        y['steps'] = min(y['steps'], 1)
        _same(x, y)


@pytest.mark.parametrize('K', [1, 3, 64])
@pytest.mark.parametrize('use_perm', [False, True], ids=['assign', 'perm'])
def test_bins_give_every_record_the_bytes_of_a_plain_fold_of_its_pairs(K, use_perm):
    B, N = 9, 63
    c = make_case(B, N, 4 + K, K != 3)
    d = _dev(c)
    empty_bin = K - 1 if K > 1 else None                            # a bin no pair goes to: its bytes must stay
    rng = np.random.default_rng(K)
    bins_np = rng.integers(0, max(K - 1, 1), B).astype(np.int32)
    bins_np[4] = K + 3                                              # outside [0, K): added nowhere
    bins_np[7] = -1
    bins = torch.from_numpy(bins_np).to(DEV)
    buf = torch.zeros(K * SIZE, dtype=torch.uint8, device=DEV)
    if empty_bin is not None:
        buf[empty_bin * SIZE:(empty_bin + 1) * SIZE] = 0xAB
    before = buf.clone()
    for live in (0, B - 1, B):
        buf.copy_(before)
        sub = {k: (v[:live] if v is not None else None) for k, v in d.items()}
        if live == 0:
            _lib.call('fgnn_qapw_fold_bins', _lib.ptr(d['assign']), None, None, _lib.ptr(d['qap']), _lib.ptr(d['planted']), None, None, B, N,
                      0, _lib.ptr(bins), K, None, None, None, _lib.ptr(buf), _lib.stream_ptr())
            assert torch.equal(buf, before)
            continue
        pc, prc, pr = _launch(sub, 0, live, use_perm, buf, bins[:live], K)
        got = _records(buf, K)
        for k in range(K):
            if k == empty_bin:
                assert torch.equal(buf[k * SIZE:(k + 1) * SIZE], before[k * SIZE:(k + 1) * SIZE])
                continue
            want = empty()
            rpc, rprc, rpr = fold_ref(want, c, 0, live, use_perm, take=bins_np == k)
            _same(got[k], want)
        assert pc.cpu().tolist() == rpc[:live].tolist() and pr.cpu().numpy().tobytes() == rpr[:live].tobytes()
        assert sum(r['pairs'] for k, r in enumerate(got) if k != empty_bin) == int(((bins_np[:live] >= 0) & (bins_np[:live] < K)).sum())


def test_a_nan_objective_propagates_and_is_not_special_cased():
    B, N = 4, 5
    c = make_case(B, N, 9, False)
    c['qap'][2] = np.float32('nan')
    c['planted'][2] = np.float32(3.0)
    d = _dev(c)
    buf = torch.zeros(SIZE, dtype=torch.uint8, device=DEV)
    _launch(d, 0, B, True, buf)
    got = _records(buf)[0]
    want = empty()
    fold_ref(want, c, 0, B, True)
    assert np.isnan(got['qap_sum']) and np.isnan(got['ratio_sum']) and not np.isnan(got['planted_sum'])
    for k in INTS:
        assert got[k] == int(want[k]), k


def test_bad_arguments_and_the_meters():
    z = torch.zeros(64, dtype=torch.int32, device=DEV)
    f = torch.zeros(8, dtype=torch.float32, device=DEV)
    buf = torch.zeros(SIZE, dtype=torch.uint8, device=DEV)
    args = lambda live=2, perm=None, refined=None: (_lib.ptr(z), perm, None, _lib.ptr(f), _lib.ptr(f), refined, None, 2, 4, live)
    with pytest.raises(RuntimeError, match='fgnn_qapw_fold: live'):
        _lib.call('fgnn_qapw_fold', *args(live=3), None, None, None, _lib.ptr(buf), _lib.stream_ptr())
    with pytest.raises(RuntimeError, match='fgnn_qapw_fold: perm and refined'):
        _lib.call('fgnn_qapw_fold', *args(perm=_lib.ptr(z)), None, None, None, _lib.ptr(buf), _lib.stream_ptr())
    with pytest.raises(RuntimeError, match='fgnn_qapw_fold: bad arguments'):
        _lib.call('fgnn_qapw_fold', *args(), None, None, None, None, _lib.stream_ptr())
    for bad_k in (0, _lib.FGNN_MAX_LEVELS + 1):
        with pytest.raises(RuntimeError, match='fgnn_qapw_fold_bins: K'):
            _lib.call('fgnn_qapw_fold_bins', *args(), _lib.ptr(z), bad_k, None, None, None, _lib.ptr(buf), _lib.stream_ptr())
    with pytest.raises(RuntimeError, match='fgnn_qapw_fold_bins: bad arguments'):
        _lib.call('fgnn_qapw_fold_bins', *args(), None, 2, None, None, None, _lib.ptr(buf), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(buf, torch.zeros_like(buf))
    # the meters: views of the record, QapMeter's result keys
    c = make_case(5, 10, 11, True)
    d = _dev(c)
    meter = WeightedQapMeter(DEV)
    _launch(d, 0, 5, True, meter.buf)
    meter._mark_refined()
    want = empty()
    fold_ref(want, c, 0, 5, True)
    rec = meter.record()
    assert rec.pop('refined') is True
    _same(rec, want)
    assert meter.qap_sum.dtype == torch.float64 and meter.pairs.dtype == torch.int64 and float(meter.qap_sum) == want['qap_sum']
    res = meter.result()
    assert res == qap_result({**want, 'refined': True}) and set(res) >= {'acc', 'qap_ratio', 'mean_ratio', 'refined_qap_ratio', 'improved'}
    assert float(meter.qap_ratio) == want['qap_sum'] / want['planted_sum']
    meter.allreduce_()                                              # a single process: the record comes back as it was
    rec = meter.record()
    rec.pop('refined')
    _same(rec, want)
    assert meter.reset().record()['pairs'] == 0 and meter.refined is False
    binned = BinnedWeightedQapMeter(DEV, 3, values=(0.0, 0.1, 0.2))
    bins = torch.tensor([0, 2, 2, 0, 2], dtype=torch.int32, device=DEV)
    _launch(d, 0, 5, False, binned.buf, bins, 3)
    recs = binned.record()
    assert [r['pairs'] for r in recs] == [2, 0, 3] and [r['noise'] for r in recs] == [0.0, 0.1, 0.2]
    assert int(binned[2].pairs) == 3 and isinstance(binned[0], WeightedQapMeter)
    with pytest.raises(RuntimeError, match='no CPU path'):
        WeightedQapMeter('cpu')
