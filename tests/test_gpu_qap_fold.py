"""GPU: the decode fold -- fgnn_qap_fold / fgnn_qap_fold_bins (csrc/qap_fold.hip) -- against the numpy restatement of
tests/qap_fold_ref.py, as raw record bytes.

Every count is an integer and the one fp64 sum is a chain of correctly rounded additions of correctly rounded quotients in pair
order, which the restatement forms in the same order: the records are compared with torch.equal on their uint8 buffers, with no
tolerance.  The per-pair outputs are sentinel-filled before each call, so an entry the kernel leaves unwritten, or writes beyond
`live`, fails here.

`steps` counts the fold calls that added a pair to a record, so it is the one field that depends on how an epoch was cut into
calls: the cutting test compares the bytes with that word masked and asserts the word separately."""
import numpy as np
import pytest
import torch

import qap_fold_ref as QR
from graph_neural_net_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -77
REC = QR.REC
STEPS = _lib.QapRecord.steps.offset


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _fold(c, live, records, bins=None, K=1, sel=None):
    """fgnn_qap_fold(_bins) of the first `live` pairs of case c (sel: of those rows of it) into `records` (K x 112 bytes on the
    device), on sentinel-filled per-pair outputs -> (correct, refined_correct, ratio)"""
    t = {k: _dev(v if sel is None or v is None else v[sel]) for k, v in c.items()}
    B, N = t['assign'].shape
    correct = torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV)
    rcorrect = torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV)
    ratio = torch.full((B,), float(SENTINEL), dtype=torch.float64, device=DEV)
    pairs = tuple(_lib.ptr(t[k]) for k in ('assign', 'perm', 'labels', 'qap', 'planted', 'refined', 'nv')) + (B, N, live)
    outs = (_lib.ptr(correct), _lib.ptr(rcorrect), _lib.ptr(ratio), _lib.ptr(records), _lib.stream_ptr())
    if bins is None:
        _lib.call('fgnn_qap_fold', *pairs, *outs)
    else:
        _lib.call('fgnn_qap_fold_bins', *pairs, _lib.ptr(bins), K, *outs)
    return correct, rcorrect, ratio


def _ref(c, live, **kw):
    return QR.fold(c['assign'], c['perm'], c['labels'], c['qap'], c['planted'], c['refined'], c['nv'], live, **kw)


def _zeros(K=1):
    return torch.zeros(K * REC, dtype=torch.uint8, device=DEV)


def _bytes(recs):
    return torch.from_numpy(QR.to_bytes(recs)).to(DEV)


def _but_steps(buf):
    out = buf.clone().view(-1, REC)
    out[:, STEPS:STEPS + 8] = 0
    return out


# B = 5: a second chunk with a single wave live; N = 64 / 65: a lane takes a second row
SHAPES = [(1, 1), (5, 5), (9, 64), (9, 65)]


@pytest.mark.parametrize('B,N', SHAPES)
@pytest.mark.parametrize('labels', [None, 'perm', 'holes'])
def test_fold_equals_the_restatement_byte_for_byte(B, N, labels):
    for ragged in (False, True):
        for refine in (True, False):
            c = QR.case(B, N, seed=1000 * B + N, ragged=ragged, labels=labels, refine=refine)
            for live in sorted({0, 1, B - 1, B}):
                records = _zeros()
                correct, rcorrect, ratio = _fold(c, live, records)
                want, wc, wr, wq = _ref(c, live)
                assert torch.equal(records, _bytes(want)), (ragged, refine, live, QR.from_bytes(records.cpu().numpy()), want)
                assert correct[:live].cpu().tolist() == wc[:live].tolist() and bool((correct[live:] == SENTINEL).all())
                assert rcorrect[:live].cpu().tolist() == wr[:live].tolist() and bool((rcorrect[live:] == SENTINEL).all())
                assert np.array_equal(ratio[:live].cpu().numpy().view(np.int64), wq[:live].view(np.int64))
                assert bool((ratio[live:] == SENTINEL).all())
                if live == 0:
                    assert not bool(records.any())
                    continue
                # a second call adds to what the first left: ratio_sum and every count carry over
                _fold(c, live, records)
                assert torch.equal(records, _bytes(_ref(c, live, start=want)[0])), (ragged, refine, live)
            rec = QR.from_bytes(records.cpu().numpy())[0]
            assert rec['pairs'] == 2 * B and rec['steps'] == 2 and rec['unmatched'] == 2 and rec['ratio_pairs'] <= 2 * (B - 1)
            if not refine:
                assert rec['refined_sum'] == rec['refined_correct'] == rec['improved'] == 0
            # live = 0 on a record that holds something: its bytes stay
            before = records.clone()
            _fold(c, 0, records)
            assert torch.equal(records, before)


def test_the_optional_outputs_and_the_refusals():
    B, N = 5, 5
    c = QR.case(B, N, seed=3)
    t = {k: _dev(v) for k, v in c.items()}
    records, full = _zeros(), _zeros()
    _fold(c, B, full)
    pairs = tuple(_lib.ptr(t[k]) for k in ('assign', 'perm', 'labels', 'qap', 'planted', 'refined', 'nv'))
    _lib.call('fgnn_qap_fold', *pairs, B, N, B, None, None, None, _lib.ptr(records), _lib.stream_ptr())
    assert torch.equal(records, full)
    before = records.clone()
    for live in (-1, B + 1):
        with pytest.raises(RuntimeError, match='fgnn_qap_fold: live'):
            _fold(c, live, records)
    with pytest.raises(RuntimeError, match='go together'):
        _fold(dict(c, refined=None), B, records)
    with pytest.raises(RuntimeError, match='bad arguments'):
        _lib.call('fgnn_qap_fold', *pairs, B, N, B, None, None, None, None, _lib.stream_ptr())
    bins = torch.zeros(B, dtype=torch.int32, device=DEV)
    for bad_k in (0, _lib.FGNN_MAX_LEVELS + 1):
        with pytest.raises(RuntimeError, match='fgnn_qap_fold_bins: K'):
            _fold(c, B, records, bins=bins, K=bad_k)
    with pytest.raises(RuntimeError, match='fgnn_qap_fold_bins: live'):
        _fold(c, B + 1, records, bins=bins, K=2)
    torch.cuda.synchronize()
    assert torch.equal(records, before)


BINS = [2, 0, 2, 3, 0, 0, 2, -1, 2]          # K = 3: bin 1 stays empty, 3 and -1 lie outside


@pytest.mark.parametrize('N', [5, 65])
def test_binned_fold_equals_plain_folds_byte_for_byte(N):
    B, K = len(BINS), 3
    c = QR.case(B, N, seed=N, labels='holes')
    bins_d = torch.tensor(BINS, dtype=torch.int32, device=DEV)
    for live in (9, 6, 0):
        records = _zeros(K)
        for call in range(2):          # from zero records, then from what the first call left
            start = records.clone()
            want = start.clone()
            for j in range(K):
                sel = [b for b in range(live) if BINS[b] == j]
                if sel:
                    _fold(c, len(sel), want[j * REC:(j + 1) * REC], sel=sel)
            o = _fold(c, live, records, bins=bins_d, K=K)
            assert torch.equal(records, want), (N, live, call)
            assert torch.equal(records[REC:2 * REC], start[REC:2 * REC])          # the empty bin's bytes are untouched
            ref = _ref(c, live, bin=BINS, K=K, start=QR.from_bytes(start.cpu().numpy()))[0]
            assert torch.equal(records, _bytes(ref))
            plain = _fold(c, live, _zeros())
            assert all(torch.equal(a, b) for a, b in zip(o, plain))
        if live == 9:
            got = QR.from_bytes(records.cpu().numpy())
            assert [r['pairs'] for r in got] == [6, 0, 8] and [r['steps'] for r in got] == [2, 0, 2]


def test_sixty_four_bins():
    """K = FGNN_MAX_LEVELS: one owner thread per record, across the workgroup's first wave"""
    K, N = _lib.FGNN_MAX_LEVELS, 5
    B = K + 6
    c = QR.case(B, N, seed=64)
    rng = np.random.default_rng(64)
    bins = rng.permutation(B) % K
    bins[3] = K                     # (outside: dropped)
    records = _zeros(K)
    _fold(c, B - 1, records, bins=_dev(bins.astype(np.int32)), K=K)
    want = _ref(c, B - 1, bin=bins, K=K)[0]
    assert torch.equal(records, _bytes(want)) and sum(r['pairs'] for r in want) == B - 2
    for k in (0, 17, K - 1):
        sel = [b for b in range(B - 1) if bins[b] == k]
        one = _zeros()
        _fold(c, len(sel), one, sel=sel)
        assert torch.equal(records[k * REC:(k + 1) * REC], one), k


def test_record_does_not_depend_on_how_the_pairs_are_cut():
    """8 pairs as one call of 8, two of 4 and eight of 1"""
    B, N = 8, 65
    c = QR.case(B, N, seed=8, labels='perm')
    bufs = []
    for step in (8, 4, 1):
        records = _zeros()
        for lo in range(0, B, step):
            _fold(c, step, records, sel=list(range(lo, lo + step)))
        bufs.append(records)
        assert QR.from_bytes(records.cpu().numpy())[0]['steps'] == B // step
    assert torch.equal(_but_steps(bufs[0]), _but_steps(bufs[1])) and torch.equal(_but_steps(bufs[0]), _but_steps(bufs[2]))
    assert torch.equal(bufs[0], _bytes(_ref(c, B)[0]))
