"""numpy restatement of the decode fold (csrc/qap_fold.hip, include/fgnn_hip.h "decode epochs"): per pair the rows whose `assign`
(and `perm`) entry is the row's target, the IEEE quotient qap / planted, and the add into one record per bin in pair order.  The
fp64 sum is a plain Python loop in pair order: every addition is one correctly rounded IEEE addition, as on the device, so records
compare as raw bytes."""
import ctypes

import numpy as np

from graph_neural_net_amd import _lib

FIELDS = tuple(name for name, _ in _lib.QapRecord._fields_)
REC = ctypes.sizeof(_lib.QapRecord)


def empty():
    rec = {name: 0 for name in FIELDS}
    rec['ratio_sum'] = 0.0
    return rec


def sizes(nvalid, B, N):
    return [N] * B if nvalid is None else [min(max(int(n), 0), N) for n in nvalid]


def pair_counts(assign, perm, labels, nvalid, live):
    """-> (correct, refined_correct): per pair b < live the rows i < n_b with assign[b, i] == target(b, i) (resp. perm; zeros without
    perm); target = labels[b, i], i without labels, none outside [0, n_b).  Pairs >= live: 0."""
    B, N = assign.shape
    correct, refined = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b, n in enumerate(sizes(nvalid, B, N)[:live]):
        for i in range(n):
            t = int(labels[b, i]) if labels is not None else i
            if 0 <= t < n:
                correct[b] += int(assign[b, i]) == t
                if perm is not None:
                    refined[b] += int(perm[b, i]) == t
    return correct, refined


def pair_ratios(qap, planted, live):
    out = np.zeros(len(qap), dtype=np.float64)
    for b in range(live):
        if qap[b] >= 0 and planted[b] > 0:
            out[b] = float(np.float64(int(qap[b])) / np.float64(int(planted[b])))
    return out


def fold(assign, perm, labels, qap, planted, refined, nvalid, live, bin=None, K=1, start=None):
    """-> (the K records as dicts, correct, refined_correct, ratio).  start: the K records to add to (None: empty ones).  A record
    that takes no pair is returned as it came."""
    B, N = assign.shape
    n_of = sizes(nvalid, B, N)
    correct, rcorrect = pair_counts(assign, perm, labels, nvalid, live)
    ratio = pair_ratios(qap, planted, live)
    recs = [dict(r) for r in start] if start is not None else [empty() for _ in range(K)]
    took = [False] * K
    for b in range(live):
        k = 0 if bin is None else int(bin[b])
        if not 0 <= k < K:
            continue
        r = recs[k]
        took[k] = True
        q, p, n = int(qap[b]), int(planted[b]), n_of[b]
        r['nodes'] += n
        r['pairs'] += 1
        r['correct'] += int(correct[b])
        r['exact'] += int(correct[b]) == n
        if perm is not None:
            r['refined_correct'] += int(rcorrect[b])
        if q < 0:
            r['unmatched'] += 1
            continue
        r['qap_sum'] += q
        r['planted_sum'] += p
        r['recovered'] += q >= p
        if p > 0:
            r['ratio_sum'] = float(np.float64(r['ratio_sum']) + np.float64(ratio[b]))
            r['ratio_pairs'] += 1
        if perm is not None:
            r['refined_sum'] += int(refined[b])
            r['improved'] += int(refined[b]) > q
    for k in range(K):
        if took[k]:
            recs[k]['steps'] += 1
    return recs, correct, rcorrect, ratio


def to_bytes(recs):
    """the records as the bytes of K fgnn_qap_record structs (a uint8 numpy array)"""
    arr = (_lib.QapRecord * len(recs))()
    for a, r in zip(arr, recs):
        for name in FIELDS:
            setattr(a, name, r[name])
    return np.frombuffer(bytes(arr), dtype=np.uint8).copy()


def from_bytes(raw):
    raw = bytes(bytearray(raw))
    arr = (_lib.QapRecord * (len(raw) // REC)).from_buffer_copy(raw)
    return [{name: getattr(a, name) for name in FIELDS} for a in arr]


def _permutation(rng, n):
    """a permutation of range(n): the identity (3 in 10), one that keeps the first half fixed, or any"""
    p, r = np.arange(n), rng.random()
    if r >= 0.3:
        lo = 0 if r < 0.65 else n // 2
        p[lo:] = lo + rng.permutation(n - lo)
    return p


def case(B, N, seed, ragged=True, labels=None, refine=True):
    """Seeded inputs of the fold.  nvalid (ragged): a pattern with one graph of n = 1 and one of n = N (where B allows).  assign / perm:
    random permutations of the valid corner, -1 in the padding; pair B // 2 is unmatched (qap = -1, some rows -1); pair B - 1 has
    planted = 0.  labels: None, 'perm' (a permutation of the corner) or 'holes' (a permutation with entries of -1 and entries >= n_b)."""
    rng = np.random.default_rng(seed)
    nv = rng.integers(1, N + 1, size=B).astype(np.int32) if ragged else np.full(B, N, dtype=np.int32)
    if ragged:
        nv[0] = N
        if B > 1:
            nv[1] = 1
    assign = np.full((B, N), -1, dtype=np.int32)
    perm = np.full((B, N), -1, dtype=np.int32)
    lab = None if labels is None else np.full((B, N), -1, dtype=np.int32)
    for b, n in enumerate(nv):
        for out in (assign, perm):
            out[b, :n] = _permutation(rng, n)
        if lab is not None:
            lab[b, :n] = rng.permutation(n)
            if rng.random() < 0.4:
                assign[b, :n] = lab[b, :n]          # (a pair that is exact against its labels, before the holes)
            if labels == 'holes' and n > 1:
                lab[b, rng.integers(0, n)] = -1
                lab[b, rng.integers(0, n)] = n + int(rng.integers(0, 3))
    planted = rng.integers(1, 4 * N + 2, size=B).astype(np.int32)
    qap = (planted + rng.integers(-3, 4, size=B)).clip(0).astype(np.int32)
    refined = (qap + rng.integers(-2, 5, size=B)).astype(np.int32)
    u = B // 2
    qap[u] = -1
    assign[u, :nv[u]:2] = -1
    planted[B - 1] = 0
    if not refine:
        perm = refined = None
    return {'assign': assign, 'perm': perm, 'labels': lab, 'qap': qap, 'planted': planted, 'refined': refined, 'nv': nv if ragged else None}
