"""Plain-loop numpy references for the confident seeds (csrc/seed_select.hip): the rule of fgnn_confident_seeds written entry by
entry, and the sums of fgnn_seed_fold.  Nothing here shares code with the package."""
import math

import numpy as np


def _first_max(values):
    """index of the largest value, the smaller index on ties (-0.0 == +0.0); values hold no NaN"""
    best = 0
    for k in range(1, len(values)):
        if values[k] > values[best]:
            best = k
    return best


def confident_pair(s, count=None, min_margin=0.0):
    """s: (n, n) float32 -> (seeds (n,) int32, nseeds, margin (n,) float32)"""
    n = s.shape[0]
    seeds, margin = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.float32)
    if n == 0:
        return seeds, 0, margin
    s = s.astype(np.float32)
    col_of_row, row_of_col = [0] * n, [-1] * n
    for i in range(n):
        row = [float(v) for v in s[i]]
        if any(math.isnan(v) for v in row):
            margin[i] = -np.inf
            continue                                                # col_of_row[i] is never used: the row is no candidate
        c = _first_max(row)
        col_of_row[i] = c
        if not math.isfinite(row[c]):
            margin[i] = -np.inf
            continue
        others = [np.float32(v) for j, v in enumerate(row) if j != c]
        top2 = max(others) if others else np.float32(-np.inf)
        with np.errstate(over='ignore'):
            margin[i] = np.float32(row[c]) - np.float32(top2)       # one float32 subtraction
    for j in range(n):
        col = [float(v) for v in s[:, j]]
        if not any(math.isnan(v) for v in col):
            row_of_col[j] = _first_max(col)
    cands = [i for i in range(n) if margin[i] != -np.inf and row_of_col[col_of_row[i]] == i and margin[i] >= np.float32(min_margin)]
    cands.sort(key=lambda i: (-float(margin[i]), i))               # margin descending, row ascending
    kept = cands if count is None else cands[:count]
    for i in kept:
        seeds[i] = col_of_row[i]
    return seeds, len(kept), margin


def confident_batch(S, nvalid=None, count=None, min_margin=0.0):
    """S: (B, N, N) float array, nvalid: None or B ints -> (seeds (B, N) int32, nseeds (B,) int32, margin (B, N) float32)"""
    B, N = S.shape[0], S.shape[-1]
    seeds, nseeds = np.full((B, N), -1, dtype=np.int32), np.zeros(B, dtype=np.int32)
    margin = np.zeros((B, N), dtype=np.float32)
    for b in range(B):
        n = N if nvalid is None else min(max(int(nvalid[b]), 0), N)
        seeds[b, :n], nseeds[b], margin[b, :n] = confident_pair(np.asarray(S[b, :n, :n], dtype=np.float32), count, min_margin)
    return seeds, nseeds, margin


def order_of(seeds_all, margin):
    """the kept rows of a count=None result in (margin descending, row ascending) order"""
    rows = [i for i in range(len(seeds_all)) if seeds_all[i] >= 0]
    return sorted(rows, key=lambda i: (-float(margin[i]), i))


FIELDS = ('seeds', 'seed_correct', 'free_nodes', 'free_correct', 'free_refined_correct', 'clean_pairs', 'exact_free', 'nodes', 'pairs',
          'steps')


def fold(record, seeds, assign, perm, labels, nvalid, live=None, bins=None, k=None):
    """Adds the pairs b < live (of bin k, with bins) to `record`, a dict over FIELDS of Python ints, as fgnn_seed_fold does."""
    B, N = assign.shape
    live = B if live is None else live
    took = 0
    for b in range(live):
        if bins is not None and int(bins[b]) != k:
            continue
        n = N if nvalid is None else min(max(int(nvalid[b]), 0), N)
        m = sc = fc = frc = 0
        for i in range(n):
            t = i if labels is None else int(labels[b, i])
            has = 0 <= t < n
            seeded = seeds is not None and int(seeds[b, i]) >= 0
            if seeded:
                m += 1
                sc += int(has and int(seeds[b, i]) == t)
            else:
                fc += int(has and int(assign[b, i]) == t)
                if perm is not None:
                    frc += int(has and int(perm[b, i]) == t)
        record['seeds'] += m
        record['seed_correct'] += sc
        record['free_nodes'] += n - m
        record['free_correct'] += fc
        if perm is not None:
            record['free_refined_correct'] += frc
        record['clean_pairs'] += int(sc == m)
        record['exact_free'] += int((frc if perm is not None else fc) == n - m)
        record['nodes'] += n
        record['pairs'] += 1
        took += 1
    if took:
        record['steps'] += 1
    return record


def empty_record():
    return dict.fromkeys(FIELDS, 0)


def record_bytes(records):
    """the records (dicts) as the bytes of fgnn_seed_record structs (a uint8 numpy array)"""
    return np.array([[r[f] for f in FIELDS] for r in records], dtype=np.int64).view(np.uint8).reshape(-1)
