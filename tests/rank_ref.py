"""Brute-force reference of the rank metrics (csrc/rank.hip, evaluation.rank_scores, metrics.match_ranks) in numpy, shared by
tests/test_ranks_host.py and tests/test_gpu_ranks.py.  Written from the rule alone, with no call into the package:

    for a row i < n with target t in [0, n):  rank = 1 + #{ j < n, j != t : column j beats column t },  and 0 without a target
    column j BEATS column t iff   s_j is NaN and s_t is not
                               or s_j > s_t
                               or j < t and (s_j == s_t or both are NaN)

-- np.argmax's order (first maximum on ties, NaN above every number, the first NaN wins, -0.0 == +0.0), so rank 1 is an arg-max hit.
The ranks are functions of comparisons on the given fp32 scores: every integer is compared for equality."""
import functools
import math

import numpy as np
import torch

NS = (1, 5, 16, 17, 64, 65, 130)
BS = (1, 3, 5, 9)
KS = (1, 3, 5, 10)
MAX_K = 8


def beats(sj, st, j, t):
    sj_nan, st_nan = sj != sj, st != st
    if sj_nan and not st_nan:
        return True
    if sj > st:
        return True
    return j < t and (sj == st or (sj_nan and st_nan))


def rank_rows_scalar(blk, want):
    """blk: (n, n) scores; want: n targets -> n ranks (0: the target is no column), by the double loop over (i, j)"""
    n = blk.shape[0]
    out = np.zeros(n, dtype=np.int64)
    for i in range(n):
        t = int(want[i])
        if not 0 <= t < n:
            continue
        st = blk[i, t]
        out[i] = 1 + sum(1 for j in range(n) if j != t and beats(blk[i, j], st, j, t))
    return out


def rank_rows(blk, want):
    """rank_rows_scalar with the loop over j written as one numpy expression per row -- the same three clauses, tested equal to the
    scalar loop by tests/test_ranks_host.py; the large cases would take minutes otherwise"""
    n = blk.shape[0]
    out = np.zeros(n, dtype=np.int64)
    j = np.arange(n)
    for i in range(n):
        t = int(want[i])
        if not 0 <= t < n:
            continue
        row, st = blk[i], blk[i, t]
        row_nan, st_nan = np.isnan(row), bool(np.isnan(st))
        with np.errstate(invalid='ignore'):
            b = (row_nan & (not st_nan)) | (row > st) | ((j < t) & ((row == st) | (row_nan & st_nan)))
        b[t] = False
        out[i] = 1 + int(b.sum())
    return out


def ranks(scores, nv, labels=None, fill=0):
    """(B, N) int64 ranks of a batch; rows >= n_b hold `fill`"""
    s = np.asarray(scores)
    B, N = s.shape[0], s.shape[1]
    out = np.full((B, N), fill, dtype=np.int64)
    for b in range(B):
        n = int(nv[b])
        out[b, :n] = rank_rows(s[b, :n, :n], np.arange(n) if labels is None else np.asarray(labels)[b, :n])
    return out


def pair_sums(rank_row, ks):
    """one pair's sums over its n rank entries: hits per k, the fp64 sum of 1 / rank (math.fsum: correctly rounded), the rank sum and
    the number of rows with a target"""
    r = [int(x) for x in rank_row if int(x) >= 1]
    return {'hits': [sum(1 for x in r if x <= k) for k in ks], 'rr': math.fsum(1.0 / x for x in r), 'rank_sum': sum(r), 'targets': len(r)}


def empty_record():
    return {'rr_sum': 0.0, 'rank_sum': 0, 'targets': 0, 'nodes': 0, 'pairs': 0, 'steps': 0, 'hits': [0] * MAX_K}


def fold_record(pair_rr, pair_hits, pair_rank_sum, pair_targets, nodes, take, start=None):
    """The arithmetic of fgnn_rank_fold on per-pair values: the pairs of `take` (ascending pair indices) added to the record in pair
    order, one at a time; a record that takes no pair stays as it is."""
    rec = dict(start) if start else empty_record()
    rec['hits'] = list(rec['hits'])
    for b in take:
        rec['rr_sum'] = rec['rr_sum'] + float(pair_rr[b])
        rec['rank_sum'] += int(pair_rank_sum[b])
        rec['targets'] += int(pair_targets[b])
        rec['nodes'] += int(nodes[b])
        rec['pairs'] += 1
        for q, h in enumerate(pair_hits[b]):
            rec['hits'][q] += int(h)
    rec['steps'] += 1 if len(take) else 0
    return rec


def nv_pattern(B, N, g):
    """Ragged vertex counts: N first, then 0 and 1 (when B allows), the rest random in [1, N]."""
    nv = torch.randint(1, N + 1, (B,), generator=g, dtype=torch.int32)
    for k, v in enumerate((N, 0, 1)[:B]):
        nv[k] = v
    return nv


def corner(nv, N):
    r = torch.arange(N)
    m = r[None, :] < nv.long()[:, None]
    return m[:, :, None] & m[:, None, :]


def label_sets(nv, N, g):
    """{'identity': None, 'perm': a random permutation of [0, n_b) per pair, 'holes': the permutation with -1 in some entries and
    values >= n_b (n_b, N, N + 7) in others}; padding entries hold -1"""
    B = nv.numel()
    perm = torch.full((B, N), -1, dtype=torch.int32)
    for b, n in enumerate(nv.tolist()):
        perm[b, :n] = torch.randperm(n, generator=g).to(torch.int32)
    holes = perm.clone()
    for b, n in enumerate(nv.tolist()):
        for i in range(n):
            u = int(torch.randint(0, 6, (1,), generator=g))
            if u == 0:
                holes[b, i] = -1
            elif u == 1:
                holes[b, i] = (n, N, N + 7)[i % 3]
    return {'identity': None, 'perm': perm, 'holes': holes}


@functools.lru_cache(maxsize=None)
def case(N, B, ragged):
    """One committed case (computed once, shared, never modified): random-normal scores rounded to quarters -- so rows hold ties --
    with NaN outside the valid corner, the vertex counts, three label sets and per label set the reference ranks and pair sums."""
    g = torch.Generator().manual_seed(7919 * N + 101 * B + (13 if ragged else 0))
    nv = nv_pattern(B, N, g) if ragged else torch.full((B,), N, dtype=torch.int32)
    s = (torch.randn(B, N, N, generator=g) * 8).round() / 4
    s = s.masked_fill(~corner(nv, N), float('nan'))
    labels = label_sets(nv, N, g)
    ref = {}
    for name, lab in labels.items():
        r = ranks(s.numpy(), nv.tolist(), None if lab is None else lab.numpy())
        ref[name] = {'rank': r, 'pairs': [pair_sums(r[b, :n], KS) for b, n in enumerate(nv.tolist())]}
    return {'scores': s, 'nv': nv, 'labels': labels, 'ref': ref}


def adversarial(N, g):
    """The rows of tests/test_gpu_eval.py::test_adversarial_rows_hold_the_argmax_rule: small-integer scores (duplicates in every row),
    NaN at several columns, +-inf, a row of -inf, a constant row -> (scores (3, N, N) with NaN padding, nv)"""
    B = 3
    nv = torch.tensor([N, N - 1, max(N - 3, 1)], dtype=torch.int32)
    s = torch.randint(-3, 4, (B, N, N), generator=g).float()
    for b in range(B):
        n = int(nv[b])
        s[b, 0, :] = float('-inf')
        s[b, 1 % n, n - 1] = float('nan')
        if n > 2:
            s[b, 2, n - 1] = float('nan')
            s[b, 2, n // 2] = float('nan')
            s[b, 2, 0] = float('inf')
        if n > 3:
            s[b, 3, n - 1] = float('inf')
            s[b, 3, n // 3] = float('inf')
        if n > 4:
            s[b, 4, :] = 2.0
    return s.masked_fill(~corner(nv, N), float('nan')), nv
