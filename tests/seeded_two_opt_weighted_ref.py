"""float64 numpy reference of the SEEDED pairwise-exchange search on real-weighted pairs, built on tests/two_opt_weighted_ref.py
(`make_pair`, `terms_of_row`): SciPy's _quadratic_assignment_2opt with maximize=True, partial_match = the seeds and partial_guess =
the start on the free rows.  The scan walks combinations_with_replacement(i_free, 2) -- the free rows ascending -- so with f free
rows and r(i) the rank of row i among them the pairs come in the order (r, r) = (0,0), (0,1), .., (0,f-1), (1,1), ..; the first pair
with a positive gain is exchanged and the scan starts over; nit counts every evaluation.  The gain of a pair is the same sum over
ALL vertices as without seeds: a seeded row never moves, but it is part of the objective.
tests/test_seeded_two_opt_weighted_host.py holds this module to SciPy itself.

The module also makes the test batches and their seed patterns and keeps one reference result per batch (`reference`)."""
import functools

import numpy as np

import two_opt_weighted_ref as R

OPTIMUM, STOPPED, REFUSED = R.OPTIMUM, R.STOPPED, R.NO_PERMUTATION
KEYS = R.KEYS


def two_opt_seeded(A, B, start, seeds, max_swaps=None):
    """A, B: (n, n) matrices; start: n columns; seeds: n entries, seeds[i] >= 0 fixes row i, < 0 leaves it free ->
    {'perm', 'qap', 'swaps', 'nit', 'status'}.  status 2 (perm = start, qap -1, swaps = nit = 0): start is no permutation of [0, n),
    or differs from a seed -- so a seed outside [0, n) and one target for two rows are refused too."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    p = np.array(start, dtype=np.int64)
    sd = np.asarray(seeds, dtype=np.int64)
    n = len(p)
    assert len(sd) == n
    if sorted(p.tolist()) != list(range(n)) or bool(((sd >= 0) & (p != sd)).any()):
        return {'perm': p, 'qap': -1.0, 'swaps': 0, 'nit': 0, 'status': REFUSED}
    if n == 0:
        return {'perm': p, 'qap': 0.0, 'swaps': 0, 'nit': 0, 'status': OPTIMUM}
    fr = np.flatnonzero(sd < 0)
    f = len(fr)
    bound = n * n if max_swaps is None else min(max_swaps, n * n)
    Bp = B[np.ix_(p, p)]
    swaps = nit = 0
    while swaps < bound:
        for ri in range(f):
            i = int(fr[ri])
            better = np.flatnonzero(R.terms_of_row(A, Bp, i).sum(1)[fr[ri + 1:]] > 0)
            if better.size:
                j = int(fr[ri + 1 + int(better[0])])
                nit += int(better[0]) + 2                          # (ri,ri) .. (ri,rj)
                break
            nit += f - ri                                          # (ri,ri) .. (ri,f-1)
        else:
            return {'perm': p, 'qap': float((A * Bp).sum()), 'swaps': swaps, 'nit': nit, 'status': OPTIMUM}
        swaps += 1
        p[[i, j]] = p[[j, i]]
        Bp = B[np.ix_(p, p)]
    return {'perm': p, 'qap': float((A * Bp).sum()), 'swaps': swaps, 'nit': nit, 'status': STOPPED}


# ------------------------------------------------------------------------------------------------------------------ the seeds
PATTERNS = ('third', 'fourth', 'all', 'all_but_one', 'all_but_two', 'none')


def seeded_rows(n, pattern, b=0):
    """-> boolean mask over the n rows: the rows that hold a seed"""
    m = np.zeros(n, dtype=bool)
    if pattern in ('third', 'fourth'):
        m[b % 2::3 if pattern == 'third' else 4] = True
    elif pattern == 'all':
        m[:] = True
    elif pattern in ('all_but_one', 'all_but_two'):
        m[:] = True
        if n:
            first = (5 * b + 1) % n
            m[first] = False
            if pattern == 'all_but_two' and n > 1:
                m[(first + 1 + (3 * b) % (n - 1)) % n] = False     # (another row: the offset lies in [1, n - 1])
    elif pattern != 'none':
        raise ValueError(pattern)
    return m


def start_on_free_rows(q, mask, k, seed):
    """the matching q with its columns on the free rows (~mask) permuted: a full shuffle (k None) or k transpositions"""
    rng = np.random.default_rng(seed)
    p = np.array(q, dtype=np.int64)
    fr = np.flatnonzero(~mask)
    if len(fr) < 2:
        return p
    if k is None:
        p[fr] = p[fr][rng.permutation(len(fr))]
        return p
    for _ in range(k):
        i, j = rng.choice(fr, 2, replace=False)
        p[[i, j]] = p[[j, i]]
    return p


def batch_of(N, B, symmetric, kind, pattern):
    """-> (As, Bs, starts, seeds): pair b has n_b vertices (0, 1 and N among them when B > 1), its seeds (pattern) are the planted
    targets, its start holds them and shuffles the planted columns of the free rows -- fully up to N = 65, by 8 transpositions
    from N = 128 up, as two_opt_weighted_ref.batch_of does, so that a search stays short."""
    rng = np.random.default_rng(11 * N + B)
    sizes = [N] * B if B == 1 else ([0, 1, N] + rng.integers(0, N + 1, B).tolist())[:B]
    As, Bs, starts, seeds = [], [], [], []
    for b, n in enumerate(sizes):
        A, Bm, q = R.make_pair(n, b, symmetric, kind)
        mask = seeded_rows(n, pattern, b)
        starts.append(start_on_free_rows(q, mask, None if N <= 65 else 8, 1000 * N + b))
        seeds.append(np.where(mask, q, -1).astype(np.int64))
        As.append(A), Bs.append(Bm)
    return As, Bs, starts, seeds


@functools.lru_cache(maxsize=None)
def reference(N, B, symmetric, kind, pattern, max_swaps=None):
    """the reference result of every pair of batch_of(N, B, symmetric, kind, pattern): a tuple of dicts, computed once, not to be
    changed"""
    As, Bs, starts, seeds = batch_of(N, B, symmetric, kind, pattern)
    return tuple(two_opt_seeded(A, Bm, s, sd, max_swaps) for A, Bm, s, sd in zip(As, Bs, starts, seeds))


# the exact cases of tests/test_gpu_two_opt_weighted_seeded.py: both sides of every instantiation's edge (32 / 64 / 128 rows in LDS,
# 256 with Bp in the workspace), one pair, a few, more pairs than a wave has lanes; every seed pattern at one size per instantiation
CASES = [(1, 5, True, 'int', 'none'), (1, 1, True, 'int', 'all'), (2, 70, False, 'dyadic', 'third'), (2, 5, True, 'int', 'all_but_two'),
         (31, 5, False, 'int', 'fourth'), (32, 1, True, 'dyadic', 'third'), (33, 70, True, 'int', 'third'),
         (33, 5, False, 'dyadic', 'all_but_two'), (33, 5, True, 'int', 'all'), (50, 5, True, 'dyadic', 'all_but_one'),
         (64, 5, True, 'dyadic', 'fourth'), (64, 1, False, 'int', 'third'), (65, 5, False, 'dyadic', 'third'),
         (65, 5, True, 'int', 'all_but_two'), (65, 1, True, 'int', 'none'), (128, 5, True, 'int', 'fourth'),
         (128, 1, False, 'dyadic', 'all_but_one'), (129, 5, False, 'int', 'third'), (129, 5, True, 'dyadic', 'all'),
         (129, 1, True, 'dyadic', 'all_but_two'), (256, 1, True, 'dyadic', 'fourth'), (256, 1, False, 'int', 'third')]
