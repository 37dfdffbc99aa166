"""Host: the seeded pairwise-exchange search on real-weighted pairs -- tests/seeded_two_opt_weighted_ref.py and the numpy route of
qap.two_opt_weighted_seeded (CPU tensors) -- against scipy.optimize.quadratic_assignment(method='2opt', options={'maximize': True,
'partial_match': the seeds, 'partial_guess': the start on the free rows}): col_ind and nit, exactly, on integer weights in [-3, 3]
and dyadic weights k/8, symmetric pairs and directed pairs with non-zero diagonals.  Seeds sit on every k-th row (their targets the
planted ones), the start is a shuffle of the planted columns over the free rows.  Also: seeds of all -1 change nothing, argument
errors go through check_seeds, the refusals, the C interface is declared and bound, and every exact case of the GPU test is a
search the reference ends as a local optimum."""
import os
import re

import numpy as np
import pytest
import torch
from scipy.optimize import quadratic_assignment

import seeded_two_opt_weighted_ref as S
import two_opt_weighted_ref as R
from graph_neural_net_amd import _lib, qap

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'fgnn_hip.h')
# (n, symmetric, weights, every k-th row seeded, free rows)
CASES = [(5, True, 'int', 2, 2), (31, False, 'int', 4, 23), (33, True, 'dyadic', 4, 24), (50, False, 'dyadic', 3, 33),
         (64, True, 'int', 5, 51), (65, False, 'int', 4, 48)]


def _case(n, symmetric, kind, k):
    A, Bm, q = R.make_pair(n, 3, symmetric, kind)
    mask = np.zeros(n, dtype=bool)
    mask[::k] = True
    start = S.start_on_free_rows(q, mask, None, 77 * n + k)
    return A, Bm, start, np.where(mask, q, -1).astype(np.int64)


def _scipy(A, Bm, start, sd):
    fixed, free = np.flatnonzero(sd >= 0), np.flatnonzero(sd < 0)
    res = quadratic_assignment(A, Bm, method='2opt', options={
        'maximize': True, 'partial_match': np.stack([fixed, sd[fixed]], 1).reshape(-1, 2),
        'partial_guess': np.stack([free, start[free]], 1).reshape(-1, 2)})
    return res.col_ind.tolist(), float(res.fun), int(res.nit)


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%d-%s-%s-k%d' % (c[0], 'sym' if c[1] else 'dir', c[2], c[3]))
def test_reference_and_host_route_equal_scipy_with_partial_match(case):
    n, symmetric, kind, k, nfree = case
    A, Bm, start, sd = _case(n, symmetric, kind, k)
    assert int((sd < 0).sum()) == nfree
    col, fun, nit = _scipy(A, Bm, start, sd)
    ref = S.two_opt_seeded(A, Bm, start, sd)
    print('n %d free %d: exchanges %d nit %d qap %r | SciPy nit %d fun %r' % (n, nfree, ref['swaps'], ref['nit'], ref['qap'], nit, fun))
    assert ref['perm'].tolist() == col and ref['nit'] == nit and ref['qap'] == fun and ref['status'] == S.OPTIMUM
    assert nfree <= 2 or ref['swaps'] >= 1                          # not an idle search
    assert (ref['perm'][sd >= 0] == sd[sd >= 0]).all()
    out = qap.two_opt_weighted_seeded(torch.from_numpy(A)[None], torch.from_numpy(Bm)[None], torch.from_numpy(start)[None], torch.from_numpy(sd)[None])
    assert set(out) == {'perm', 'qap', 'qap0', 'acc', 'swaps', 'nit', 'status'}
    assert out['perm'][0].tolist() == col and int(out['nit'][0]) == nit and float(out['qap'][0]) == fun
    assert int(out['swaps'][0]) == ref['swaps'] and int(out['status'][0]) == 0
    assert float(out['qap0'][0]) == R.objective(A, Bm, start)


def test_free_rows_of_zero_one_and_every_row():
    n = 12
    A, Bm, q = R.make_pair(n, 5, False, 'dyadic')
    for nfree, nit in ((0, 0), (1, 1)):
        sd = q.copy()
        sd[:nfree] = -1
        ref = S.two_opt_seeded(A, Bm, q, sd)
        assert (ref['perm'].tolist(), ref['swaps'], ref['nit'], ref['status']) == (q.tolist(), 0, nit, S.OPTIMUM)
        out = qap.two_opt_weighted_seeded(torch.from_numpy(A)[None], torch.from_numpy(Bm)[None], torch.from_numpy(q)[None], torch.from_numpy(sd)[None])
        assert (out['perm'][0].tolist(), int(out['swaps'][0]), int(out['nit'][0]), int(out['status'][0])) == (q.tolist(), 0, nit, 0)
        if nfree == 1:
            assert _scipy(A, Bm, q, sd)[::2] == (q.tolist(), nit)
    start = np.random.default_rng(3).permutation(n)
    free = S.two_opt_seeded(A, Bm, start, np.full(n, -1))
    plain = R.two_opt(A, Bm, start)
    assert all(np.array_equal(free[k], plain[k]) for k in S.KEYS) and plain['swaps'] > 0


def test_seeds_of_minus_one_equal_the_unseeded_call_key_for_key():
    case = (33, 5, False, 'dyadic')
    As, Bs, starts = R.batch_of(*case)
    N, B = case[:2]
    x1, x2 = torch.zeros(B, N, N, dtype=torch.float64), torch.zeros(B, N, N, dtype=torch.float64)
    assign = torch.full((B, N), -1, dtype=torch.int64)
    for b, (A, Bm, s) in enumerate(zip(As, Bs, starts)):
        x1[b, :len(A), :len(A)], x2[b, :len(A), :len(A)] = torch.from_numpy(A), torch.from_numpy(Bm)
        assign[b, :len(s)] = torch.from_numpy(s)
    nv = torch.tensor([len(s) for s in starts])
    plain = qap.two_opt_weighted(x1, x2, assign, nvalid=nv)
    seeded = qap.two_opt_weighted_seeded(x1, x2, assign, torch.full((B, N), -1, dtype=torch.int32), nvalid=nv)
    assert set(plain) == set(seeded) and all(torch.equal(plain[k], seeded[k]) and plain[k].dtype == seeded[k].dtype for k in plain)
    assert int(plain['swaps'].sum()) > 0


def test_refusals_of_the_host_route():
    n = 9
    pairs = [R.make_pair(n, b, True, 'int') for b in range(4)]
    x1 = torch.from_numpy(np.stack([p[0] for p in pairs]))
    x2 = torch.from_numpy(np.stack([p[1] for p in pairs]))
    starts = np.stack([R.transposed(p[2], 2, b) for b, p in enumerate(pairs)])
    seeds = np.full((4, n), -1, dtype=np.int64)
    seeds[:, 2] = starts[:, 2]
    seeds[0, 4] = n                                                  # outside the corner
    seeds[1, 5] = starts[1, 2]                                       # one target for two rows
    seeds[2, 6] = starts[2, 7]                                       # the start has another column there
    out = qap.two_opt_weighted_seeded(x1, x2, torch.from_numpy(starts), torch.from_numpy(seeds))
    assert out['status'].tolist() == [2, 2, 2, 0] and out['swaps'].tolist()[:3] == [0, 0, 0] and out['nit'].tolist()[:3] == [0, 0, 0]
    assert np.array_equal(out['perm'][:3].numpy(), starts[:3]) and out['qap'].tolist()[:3] == [-1.0, -1.0, -1.0]
    ref = S.two_opt_seeded(pairs[3][0], pairs[3][1], starts[3], seeds[3])
    assert out['perm'][3].tolist() == ref['perm'].tolist() and int(out['nit'][3]) == ref['nit'] and int(out['perm'][3, 2]) == seeds[3, 2]
    for b in range(3):
        assert S.two_opt_seeded(pairs[b][0], pairs[b][1], starts[b], seeds[b])['status'] == S.REFUSED


@pytest.mark.parametrize('bad', [torch.zeros(2, 5), torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, 5, dtype=torch.bool),
                                 [[0] * 5] * 2, 'scores'])
def test_argument_errors_go_through_check_seeds(bad):
    x = torch.zeros(2, 5, 5)
    assign = torch.arange(5).expand(2, 5)
    with pytest.raises(ValueError, match=r'two_opt_weighted_seeded: seeds must be a \(2, 5\) integer tensor'):
        qap.two_opt_weighted_seeded(x, x, assign, bad)
    ok = qap.two_opt_weighted_seeded(x, x, assign, np.full((2, 5), -1))
    assert ok['status'].tolist() == [0, 0]


def test_the_c_interface_is_declared_and_bound():
    text = open(HEADER).read()
    m = re.search(r'\bint\s+fgnn_qapw_2opt_seeded\s*\(([^;]*)\);', text)
    names = [a.split()[-1].lstrip('*') for a in re.sub(r'/\*.*?\*/', '', m.group(1)).split(',')]
    assert names == ['a1', 'a2', 'gstride', 'ld', 'assign', 'seeds', 'nvalid', 'B', 'N', 'max_swaps', 'ws', 'ws_bytes', 'perm', 'swaps',
                     'nit', 'status', 'stream']
    assert 'fgnn_qapw_2opt_seeded' in _lib.EXPORTS and len(_lib._SIGNATURES['fgnn_qapw_2opt_seeded']) == len(names)
    assert len(_lib._SIGNATURES['fgnn_qapw_2opt']) == len(names) - 1
    assert hasattr(_lib.load(), 'fgnn_qapw_2opt_seeded')


@pytest.mark.parametrize('case', S.CASES, ids=lambda c: '%d-%d-%s-%s-%s' % (c[0], c[1], 'sym' if c[2] else 'dir', c[3], c[4]))
def test_every_gpu_case_ends_as_a_local_optimum_that_holds_its_seeds(case):
    As, Bs, starts, seeds = S.batch_of(*case)
    refs = S.reference(*case)
    for A, s, sd, ref in zip(As, starts, seeds, refs):
        n = len(A)
        assert ref['status'] == S.OPTIMUM and ref['swaps'] < max(n * n, 1)
        assert sorted(ref['perm'].tolist()) == list(range(n)) and (ref['perm'][sd >= 0] == sd[sd >= 0]).all()
    free = max(int((sd < 0).sum()) for sd in seeds)
    assert free <= 2 or sum(r['swaps'] for r in refs) > 0, 'an idle batch'
    if case[4] == 'none':
        assert all(np.array_equal(r[k], p[k]) for A, Bm, s, r in zip(As, Bs, starts, refs) for p in [R.two_opt(A, Bm, s)] for k in S.KEYS)
