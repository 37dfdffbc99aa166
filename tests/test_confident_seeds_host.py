"""CPU: the host side of the confident seeds (no launch): qap.confident_seeds on CPU tensors -- the numpy restatement of
fgnn_confident_seeds -- against the plain loops of confident_ref, exactly; its refusals; the seed spec of the decode; seed_result
and the ctypes mirror of fgnn_seed_record against numpy integer sums and include/fgnn_hip.h; and that the C interface is declared
and bound."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import confident_ref as R
from graph_neural_net_amd import _lib, evaluation, qap
from graph_neural_net_amd.masked import MaskedTensor

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'fgnn_hip.h')
SYMBOLS = {'fgnn_confident_seeds': 12, 'fgnn_seed_fold': 10, 'fgnn_seed_fold_bins': 12}


def _same(out, want):
    seeds, nseeds, margin = want
    assert out['seeds'].dtype == torch.int32 and out['nseeds'].dtype == torch.int32
    assert torch.equal(out['seeds'], torch.from_numpy(seeds))
    assert torch.equal(out['nseeds'], torch.from_numpy(nseeds))
    if 'margin' in out:
        assert out['margin'].dtype == torch.float32 and torch.equal(out['margin'], torch.from_numpy(margin))


def _scores(kind, B, N, seed):
    g = np.random.default_rng(seed)
    if kind == 'ties':                                   # ties in both arg-maxes, equal margins across rows
        return g.integers(0, 3, size=(B, N, N)).astype(np.float32)
    if kind == 'peaked':                                 # a permutation stands out: many candidates with distinct margins
        S = g.standard_normal((B, N, N)).astype(np.float32)
        for b in range(B):
            p = g.permutation(N)
            S[b, np.arange(N), p] += g.uniform(0, 4, size=N).astype(np.float32)
        return S
    return g.standard_normal((B, N, N)).astype(np.float32)


@pytest.mark.parametrize('kind', ['ties', 'peaked', 'normal'])
def test_host_route_equals_the_plain_loops(kind):
    B, N = 6, 13
    S = _scores(kind, B, N, 3)
    nv = np.array([13, 0, 1, 2, 7, 12])
    for b in range(B):
        S[b, nv[b]:, :] = np.nan
        S[b, :, nv[b]:] = np.nan
    for count in (None, 0, 1, 3, 13, 18):
        for mm in (0.0, 1.0, 2.5):
            out = qap.confident_seeds(torch.from_numpy(S), torch.from_numpy(nv), count=count, min_margin=mm, return_margin=True)
            _same(out, R.confident_batch(S, nv, count, mm))
    out = qap.confident_seeds(torch.from_numpy(S[:1]))
    assert set(out) == {'seeds', 'nseeds'}
    _same(out, R.confident_batch(S[:1]))


def test_prefix_property_and_validity():
    B, N = 4, 17
    S = _scores('ties', B, N, 5)
    S[2] = _scores('peaked', 1, N, 6)[0]
    full, _, margin = R.confident_batch(S)
    for count in (0, 1, 3, N, N + 5):
        out = qap.confident_seeds(torch.from_numpy(S), count=count)
        for b in range(B):
            order = R.order_of(full[b], margin[b])
            kept = sorted(order[:count])
            assert torch.nonzero(out['seeds'][b] >= 0).flatten().tolist() == kept
            tg = out['seeds'][b][out['seeds'][b] >= 0].tolist()
            assert len(set(tg)) == len(tg) and all(0 <= j < N for j in tg)
            assert int(out['nseeds'][b]) == len(kept)


def test_non_finite_scores():
    n = 6
    S = np.arange(n * n, dtype=np.float32).reshape(n, n) % 7
    S[np.arange(n), [3, 0, 4, 1, 5, 2]] = 9.0            # a clear permutation
    S[0, 1] = np.nan                                     # strikes row 0 and column 1 (row 3's choice)
    S[2, 4] = np.inf                                     # row 2's maximum is not finite
    S[4, :] = -np.inf                                    # a row of -inf
    S[5, 0] = -np.inf                                    # a -inf that is nobody's maximum changes nothing
    out = qap.confident_seeds(torch.from_numpy(S[None]), return_margin=True)
    _same(out, R.confident_batch(S[None]))
    assert out['seeds'][0].tolist() == [-1, 0, -1, -1, -1, 2]
    assert out['margin'][0, [0, 2, 4]].tolist() == [-math.inf] * 3
    one = qap.confident_seeds(torch.tensor([[[2.0]], [[math.nan]], [[-math.inf]]]), return_margin=True)
    assert one['seeds'].flatten().tolist() == [0, -1, -1] and one['margin'].flatten().tolist() == [math.inf, -math.inf, -math.inf]


def test_masked_tensor_strided_and_float64_input():
    B, N = 3, 9
    S = _scores('peaked', B, N, 8)
    nv = torch.tensor([9, 4, 6])
    want = R.confident_batch(S, nv.numpy())
    _same(qap.confident_seeds(MaskedTensor(torch.from_numpy(S), nv, (1, 2)), return_margin=True), want)
    big = torch.full((B, N + 3, N + 5), math.nan)
    big[:, 1:N + 1, 2:N + 2] = torch.from_numpy(S)
    _same(qap.confident_seeds(big[:, 1:N + 1, 2:N + 2], nv, return_margin=True), want)
    # float64 scores are rounded to float32 first, as the device route does: the margin is a float32 subtraction of those
    _same(qap.confident_seeds(torch.from_numpy(S.astype(np.float64)), nv, return_margin=True), want)


def test_refusals():
    S = torch.zeros(2, 5, 5)
    for bad in (-1, 1.5, True, '3'):
        with pytest.raises(ValueError, match='count'):
            qap.confident_seeds(S, count=bad)
    for bad in (-0.5, math.nan, None, 'x'):
        with pytest.raises(ValueError, match='min_margin'):
            qap.confident_seeds(S, min_margin=bad)
    for bad in (torch.zeros(5, 5), torch.zeros(2, 5, 4), torch.zeros(2, 5, 5, dtype=torch.int64), np.zeros((2, 5, 5)), torch.zeros(0, 5, 5)):
        with pytest.raises(ValueError, match='confident_seeds'):
            qap.confident_seeds(bad)
    with pytest.raises(ValueError, match='nvalid'):
        qap.confident_seeds(S, nvalid=torch.tensor([5.0, 5.0]))


def test_seed_spec():
    assert evaluation.seed_spec('t', None) is None and evaluation.seed_spec('t', torch.zeros(2, 3, dtype=torch.int32)) is None
    assert evaluation.seed_spec('t', 'scores') == {'count': -1, 'min_margin': 0.0}
    assert evaluation.seed_spec('t', {'from': 'scores', 'count': 4, 'min_margin': 1.5}) == {'count': 4, 'min_margin': 1.5}
    assert evaluation.seed_spec('t', {'count': 0}) == {'count': 0, 'min_margin': 0.0}
    for bad in ('labels', {'from': 'labels'}, {'from': 'scores', 'k': 3}, {'count': -2}, {'min_margin': -1.0}):
        with pytest.raises(ValueError, match='seeds'):
            evaluation.seed_spec('t', bad)


def test_seed_result_matches_integer_sums():
    g = np.random.default_rng(2)
    B, N = 9, 11
    nv = np.array([11, 0, 3, 11, 7, 1, 11, 5, 9])
    labels = np.stack([g.permutation(N) for _ in range(B)]).astype(np.int32)
    labels[3, 2] = -1
    assign = np.where(g.random((B, N)) < 0.6, labels, g.integers(0, N, size=(B, N))).astype(np.int32)
    perm = np.where(g.random((B, N)) < 0.8, labels, g.integers(0, N, size=(B, N))).astype(np.int32)
    seeds = np.where(g.random((B, N)) < 0.3, np.where(g.random((B, N)) < 0.9, labels, 0), -1).astype(np.int32)
    rec = R.fold(R.empty_record(), seeds, assign, perm, labels, nv)
    res = evaluation.seed_result(rec)
    assert set(res) == {'seed_precision', 'seeds_per_pair', 'free_acc', 'free_refined_acc', 'clean', 'exact_free', 'seeds',
                        'free_nodes', 'nodes', 'pairs'}
    inside = np.arange(N)[None, :] < nv[:, None]
    has = (labels >= 0) & (labels < nv[:, None])
    sd, fr = inside & (seeds >= 0), inside & (seeds < 0)
    assert res['seeds'] == int(sd.sum()) and res['free_nodes'] == int(fr.sum()) and res['nodes'] == int(nv.sum()) and res['pairs'] == B
    assert res['seed_precision'] == int((sd & has & (seeds == labels)).sum()) / int(sd.sum())
    assert res['free_acc'] == int((fr & has & (assign == labels)).sum()) / int(fr.sum())
    assert res['free_refined_acc'] == int((fr & has & (perm == labels)).sum()) / int(fr.sum())
    assert res['seeds_per_pair'] == int(sd.sum()) / B
    clean = sum(int(((sd & has & (seeds == labels))[b]).sum() == sd[b].sum()) for b in range(B))
    exact = sum(int(((fr & has & (perm == labels))[b]).sum() == fr[b].sum()) for b in range(B))
    assert res['clean'] == clean / B and res['exact_free'] == exact / B
    empty = evaluation.seed_result(R.empty_record())
    assert all(math.isnan(empty[k]) for k in ('seed_precision', 'seeds_per_pair', 'free_acc', 'free_refined_acc', 'clean', 'exact_free'))
    no_seeds = evaluation.seed_result(R.fold(R.empty_record(), None, assign, None, labels, nv))
    assert math.isnan(no_seeds['seed_precision']) and no_seeds['seeds_per_pair'] == 0.0 and no_seeds['clean'] == 1.0


def test_record_mirror_and_meter_classes():
    with open(HEADER) as f:
        text = f.read()
    body = re.search(r'typedef struct \{([^}]*)\} fgnn_seed_record;', text).group(1)
    fields = re.findall(r'long long (\w+);', body)
    assert 'double' not in body and tuple(fields) == R.FIELDS == tuple(n for n, _ in _lib.SeedRecord._fields_)
    assert ctypes.sizeof(_lib.SeedRecord) == 8 * len(fields)
    assert all(t is ctypes.c_longlong for _, t in _lib.SeedRecord._fields_)
    assert evaluation.SeedMeter.RECORD is _lib.SeedRecord and evaluation.BinnedSeedMeter.PLAIN is evaluation.SeedMeter
    assert not evaluation.SeedMeter.HEAD_FP64 and not evaluation.BinnedSeedMeter.HEAD_FP64 and evaluation.QapMeter.HEAD_FP64
    with pytest.raises(RuntimeError, match='GPU'):
        evaluation.SeedMeter('cpu')
    with pytest.raises(ValueError):
        evaluation.BinnedSeedMeter._check_bins(0, None)


def test_c_interface_is_declared_and_bound():
    with open(HEADER) as f:
        text = f.read()
    lib = _lib.load()
    for name, nargs in SYMBOLS.items():
        args = re.sub(r'/\*.*?\*/', '', re.search(r'\bint %s\(([^;]*)\);' % name, text).group(1))
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert len(_lib._SIGNATURES[name]) == len(args.split(',')) == nargs, name          # one ctypes type per C parameter
        assert _lib._SIGNATURES[name][-1] is ctypes.c_void_p                                # the stream
    assert _lib._SIGNATURES['fgnn_confident_seeds'][:3] == [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int]
    assert _lib._SIGNATURES['fgnn_confident_seeds'][6:8] == [ctypes.c_int, ctypes.c_float]
