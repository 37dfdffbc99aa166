"""CPU: the matching decode on real-weighted pairs, off the device.  tests/qap_weighted_ref.py (numpy + SciPy float64 restatement of
toolbox/utils.py:225-256 and of the all_acc_qap arithmetic for real matrices) equals the reference's recorded results
(tests/golden/qap_weighted.npz, made by tests/golden/make_qap_weighted.py); the host route of graph_neural_net_amd.qap with
weighted=True equals the restatement; the new C declarations have their ctypes signatures.  The exact groups compare exactly; the
spectral group (real weights, two evaluation orders of one float64 sum) to 1e-12 relative."""
import os
import re

import numpy as np
import pytest
import torch

import qap_weighted_ref as R
from graph_neural_net_amd import _lib, qap
from util import ROOT

TS, GREEDY_KEYS = R.TS, R.GREEDY_KEYS
GROUPS = R.fixture_groups()
EXACT = [g for g in sorted(GROUPS) if g != 'spectral']


def _pair(g, b):
    n = int(g['nvalid'][b])
    return n, g['a1'][b, :n, :n].astype(np.float64), g['a2'][b, :n, :n].astype(np.float64)


def test_fixture_covers_what_it_must():
    assert set(GROUPS) == set(R.EXACT_GROUPS) | {'spectral'}
    assert sorted(GROUPS['ragged']['nvalid'].tolist())[:2] == [0, 1]
    assert max(g['a1'].shape[1] for g in GROUPS.values()) > 128
    for name in EXACT:
        g = GROUPS[name]
        scale = 8 if name == 'dyadic' else 1
        for k in ('a1', 'a2'):
            w = g[k] * scale
            assert np.array_equal(w, np.round(w)) and w.min() >= 0 and w.max() <= 15, (name, k)
        sym = all(np.array_equal(m, m.transpose(0, 2, 1)) for m in (g['a1'], g['a2']))
        assert sym == (name != 'int_nonsym')
    _, A, B = _pair(GROUPS['int_nonsym'], 1)
    q, t = R.objective(A, B, GROUPS['int_nonsym']['assign0'][1])[:2]
    assert q != t                                                     # all_acc_qap's form and score()'s differ here
    sp = GROUPS['spectral']
    assert not np.array_equal(sp['a1'], np.round(sp['a1'])) and 'T10/s_best' not in sp
    improved = sum(int((GROUPS[n]['T10/T_best'] > 0).sum()) for n in EXACT)
    kept = sum(int(((GROUPS[n]['T10/s_best'] == GROUPS[n]['score0']) & (GROUPS[n]['nvalid'] > 1)).sum()) for n in EXACT)
    quirk = sum(int(((GROUPS[n]['T10/T_best'] == 0) & (GROUPS[n]['T10/acc_best'] != GROUPS[n]['acc'])).sum()) for n in EXACT)
    assert improved >= 3 and kept >= 3 and quirk >= 1, (improved, kept, quirk)


@pytest.mark.parametrize('name', sorted(GROUPS))
def test_restatement_equals_fixture(name):
    g = GROUPS[name]
    for b in range(len(g['nvalid'])):
        n, A, B = _pair(g, b)
        if n == 0:
            assert (g['assign0'][b] == -1).all()
            continue
        cost = -torch.log_softmax(torch.from_numpy(g['scores'][b, :n, :n]), -1).numpy()
        col, acc, q, planted = R.acc_qap_pair(cost, A, B)
        assert np.array_equal(col, g['assign0'][b, :n]) and (g['assign0'][b, n:] == -1).all()
        P = R.perm_matrix(np.arange(n), col)
        assert (acc, q, planted) == (g['acc'][b], g['qap'][b], g['planted'][b])
        if name == 'spectral':                                        # (a BLAS may order the float64 sums of real weights differently)
            assert np.allclose(R.score(A, B, P), (g['score0'][b], g['na'][b], g['nb'][b]), rtol=1e-12, atol=0)
        else:
            assert R.score(A, B, P) == (g['score0'][b], g['na'][b], g['nb'][b])
        qi, ti, pl, na, nb = R.objective(A, B, col)
        want = (g['qap'][b], 2 * g['score0'][b], g['planted'][b], 2 * g['na'][b], 2 * g['nb'][b])
        if name == 'spectral':
            assert np.allclose((qi, ti, pl, na, nb), want, rtol=1e-12, atol=0)
            continue
        assert (qi, ti, pl, na, nb) == want
        for T in TS:
            got = R.greedy_qap(A, B, P, T)
            assert got[:5] == tuple(g['T%d/%s' % (T, k)][b] for k in GREEDY_KEYS), (name, b, T)
            assert R.score(A, B, R.perm_matrix(np.arange(n), got[5]))[0] == got[0]        # the sixth value is the matching of s_best


def _as_torch(g, channels):
    """the group as CPU tensors; channels > 0: (B, C, N, N) batches whose channel 0 holds the matrices (the others: noise)"""
    a1, a2 = torch.from_numpy(g['a1']), torch.from_numpy(g['a2'])
    if channels:
        gen = torch.Generator().manual_seed(1)
        x1 = torch.randn(a1.shape[0], channels, *a1.shape[1:], generator=gen)
        x2 = torch.randn(a1.shape[0], channels, *a1.shape[1:], generator=gen)
        x1[:, 0], x2[:, 0] = a1, a2
        a1, a2 = x1, x2
    ragged = bool((g['nvalid'] != g['a1'].shape[1]).any())
    return a1, a2, torch.from_numpy(g['assign0']), torch.from_numpy(g['nvalid']) if ragged else None, torch.from_numpy(g['scores'])


@pytest.mark.parametrize('channels', [0, 4])
@pytest.mark.parametrize('name', sorted(GROUPS))
def test_host_route_equals_restatement_and_fixture(name, channels):
    g = GROUPS[name]
    a1, a2, a0, nvalid, scores = _as_torch(g, channels)
    acc, q, planted = qap.all_acc_qap(scores, a1, a2, nvalid, weighted=True)
    assert acc.dtype == torch.int64 and q.dtype == planted.dtype == torch.float64
    assert np.array_equal(acc.numpy(), g['acc']) and np.array_equal(q.numpy(), g['qap']) and np.array_equal(planted.numpy(), g['planted'])
    obj = qap.qap_objective(a1, a2, a0, nvalid, weighted=True)
    assert set(obj) == {'qap', 'planted', 'na', 'nb'}
    assert np.array_equal(obj['qap'].numpy(), g['qap']) and np.array_equal(obj['planted'].numpy(), g['planted'])
    for b in range(len(g['nvalid'])):
        n, A, B = _pair(g, b)
        if name == 'spectral':
            assert np.allclose((obj['na'][b].item(), obj['nb'][b].item()), (A.sum(), B.sum()), rtol=1e-12, atol=0)
        else:
            assert (obj['na'][b].item(), obj['nb'][b].item()) == (A.sum(), B.sum())
    for T in TS:
        out = qap.greedy_qap(a1, a2, a0, T, nvalid, weighted=True)
        for b in range(len(g['nvalid'])):
            n, A, B = _pair(g, b)
            perm = out['perm'][b].numpy()
            assert sorted(perm[:n].tolist()) == list(range(n)) and (perm[n:] == -1).all()
            if n == 0:
                assert tuple(out[k][b].item() for k in GREEDY_KEYS) == (0, 0, 0, 0, 0)
                continue
            want = R.greedy_qap(A, B, R.perm_matrix(np.arange(n), g['assign0'][b, :n]), T)          # also on the spectral group
            assert tuple(out[k][b].item() for k in GREEDY_KEYS) == want[:5], (name, T, b)
            assert np.array_equal(perm[:n], want[5])
        if name != 'spectral':
            for k in GREEDY_KEYS:
                want = g['T%d/%s' % (T, k)]
                assert out[k].dtype == (torch.float64 if want.dtype == np.float64 else torch.int64)
                assert np.array_equal(out[k].numpy(), want), (name, T, k)


def test_host_route_conventions():
    g = GROUPS['int_nonsym']
    a1, a2, a0, _, _ = _as_torch(g, 0)
    holed = a0.clone()
    holed[1, 4] = -1
    q = qap.qap_objective(a1, a2, holed, weighted=True)['qap']
    assert q[1].item() == -1.0 and q[0].item() == g['qap'][0]
    with pytest.raises(RuntimeError, match='incomplete'):
        qap.greedy_qap(a1, a2, holed, 1, weighted=True)
    with pytest.raises(ValueError):
        qap.greedy_qap(a1, a2, a0, -1, weighted=True)
    with pytest.raises(RuntimeError, match='weighted input'):
        qap.qap_objective(a1.long(), a2.long(), a0, weighted=True)
    # without the keyword a weighted batch is refused as before
    x = torch.zeros(a1.shape[0], 2, *a1.shape[1:])
    x[:, 0] = a1
    with pytest.raises(RuntimeError, match='NOT the tensor representation'):
        qap.qap_objective(x, x, a0)
    # garbage outside the corners of a ragged batch is never looked at
    r = GROUPS['ragged']
    b1, b2, r0, nv, _ = _as_torch(r, 0)
    n1, n2 = b1.clone(), b2.clone()
    for b, n in enumerate(r['nvalid']):
        n1[b, n:, :], n1[b, :, n:], n2[b, n:, :], n2[b, :, n:] = float('nan'), float('nan'), float('nan'), float('nan')
    clean, dirty = qap.greedy_qap(b1, b2, r0, 10, nv, weighted=True), qap.greedy_qap(n1, n2, r0, 10, nv, weighted=True)
    assert all(torch.equal(clean[k], dirty[k]) for k in clean)


def test_new_declarations_have_signatures():
    hdr = open(os.path.join(ROOT, 'include', 'fgnn_hip.h')).read()
    new = ['fgnn_qapw_objective', 'fgnn_qapw_improve_cost', 'fgnn_greedy_qapw_ws_bytes', 'fgnn_greedy_qapw']
    lib = _lib.load()
    for name in new:
        m = re.search(r'\b(int|long long)\s+%s\s*\(([^;]*)\);' % name, hdr)
        assert m, '%s is not declared in include/fgnn_hip.h' % name
        assert name in _lib._SIGNATURES and hasattr(lib, name)
        assert len(_lib._SIGNATURES[name]) == len(m.group(2).split(',')), name            # one ctypes type per C parameter
        assert (_lib._RESTYPES.get(name) is not None) == (m.group(1) == 'long long')
    assert _lib.FGNN_QAPW_MAX_N == int(re.search(r'#define FGNN_QAPW_MAX_N (\d+)', hdr).group(1))
    assert lib.fgnn_greedy_qapw_ws_bytes(8, 256) >= 8 * 256 * 256 * 4 + 8 * 256 * 4 + 2 * 8 * 4
    assert lib.fgnn_greedy_qapw_ws_bytes(0, 5) == 0
