"""GPU: fgnn_sinkhorn through qap.sinkhorn against the float64 restatement of tests/sinkhorn_ref.py.

Shapes (sinkhorn_ref.SIZES): B = 3 ragged pairs at N = 1, 2, 31, 32, 33 (half a wave and its neighbours), 64 and 65 (the 64-row
form and the first size of the 192-row form), 192 and 193 (FGNN_SINKHORN_LDS_MAX_N: the last size whose scores stay in LDS and
the first that re-reads them) and 256; every batch has a pair of N vertices, a ragged one and one of 0 or 1 vertices, and NaN
around every corner.  Scores are uniform in [-32, 32] at tau = 1, plus [-1, 1] at tau = 0.05 (|S / tau| <= 20)."""
import functools

import numpy as np
import pytest
import torch

import sinkhorn_ref as R
from graph_neural_net_amd import _lib, qap
from graph_neural_net_amd.masked import MaskedTensor

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# The largest |P - P_ref| against tests/sinkhorn_ref.py over every case of this file, measured on an MI355X: 8.575e-07 (N = 192,
# tau = 1; the other cases of test_against_the_restatement gave 4.2e-07 .. 7.7e-07, the degenerate batches below 1e-07).  The
# tolerance is 4 x that, since fp32 exp / log differ between ROCm builds.  DESIGN.md section 11.6 records the figure.
MEASURED_MAX_ERR = 8.575e-7
TOL = 4 * MEASURED_MAX_ERR
CASES = [(N, 1.0, 32.0) for N in R.SIZES] + [(33, 0.05, 1.0), (193, 0.05, 1.0)]


@functools.lru_cache(maxsize=None)
def _case(N, tau, bound, iters=20):
    """-> (scores, nvalid, (P, err, status) of the restatement), computed once and shared; nobody writes to them"""
    s, nv = R.batch(N, bound=bound)
    return s, nv, R.sinkhorn(s, nv, tau, iters)


def _run(s, nv, **kw):
    return qap.sinkhorn(torch.from_numpy(s).to(DEV), None if nv is None else torch.from_numpy(np.asarray(nv)).to(DEV), **kw)


@pytest.mark.parametrize('N,tau,bound', CASES)
def test_against_the_restatement(N, tau, bound):
    s, nv, (P, err, status) = _case(N, tau, bound)
    out = _run(s, nv, tau=tau, iters=20)
    assert out['P'].dtype == torch.float32 and out['err'].dtype == torch.float32 and out['status'].dtype == torch.int64
    got = out['P'].cpu().numpy().astype(np.float64)
    assert out['status'].cpu().tolist() == status.tolist()
    worst = float(np.abs(got - P).max())
    print('N %d tau %g: max |P - P_ref| = %.3e, max |err - err_ref| = %.3e' % (N, tau, worst, np.abs(out['err'].cpu().numpy() - err).max()))
    assert worst <= TOL
    # structure
    e = out['err'].cpu().numpy().astype(np.float64)
    for b, n in enumerate(nv):
        assert not got[b, n:].any() and not got[b, :, n:].any()                       # exactly zero around the corner
        if n == 0:
            assert status[b] == 1 and e[b] == 0.0
            continue
        assert np.abs(got[b, :n, :n].sum(0) - 1.0).max() <= 1e-4                      # g came last: the columns
        assert abs(e[b] - np.abs(got[b, :n, :n].sum(1) - 1.0).max()) <= 1e-5          # err is the row deviation of the P written
    # determinism: a second launch, and every pair alone in a batch of one
    again = _run(s, nv, tau=tau, iters=20)
    assert all(torch.equal(out[k], again[k]) for k in out)
    for b in (0, 1):
        one = _run(s[b:b + 1], nv[b:b + 1], tau=tau, iters=20)
        assert torch.equal(one['P'][0], out['P'][b]) and torch.equal(one['err'][0], out['err'][b])


def test_position_in_the_batch_strided_views_and_masked_tensors():
    N = 65
    s, nv, _ = _case(N, 1.0, 32.0)
    out = _run(s, nv)
    # the same pairs in another order inside a larger batch
    order = [2, 0, 1, 0, 2]
    big = _run(s[order], nv[order])
    for k, b in enumerate(order):
        assert torch.equal(big['P'][k], out['P'][b]) and torch.equal(big['err'][k], out['err'][b])
    # a pitched, non-contiguous view is read in place; a transposed one is copied
    wide = torch.full((3, N + 3, N + 5), float('nan'), device=DEV)
    wide[:, :N, :N] = torch.from_numpy(s).to(DEV)
    view = wide[:, :N, :N]
    assert not view.is_contiguous() and qap._chan0_ok(view)
    nvd = torch.from_numpy(nv).to(DEV)
    strided = qap.sinkhorn(view, nvd)
    assert all(torch.equal(strided[k], out[k]) for k in out)
    st = torch.from_numpy(np.ascontiguousarray(np.swapaxes(s, 1, 2))).to(DEV).transpose(1, 2)
    assert not st.is_contiguous() and not qap._chan0_ok(st)
    assert all(torch.equal(v, out[k]) for k, v in qap.sinkhorn(st, nvd).items())
    # a MaskedTensor brings its vertex counts; float64 scores are converted
    mt = qap.sinkhorn(MaskedTensor(torch.from_numpy(s).to(DEV), nvd, (1, 2)))
    assert all(torch.equal(mt[k], out[k]) for k in out)
    assert all(torch.equal(v, out[k]) for k, v in qap.sinkhorn(torch.from_numpy(s).to(DEV).double(), nvd).items())
    # nvalid=None: the whole matrix
    full = np.ascontiguousarray(s[:1])
    whole = _run(full, None)
    assert torch.equal(whole['P'], out['P'][:1])


@pytest.mark.parametrize('N', [33, 193, 256])
def test_many_iterations_converge_on_a_positive_corner(N):
    s = np.random.default_rng(N).uniform(-2, 2, (2, N, N)).astype(np.float32)
    out = _run(s, [N, N - 7], iters=200)
    print('N %d iters 200: err %r' % (N, out['err'].cpu().tolist()))
    assert out['status'].cpu().tolist() == [0, 0] and float(out['err'].max()) < 1e-4
    P = out['P'].cpu().numpy().astype(np.float64)
    assert np.abs(P[0].sum(0) - 1).max() <= 1e-4 and np.abs(P[0].sum(1) - 1).max() <= 1e-4


@pytest.mark.parametrize('N', [9, 70, 200])
def test_degenerate_pairs_leave_their_neighbours_alone(N):
    rng = np.random.default_rng(5 + N)
    clean = rng.uniform(-3, 3, (8, N, N)).astype(np.float32)
    nv = np.array([N, N, N - 2, N, N - 1, 0, N, N - 3])
    s = clean.copy()
    s[0, N // 2, 1] = np.nan                               # a NaN in the corner
    s[1, 0, N - 1] = np.inf                                # a +inf
    s[2, 3, :] = -np.inf                                   # a row of -inf
    s[4, :, 2] = -np.inf                                   # a column of -inf
    # pair 3: clean; pair 5: n = 0; pair 6: isolated -inf entries; pair 7: a NaN outside its corner only
    s[6, 1, 2] = s[6, N - 1, N - 1] = s[6, 4, 0] = -np.inf
    s[7, N - 1, 0] = s[7, 0, N - 2] = np.nan
    out, ref = _run(s, nv), _run(clean, nv)
    assert out['status'].cpu().tolist() == [1, 1, 1, 0, 1, 1, 0, 0] and ref['status'].cpu().tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
    P = out['P'].cpu().numpy()
    for b in (0, 1, 2, 4, 5):
        n = int(nv[b])
        assert float(out['err'][b]) == 0.0
        assert not P[b, n:].any() and not P[b, :, n:].any()
        if n:
            assert (P[b, :n, :n] == np.float32(1.0 / n)).all()
    for b in (3, 7):                                       # the neighbours, bit for bit
        assert torch.equal(out['P'][b], ref['P'][b]) and torch.equal(out['err'][b], ref['err'][b])
    assert P[6, 1, 2] == 0 and P[6, N - 1, N - 1] == 0 and P[6, 4, 0] == 0 and np.isfinite(P).all()
    want = R.sinkhorn(s, nv, 1.0, 20)
    worst = float(np.abs(P.astype(np.float64) - want[0]).max())
    print('N %d degenerate batch: max |P - P_ref| = %.3e' % (N, worst))
    assert want[2].tolist() == out['status'].cpu().tolist() and worst <= TOL
    assert np.abs(P[6].astype(np.float64).sum(0) - 1).max() <= 1e-4


def test_the_entry_point_reports_argument_errors():
    s = torch.zeros(2, 4, 4, device=DEV)
    P, err, st = torch.empty(2, 4, 4, device=DEV), torch.empty(2, device=DEV), torch.empty(2, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    args = lambda **kw: (_lib.ptr(s), kw.get('stride', 16), kw.get('ld', 4), None, 2, kw.get('N', 4), kw.get('tau', 1.0),
                         kw.get('iters', 20), _lib.ptr(P), _lib.ptr(err), _lib.ptr(st), _lib.stream_ptr())
    assert lib.fgnn_sinkhorn(*args()) == 0
    for kw, word in (({'tau': 0.0}, 'tau'), ({'iters': 0}, 'iters'), ({'ld': 3}, 'ld'), ({'stride': 15}, 'pair_stride'),
                     ({'N': 257, 'ld': 257, 'stride': 257 * 257}, 'at most 256')):
        assert lib.fgnn_sinkhorn(*args(**kw)) == 1 and word in _lib.last_error()
    torch.cuda.synchronize()
