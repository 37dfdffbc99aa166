"""GPU: the kernels of the weighted step -- fgnn_score_ce_bwd_w (csrc/pool_score.hip), fgnn_pair_weights and
fgnn_pair_loss_w (csrc/pair_weights.hip) -- on every form of the score backward, against tests/pair_weights_ref.py on the GPU's own
scores / embeddings, bit for bit against the unweighted entry points under w = 1, and with NaN-filled switched-off pairs.

Inputs carry NaN in their padding, every output is NaN-filled, sized exactly and followed by a NaN-filled guard region.

The library does not expose which backward form a launch took; fgnn_score_ce_bwd_w selects by the rules of launch_score_bwd, which
tests/test_gpu_score_loss.py restates (_bwd_form).  With C = 32 the issue's grid B in {1, 3, 32} x N in {1, 2, 17, 50, 64, 65, 130}
reaches 'staged/8' (N <= 64) and 'blocked/16' (N > 64) only, so three shapes are added by those rules: (64, 50) and (64, 65) for
'staged/4' (B * 4 >= 256) and (48, 130) for 'blocked/64' (B * 4 < 256 and B * 4 * ceil(N / 64) >= 512)."""
import numpy as np
import pytest
import torch

import ce_labels_ref as R
import pair_weights_ref as P
import test_gpu_ce_labels as CL
import test_gpu_score_loss as SL
from graph_neural_net_amd import _lib

pytestmark = pytest.mark.gpu
DEV, NAN = SL.DEV, SL.NAN
Cc = 32
FWD_TOL, BWD_TOL = CL.FWD_TOL, CL.BWD_TOL      # the bounds of the unweighted entry points (tests/test_gpu_ce_labels.py)
SUM_TOL = 1e-6 + 2.0 ** -24                    # fgnn_sum_scale's bound (test_sum_scale: 1e-6 * sum |x|) plus the one rounding of w * p
GRID = [(B, N) for B in (1, 3, 32) for N in (1, 2, 17, 50, 64, 65, 130)] + [(64, 50), (64, 65), (48, 130)]
WORST = {}


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


def test_grid_reaches_every_form():
    forms = {SL._bwd_form(B, Cc, N) for B, N in GRID}
    assert forms == {'staged/8', 'staged/4', 'blocked/16', 'blocked/64'}
    assert SL._bwd_form(64, Cc, 65) == 'staged/4' and SL._bwd_form(48, Cc, 130) == 'blocked/64' and SL._bwd_form(32, Cc, 130) == 'blocked/16'


def _bwd_w(e1d, e2d, sd, ld, nvd, labd, wd, gsd, B, N):
    (d1, g1), (d2, g2) = CL._guarded(B, Cc, N), CL._guarded(B, Cc, N)
    _lib.call('fgnn_score_ce_bwd_w', _lib.ptr(e1d), _lib.ptr(e2d), _lib.ptr(sd), _lib.ptr(ld), _lib.ptr(nvd), _lib.ptr(labd), _lib.ptr(wd),
              _lib.ptr(gsd), B, Cc, N, _lib.ptr(d1), _lib.ptr(d2), _lib.stream_ptr())
    CL._intact(g1, g2)
    return d1.cpu(), d2.cpu()


def _loss_w(pld, rb, wd, B):
    out, g = CL._guarded(1)
    _lib.call('fgnn_pair_loss_w', _lib.ptr(pld), rb, _lib.ptr(wd), B, _lib.ptr(out), _lib.stream_ptr())
    CL._intact(g)
    return out.cpu()


def _weights(B, g):
    """random weights in [0.1, 2.5) with every third pair switched off, the first one included (B = 1: the only one)"""
    w = torch.rand(B, generator=g) * 2.4 + 0.1
    w[0::3] = 0.0
    return w


@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('B,N', GRID)
def test_weighted_score_backward_and_loss(B, N, ragged):
    g = torch.Generator().manual_seed(977 * B + 13 * N + ragged)
    nv = SL._nv_pattern(B, N, g) if ragged else torch.full((B,), N, dtype=torch.int32)      # ragged: N, 0, 1, then random
    nvn = nv.numpy()
    e1, e2 = SL._embeddings(B, Cc, N, nv, g)
    e1d, e2d = e1.to(DEV), e2.to(DEV)
    nvd = nv.to(DEV) if ragged else None
    corner, cols = SL._corner(nv, N), SL._cols(nv, N).expand(B, Cc, N)
    rows = torch.arange(N)[None, :] < nv.long()[:, None]
    gscale = 0.37
    gsd = torch.tensor([gscale], device=DEV)
    rb = _lib.load().fgnn_score_row_blocks(B, N)
    holes = CL._cases(B, N, nv, 1000 * N + B)['holes']             # a permutation with no-target rows; far-out labels in the padding
    ones = torch.ones(B, device=DEV)
    w = _weights(B, g)
    wn = w.double().numpy()
    off = w == 0
    wd = w.to(DEV)
    for lab in (None, holes):
        labd = None if lab is None else torch.from_numpy(lab).to(DEV)
        s0, l0, p0 = CL._fwd(e1d, e2d, nvd, labd, B, Cc, N, rb)
        s0c, l0c = s0.cpu(), l0.cpu()
        sd = s0c.masked_fill(~corner, NAN).to(DEV)
        ld = l0c.masked_fill(~rows, NAN).to(DEV)

        # ---- invariant 2: w = 1 has the bits of the unweighted launches
        u1, u2 = (t.cpu() for t in CL._bwd(e1d, e2d, sd, ld, nvd, labd, gsd, B, Cc, N))
        a1, a2 = _bwd_w(e1d, e2d, sd, ld, nvd, labd, ones, gsd, B, N)
        assert torch.equal(a1, u1) and torch.equal(a2, u2), lab is None
        plain = SL._nan(1)
        _lib.call('fgnn_sum_scale', _lib.ptr(p0), B * rb, 1, 1.0, _lib.ptr(plain), _lib.stream_ptr())
        assert torch.equal(_loss_w(p0, rb, ones, B), plain.cpu())

        # ---- invariant 3: the switched-off pairs hold NaN in scores, lse, partials and embeddings
        offd = off.to(DEV)
        sn = sd.masked_fill(offd[:, None, None], NAN)
        ln = ld.masked_fill(offd[:, None], NAN)
        pn = p0.view(B, rb).masked_fill(offd[:, None], NAN).reshape(-1).contiguous()
        e1n, e2n = e1d.masked_fill(offd[:, None, None], NAN), e2d.masked_fill(offd[:, None, None], NAN)
        d1, d2 = _bwd_w(e1n, e2n, sn, ln, nvd, labd, wd, gsd, B, N)
        loss = _loss_w(pn, rb, wd, B)
        for d in (d1, d2):
            assert torch.equal(d[off], torch.zeros(int(off.sum()), Cc, N)) and not bool(torch.signbit(d[off]).any())
            assert torch.equal(d[~cols], torch.zeros(int((~cols).sum()))) and bool(torch.isfinite(d).all())
        assert bool(torch.isfinite(loss).all())
        # ... and the same launches on the intact inputs give the same bits: nothing of a switched-off pair is used
        b1, b2 = _bwd_w(e1d, e2d, sd, ld, nvd, labd, wd, gsd, B, N)
        assert torch.equal(b1, d1) and torch.equal(b2, d2) and torch.equal(_loss_w(p0, rb, wd, B), loss)
        # run-to-run determinism
        c1, c2 = _bwd_w(e1n, e2n, sn, ln, nvd, labd, wd, gsd, B, N)
        assert torch.equal(c1, d1) and torch.equal(c2, d2) and torch.equal(_loss_w(pn, rb, wd, B), loss)

        # ---- random weights against the fp64 reference on the GPU's own scores, lse and embeddings
        s64, l64 = s0c.double().numpy(), l0c.double().numpy()
        _, _, dS = P.weighted_ce(s64, lab, nvn, wn, gscale, lse=l64)
        r1, r2 = (torch.from_numpy(x) for x in P.weighted_embedding_grads(e1.numpy(), e2.numpy(), dS, nvn, wn))
        _, _, dS1 = P.weighted_ce(s64, lab, nvn, (wn != 0).astype(np.float64), gscale, lse=l64)
        q1, q2 = (torch.from_numpy(x) for x in P.weighted_embedding_grads(e1.numpy(), e2.numpy(), dS1, nvn, wn))
        for d, r, q in ((d1, r1, q1), (d2, r2, q2)):
            # the unweighted bound (max-norm relative to the unweighted gradient of the pairs that count), scaled by max w
            bound = BWD_TOL * float(wn.max()) * float(q.abs().max())
            err = float((d.double() - r)[cols].abs().max()) if bool(cols.any()) else 0.0
            assert err <= bound, (lab is None, err, bound)
            if bound > 0:
                _note('dE', err / bound)
        labn = P.identity_labels(B, N, nvn) if lab is None else lab
        lse_ref, ce_ref, _ = R.batch_ce(s64, labn, nvn)
        scale = R.ce_scale(s64, lse_ref, labn, nvn)
        part = p0.cpu().double().view(B, rb).numpy()
        want_sum = float((wn[:, None] * part)[wn != 0].sum())
        sum_bound = SUM_TOL * float(np.abs(wn[:, None] * part)[wn != 0].sum())
        got = float(loss.double().item())
        assert abs(got - want_sum) <= sum_bound, (got, want_sum, sum_bound)              # the weighted sum of the GPU's partials
        ref_loss = float((wn * ce_ref)[wn != 0].sum())
        bound = FWD_TOL * float((wn * scale).sum()) + sum_bound                           # per pair the unweighted bound times w_b
        assert abs(got - ref_loss) <= bound, (got, ref_loss, bound)
        if bound > 0:
            _note('loss', abs(got - ref_loss) / bound)
            _note('loss sum', abs(got - want_sum) / max(sum_bound, 1e-300))
    print('B=%d N=%d ragged=%s form=%s worst error / bound so far: %s' % (B, N, ragged, SL._bwd_form(B, Cc, N), WORST))


@pytest.mark.parametrize('B,N', [(1, 1), (3, 17), (32, 50), (300, 130)])
def test_pair_weights(B, N):
    """both modes, live in {0, 1, B - 1, B} and None, from a host-set device scalar; n_b = 0 pairs get w = 0 and do not count in D; w to
    1 ulp of fp32 1 / n (with user factors one rounding more: 2 ulp); D exact (integers, resp. sums of quarters)."""
    g = torch.Generator().manual_seed(B + N)
    nv = SL._nv_pattern(B, N, g)
    if B > 4:
        nv[4] = 0
    user = (torch.randint(0, 9, (B,), generator=g).float() * 0.25)
    for ragged in (False, True):
        nvn = nv.numpy() if ragged else np.full(B, N)
        nvd = nv.to(DEV) if ragged else None
        for mode in ('mean', 'mean_of_mean'):
            for u in (None, user):
                for live in sorted({0, 1, B - 1, B}) + [None, B + 7, -3]:
                    ld = None if live is None else torch.tensor([live], dtype=torch.int32, device=DEV)
                    (w, gw), (D, gD) = CL._guarded(B), CL._guarded(1)
                    args = (_lib.ptr(nvd), _lib.ptr(ld), 1 if mode == 'mean_of_mean' else 0, None if u is None else _lib.ptr(u.to(DEV)), B, N,
                            _lib.ptr(w), _lib.ptr(D), _lib.stream_ptr())
                    _lib.call('fgnn_pair_weights', *args)
                    CL._intact(gw, gD)
                    w1, D1 = w.cpu(), D.cpu()
                    wr, Dr = P.reduction_weights(mode, nvn, live, None if u is None else u.numpy())
                    assert D1.item() == Dr, (mode, ragged, live, D1.item(), Dr)
                    ulp = (1 if u is None else 2) * 2.0 ** -23
                    assert bool((np.abs(w1.double().numpy() - wr) <= ulp * np.abs(wr)).all()), (mode, ragged, live)
                    assert bool(((w1.numpy() == 0) == (wr == 0)).all())
                    if mode == 'mean_of_mean' and ragged:
                        assert bool((w1[nv == 0] == 0).all())
                    if mode == 'mean' and u is None:
                        assert bool(((w1 == 0) | (w1 == 1)).all())
                    _lib.call('fgnn_pair_weights', *args)                                    # run-to-run determinism
                    assert torch.equal(w.cpu(), w1) and torch.equal(D.cpu(), D1)


def test_weighted_launches_are_capturable():
    """the three launches in one HIP graph: `live` and the user weights change in their static buffers between replays"""
    B, N = 4, 20
    g = torch.Generator().manual_seed(9)
    nv = torch.full((B,), N, dtype=torch.int32)
    e1, e2 = SL._embeddings(B, Cc, N, nv, g)
    e1d, e2d = e1.to(DEV), e2.to(DEV)
    rb = _lib.load().fgnn_score_row_blocks(B, N)
    gsd = torch.tensor([0.5], device=DEV)
    s, lse, pl = SL._nan(B, N, N), SL._nan(B, N), SL._nan(B * rb)
    _lib.call('fgnn_score_ce_fwd_blocks', _lib.ptr(e1d), _lib.ptr(e2d), None, B, Cc, N, rb, _lib.ptr(s), _lib.ptr(lse), _lib.ptr(pl),
              _lib.stream_ptr())
    live = torch.tensor([B], dtype=torch.int32, device=DEV)
    user = torch.ones(B, device=DEV)
    w, D, loss = SL._nan(B), SL._nan(1), SL._nan(1)
    d1, d2 = SL._nan(B, Cc, N), SL._nan(B, Cc, N)

    def work():
        st = _lib.stream_ptr()
        _lib.call('fgnn_pair_weights', None, _lib.ptr(live), 1, _lib.ptr(user), B, N, _lib.ptr(w), _lib.ptr(D), st)
        _lib.call('fgnn_pair_loss_w', _lib.ptr(pl), rb, _lib.ptr(w), B, _lib.ptr(loss), st)
        _lib.call('fgnn_score_ce_bwd_w', _lib.ptr(e1d), _lib.ptr(e2d), _lib.ptr(s), _lib.ptr(lse), None, None, _lib.ptr(w), _lib.ptr(gsd),
                  B, Cc, N, _lib.ptr(d1), _lib.ptr(d2), st)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        work()
    for k, u in ((B, None), (2, None), (0, None), (3, [0.5, 2.0, 0.0, 1.0]), (B, None)):
        live.fill_(k)
        user.copy_(torch.ones(B) if u is None else torch.tensor(u))
        graph.replay()
        got = [t.clone() for t in (w, D, loss, d1, d2)]
        work()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, (w, D, loss, d1, d2))), k
        assert D.item() == (k if u is None else 2.5) and bool((w[k:] == 0).all()) and bool((d1[k:] == 0).all())
