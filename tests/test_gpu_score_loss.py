"""GPU: the end of every training step -- the siamese score product, the row log-sum-exp and cross-entropy against the
identity matching, their gradients, the loss reduction and the arg-max accuracy (csrc/pool_score.hip, csrc/norm.hip,
csrc/train_ops.hip) -- against fp64 references on the CPU, on every launch form the host code picks from (B, C, N).

Inputs carry NaN in their padding (columns and rows >= nvalid) and outputs are NaN-filled before each call, so a kernel that
reads padding or leaves an output element unwritten fails here."""
import math

import numpy as np
import pytest
import torch

from graph_neural_net_amd import _lib
from util import rel

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
SPLIT = _lib.FGNN_SCORE_SPLIT
LDS_MAX = 160 * 1024            # bytes of LDS a workgroup may opt in to on gfx950


def _nv_pattern(B, N, g):
    """Ragged vertex counts: N first, then 0 and 1 (when B allows), the rest random in [1, N]."""
    nv = torch.randint(1, N + 1, (B,), generator=g, dtype=torch.int32)
    for k, v in enumerate((N, 0, 1)[:B]):
        nv[k] = v
    return nv


def _corner(nv, N):
    """(B, N, N) bool: the valid block of each graph."""
    r = torch.arange(N)
    m = r[None, :] < nv.long()[:, None]
    return m[:, :, None] & m[:, None, :]


def _cols(nv, N):
    """(B, 1, N) bool: valid columns of a (B, C, N) embedding."""
    return (torch.arange(N)[None, :] < nv.long()[:, None])[:, None, :]


def _embeddings(B, Cc, N, nv, g):
    """(B, C, N) fp32 pair embeddings scaled so that scores have a standard deviation of about 2; NaN in the padding."""
    s = math.sqrt(2.0) / Cc ** 0.25
    e1 = torch.randn(B, Cc, N, generator=g) * s
    e2 = torch.randn(B, Cc, N, generator=g) * s
    m = _cols(nv, N)
    return e1.masked_fill(~m, NAN), e2.masked_fill(~m, NAN)


def _ref_fwd(e1, e2, nv):
    """fp64: scores (zero outside the valid corner), lse (zero on padding rows) and the per-pair CE sum."""
    B, _, N = e1.shape
    m = _cols(nv, N)
    a, b = e1.double().masked_fill(~m, 0), e2.double().masked_fill(~m, 0)
    s = torch.matmul(a.transpose(1, 2), b)
    lse, ce = _ref_ce(s, nv)
    return s, lse, ce


def _ref_ce(s, nv):
    """fp64 row logsumexp over the valid columns and the per-pair CE sum against arange(n)."""
    B, N, _ = s.shape
    lse = torch.zeros(B, N, dtype=torch.float64)
    ce = torch.zeros(B, dtype=torch.float64)
    for b in range(B):
        n = int(nv[b])
        if n:
            blk = s[b, :n, :n].double()
            lse[b, :n] = torch.logsumexp(blk, -1)
            ce[b] = (lse[b, :n] - blk.diagonal()).sum()
    return lse, ce


def _ce_scale(s, lse, nv):
    """Per pair sum of |lse_i| + |s_ii| over the valid rows: the magnitude an fp32 CE sum is rounded against."""
    B, N, _ = s.shape
    out = torch.zeros(B, dtype=torch.float64)
    for b in range(B):
        n = int(nv[b])
        out[b] = (lse[b, :n].abs() + s[b, :n, :n].diagonal().double().abs()).sum()
    return out


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. forward: fgnn_score_ce_fwd_blocks on every row-block form
# ---------------------------------------------------------------------------------------------------------------------------

def _row_blocks(B, N):
    """Restatement of fgnn_score_row_blocks."""
    return SPLIT if B * SPLIT >= 512 else (N + 3) // 4


def _fwd_lds(Cc, N, row_blocks):
    """Restatement of the LDS size fgnn_score_ce_fwd_blocks asks for (and refuses above LDS_MAX)."""
    rows = -(-N // row_blocks)
    return (Cc * N + Cc * rows + rows * N + 4) * 4


def _fwd(e1d, e2d, nvd, B, Cc, N, row_blocks):
    scores, lse, pl = _nan(B, N, N), _nan(B, N), _nan(B * row_blocks)
    _lib.call('fgnn_score_ce_fwd_blocks', _lib.ptr(e1d), _lib.ptr(e2d), _lib.ptr(nvd), B, Cc, N, row_blocks,
              _lib.ptr(scores), _lib.ptr(lse), _lib.ptr(pl), _lib.stream_ptr())
    return scores.cpu(), lse.cpu(), pl.cpu()


def _row_block_forms(N):
    # 1, FGNN_SCORE_SPLIT, the small-batch choice, the large-batch choice, one row per block, three empty blocks at the end
    return sorted({1, SPLIT, _row_blocks(1, N), _row_blocks(128, N), N, N + 3})


FWD_SHAPES = [(c, n) for c in (1, 3, 32, 33, 64) for n in (1, 2, 63, 64, 65, 128, 200, 256)]


@pytest.mark.parametrize('Cc,N', FWD_SHAPES)
def test_score_ce_fwd_row_blocks(Cc, N):
    assert _lib.load().fgnn_score_row_blocks(1, N) == _row_blocks(1, N)
    assert _lib.load().fgnn_score_row_blocks(128, N) == _row_blocks(128, N)
    B = 5
    g = torch.Generator().manual_seed(7919 * Cc + N)
    nv = _nv_pattern(B, N, g)
    e1, e2 = _embeddings(B, Cc, N, nv, g)
    s_ref, lse_ref, ce_ref = _ref_fwd(e1, e2, nv)
    scale = _ce_scale(s_ref, lse_ref, nv)
    corner = _corner(nv, N)
    rows = torch.arange(N)[None, :] < nv.long()[:, None]
    e1d, e2d, nvd = e1.to(DEV), e2.to(DEV), nv.to(DEV)
    first = None
    ran = 0
    for rb in _row_block_forms(N):
        if _fwd_lds(Cc, N, rb) > LDS_MAX:
            with pytest.raises(RuntimeError, match='fgnn_score_ce_fwd'):
                _fwd(e1d, e2d, nvd, B, Cc, N, rb)
            continue
        ran += 1
        s, lse, pl = _fwd(e1d, e2d, nvd, B, Cc, N, rb)
        assert rel(s[corner], s_ref[corner]) < 2e-6, rb
        assert torch.equal(s[~corner], torch.zeros(int((~corner).sum()))), rb
        assert rel(lse[rows], lse_ref[rows]) < 2e-6, rb
        assert torch.equal(lse[~rows], torch.zeros(int((~rows).sum()))), rb
        pair = pl.double().view(B, rb).sum(1)
        assert bool(((pair - ce_ref).abs() <= 2e-6 * scale).all()), (rb, pair, ce_ref)
        assert pair[1] == 0 and pair[2] == 0, rb                  # nv = 0 and nv = 1: no loss
        if first is None:
            first = (s, lse)
        else:                                                     # same fmaf order and per-row wave reduction
            assert torch.equal(s, first[0]) and torch.equal(lse, first[1]), rb
    assert ran >= 2


@pytest.mark.parametrize('Cc,N', [(32, 50), (33, 65), (64, 128), (3, 200)])
def test_score_ce_fwd_pair_alone_equals_pair_in_batch(Cc, N):
    """Pair k of a B = 128 batch (FGNN_SCORE_SPLIT row blocks) has the scores and lse it has alone (ceil(N / 4) blocks)."""
    B, k = 128, 77
    g = torch.Generator().manual_seed(N)
    nv = torch.randint(1, N + 1, (B,), generator=g, dtype=torch.int32)
    e1, e2 = _embeddings(B, Cc, N, nv, g)
    e1d, e2d, nvd = e1.to(DEV), e2.to(DEV), nv.to(DEV)
    scores, lse, pl = _nan(B, N, N), _nan(B, N), _nan(B * SPLIT)
    _lib.call('fgnn_score_ce_fwd', _lib.ptr(e1d), _lib.ptr(e2d), _lib.ptr(nvd), B, Cc, N, _lib.ptr(scores), _lib.ptr(lse),
              _lib.ptr(pl), _lib.stream_ptr())
    rb = _lib.load().fgnn_score_row_blocks(1, N)
    assert rb != SPLIT
    s1, l1, _ = _fwd(e1d[k:k + 1].contiguous(), e2d[k:k + 1].contiguous(), nvd[k:k + 1].contiguous(), 1, Cc, N, rb)
    assert torch.equal(scores[k].cpu(), s1[0])
    assert torch.equal(lse[k].cpu(), l1[0])
    s_ref, _, ce_ref = _ref_fwd(e1, e2, nv)
    assert rel(scores.cpu(), s_ref) < 2e-6
    assert rel(pl.cpu().double().sum(), ce_ref.sum()) < 2e-6


def test_score_ce_fwd_refuses_lds_overflow():
    """C * N beyond what LDS can stage: a host-side RuntimeError naming the entry point, no launch."""
    B, Cc, N = 1, 64, 700
    assert _fwd_lds(Cc, N, SPLIT) > LDS_MAX
    e1, e2 = torch.zeros(B, Cc, N, device=DEV), torch.zeros(B, Cc, N, device=DEV)
    scores, lse, pl = _nan(B, N, N), _nan(B, N), _nan(B * SPLIT)
    with pytest.raises(RuntimeError, match='fgnn_score_ce_fwd'):
        _lib.call('fgnn_score_ce_fwd', _lib.ptr(e1), _lib.ptr(e2), None, B, Cc, N, _lib.ptr(scores), _lib.ptr(lse),
                  _lib.ptr(pl), _lib.stream_ptr())
    assert bool(torch.isnan(scores.cpu()).all())


# ---------------------------------------------------------------------------------------------------------------------------
# 2. backward: fgnn_score_ce_bwd and fgnn_score_bwd on the four forms of launch_score_bwd
# ---------------------------------------------------------------------------------------------------------------------------

def _bwd_form(B, Cc, N):
    """Restatement of the selection rule of launch_score_bwd (csrc/pool_score.hip)."""
    def lds(csplit, stage):
        cper = -(-Cc // csplit)
        return (2 * cper * N + (N * (N + 1) if stage else 0)) * 4
    if lds(4, True) <= LDS_MAX and (N <= 64 or B * 4 >= 256):
        return 'staged/8' if B * 4 < 256 else 'staged/4'
    return 'blocked/64' if B * 4 * (-(-N // 64)) >= 512 else 'blocked/16'


BWD_SHAPES = [(3, 32, 50), (3, 1, 50), (5, 33, 9),
              (64, 32, 50), (64, 3, 50), (64, 32, 120), (64, 33, 120), (64, 1, 200),
              (8, 32, 200), (2, 64, 256), (8, 33, 200), (2, 3, 130),
              (32, 32, 200), (64, 32, 200), (32, 3, 200), (48, 33, 129)]


def test_bwd_shapes_reach_every_form():
    forms = {_bwd_form(*s) for s in BWD_SHAPES}
    assert forms == {'staged/8', 'staged/4', 'blocked/16', 'blocked/64'}
    # the 4-group staging above N = 64, with more than 64 KiB of LDS
    assert _bwd_form(64, 32, 120) == 'staged/4' and (2 * 8 * 120 + 120 * 121) * 4 > 64 * 1024


def _ref_grads(e1, e2, nv, ds):
    """fp64 de1 = e2 dS^T, de2 = e1 dS per pair (dS zero outside the corner), zero on padding columns."""
    m = _cols(nv, e1.shape[-1])
    a, b = e1.double().masked_fill(~m, 0), e2.double().masked_fill(~m, 0)
    return torch.matmul(b, ds.transpose(1, 2)), torch.matmul(a, ds)


def _ce_inputs(e1, e2, nv):
    """fp32 scores and lse rounded from fp64, NaN in their padding (the kernels must not read it)."""
    s_ref, lse_ref, _ = _ref_fwd(e1, e2, nv)
    N = s_ref.shape[-1]
    rows = torch.arange(N)[None, :] < nv.long()[:, None]
    return s_ref.float().masked_fill(~_corner(nv, N), NAN), lse_ref.float().masked_fill(~rows, NAN)


def _bwd(name, e1d, e2d, first, nvd, B, Cc, N):
    d1, d2 = _nan(B, Cc, N), _nan(B, Cc, N)
    if name == 'fgnn_score_ce_bwd':
        scores, lse, gs = first
        _lib.call(name, _lib.ptr(e1d), _lib.ptr(e2d), _lib.ptr(scores), _lib.ptr(lse), _lib.ptr(nvd), _lib.ptr(gs),
                  B, Cc, N, _lib.ptr(d1), _lib.ptr(d2), _lib.stream_ptr())
    else:
        _lib.call(name, _lib.ptr(e1d), _lib.ptr(e2d), _lib.ptr(first), _lib.ptr(nvd), B, Cc, N, _lib.ptr(d1), _lib.ptr(d2),
                  _lib.stream_ptr())
    return d1, d2


@pytest.mark.parametrize('B,Cc,N', BWD_SHAPES)
def test_score_bwd_forms(B, Cc, N):
    g = torch.Generator().manual_seed(31 * B + 7 * Cc + N)
    nv = _nv_pattern(B, N, g)
    e1, e2 = _embeddings(B, Cc, N, nv, g)
    cols = _cols(nv, N).expand(B, Cc, N)
    corner = _corner(nv, N)
    e1d, e2d, nvd = e1.to(DEV), e2.to(DEV), nv.to(DEV)
    gscale = 0.37

    # CE mode against fp64 autograd of gscale * sum of the per-pair CE
    s32, lse32 = _ce_inputs(e1, e2, nv)
    a = e1.double().masked_fill(~_cols(nv, N), 0).requires_grad_(True)
    b = e2.double().masked_fill(~_cols(nv, N), 0).requires_grad_(True)
    s = torch.matmul(a.transpose(1, 2), b)
    loss = sum(torch.nn.functional.cross_entropy(s[k, :n, :n], torch.arange(n), reduction='sum')
               for k, n in enumerate(nv.tolist()) if n)
    (gscale * loss).backward()
    sd, ld = s32.to(DEV), lse32.to(DEV)
    gsd = torch.tensor([gscale], device=DEV)
    d1, d2 = _bwd('fgnn_score_ce_bwd', e1d, e2d, (sd, ld, gsd), nvd, B, Cc, N)
    d1, d2 = d1.cpu(), d2.cpu()
    assert rel(d1[cols], a.grad[cols]) < 5e-6 and rel(d2[cols], b.grad[cols]) < 5e-6
    assert torch.equal(d1[~cols], torch.zeros(int((~cols).sum()))) and torch.equal(d2[~cols], d1[~cols])

    # composition: fgnn_score_bwd(fgnn_ce_bwd(scores, lse)) is fgnn_score_ce_bwd bit for bit
    dsd = _nan(B, N, N)
    _lib.call('fgnn_ce_bwd', _lib.ptr(sd), _lib.ptr(ld), _lib.ptr(nvd), _lib.ptr(gsd), B, N, _lib.ptr(dsd), _lib.stream_ptr())
    c1, c2 = _bwd('fgnn_score_bwd', e1d, e2d, dsd, nvd, B, Cc, N)
    assert torch.equal(c1.cpu(), d1) and torch.equal(c2.cpu(), d2)

    # plain mode on a general dS (fp32, NaN in its padding) against the fp64 products of the same values
    ds = torch.randn(B, N, N, generator=g).masked_fill(~corner, NAN)
    r1, r2 = _ref_grads(e1, e2, nv, ds.double().masked_fill(~corner, 0))
    p1, p2 = _bwd('fgnn_score_bwd', e1d, e2d, ds.to(DEV), nvd, B, Cc, N)
    p1, p2 = p1.cpu(), p2.cpu()
    assert rel(p1[cols], r1[cols]) < 5e-6 and rel(p2[cols], r2[cols]) < 5e-6
    assert torch.equal(p1[~cols], torch.zeros(int((~cols).sum()))) and torch.equal(p2[~cols], p1[~cols])


@pytest.mark.parametrize('Cc,N,B', [(32, 50, 64), (3, 50, 64), (32, 120, 64), (33, 200, 32), (32, 200, 64), (1, 200, 64)])
@pytest.mark.parametrize('name', ['fgnn_score_ce_bwd', 'fgnn_score_bwd'])
def test_score_bwd_pair_alone_equals_pair_in_batch(name, Cc, N, B):
    """All four forms accumulate fmaf in the same j / i order over the same dS expression: one pair's gradient does not
    depend on the form its batch takes."""
    k = B // 3
    g = torch.Generator().manual_seed(N + Cc)
    nv = torch.randint(1, N + 1, (B,), generator=g, dtype=torch.int32)
    nv[k] = N - 3
    e1, e2 = _embeddings(B, Cc, N, nv, g)
    s32, lse32 = _ce_inputs(e1, e2, nv)
    ds = torch.randn(B, N, N, generator=g).masked_fill(~_corner(nv, N), NAN)
    gsd = torch.tensor([1.7], device=DEV)
    alone, batch = _bwd_form(1, Cc, N), _bwd_form(B, Cc, N)
    assert alone in ('staged/8', 'blocked/16') and batch in ('staged/4', 'blocked/64'), (alone, batch)

    def run(sl, Bn):
        dev = [t[sl].contiguous().to(DEV) for t in (e1, e2, nv, s32, lse32, ds)]
        first = (dev[3], dev[4], gsd) if name == 'fgnn_score_ce_bwd' else dev[5]
        d1, d2 = _bwd(name, dev[0], dev[1], first, dev[2], Bn, Cc, N)
        return d1.cpu(), d2.cpu()

    b1, b2 = run(slice(None), B)
    a1, a2 = run(slice(k, k + 1), 1)
    assert not torch.isnan(a1).any() and not torch.isnan(b1).any()
    assert torch.equal(a1[0], b1[k]) and torch.equal(a2[0], b2[k]), (alone, batch)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. standalone CE (fgnn_ce_fwd / fgnn_ce_bwd) and the module loss
# ---------------------------------------------------------------------------------------------------------------------------

def _hard_scores(B, N, nv, g):
    """Per pair a different row regime: plain, magnitude 1e4 (naive exp overflows), -1e4 (underflows), exact ties,
    saturated (one entry 60 above the rest, often on the diagonal)."""
    s = torch.randn(B, N, N, generator=g) * 3
    for b in range(B):
        kind = b % 5
        if kind == 1:
            s[b] = 1e4 + s[b]
        elif kind == 2:
            s[b] = -1e4 + s[b]
        elif kind == 3:
            s[b] = torch.randint(-2, 3, (N, N), generator=g).float()
        elif kind == 4:
            j = torch.randint(0, max(int(nv[b]), 1), (N,), generator=g)
            j[::2] = torch.arange(N)[::2].clamp(max=max(int(nv[b]) - 1, 0))
            s[b, torch.arange(N), j] += 60.0
    return s.masked_fill(~_corner(nv, N), NAN)


def _ce_fwd(sd, nvd, B, N):
    lse, pl = _nan(B, N), _nan(B)
    _lib.call('fgnn_ce_fwd', _lib.ptr(sd), _lib.ptr(nvd), B, N, _lib.ptr(lse), _lib.ptr(pl), _lib.stream_ptr())
    return lse, pl


@pytest.mark.parametrize('N', [1, 2, 50, 64, 65, 200, 300])
def test_ce_fwd_bwd(N):
    B = 10
    g = torch.Generator().manual_seed(100 + N)
    nv = _nv_pattern(B, N, g)
    s = _hard_scores(B, N, nv, g)
    sd, nvd = s.to(DEV), nv.to(DEV)
    lse, pl = _ce_fwd(sd, nvd, B, N)
    lse_c, pl_c = lse.cpu(), pl.cpu()
    lse_ref, ce_ref = _ref_ce(s.masked_fill(~_corner(nv, N), 0).double(), nv)
    rows = torch.arange(N)[None, :] < nv.long()[:, None]
    assert rel(lse_c[rows], lse_ref[rows]) < 2e-6
    assert torch.equal(lse_c[~rows], torch.zeros(int((~rows).sum())))
    for b in range(B):                     # each regime on its own: the 1e4 rows must not hide the others
        n = int(nv[b])
        assert rel(lse_c[b, :n], lse_ref[b, :n]) < 2e-6, b
    scale = _ce_scale(s.masked_fill(~_corner(nv, N), 0), lse_ref, nv)
    assert bool(((pl_c.double() - ce_ref).abs() <= 1e-5 * scale).all()), (pl_c, ce_ref)
    assert pl_c[1] == 0 and pl_c[2] == 0                          # nv = 0, nv = 1: exactly no loss

    gs = 0.61
    dsd = _nan(B, N, N)
    _lib.call('fgnn_ce_bwd', _lib.ptr(sd), _lib.ptr(lse), _lib.ptr(nvd), _lib.ptr(torch.tensor([gs], device=DEV)), B, N,
              _lib.ptr(dsd), _lib.stream_ptr())
    ds = dsd.cpu()
    corner = _corner(nv, N)
    # fp64 dS on the kernel's own fp32 lse (an fp32 lse of a 1e4 row carries its own rounding of ~5e-4)
    eye = torch.eye(N, dtype=torch.float64)
    ref = ((s.double() - lse_c.double()[:, :, None]).exp() - eye) * gs
    assert rel(ds[corner], ref[corner]) < 5e-6
    assert torch.equal(ds[~corner], torch.zeros(int((~corner).sum())))
    assert torch.equal(ds[1:3], torch.zeros(2, N, N))           # nv = 0, nv = 1: exactly no gradient
    # the softmax part of each valid row sums to 1 (up to the fp32 lse)
    rs = (ds[corner.any(-1)].double().sum(-1) / gs)
    assert bool((rs.abs() < 2e-3).all())


@pytest.mark.parametrize('Cc,N', [(32, 50), (3, 65), (64, 256)])
def test_ce_fwd_lse_equals_score_ce_fwd_lse(Cc, N):
    B = 6
    g = torch.Generator().manual_seed(N)
    nv = _nv_pattern(B, N, g)
    e1, e2 = _embeddings(B, Cc, N, nv, g)
    e1d, e2d, nvd = e1.to(DEV), e2.to(DEV), nv.to(DEV)
    scores, lse, pl = _nan(B, N, N), _nan(B, N), _nan(B * SPLIT)
    _lib.call('fgnn_score_ce_fwd', _lib.ptr(e1d), _lib.ptr(e2d), _lib.ptr(nvd), B, Cc, N, _lib.ptr(scores), _lib.ptr(lse),
              _lib.ptr(pl), _lib.stream_ptr())
    lse2, pl2 = _ce_fwd(scores, nvd, B, N)
    assert torch.equal(lse.cpu(), lse2.cpu())
    assert rel(pl2.cpu().double(), pl.cpu().double().view(B, SPLIT).sum(1)) < 2e-6


def _triplet_ref(s, nv, reduction):
    """toolbox/losses.py: per-graph CE sum over its n x n block, divided by the total node count ('mean') or divided by n and
    averaged over the graphs ('mean_of_mean')."""
    ce = []
    for b, n in enumerate(nv.tolist()):
        ce.append(torch.nn.functional.cross_entropy(s[b, :n, :n], torch.arange(n), reduction='sum') if n else s.sum() * 0)
    ce = torch.stack(ce)
    n = nv.double()
    if reduction == 'mean':
        return ce.sum() / n.sum()
    return (ce / n).mean()


@pytest.mark.parametrize('reduction', ['mean', 'mean_of_mean'])
@pytest.mark.parametrize('N', [9, 65, 200])
def test_triplet_loss_module(reduction, N):
    from graph_neural_net_amd.losses import triplet_loss
    from graph_neural_net_amd.masked import MaskedTensor
    crit = triplet_loss(reduction)
    B = 7
    g = torch.Generator().manual_seed(N)
    # dense (scores of magnitude 1e4 stay out: an fp32 lse there is only good to ~5e-4, which the gradient inherits)
    s = torch.randn(B, N, N, generator=g) * 3
    s[:, torch.arange(0, N, 2), torch.arange(0, N, 2)] += 40.0          # saturated rows
    s[1] = torch.randint(-2, 3, (N, N), generator=g).float()          # exact ties
    sd = s.to(DEV).requires_grad_(True)
    out = crit(sd)
    out.backward()
    s64 = s.double().requires_grad_(True)
    ref = _triplet_ref(s64, torch.full((B,), N, dtype=torch.int32), reduction)
    ref.backward()
    assert rel(out.detach().cpu(), ref.detach()) < 2e-6
    assert rel(sd.grad.cpu(), s64.grad) < 5e-6
    # ragged: MaskedTensor with one empty graph for 'mean' (mean_of_mean divides by each graph's n)
    nv = torch.randint(1, N + 1, (B,), generator=g, dtype=torch.int32)
    nv[0] = N
    if reduction == 'mean':
        nv[1] = 0
    s = torch.randn(B, N, N, generator=g) * 2
    s = s.masked_fill(~_corner(nv, N), 0)
    sd = s.to(DEV).requires_grad_(True)
    out = crit(MaskedTensor(sd, nv.to(DEV), (1, 2)))
    out.backward()
    s64 = s.double().requires_grad_(True)
    ref = _triplet_ref(s64, nv, reduction)
    ref.backward()
    assert rel(out.detach().cpu(), ref.detach()) < 2e-6
    assert rel(sd.grad.cpu(), s64.grad) < 5e-6
    corner = _corner(nv, N)
    assert torch.equal(sd.grad.cpu()[~corner], torch.zeros(int((~corner).sum())))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. reductions: fgnn_sum_scale and fgnn_inv_node_count
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('rows', [1, 3, 4, 5, 400, 1024])
@pytest.mark.parametrize('cols', [1, 65, 200])
def test_sum_scale(rows, cols):
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    # small integers with a power-of-two scale: every partial sum is exact in fp32, so the result is exact
    x = torch.randint(-8, 9, (rows, cols), generator=g).float()
    out = _nan(cols + 1)
    _lib.call('fgnn_sum_scale', _lib.ptr(x.to(DEV)), rows, cols, 0.125, _lib.ptr(out), _lib.stream_ptr())
    o = out.cpu()
    assert torch.equal(o[:cols], (x.double().sum(0) * 0.125).float())
    assert math.isnan(o[cols])                                   # nothing written past `cols`
    # general values and scale against fp64
    x = torch.randn(rows, cols, generator=g)
    scale = 1.0 / 3.0
    out = _nan(cols)
    _lib.call('fgnn_sum_scale', _lib.ptr(x.to(DEV)), rows, cols, scale, _lib.ptr(out), _lib.stream_ptr())
    ref = x.double().sum(0) * scale
    bound = 1e-6 * (x.double().abs().sum(0) * scale + 1e-30)
    assert bool(((out.cpu().double() - ref).abs() <= bound).all())


@pytest.mark.parametrize('B', [1, 63, 64, 65, 300])
def test_inv_node_count(B):
    g = torch.Generator().manual_seed(B)
    nv = torch.randint(0, 300, (B,), generator=g, dtype=torch.int32)
    nv[0] = 0 if B > 1 else 5
    for v, expect in ((nv, np.float32(1.0) / np.float32(int(nv.sum()))), (torch.zeros(B, dtype=torch.int32), np.float32(0))):
        out = _nan(1)
        _lib.call('fgnn_inv_node_count', _lib.ptr(v.to(DEV)), B, _lib.ptr(out), _lib.stream_ptr())
        assert out.item() == expect, (B, out.item(), expect)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. arg-max accuracy: fgnn_accuracy_max and metrics.accuracy_max against np.argmax
# ---------------------------------------------------------------------------------------------------------------------------

def _np_correct(s, nv):
    return [int(np.sum(np.argmax(s[b, :n, :n].numpy(), 1) == np.arange(n))) if n else 0 for b, n in enumerate(nv.tolist())]


def _acc_scores(B, N, nv, g):
    """Small integers (ties everywhere), ties planted on the diagonal against columns 64 and 128 away (the same lane) and
    1, 63 and 65 away (other lanes), +inf entries, all -inf rows and rows holding NaN."""
    s = torch.randint(-3, 4, (B, N, N), generator=g).float()
    inf = float('inf')
    for b in range(B):
        n = int(nv[b])
        for i in range(n):
            kind = (i + b) % 9
            row = s[b, i]
            if kind in (0, 1, 2, 3, 4):         # tie between i and i +- d: the lower index wins
                d = (64, 128, 1, 63, 65)[kind]
                for j in (i - d, i + d):
                    if 0 <= j < n:
                        row[i] = row[j] = 5
                        break
            elif kind == 5 and n > 1:           # +inf twice: the first wins
                row[(i + 1) % n] = inf
                row[i] = inf
            elif kind == 6:                     # all -inf: np.argmax gives column 0
                row[:n] = -inf
            elif kind == 7:                     # a NaN wins over everything, the first NaN over later ones
                row[i] = NAN
                if i + 3 < n:
                    row[i + 3] = NAN
            elif kind == 8 and n > 2:
                row[i] = inf
                row[(i + 2) % n] = NAN
    return s.masked_fill(~_corner(nv, N), NAN)


@pytest.mark.parametrize('N', [1, 63, 64, 65, 127, 128, 129, 200, 300])
def test_accuracy_max(N):
    from graph_neural_net_amd.masked import MaskedTensor
    from graph_neural_net_amd.metrics import accuracy_max
    B = 9
    g = torch.Generator().manual_seed(N)
    nv = _nv_pattern(B, N, g)
    s = _acc_scores(B, N, nv, g)
    ref = _np_correct(s, nv)
    sd, nvd = s.to(DEV), nv.to(DEV)
    correct = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    _lib.call('fgnn_accuracy_max', _lib.ptr(sd), _lib.ptr(nvd), B, N, _lib.ptr(correct), _lib.stream_ptr())
    assert correct.cpu().tolist() == ref
    # row 0 of an all -inf row counts (argmax 0), as does a NaN on the diagonal: the cases are present
    assert sum(ref) > 0
    assert accuracy_max(MaskedTensor(sd, nvd, (1, 2))) == (sum(ref), int(nv.sum()))
    assert accuracy_max(MaskedTensor(s, nv, (1, 2))) == (sum(ref), int(nv.sum()))     # the host route agrees
    # dense: the whole N x N block of every pair
    dense = _acc_scores(B, N, torch.full((B,), N, dtype=torch.int32), g)
    refd = _np_correct(dense, torch.full((B,), N, dtype=torch.int32))
    assert accuracy_max(dense.to(DEV)) == (sum(refd), B * N)
    per = accuracy_max(dense.to(DEV), aggregate_score=False)
    assert per == [c / N for c in refd]
