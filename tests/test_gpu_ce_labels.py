"""GPU: the cross-entropy against labels -- fgnn_score_ce_fwd_blocks_labels, fgnn_score_ce_bwd_labels,
fgnn_ce_fwd_labels, fgnn_ce_bwd_labels (csrc/pool_score.hip) and fgnn_eval_pairs_labels (csrc/eval.hip) -- on every launch form
of their label-less twins, against tests/ce_labels_ref.py on the GPU's own scores / embeddings, and bit for bit against the
label-less entry points under identity labels.

Inputs carry NaN in their padding, every output is NaN-filled, sized exactly and followed by a NaN-filled guard region."""
import numpy as np
import pytest
import torch

import ce_labels_ref as R
import test_gpu_score_loss as SL
from eval_ref import CE_BOUND                   # the bound on fgnn_ce_fwd's pair loss (tests/test_gpu_score_loss.py, tests/test_gpu_eval.py)
from graph_neural_net_amd import _lib
from util import rel

pytestmark = pytest.mark.gpu
DEV = SL.DEV
NAN = SL.NAN
# The bounds tests/test_gpu_score_loss.py holds the label-less entry points to.  It states them inline, so they are quoted here:
FWD_TOL = 2e-6      # test_score_ce_fwd_row_blocks: lse (max-norm relative) and |pair loss - ref| <= FWD_TOL * sum(|lse_i| + |s_it|)
BWD_TOL = 5e-6      # test_score_bwd_forms / test_ce_fwd_bwd: de1, de2 and dS, max-norm relative
GUARD = 64
WORST = {}


def _guarded(*shape, dtype=torch.float32):
    """an exactly sized, filled output followed by a filled guard region: (view, guard)"""
    n = int(np.prod(shape))
    fill = NAN if dtype.is_floating_point else -77
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    return buf[:n].view(*shape), buf[n:]


def _intact(*guards):
    for g in guards:
        c = g.cpu()
        assert bool(torch.isnan(c).all()) if c.is_floating_point() else bool((c == -77).all()), 'a write past the end of an output'


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


# every (B, C, N) of the label-less backward test (all four forms of launch_score_bwd), plus the small and the edge sizes
GRID = SL.BWD_SHAPES + [(2, 32, 1), (3, 3, 2), (5, 32, 17), (70, 4, 17), (3, 32, 64), (70, 8, 64), (3, 32, 65), (2, 32, 130)]


def test_grid_reaches_every_form():
    assert {SL._bwd_form(*s) for s in GRID} == {'staged/8', 'staged/4', 'blocked/16', 'blocked/64'}
    assert {1, 2, 17, 50, 64, 65, 130, 200} <= {s[2] for s in GRID}
    assert any(s[0] * 4 < 256 for s in GRID) and any(s[0] * 4 >= 256 for s in GRID)
    assert any(SL._row_blocks(s[0], s[2]) == 1 for s in GRID) and any(SL._row_blocks(s[0], s[2]) > 1 for s in GRID)


def _row_block_choices(B, Cc, N):
    return [rb for rb in sorted({1, SL.SPLIT, _lib.load().fgnn_score_row_blocks(B, N)}) if SL._fwd_lds(Cc, N, rb) <= SL.LDS_MAX]


def _fwd(e1d, e2d, nvd, labd, B, Cc, N, rb):
    (s, gs), (lse, gl), (pl, gp) = _guarded(B, N, N), _guarded(B, N), _guarded(B * rb)
    if labd is None:
        _lib.call('fgnn_score_ce_fwd_blocks', _lib.ptr(e1d), _lib.ptr(e2d), _lib.ptr(nvd), B, Cc, N, rb, _lib.ptr(s), _lib.ptr(lse),
                  _lib.ptr(pl), _lib.stream_ptr())
    else:
        _lib.call('fgnn_score_ce_fwd_blocks_labels', _lib.ptr(e1d), _lib.ptr(e2d), _lib.ptr(nvd), _lib.ptr(labd), B, Cc, N, rb,
                  _lib.ptr(s), _lib.ptr(lse), _lib.ptr(pl), _lib.stream_ptr())
    _intact(gs, gl, gp)
    return s, lse, pl


def _bwd(e1d, e2d, sd, ld, nvd, labd, gsd, B, Cc, N):
    (d1, g1), (d2, g2) = _guarded(B, Cc, N), _guarded(B, Cc, N)
    if labd is None:
        _lib.call('fgnn_score_ce_bwd', _lib.ptr(e1d), _lib.ptr(e2d), _lib.ptr(sd), _lib.ptr(ld), _lib.ptr(nvd), _lib.ptr(gsd), B, Cc, N,
                  _lib.ptr(d1), _lib.ptr(d2), _lib.stream_ptr())
    else:
        _lib.call('fgnn_score_ce_bwd_labels', _lib.ptr(e1d), _lib.ptr(e2d), _lib.ptr(sd), _lib.ptr(ld), _lib.ptr(nvd), _lib.ptr(labd),
                  _lib.ptr(gsd), B, Cc, N, _lib.ptr(d1), _lib.ptr(d2), _lib.stream_ptr())
    _intact(g1, g2)
    return d1, d2


def _ce_fwd(sd, nvd, labd, B, N):
    (lse, gl), (pl, gp) = _guarded(B, N), _guarded(B)
    if labd is None:
        _lib.call('fgnn_ce_fwd', _lib.ptr(sd), _lib.ptr(nvd), B, N, _lib.ptr(lse), _lib.ptr(pl), _lib.stream_ptr())
    else:
        _lib.call('fgnn_ce_fwd_labels', _lib.ptr(sd), _lib.ptr(nvd), _lib.ptr(labd), B, N, _lib.ptr(lse), _lib.ptr(pl), _lib.stream_ptr())
    _intact(gl, gp)
    return lse, pl


def _ce_bwd(sd, ld, nvd, labd, gsd, B, N):
    ds, g = _guarded(B, N, N)
    if labd is None:
        _lib.call('fgnn_ce_bwd', _lib.ptr(sd), _lib.ptr(ld), _lib.ptr(nvd), _lib.ptr(gsd), B, N, _lib.ptr(ds), _lib.stream_ptr())
    else:
        _lib.call('fgnn_ce_bwd_labels', _lib.ptr(sd), _lib.ptr(ld), _lib.ptr(nvd), _lib.ptr(labd), _lib.ptr(gsd), B, N, _lib.ptr(ds),
                  _lib.stream_ptr())
    _intact(g)
    return ds


def _cases(B, N, nv, seed):
    cases = R.label_cases(B, N, nv.numpy(), np.random.default_rng(seed))
    cases['none'] = np.full((B, N), -1, dtype=np.int32)          # no row has a target
    # the padding of the labels is never read: put labels there that would index far outside
    rows = np.arange(N)[None, :] < nv.numpy()[:, None]
    return {k: np.where(rows, v, 1 << 30).astype(np.int32) for k, v in cases.items()}


@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('B,Cc,N', GRID)
def test_score_ce_labels_on_every_form(B, Cc, N, ragged):
    g = torch.Generator().manual_seed(131 * B + 17 * Cc + N + ragged)
    nv = SL._nv_pattern(B, N, g) if ragged else torch.full((B,), N, dtype=torch.int32)
    e1, e2 = SL._embeddings(B, Cc, N, nv, g)
    e1d, e2d = e1.to(DEV), e2.to(DEV)
    nvd = nv.to(DEV) if ragged else None
    corner, cols = SL._corner(nv, N), SL._cols(nv, N).expand(B, Cc, N)
    rows = torch.arange(N)[None, :] < nv.long()[:, None]
    gscale = 0.37
    gsd = torch.tensor([gscale], device=DEV)
    cases = _cases(B, N, nv, 1000 * N + B)
    nvn = nv.numpy()

    # ---- forward: every row-block form; scores and lse do not depend on the labels, the loss is the reference's on the GPU's scores
    plain = {}
    for rb in _row_block_choices(B, Cc, N):
        s0, l0, p0 = (t.cpu() for t in _fwd(e1d, e2d, nvd, None, B, Cc, N, rb))
        plain[rb] = (s0, l0, p0)
        sref = s0.double().numpy()
        for name, lab in cases.items():
            labd = torch.from_numpy(lab).to(DEV)
            s, l, p = (t.cpu() for t in _fwd(e1d, e2d, nvd, labd, B, Cc, N, rb))
            assert torch.equal(s, s0) and torch.equal(l, l0), (rb, name)
            lse_ref, ce_ref, _ = R.batch_ce(sref, lab, nvn)
            assert rel(l[rows], torch.from_numpy(lse_ref)[rows]) < FWD_TOL, (rb, name)
            scale = R.ce_scale(sref, lse_ref, lab, nvn)
            pair = p.double().view(B, rb).sum(1).numpy()
            err = np.abs(pair - ce_ref)
            assert (err <= FWD_TOL * scale).all(), (rb, name, pair, ce_ref)
            _note('score fwd loss', (err / np.maximum(FWD_TOL * scale, 1e-300)).max())
            if name == 'identity':
                assert torch.equal(p, p0), rb
            if name == 'none':
                assert torch.equal(p, torch.zeros(B * rb)), rb                    # no target: exactly no loss
    rb = max(plain)
    s0, l0, _ = plain[rb]

    # ---- backward on the GPU's scores and lse (NaN in their padding): dE against the reference on the same values
    sd = s0.masked_fill(~corner, NAN).to(DEV)
    ld = l0.masked_fill(~rows, NAN).to(DEV)
    p1, p2 = (t.cpu() for t in _bwd(e1d, e2d, sd, ld, nvd, None, gsd, B, Cc, N))
    for name, lab in cases.items():
        labd = torch.from_numpy(lab).to(DEV)
        d1, d2 = (t.cpu() for t in _bwd(e1d, e2d, sd, ld, nvd, labd, gsd, B, Cc, N))
        _, _, dS = R.batch_ce(s0.double().numpy(), lab, nvn, gscale, lse=l0.double().numpy())
        r1, r2 = (torch.from_numpy(x) for x in R.embedding_grads(e1.numpy(), e2.numpy(), dS, nvn))
        assert torch.equal(d1[~cols], torch.zeros(int((~cols).sum()))) and torch.equal(d2[~cols], d1[~cols]), name
        if name == 'none':
            assert torch.equal(d1, torch.zeros(B, Cc, N)) and torch.equal(d2, d1)      # no target: exactly no gradient
            continue
        if bool(cols.any()):
            e = max(rel(d1[cols], r1[cols]), rel(d2[cols], r2[cols]))
            assert e < BWD_TOL, (name, e)
            _note('score bwd dE', e / BWD_TOL)
        if name == 'identity':
            assert torch.equal(d1, p1) and torch.equal(d2, p2)
        # composition: fgnn_score_bwd(fgnn_ce_bwd_labels(scores, lse)) is fgnn_score_ce_bwd_labels bit for bit
        ds = _ce_bwd(sd, ld, nvd, labd, gsd, B, N)
        (c1, g1), (c2, g2) = _guarded(B, Cc, N), _guarded(B, Cc, N)
        _lib.call('fgnn_score_bwd', _lib.ptr(e1d), _lib.ptr(e2d), _lib.ptr(ds), _lib.ptr(nvd), B, Cc, N, _lib.ptr(c1), _lib.ptr(c2),
                  _lib.stream_ptr())
        assert torch.equal(c1.cpu(), d1) and torch.equal(c2.cpu(), d2), name
    print('B=%d C=%d N=%d ragged=%s form=%s worst error / bound so far: %s' % (B, Cc, N, ragged, SL._bwd_form(B, Cc, N), WORST))


@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('N', [1, 2, 17, 50, 64, 65, 130, 200, 300])
def test_module_ce_labels(N, ragged):
    """fgnn_ce_fwd_labels / fgnn_ce_bwd_labels on the hard score regimes of the label-less test"""
    B = 10
    g = torch.Generator().manual_seed(300 + N + ragged)
    nv = SL._nv_pattern(B, N, g) if ragged else torch.full((B,), N, dtype=torch.int32)
    s = SL._hard_scores(B, N, nv, g)
    sd = s.to(DEV)
    nvd = nv.to(DEV) if ragged else None
    nvn = nv.numpy()
    corner = SL._corner(nv, N)
    rows = torch.arange(N)[None, :] < nv.long()[:, None]
    s64 = s.masked_fill(~corner, 0).double().numpy()
    gs = 0.61
    gsd = torch.tensor([gs], device=DEV)
    l0, p0 = _ce_fwd(sd, nvd, None, B, N)
    d0 = _ce_bwd(sd, l0, nvd, None, gsd, B, N)
    for name, lab in _cases(B, N, nv, N).items():
        labd = torch.from_numpy(lab).to(DEV)
        lse, pl = _ce_fwd(sd, nvd, labd, B, N)
        assert torch.equal(lse, l0), name
        lse_c, pl_c = lse.cpu(), pl.cpu()
        lse_ref, ce_ref, _ = R.batch_ce(s64, lab, nvn)
        for b in range(B):                      # each regime on its own: the 1e4 rows must not hide the others
            n = int(nv[b])
            assert rel(lse_c[b, :n], torch.from_numpy(lse_ref)[b, :n]) < FWD_TOL, (name, b)
        assert torch.equal(lse_c[~rows], torch.zeros(int((~rows).sum())))
        scale = R.ce_scale(s64, lse_ref, lab, nvn)
        err = np.abs(pl_c.double().numpy() - ce_ref)
        assert (err <= CE_BOUND * scale).all(), (name, pl_c, ce_ref)
        _note('ce fwd loss', (err / np.maximum(CE_BOUND * scale, 1e-300)).max())
        ds = _ce_bwd(sd, lse, nvd, labd, gsd, B, N).cpu()
        _, _, ref = R.batch_ce(s64, lab, nvn, gs, lse=lse_c.double().numpy())      # on the kernel's own fp32 lse
        ref = torch.from_numpy(ref)
        ok = torch.from_numpy(R.has_target(lab, nvn))
        assert torch.equal(ds[~corner], torch.zeros(int((~corner).sum()))), name
        assert torch.equal(ds[~ok], torch.zeros(int((~ok).sum()), N)), name           # rows without a target: exactly zero
        if bool(corner.any()) and name != 'none':
            e = rel(ds[corner], ref[corner])
            assert e < BWD_TOL, (name, e)
            _note('ce bwd dS', e / BWD_TOL)
        if name == 'identity':
            assert torch.equal(pl, p0) and torch.equal(ds, d0.cpu())
        if name == 'none':
            assert torch.equal(pl_c, torch.zeros(B))
    print('N=%d ragged=%s worst error / bound so far: %s' % (N, ragged, WORST))


@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('N', [1, 2, 16, 17, 50, 65, 200])
def test_eval_pairs_labels(N, ragged):
    """fgnn_eval_pairs_labels: row_ce against the labels (per row, the bound of tests/test_gpu_eval.py: CE_BOUND (|lse| + |s|));
    lse through the cost corner, row_hit and the solver's counts are those of fgnn_eval_pairs with the same labels, exactly."""
    from graph_neural_net_amd.evaluation import evaluate_scores
    B = 6
    g = torch.Generator().manual_seed(500 + N + ragged)
    nv = SL._nv_pattern(B, N, g) if ragged else torch.full((B,), N, dtype=torch.int32)
    corner = SL._corner(nv, N)
    s = (torch.randn(B, N, N, generator=g) * 3).masked_fill(~corner, NAN)
    sd = s.to(DEV)
    nvd = nv.to(DEV) if ragged else None
    nvn = nv.numpy()
    rows = torch.arange(N)[None, :] < nv.long()[:, None]
    s64 = s.masked_fill(~corner, 0).double().numpy()

    def launch(name, labd):
        (cost, gc), (ce, ge), (hit, gh) = _guarded(B, N, N), _guarded(B, N), _guarded(B, N, dtype=torch.int32)
        _lib.call(name, _lib.ptr(sd), _lib.ptr(nvd), _lib.ptr(labd), B, N, _lib.ptr(cost), N * N, N, _lib.ptr(ce), _lib.ptr(hit),
                  _lib.stream_ptr())
        _intact(gc, ge, gh)
        return cost.cpu(), ce.cpu(), hit.cpu()

    for name, lab in _cases(B, N, nv, 7 * N).items():
        labd = torch.from_numpy(lab).to(DEV)
        c0, ce0, h0 = launch('fgnn_eval_pairs', labd)
        c1, ce1, h1 = launch('fgnn_eval_pairs_labels', labd)
        assert torch.equal(c1[corner], c0[corner]) and bool(torch.isnan(c1[~corner]).all()), name
        assert torch.equal(h1[rows], h0[rows]) and bool((h1[~rows] == -77).all()), name
        assert bool(torch.isnan(ce1[~rows]).all()), name
        lse_ref, _, _ = R.batch_ce(s64, lab, nvn)
        ok = R.has_target(lab, nvn)
        t = np.clip(lab, 0, N - 1).astype(np.int64)
        st = np.take_along_axis(s64, t[:, :, None], 2)[:, :, 0]
        want = np.where(ok, lse_ref - st, 0.0)
        bound = CE_BOUND * (np.abs(lse_ref) + np.abs(st))
        got = ce1.double().numpy()
        live = rows.numpy()
        assert (np.abs(got - want)[live] <= bound[live]).all(), name
        assert (got[live & ~ok] == 0).all(), name                   # no target: exactly zero
        if (live & ok).any():
            _note('eval row_ce', (np.abs(got - want)[live & ok] / bound[live & ok]).max())
        if name == 'identity':
            assert torch.equal(ce1[rows], ce0[rows])
        # through evaluate_scores: the counts of the solver and of the arg-max do not depend on where the loss looks
        a = evaluate_scores(sd, nvalid=nvd, labels=labd)
        b = evaluate_scores(sd, nvalid=nvd, labels=labd, loss_on_labels=True)
        for k in ('correct_lsap', 'correct_max', 'assign', 'n'):
            assert torch.equal(a[k], b[k]), (name, k)
        _, ce_ref, _ = R.batch_ce(s64, lab, nvn)
        scale = R.ce_scale(s64, lse_ref, lab, nvn)
        assert (np.abs(b['ce'].cpu().numpy() - ce_ref) <= CE_BOUND * scale).all(), name
        assert b['meter'].record()['nodes'] == int(nv.sum())        # the normaliser stays the node count
    print('N=%d ragged=%s worst error / bound so far: %s' % (N, ragged, WORST))


def test_labelled_launches_are_capturable():
    """the two score launches in a HIP graph: fresh labels in the static buffer between replays"""
    B, Cc, N = 4, 32, 20
    g = torch.Generator().manual_seed(9)
    nv = torch.full((B,), N, dtype=torch.int32)
    e1, e2 = SL._embeddings(B, Cc, N, nv, g)
    e1d, e2d = e1.to(DEV), e2.to(DEV)
    rb = _lib.load().fgnn_score_row_blocks(B, N)
    gsd = torch.tensor([0.5], device=DEV)
    lab = torch.zeros(B, N, dtype=torch.int32, device=DEV)
    s, lse, pl = SL._nan(B, N, N), SL._nan(B, N), SL._nan(B * rb)
    d1, d2 = SL._nan(B, Cc, N), SL._nan(B, Cc, N)

    def work():
        st = _lib.stream_ptr()
        _lib.call('fgnn_score_ce_fwd_blocks_labels', _lib.ptr(e1d), _lib.ptr(e2d), None, _lib.ptr(lab), B, Cc, N, rb, _lib.ptr(s),
                  _lib.ptr(lse), _lib.ptr(pl), st)
        _lib.call('fgnn_score_ce_bwd_labels', _lib.ptr(e1d), _lib.ptr(e2d), _lib.ptr(s), _lib.ptr(lse), None, _lib.ptr(lab),
                  _lib.ptr(gsd), B, Cc, N, _lib.ptr(d1), _lib.ptr(d2), st)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        work()
    for seed in (1, 2):
        perm = torch.stack([torch.randperm(N, generator=torch.Generator().manual_seed(seed * 10 + b)) for b in range(B)]).to(torch.int32)
        lab.copy_(perm)
        graph.replay()
        got = [t.clone() for t in (pl, d1, d2)]
        work()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, (pl, d1, d2)))
