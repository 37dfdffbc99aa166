"""GPU: the bf16 HIP path (engine16, through the C ABI) against oracle/fgnn_oracle_bf16.py -- a CPU restatement that rounds
to bf16 at the same points -- and against the fixtures generated from the reference run in fp32 / fp64 / bf16.

What can be bit-exact is: the first block's MLP outputs (identical exact inputs, identical rounding points; an element may
still flip by one bf16 ulp where the fp32 accumulation order differs) and everything integer (padding zeros, shapes).
Beyond that four blocks of 16-bit activations are chaotic (an arg-max flip in the pooling re-routes a gradient), so the
end-to-end gates are statistical:
  * HIP vs the same-point oracle: distance <= SAME_POINT x the bf16 scheme's own distance to the fp32 oracle
    (both are equally valid bf16 evaluations; they must sit well inside the same noise ball);
  * HIP vs the fp64 truth of the reference fixture: <= BF16_CLASS x the distance of the reference's own bf16 run
    (tests/util.py, measured spread in tests/test_oracle_bf16.py).
"""
import pytest
import torch

from graph_neural_net_amd import synthetic
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.engine16 import FgnnEngineBF16
from oracle import fgnn_oracle as O, fgnn_oracle_bf16 as OB
from util import BF16_CLASS, flat_of, is_zero_grad, l2rel, load_golden, rel, sub, unpack_pairs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SAME_POINT = 0.5
ULP = 2.0 ** -7          # one bf16 ulp relative to the value (8 significant bits)


def _sd(num_blocks, seed):
    torch.manual_seed(seed)
    sd = O.init_state_dict(num_blocks=num_blocks)
    g = torch.Generator().manual_seed(seed + 1)
    for k, v in sd.items():
        if k.endswith('.bias') and v.dim() == 1:
            v.add_(0.1 * torch.randn(v.shape, generator=g))
        elif k.endswith('gn.weight'):
            v.mul_(1 + 0.2 * torch.randn(v.shape, generator=g))
        elif k.endswith('gn.bias'):
            v.add_(0.05 * torch.randn(v.shape, generator=g))
    return sd


def _run(sd, x1, x2, nblk):
    lay = ParamLayout(2, nblk, 32, 32, 3)
    params = lay.flatten(sd, DEV)
    grads = torch.zeros_like(params)
    eng = FgnnEngineBF16(lay, 2 * x1.shape[0], x1.shape[-1], DEV)
    x = torch.cat([x1, x2]).contiguous().to(DEV)
    scores, loss = eng.step(params, grads, x)
    torch.cuda.synchronize()
    return eng, lay, scores.cpu(), loss.item(), lay.unflatten(grads.cpu())


def _ulp_close(got, ref, max_frac):
    """every element within one bf16 ulp of the reference value; at most max_frac of them differ at all"""
    got, ref = got.float().cpu(), ref.float()
    diff = (got - ref).abs()
    assert (diff <= ULP * ref.abs() + 1e-30).all(), (diff / (ref.abs() + 1e-30)).max().item()
    frac = (diff > 0).float().mean().item()
    assert frac <= max_frac, frac


@pytest.mark.parametrize('N,B', [(20, 2), (50, 2), (37, 1), (200, 1)])
def test_first_block_is_exact_up_to_rounding_flips(N, B):
    """Block 1: inputs are exact (0/1 and small integers), so z1 / z2 / mult / z3 must equal the oracle's bf16 values except
    for isolated one-ulp rounding flips (N=37: row pitch 40, padded columns; N=200: the cfg4 size)."""
    sd = _sd(1, 10 + N)
    x1, x2 = synthetic.make_batch(N, B, N, 'ErdosRenyi', 0.3 if N < 100 else 0.5, 0.1)
    keep = {}
    s_ref, l_ref, g_ref = OB.step_fwd_bwd(x1, x2, sd, keep=keep)
    eng, lay, scores, loss, grads = _run(sd, x1, x2, 1)
    _ulp_close(eng.dense(eng.z[(1, 1)]), keep[(1, 'z1')], 1e-3)
    _ulp_close(eng.dense(eng.z[(1, 2)]), keep[(1, 'z2')], 1e-3)
    _ulp_close(eng.dense(eng.mult[1]), keep[(1, 'mult')], 2e-2)
    # padding of the stored slabs (columns N .. ldr-1) is exactly zero
    raw = eng.z[(1, 3)].view(2 * B, 32, eng.ldp)[:, :, :N * eng.ldr].view(2 * B, 32, N, eng.ldr)
    assert raw[..., N:].float().abs().sum().item() == 0
    # one block: scores / loss / gradients close to the same-point oracle
    assert rel(scores, s_ref) < 2e-2
    assert abs(loss - l_ref.item()) < 2e-3 * abs(l_ref.item())
    keys = [k for k in g_ref if not is_zero_grad(k)]
    assert l2rel(flat_of(grads, keys), flat_of(g_ref, keys)) < 5e-2


def test_cfg4_full_size_against_same_point_oracle():
    """BASELINE config 3 at full size: N=200 dense ER pairs, batch 8, 4 blocks, bf16."""
    sd = sub(load_golden('cfg2_reg_n50_b2_4blk.npz'), 'sd/')
    x1, x2 = synthetic.make_batch(4000, 8, 200, 'ErdosRenyi', 0.5, 0.1)
    s16, l16, g16 = OB.step_fwd_bwd(x1, x2, sd)
    s32, l32, g32 = O.step_fwd_bwd(x1, x2, sd)
    eng, lay, scores, loss, grads = _run(sd, x1, x2, 4)
    assert torch.isfinite(scores).all() and all(torch.isfinite(g).all() for g in grads.values())
    keys = [k for k in g32 if not is_zero_grad(k)]
    f = lambda g: flat_of(g, keys)
    assert l2rel(scores, s16) <= SAME_POINT * l2rel(s16, s32), (l2rel(scores, s16), l2rel(s16, s32))
    assert l2rel(f(grads), f(g16)) <= SAME_POINT * l2rel(f(g16), f(g32)), (l2rel(f(grads), f(g16)), l2rel(f(g16), f(g32)))
    assert abs(loss - l16.item()) < 2e-3 * abs(l16.item())
    # the HIP result is as close to the fp32 result as the scheme allows
    assert l2rel(scores, s32) <= 1.5 * l2rel(s16, s32) and l2rel(f(grads), f(g32)) <= 1.5 * l2rel(f(g16), f(g32))
    # run-to-run determinism (fixed-order reductions): bit-exact
    eng2, _, scores2, loss2, grads2 = _run(sd, x1, x2, 4)
    assert torch.equal(scores, scores2) and loss == loss2 and all(torch.equal(grads[k], grads2[k]) for k in grads)


def test_cfg4_against_reference_bf16_yardstick():
    """The reference-generated fixture (N=200, one pair): distance to the fp64 truth vs the reference's own bf16 run."""
    d = load_golden('cfg4_er_n200_b1_4blk.npz')
    sd = sub(load_golden('cfg2_reg_n50_b2_4blk.npz'), 'sd/')
    n = int(d['n'])
    x1, x2 = unpack_pairs(d['bits1'], n), unpack_pairs(d['bits2'], n)
    eng, lay, scores, loss, grads = _run(sd, x1, x2, 4)
    keys = [k for k in sub(d, 'grad/') if not is_zero_grad(k)]
    g64 = flat_of(sub(d, 'grad64/'), keys)
    s64 = d['scores64_as_f32']
    assert l2rel(scores, s64) <= BF16_CLASS * l2rel(d['scores_refbf16'], s64)
    assert l2rel(flat_of(grads, keys), g64) <= BF16_CLASS * l2rel(flat_of(sub(d, 'grad_refbf16/'), keys), g64)
    assert abs(loss - d['loss64'].item()) <= BF16_CLASS * abs(d['loss_refbf16'].item() - d['loss64'].item()) + 1e-3


def test_cfg2_shape_in_bf16():
    """N=50 regular pairs, 4 blocks (the headline shape) through the bf16 engine: statistical gates as above."""
    d = load_golden('cfg2_reg_n50_b2_4blk.npz')
    sd = sub(d, 'sd/')
    x1, x2 = synthetic.make_batch(2000, 8, 50, 'Regular', 0.2, 0.1)
    s16, l16, g16 = OB.step_fwd_bwd(x1, x2, sd)
    s32, l32, g32 = O.step_fwd_bwd(x1, x2, sd)
    eng, lay, scores, loss, grads = _run(sd, x1, x2, 4)
    keys = [k for k in g32 if not is_zero_grad(k)]
    f = lambda g: flat_of(g, keys)
    assert l2rel(scores, s16) <= SAME_POINT * l2rel(s16, s32)
    assert l2rel(f(grads), f(g16)) <= SAME_POINT * l2rel(f(g16), f(g32))


def test_bf16_trainer_captured_equals_eager_and_tracks_fp32():
    """FgnnTrainer(precision='bf16'): the captured step equals the eager step bit for bit, and the loss trajectory of the
    16-bit trainer stays close to the fp32 trainer's on the same batches (the reference's precision=16 training)."""
    from graph_neural_net_amd.trainer import FgnnTrainer
    lay = ParamLayout(2, 2, 32, 32, 3)
    p0 = lay.init_flat(3, DEV)
    batches = [synthetic.make_batch(7100 + i, 4, 24, 'ErdosRenyi', 0.3, 0.05) for i in range(3)]
    runs = {}
    for name, kw in (('eager16', dict(precision='bf16')), ('graph16', dict(precision='bf16', capture=True)), ('fp32', {})):
        tr = FgnnTrainer(lay, p0.clone(), lr=1e-3, **kw)
        losses = []
        for s in range(6):
            x1, x2 = batches[s % 3]
            loss, _ = tr.train_step(x1.to(DEV), x2.to(DEV))
            losses.append(loss.item())
        runs[name] = (losses, tr.params.clone())
    assert runs['eager16'][0] == runs['graph16'][0]
    assert torch.equal(runs['eager16'][1], runs['graph16'][1])
    # Adam turns the 16-bit gradient noise into +-lr parameter steps, so the trajectories drift apart slowly (measured:
    # 0.1 % at step 0, 2.5 % after six steps); both must descend
    for a, b in zip(runs['eager16'][0], runs['fp32'][0]):
        assert abs(a - b) < 5e-2 * abs(b), (runs['eager16'][0], runs['fp32'][0])
    assert abs(runs['eager16'][0][0] - runs['fp32'][0][0]) < 5e-3 * abs(runs['fp32'][0][0])
    assert runs['fp32'][0][-1] < runs['fp32'][0][0] and runs['eager16'][0][-1] < runs['eager16'][0][0]


@pytest.mark.parametrize('N', [40, 72, 200])
def test_matmul16_entry_points_agree(N):
    """Kernel level, through the C ABI: fgnn_chan_matmul_fwd16 against a torch product of the rounded operands, and the two
    backward entry points against each other -- the plain one re-reads the raw slabs for S2, the _t one derives S2 from the
    trace term <dM, M> (given here as one tile partial per (g, c)).  Outputs and S1 must be bit-identical, S2 must agree to
    bf16-noise level."""
    import ctypes as C
    from graph_neural_net_amd import _lib
    _lib.load()
    G, Cc = 2, 32
    ldr = (N + 7) // 8 * 8
    ldp = (N * ldr + 63) // 64 * 64
    tpg = _lib.load().fgnn_tiles_per_graph16(N, ldr)
    gen = torch.Generator().manual_seed(N)
    def slab(scale, shift):
        t = torch.zeros(G, Cc, ldp)
        v = torch.randn(G, Cc, N, N, generator=gen) * scale + shift
        t[:, :, :N * ldr].view(G, Cc, N, ldr)[..., :N] = v
        return t.to(torch.bfloat16).to(DEV).contiguous()
    za, zb, dm = slab(0.3, 1.5), slab(0.2, -0.7), slab(0.05, 0.0)
    nrm_a = torch.zeros(G * Cc, 4); nrm_b = torch.zeros(G * Cc, 4)
    nrm_a[:, 0], nrm_a[:, 1] = 1.5, 0.8
    nrm_b[:, 0], nrm_b[:, 1] = -0.7, 1.3
    nrm_a, nrm_b = nrm_a.to(DEV).contiguous(), nrm_b.to(DEV).contiguous()
    beta_a = (0.1 * torch.randn(Cc, generator=gen)).to(DEV)
    beta_b = (0.1 * torch.randn(Cc, generator=gen)).to(DEV)
    sa = _lib.make_slab16(za, Cc * ldp, ldp, Cc, nrm=nrm_a, beta=beta_a)
    sb = _lib.make_slab16(zb, Cc * ldp, ldp, Cc, nrm=nrm_b, beta=beta_b)
    st = _lib.stream_ptr()
    out = torch.zeros(G * Cc * ldp, dtype=torch.bfloat16, device=DEV)
    _lib.call('fgnn_chan_matmul_fwd16', C.byref(sa), C.byref(sb), None, G, N, ldr, _lib.ptr(out), Cc * ldp, ldp, st)
    def dense(t):
        return t.view(G, Cc, ldp)[:, :, :N * ldr].reshape(G, Cc, N, ldr)[..., :N].float().cpu()
    # the kernel normalises with one fma, y = R(z a + (beta - mean a)); torch rounds twice, so an operand may differ by one
    # bf16 ulp here and there: the product is compared in L2 (the element-wise half-ulp check with exact operands is
    # test_random_operands_element_wise in tests/test_gpu_matmul16_exact.py)
    ya = (dense(za) * 0.8 + (beta_a.cpu().view(1, Cc, 1, 1) - 1.5 * 0.8)).to(torch.bfloat16).float()
    yb = (dense(zb) * 1.3 + (beta_b.cpu().view(1, Cc, 1, 1) + 0.7 * 1.3)).to(torch.bfloat16).float()
    m_ref = torch.matmul(ya.double(), yb.double()).float()
    m_got = dense(out)
    assert (m_got - m_ref).norm() < 3e-3 * m_ref.norm()
    # T per (g, c) from the stored product, handed over in tile 0
    tpart = torch.zeros(G, Cc, tpg)
    tpart[:, :, 0] = (dense(dm) * m_got).sum((-1, -2))
    tpart = tpart.to(DEV).contiguous()
    res = []
    for with_t in (False, True):
        da = torch.zeros_like(out); db = torch.zeros_like(out)
        s12a = torch.zeros(G * Cc * 2, device=DEV); s12b = torch.zeros(G * Cc * 2, device=DEV)
        if with_t:
            _lib.call('fgnn_chan_matmul_bwd16_t', C.byref(sa), C.byref(sb), _lib.ptr(dm), Cc * ldp, ldp, _lib.ptr(tpart), tpg, None,
                      G, N, ldr, _lib.ptr(da), _lib.ptr(db), Cc * ldp, ldp, _lib.ptr(s12a), _lib.ptr(s12b), st)
        else:
            _lib.call('fgnn_chan_matmul_bwd16', C.byref(sa), C.byref(sb), _lib.ptr(dm), Cc * ldp, ldp, None, G, N, ldr,
                      _lib.ptr(da), _lib.ptr(db), Cc * ldp, ldp, _lib.ptr(s12a), _lib.ptr(s12b), st)
        torch.cuda.synchronize()
        res.append((da.cpu(), db.cpu(), s12a.cpu().view(-1, 2), s12b.cpu().view(-1, 2)))
    (da0, db0, a0, b0), (da1, db1, a1, b1) = res
    assert torch.equal(da0.view(torch.int16), da1.view(torch.int16)) and torch.equal(db0.view(torch.int16), db1.view(torch.int16))
    da_ref = torch.matmul(dense(dm).double(), yb.double().transpose(-1, -2)).float()
    assert (dense(da0.to(DEV)) - da_ref).norm() < 3e-3 * da_ref.norm()
    assert torch.equal(a0[:, 0], a1[:, 0]) and torch.equal(b0[:, 0], b1[:, 0])                  # S1: same sums
    for s_plain, s_t in ((a0[:, 1], a1[:, 1]), (b0[:, 1], b1[:, 1])):
        scale = s_plain.abs().mean()
        assert (s_plain - s_t).abs().max() < 3e-2 * scale, ((s_plain - s_t).abs().max().item(), scale.item())


def test_ragged_bf16_against_per_pair_oracle():
    """Ragged batch in 16 bit (Nmax = 120: the 64 < N <= 128 class of the matmul kernels, padding in every tensor) against the
    same-point oracle run pair by pair on the un-padded graphs, gradients summed under the global node normaliser."""
    import numpy as np
    d = load_golden('cfg2_reg_n50_b2_4blk.npz')
    sd = {k: v for k, v in sub(d, 'sd/').items() if k.startswith('ne_bm_block1') or k.startswith('ne_bm_block2')}
    rng = np.random.default_rng(11)
    ns = [120, 75, 97]
    B, N = len(ns), max(ns)
    xs, ys = [], []
    for i, n in enumerate(ns):
        a, b = synthetic.make_batch(9000 + i, 1, n, 'ErdosRenyi', 0.3, 0.05)
        xs.append(a[0]); ys.append(b[0])
    total = float(sum(ns))
    s16, g16, g32 = [], None, None
    for a, b in zip(xs, ys):
        s, _, g = OB.step_fwd_bwd(a[None], b[None], sd, total_nodes=total)
        _, _, gf = OB.step_fwd_bwd(a[None], b[None], sd, rounding=False, total_nodes=total)
        s16.append(s[0])
        g16 = g if g16 is None else {k: g16[k] + g[k] for k in g}
        g32 = gf if g32 is None else {k: g32[k] + gf[k] for k in gf}
    x1, nv = O.pad_graph_list(xs)
    x2, _ = O.pad_graph_list(ys)
    lay = ParamLayout(2, 2, 32, 32, 3)
    params = lay.flatten(sd, DEV)
    grads = torch.zeros_like(params)
    eng = FgnnEngineBF16(lay, 2 * B, N, DEV, ragged=True)
    scores, loss = eng.step(params, grads, torch.cat([x1, x2]).contiguous().to(DEV), nvalid=torch.cat([nv, nv]).to(DEV))
    torch.cuda.synchronize()
    scores, got = scores.cpu(), lay.unflatten(grads.cpu())
    for i, n in enumerate(ns):
        assert scores[i, n:, :].abs().sum() == 0 and scores[i, :, n:].abs().sum() == 0          # exact zeros in the padding
        assert l2rel(scores[i, :n, :n], s16[i]) < 2e-2
    keys = [k for k in g16 if not is_zero_grad(k)]
    f = lambda g: flat_of(g, keys)
    # same-point gate: well inside the bf16 scheme's own distance to the un-rounded evaluation
    assert l2rel(f(got), f(g16)) <= SAME_POINT * l2rel(f(g16), f(g32)), (l2rel(f(got), f(g16)), l2rel(f(g16), f(g32)))


def test_module_half_switch_runs_the_bf16_engine():
    """Network.half() (models/utils.py:71-74) / Siamese_Node_Exp(precision='bf16'): the module surface in 16 bit equals the
    bf16 engine driven directly (same kernels, same flat parameters) and stays in the bf16 class around the fp32 module."""
    from graph_neural_net_amd.siamese import Siamese_Node_Exp
    d = load_golden('cfg2_reg_n50_b2_4blk.npz')
    sd = sub(d, 'sd/')
    ne = dict(type='node_embedding', block_init='block_emb', block_inside='block', num_blocks=4,
              in_features=32, out_features=32, depth_of_mlp=3)
    x1, x2 = synthetic.make_batch(2000, 4, 50, 'Regular', 0.2, 0.1)
    outs = {}
    for name in ('fp32', 'ctor', 'half'):
        model = Siamese_Node_Exp(2, ne, precision='bf16' if name == 'ctor' else 'fp32').to(DEV)
        model.load_state_dict({'node_embedder.' + k: v for k, v in sd.items()})
        if name == 'half':
            assert model.node_embedder.half() is model.node_embedder
        scores = model(x1.to(DEV), x2.to(DEV))
        loss = model.loss(scores)
        loss.backward()
        outs[name] = (scores.detach().cpu(), loss.item(),
                      torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu())
        assert all(p.dtype == torch.float32 for p in model.parameters())           # master parameters stay fp32
    assert torch.equal(outs['ctor'][0], outs['half'][0]) and torch.equal(outs['ctor'][2], outs['half'][2])
    eng, lay, s_eng, l_eng, g_eng = _run(sd, x1, x2, 4)
    assert torch.equal(outs['ctor'][0], s_eng)                                      # same kernels as the engine
    assert abs(outs['ctor'][1] - l_eng) < 1e-6 * abs(l_eng)
    assert l2rel(outs['ctor'][2], lay.flatten(g_eng, 'cpu')) < 1e-5
    assert 1e-4 < l2rel(outs['ctor'][0], outs['fp32'][0]) < 0.2                     # really 16-bit, and in its class


def test_bf16_ragged_trainer_step_with_filler_graphs():
    """FgnnTrainer(precision='bf16').train_step_ragged: size-bucketed ragged batch (the engine is built for a rounded-up graph
    count, the surplus graphs have zero vertices) -- first-step loss and update direction agree with the fp32 trainer."""
    from graph_neural_net_amd.trainer import FgnnTrainer
    lay = ParamLayout(2, 2, 32, 32, 3)
    p0 = lay.init_flat(8, DEV)
    xs, ys = [], []
    for i, n in enumerate([9, 33, 14, 40, 21]):                # five pairs: graph counts are rounded up to multiples of 4
        a, b = synthetic.make_batch(7800 + i, 1, n, 'ErdosRenyi', 0.3, 0.05)
        xs.append(a[0].to(DEV)); ys.append(b[0].to(DEV))
    res = {}
    for prec in ('fp32', 'bf16'):
        tr = FgnnTrainer(lay, p0.clone(), lr=1e-3, precision=prec)
        loss, _ = tr.train_step_ragged(xs, ys)
        torch.cuda.synchronize()
        assert torch.isfinite(tr.params).all()
        res[prec] = (loss.item(), (tr.params - p0).cpu())
    assert abs(res['bf16'][0] - res['fp32'][0]) < 5e-3 * abs(res['fp32'][0])
    d16, d32 = res['bf16'][1], res['fp32'][1]
    cos = torch.dot(d16, d32) / (d16.norm() * d32.norm())
    assert cos > 0.8, cos.item()                                    # Adam's first step is +-lr per parameter: signs must agree


@pytest.mark.parametrize('ns', [[120, 75, 97, 33], [50, 7, 1, 24], [200, 40], [64, 64, 30, 9]])
def test_bf16_ragged_padding_tiles_are_skipped_not_trusted(ns):
    """bf16 ragged engine: padding-only tiles (64 elements of the ldr-pitched planes) are stepped over.  Scores bit-identical
    to the engine that computes every tile, gradients equal up to the summation order of the workgroup partials; workspaces
    poisoned with NaN bit patterns / a previous full-size batch do not leak (bit-identical to the first run)."""
    import numpy as np
    d = load_golden('cfg2_reg_n50_b2_4blk.npz')
    sd = {k: v for k, v in sub(d, 'sd/').items() if k.startswith('ne_bm_block1') or k.startswith('ne_bm_block2')}
    rng = np.random.default_rng(sum(ns))
    xs, ys = [], []
    for n in ns:
        a, b = synthetic.make_pair(rng, n, 'ErdosRenyi', 0.3, 0.1)
        xs.append(torch.from_numpy(a)); ys.append(torch.from_numpy(b))
    x1, nv = O.pad_graph_list(xs)
    x2, _ = O.pad_graph_list(ys)
    x = torch.cat([x1, x2]).contiguous().to(DEV)
    nvd = torch.cat([nv, nv]).to(DEV)
    G, N = x.shape[0], x.shape[-1]
    lay = ParamLayout(2, 2, 32, 32, 3)
    params = lay.flatten(sd, DEV)

    def run(eng, xin=x, nvin=nvd):
        g = torch.zeros_like(params)
        s, l = eng.step(params, g, xin, nvalid=nvin)
        torch.cuda.synchronize()
        return s.clone(), l.clone(), g

    skip = FgnnEngineBF16(lay, G, N, DEV, ragged=True)
    assert skip.ranges is not None
    s1, l1, g1 = run(skip)
    FgnnEngineBF16.SKIP_PADDING_TILES = False
    try:
        full = FgnnEngineBF16(lay, G, N, DEV, ragged=True)
    finally:
        FgnnEngineBF16.SKIP_PADDING_TILES = True
    assert full.ranges is None
    s0, l0, g0 = run(full)
    assert torch.isfinite(s1).all() and torch.isfinite(g1).all()
    assert torch.equal(s1, s0)
    assert abs(l1.item() - l0.item()) <= 1e-6 * abs(l0.item())
    assert (g1 - g0).norm().item() <= 1e-5 * g0.norm().item() + 1e-7
    # poison: every bf16 / fp32 workspace tensor of the engine
    W = skip._bwd
    ts = (list(skip.z.values()) + list(skip.mult.values()) + list(skip.nrm.values()) + list(skip.part) + [skip.cnt, skip.E, skip.scores, skip.lse, skip.x16])
    for v in W.values():
        if torch.is_tensor(v):
            ts.append(v)
        elif isinstance(v, dict):
            ts += [t for t in v.values() if torch.is_tensor(t)]
        elif isinstance(v, (list, tuple)):
            ts += [t for t in v if torch.is_tensor(t)]
    for t in ts:
        if t is W.get('gscale'):
            continue
        if t.dtype in (torch.float32,):
            t.fill_(float('nan'))
        elif t.dtype in (torch.bfloat16,):
            t.fill_(float('nan'))
        elif t.dtype in (torch.int16, torch.uint16):
            t.fill_(0x7fc0)
    s2, l2, g2 = run(skip)
    assert torch.equal(s2, s1) and torch.equal(l2, l1) and torch.equal(g2, g1)
    xf1, xf2 = synthetic.make_batch(5300, G // 2, N, 'ErdosRenyi', 0.3, 0.1)
    run(skip, torch.cat([xf1, xf2]).contiguous().to(DEV), torch.full((G,), N, dtype=torch.int32, device=DEV))
    s3, l3, g3 = run(skip)
    assert torch.equal(s3, s1) and torch.equal(l3, l1) and torch.equal(g3, g1)


# ---------------------------------------------------------------------------------------------------------------------
# round 3: pinned to the reference where bf16 is not yet chaotic, and the backward kernels element by element
def test_one_block_against_the_reference_bf16_run():
    """The HIP bf16 engine on the reference-generated ONE-block fixtures (the reference itself run in bf16 / fp32 / fp64):
    at least as close to the fp64 truth as the reference's own bf16 run -- the gates of tests/test_oracle_bf16.py
    (flat gradient <= 1.0 x, per-tensor median <= 1.0 x and worst <= 3.0 x, scores <= 1.5 x)."""
    from test_oracle_bf16 import ONE_BLOCK_FIXTURES, one_block_gates
    for name in ONE_BLOCK_FIXTURES:
        d = load_golden(name)
        n = int(d['n'])
        x1, x2 = unpack_pairs(d['bits1'], n), unpack_pairs(d['bits2'], n)
        eng, lay, scores, loss, grads = _run(sub(d, 'sd/'), x1, x2, 1)
        one_block_gates(scores, grads, d)
        assert abs(loss - d['loss64'].item()) <= 1.0 * abs(d['loss_refbf16'].item() - d['loss64'].item()) + 2e-4


def _ulp_close_grad(got, ref, max_frac, what, flips=1e-2):
    """Gradient slabs: elements within one bf16 ulp of the oracle's value -- one ulp of the value itself or, for the entries
    that are small because their 32..64 products cancel (there the order of the fp32 accumulation and a one-ulp flip of an
    operand move the tiny result by more than ITS ulp), one ulp of the slab's root-mean-square magnitude -- and at most
    max_frac of the elements differing at all.  The MLP backward re-derives two ReLU masks from recomputed activations: where
    a pre-activation sits within rounding distance of 0 the mask -- and with it one of the 32 terms of that pixel's sums --
    may differ; such pixels are allowed for at most `flips` of the elements and stay below a quarter of the scale."""
    got, ref = got.float().cpu(), ref.float()
    diff = (got - ref).abs()
    scale = torch.maximum(ref.abs(), ref.pow(2).mean().sqrt().expand_as(ref))
    beyond = diff > ULP * scale + 1e-30
    assert beyond.float().mean().item() <= flips, (what, beyond.float().mean().item())
    assert (diff <= 0.25 * scale).all(), (what, (diff / scale).max().item())
    frac = (diff > 0).float().mean().item()
    assert frac <= max_frac, (what, frac)


@pytest.mark.parametrize('N,B', [(24, 2), (50, 2), (200, 1), (240, 1)])      # 240: the eight-column strip form of the products
def test_backward_kernels_element_wise_on_identical_inputs(N, B):
    """fgnn_colmax_bwd16, fgnn_mlp_bwd16 (mlp3: two input gradients; mlp1 / mlp2: read-modify-write of the block-input
    gradient) and fgnn_chan_matmul_bwd16 through the C ABI, each fed the ORACLE's bf16 values (forward slabs, arg-max indices,
    dE and, stage by stage, the previous kernel's output) and compared with oracle/fgnn_oracle_bf16.py's corresponding step:
    elements within one bf16 ulp (up to 1 % ReLU-flip pixels -- measured 0.2-0.7 % -- see _ulp_close_grad).  How many elements differ AT ALL
    depends on the depth of the rounded chain: at most 2 % for the matmul (one rounding after one product; measured 1.0 %); the MLP backward
    rounds dz, dpre_1 and dpre_0 to bf16 before each of its three dgrad GEMMs, a one-ulp flip of one of a sum's 32 operands
    moves the sum by ~0.2 ulp and re-rounds it with that probability, so the differing fraction grows ~6 x per stage
    (1e-3 -> 0.6 % -> 3.5 % -> 15-30 % measured on dmult / din3, 37-44 % after the accumulation of mlp1's share has rounded the
    block-input gradient once more; every one of them a single ulp).  Two blocks, so the
    accumulating variants run too."""
    sd = _sd(2, 40 + N)
    x1, x2 = synthetic.make_batch(300 + N, B, N, 'ErdosRenyi', 0.3 if N < 100 else 0.5, 0.1)
    keep = {}
    s_ref, l_ref, g_ref = OB.step_fwd_bwd(x1, x2, sd, keep=keep)
    lay = ParamLayout(2, 2, 32, 32, 3)
    params = lay.flatten(sd, DEV)
    grads = torch.zeros_like(params)
    eng = FgnnEngineBF16(lay, 2 * B, N, DEV)
    x = torch.cat([x1, x2]).contiguous().to(DEV)
    eng.forward(params, x, defer_loss=True)
    # identical inputs: the oracle's forward slabs, arg-max indices and dE replace the engine's own
    for k in (1, 2):
        eng.load_dense(eng.z[(k, 1)], keep[(k, 'z1')])
        eng.load_dense(eng.z[(k, 2)], keep[(k, 'z2')])
        eng.load_dense(eng.mult[k], keep[(k, 'mult')])
        eng.load_dense(eng.z[(k, 3)], keep[(k, 'z3')])
    eng.idx.copy_(keep['idx'].to(torch.int32))
    W = eng._alloc_bwd()
    seen = []

    def hook(stage, k):
        dy_in = W['dy'][(2 - k) % 2]             # gradient slab this block's mlp3 consumes
        din = W['dy'][(2 - k + 1) % 2]           # ... and the one its three MLPs produce (blocks > 1)
        if stage == 'colmax_bwd':
            assert torch.equal(eng.dense(dy_in).cpu(), keep['dy_last'])          # a pure scatter of bf16 values: exact
        elif stage == 'mlp3_bwd':
            _ulp_close_grad(eng.dense(W['dmult']), keep[(k, 'dmult')], 0.35, ('dmult', k))
            eng.load_dense(W['dmult'], keep[(k, 'dmult')])
            if k > 1:
                _ulp_close_grad(eng.dense(din), keep[(k, 'din3')], 0.35, ('din3', k))
                eng.load_dense(din, keep[(k, 'din3')])
        elif stage == 'matmul_bwd':
            _ulp_close_grad(eng.dense(W['dy1']), keep[(k, 'dy1')], 2e-2, ('dy1', k), flips=1e-4)     # no masks; isolated operand flips under cancellation
            _ulp_close_grad(eng.dense(W['dy2']), keep[(k, 'dy2')], 2e-2, ('dy2', k), flips=1e-4)
            eng.load_dense(W['dy1'], keep[(k, 'dy1')])
            eng.load_dense(W['dy2'], keep[(k, 'dy2')])
        elif stage == 'mlp1_bwd' and k > 1:
            _ulp_close_grad(eng.dense(din), keep[(k, 'din31')], 0.6, ('din31', k))
            eng.load_dense(din, keep[(k, 'din31')])
        elif stage == 'mlp2_bwd' and k > 1:
            _ulp_close_grad(eng.dense(din), keep[(k, 'din')], 0.6, ('din', k))
            eng.load_dense(din, keep[(k, 'din')])
        seen.append((stage, k))

    hook.per_mlp = True          # the two single-MLP launches (the pair kernel has no state between mlp1 and mlp2 to look at)
    eng.backward_from_dE(params, grads, keep['dE'].to(DEV).contiguous(), hook=hook)
    torch.cuda.synchronize()
    assert [s for s, _ in seen] == ['colmax_bwd'] + ['mlp3_bwd', 'matmul_bwd', 'mlp1_bwd', 'mlp2_bwd'] * 2
    # with every kernel on the oracle's inputs the parameter gradients (fp32 sums of bf16 products; the operands still carry
    # the kernels' own one-ulp flips and ReLU-flip pixels) agree to better than 1 % (measured 0.2-0.7 %; the end-to-end gate of
    # test_first_block_is_exact_up_to_rounding_flips is 5 %)
    got = lay.unflatten(grads.cpu())
    keys = [k for k in g_ref if not is_zero_grad(k)]
    assert l2rel(flat_of(got, keys), flat_of(g_ref, keys)) < 1e-2


@pytest.mark.parametrize('N,B', [(24, 3), (50, 8), (200, 2)])
def test_pair_backward16_equals_the_two_launches_it_replaces(N, B):
    """fgnn_mlp_bwd16_pair (mlp1 + mlp2 of a block in one launch): scores, loss and the stored block-input gradient slabs are
    bit-identical to the two read-modify-write fgnn_mlp_bwd16 launches -- R(R(d_in3 + dx1) + dx2) in both -- and the parameter
    gradients agree up to the association of the per-wave fp32 partial sums; bit-reproducible run to run."""
    sd = _sd(3, 70 + N)
    x1, x2 = synthetic.make_batch(800 + N, B, N, 'ErdosRenyi', 0.3 if N < 100 else 0.5, 0.1)
    lay = ParamLayout(2, 3, 32, 32, 3)
    params = lay.flatten(sd, DEV)
    x = torch.cat([x1, x2]).contiguous().to(DEV)
    out = []
    for pair in (False, True):
        old = FgnnEngineBF16.PAIR_BWD
        FgnnEngineBF16.PAIR_BWD = pair
        try:
            eng = FgnnEngineBF16(lay, 2 * B, N, DEV)
            g = torch.zeros_like(params)
            sc, loss = eng.step(params, g, x)
            torch.cuda.synchronize()
            out.append((sc.clone(), loss.clone(), g.clone(), eng.dense(eng._bwd['dy'][0]).clone(), eng.dense(eng._bwd['dy'][1]).clone()))
            g2 = torch.zeros_like(params)
            eng.step(params, g2, x)
            torch.cuda.synchronize()
            assert torch.equal(g, g2)
        finally:
            FgnnEngineBF16.PAIR_BWD = old
    a, b = out
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    assert ((a[2] - b[2]).norm() / a[2].norm()).item() < 1e-6
