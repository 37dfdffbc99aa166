"""GPU: inputs of 1 .. 32 channels on the bf16 engine -- the one-pass input conversion (fgnn_to_bf16_pad), FgnnEngineBF16 on a
32-channel layout, narrow / spectral models through Siamese_Node_Exp(...).half() and FgnnTrainer, and the paths that must not move.

The gates against oracle/fgnn_oracle_bf16.py are the ones tests/test_gpu_bf16.py applies to the 2-channel engine (imported, not
restated): distance to the same-point oracle <= SAME_POINT x the bf16 scheme's own distance to the un-rounded evaluation, loss
within 2e-3.  The oracle is generic in the input width but not in the block width (it splits mlp3's input gradient at channel 32),
so a narrow model is handed to it as its zero-padded image -- the same function: the extra channels carry exact zeros."""
import hashlib
import json
import os

import pytest
import torch

from graph_neural_net_amd import _lib, qap
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.engine16 import FgnnEngineBF16
from graph_neural_net_amd.masked import MaskedTensor
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.siamese import Siamese_Node_Exp
from graph_neural_net_amd.trainer import FgnnTrainer
from oracle import fgnn_oracle as O, fgnn_oracle_bf16 as OB
from test_gpu_bf16 import SAME_POINT
from util import BF16_CLASS, GOLDEN, flat_of, is_zero_grad, l2rel, load_golden, sub

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NE = dict(type='node_embedding', block_init='block_emb', block_inside='block', num_blocks=2, in_features=32, out_features=32,
          depth_of_mlp=3)


def _pitches(N):
    ldr = (N + 7) // 8 * 8
    return ldr, (N * ldr + 63) // 64 * 64


# ---------------------------------------------------------------------------------------------- 1. the conversion kernel alone
@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('N', [7, 8, 9, 33, 50])
def test_conversion_kernel_rounds_the_corner_and_zero_fills_the_rest(N, ragged):
    G = 4
    ldr, ldp = _pitches(N)
    gen = torch.Generator().manual_seed(100 * N + ragged)
    nvalid = [N, 1, 0, int(torch.randint(2, N, (1,), generator=gen))] if ragged else [N] * G
    for c, CP in ((1, 2), (2, 2), (1, 32), (2, 32), (3, 32), (4, 32), (31, 32), (32, 32)):      # (c <= 2: both slab widths)
        x = torch.randn(G, c, N, N, generator=gen) * 3
        # ties and carries: 1 + 2^-8 (tie -> even, down), 1 + 3 * 2^-8 (tie -> even, up), the largest fp32 below 2 (rounds up across the
        # binade to 2.0), 255.5 -> 256, a denormal, a value below half the smallest bf16 denormal's ulp, negative zero
        special = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 2 - 2.0 ** -23, 255.5, 1e-40, -1e-40, 2.0 ** -149, -0.0,
                                -(2 - 2.0 ** -23), 3.3895314e38])
        x.view(G, -1)[:, :special.numel()] = special
        for g, n in enumerate(nvalid):          # nothing outside the corner may be read
            x[g, :, n:, :] = float('nan')
            x[g, :, :, n:] = float('nan')
        y = torch.full((G * CP * ldp,), 0x7fc0, dtype=torch.int16, device=DEV)
        nv = torch.tensor(nvalid, dtype=torch.int32, device=DEV) if ragged else None
        xd = x.to(DEV)
        _lib.call('fgnn_to_bf16_pad', _lib.ptr(xd), _lib.ptr(nv), G, c, CP, N, ldr, _lib.ptr(y), ldp, _lib.stream_ptr())
        torch.cuda.synchronize()
        got = y.cpu().view(G, CP, ldp)
        want = torch.zeros(G, CP, ldp, dtype=torch.int16)
        plane = want[:, :, :N * ldr].view(G, CP, N, ldr)
        for g, n in enumerate(nvalid):
            plane[g, :c, :n, :n] = x[g, :, :n, :n].to(torch.bfloat16).view(torch.int16)
        assert torch.equal(got, want), (c, CP, (got != want).nonzero()[:4])


def test_conversion_kernel_takes_an_unaligned_input_and_refuses_bad_arguments():
    N, G, c = 8, 2, 3                     # N % 4 == 0: the 16-byte loads; a view 4 bytes into its storage must take the scalar ones
    ldr, ldp = _pitches(N)
    base = torch.randn(G * c * N * N + 1, device=DEV)
    x = base[1:].view(G, c, N, N)
    y = torch.full((G * 32 * ldp,), 0x7fc0, dtype=torch.int16, device=DEV)
    _lib.call('fgnn_to_bf16_pad', _lib.ptr(x), None, G, c, 32, N, ldr, _lib.ptr(y), ldp, _lib.stream_ptr())
    got = y.view(G, 32, ldp)[:, :c, :N * ldr].view(G, c, N, ldr)[..., :N]
    assert torch.equal(got, x.to(torch.bfloat16).view(torch.int16))
    for kw in (dict(c=0), dict(c=33), dict(c=3, CP=2), dict(CP=4), dict(ldr=N + 4), dict(ldp=ldp + 8)):
        a = dict(dict(c=c, CP=32, ldr=ldr, ldp=ldp), **kw)
        with pytest.raises(RuntimeError, match='fgnn_to_bf16_pad'):
            _lib.call('fgnn_to_bf16_pad', _lib.ptr(x), None, G, a['c'], a['CP'], N, a['ldr'], _lib.ptr(y), a['ldp'], _lib.stream_ptr())


# ---------------------------------------------------------------------------------------------- 2. the c0 = 32 engine
def _sd32(c0, num_blocks, seed, width=32):
    torch.manual_seed(seed)
    sd = O.init_state_dict(original_features_num=c0, num_blocks=num_blocks, in_features=width, out_features=width)
    g = torch.Generator().manual_seed(seed + 1)
    for k, v in sd.items():
        if k.endswith('.bias') and v.dim() == 1:
            v.add_(0.1 * torch.randn(v.shape, generator=g))
        elif k.endswith('gn.weight'):
            v.mul_(1 + 0.2 * torch.randn(v.shape, generator=g))
        elif k.endswith('gn.bias'):
            v.add_(0.05 * torch.randn(v.shape, generator=g))
    return sd


def _gates(scores, loss, grads, x1, x2, sd, what):
    """The same-point gates of tests/test_gpu_bf16.py (test_cfg4_full_size_against_same_point_oracle) on one dense batch."""
    s16, l16, g16 = OB.step_fwd_bwd(x1, x2, sd)
    s32, l32, g32 = O.step_fwd_bwd(x1, x2, sd)
    keys = [k for k in g32 if not is_zero_grad(k)]
    f = lambda g: flat_of(g, keys)
    ds, ys = l2rel(scores, s16), l2rel(s16, s32)
    dg, yg = l2rel(f(grads), f(g16)), l2rel(f(g16), f(g32))
    dl = abs(loss - l16.item()) / abs(l16.item())
    print('%s: scores %.3e vs yard %.3e (%.2f), grads %.3e vs yard %.3e (%.2f), loss rel %.2e'
          % (what, ds, ys, ds / ys, dg, yg, dg / yg, dl))
    assert torch.isfinite(scores).all() and all(torch.isfinite(g).all() for g in grads.values())
    assert ds <= SAME_POINT * ys, (what, ds, ys)
    assert dg <= SAME_POINT * yg, (what, dg, yg)
    assert dl < 2e-3, (what, dl)
    return g16


def _run32(sd, x1, x2):
    lay = ParamLayout(32, 2, 32, 32, 3)
    params = lay.flatten(sd, DEV)
    grads = torch.zeros_like(params)
    eng = FgnnEngineBF16(lay, x1.shape[0] * 2, x1.shape[-1], DEV)
    x = torch.cat([x1, x2]).contiguous().to(DEV)
    scores, loss = eng.step(params, grads, x)
    torch.cuda.synchronize()
    return eng, lay, params, x, scores, loss, grads


@pytest.mark.parametrize('N,B', [(7, 2), (8, 2), (9, 1), (33, 2), (50, 2)])
def test_c32_engine_against_the_same_point_oracle(N, B):
    """Scores, loss and every gradient tensor of a 32/32/32 model on a random (G, 32, N, N) input.  N = 7, 8, 9: the same-point gates
    of the 2-channel engine.  N = 33 and 50 do not fit them -- measured distance to the oracle / the oracle's own distance to the
    un-rounded evaluation: scores 0.59 and 0.69, flat gradient 0.58 and 0.86, against SAME_POINT = 0.5; 32 real-valued input
    channels leave block 1 with rounding flips the exact 0/1 inputs of the 2-channel engine do not have, and with ~10^5 pooled
    candidates some arg-max decisions differ -- so these two shapes are held to the reference's own bf16 run instead
    (tests/golden/make_bf16_c32.py), at the margin of the other multi-block reference fixtures (BF16_CLASS)."""
    if N < 33:
        sd = _sd32(32, 2, 40 + N)
        gen = torch.Generator().manual_seed(N)
        x1, x2 = torch.randn(B, 32, N, N, generator=gen), torch.randn(B, 32, N, N, generator=gen)
        eng, lay, params, x, scores, loss, grads = _run32(sd, x1, x2)
        _gates(scores.cpu(), loss.item(), lay.unflatten(grads.cpu()), x1, x2, sd, 'c32 N=%d B=%d' % (N, B))
    else:
        from golden.make_bf16_c32 import bf16c32_inputs
        d = load_golden('bf16c32_n%d_b%d_2blk.npz' % (N, B))
        x1, x2, digest = bf16c32_inputs(N, B)
        assert digest == bytes(d['x_sha256'].numpy()).hex(), 'the regenerated inputs are not the recorded ones'
        sd = sub(d, 'sd/')
        eng, lay, params, x, scores, loss, grads = _run32(sd, x1, x2)
        got = lay.unflatten(grads.cpu())
        keys = [k for k in sub(d, 'grad/') if not is_zero_grad(k)]
        g64, s64 = flat_of(sub(d, 'grad64/'), keys), d['scores64_as_f32']
        rs = l2rel(scores, s64) / l2rel(d['scores_refbf16'], s64)
        rg = l2rel(flat_of(got, keys), g64) / l2rel(flat_of(sub(d, 'grad_refbf16/'), keys), g64)
        print('c32 N=%d B=%d vs the reference bf16 run: scores %.2f x, flat gradient %.2f x, loss %.2e vs %.2e'
              % (N, B, rs, rg, abs(loss.item() - d['loss64'].item()), abs(d['loss_refbf16'].item() - d['loss64'].item())))
        assert torch.isfinite(scores).all() and torch.isfinite(grads).all()
        assert rs <= BF16_CLASS and rg <= BF16_CLASS, (rs, rg)
        assert abs(loss.item() - d['loss64'].item()) <= BF16_CLASS * abs(d['loss_refbf16'].item() - d['loss64'].item()) + 1e-3
    # the two single-MLP backward launches (what a ragged batch takes) instead of the pair launch: the same bf16 operands summed
    # in fp32 in another order, so the flat gradients agree to fp32 accumulation noise (n 2^-24 per sum, far below 1e-4 in L2)
    g2 = torch.zeros_like(params)
    eng.PAIR_BWD = False
    eng.step(params, g2, x)
    assert l2rel(g2, grads) < 1e-4


@pytest.mark.parametrize('c', [1, 2, 4])
@pytest.mark.parametrize('ragged', [False, True])
def test_fewer_channels_on_the_c32_engine_equal_the_zero_padded_image(c, ragged):
    """A (G, c, N, N) input with c below the slab's 32 channels -- c = 1, 2 included, where a 2-channel slab also exists -- gives the
    bits of its zero-padded 32-channel image: scores, loss, gradients and the whole input slab (pre-filled with NaN patterns)."""
    N, B = 9, 2
    lay = ParamLayout(32, 2, 32, 32, 3)
    params = lay.init_flat(c, DEV)
    gen = torch.Generator().manual_seed(c)
    x = torch.randn(2 * B, c, N, N, generator=gen)
    nv = torch.tensor([9, 4, 9, 4], dtype=torch.int32, device=DEV) if ragged else None
    if ragged:
        x[1, :, 4:, :] = x[1, :, :, 4:] = x[3, :, 4:, :] = x[3, :, :, 4:] = 0
    xp = torch.zeros(2 * B, 32, N, N)
    xp[:, :c] = x
    out = []
    for inp in (x, xp):
        eng = FgnnEngineBF16(lay, 2 * B, N, DEV, ragged=ragged)
        eng.x16.view(torch.int16).fill_(0x7fc0)
        grads = torch.full_like(params, float('nan'))
        scores, loss = eng.step(params, grads, inp.contiguous().to(DEV), nvalid=nv)
        torch.cuda.synchronize()
        assert torch.isfinite(grads).all() and torch.isfinite(scores).all()
        out.append((scores.clone(), loss.clone(), grads, eng.x16.view(torch.int16).clone()))
    assert all(torch.equal(a, b) for a, b in zip(*out))
    with pytest.raises(RuntimeError, match='1 <= c <= 32'):
        eng.embed(params, torch.zeros(2 * B, 33, N, N, device=DEV), nv)
    with pytest.raises(RuntimeError, match='1 <= c <= 2'):
        FgnnEngineBF16(ParamLayout(2, 1, 32, 32, 3), 2 * B, N, DEV).embed(params, torch.zeros(2 * B, 3, N, N, device=DEV))


def test_modules_and_captured_steps_insist_on_their_channel_count():
    x4, x2 = torch.randn(2, 4, 8, 8, device=DEV), torch.randn(2, 2, 8, 8, device=DEV)
    for c0 in (4, 32):                       # a padded and an unpadded 16-bit module
        model = Siamese_Node_Exp(c0, NE).to(DEV).half()
        for call in (lambda: model(x2, x2), lambda: model.fused_step(x2, x2, capture=False), lambda: model.match(x2, x2, weighted=True)):
            with pytest.raises(RuntimeError, match='original_features_num = %d' % c0):
                call()
    lay = ParamLayout(32, 1, 32, 32, 3)
    tr = FgnnTrainer(lay, lay.init_flat(0, DEV), capture=True, precision='bf16')
    tr.train_step(x4, x4)
    for bad in (x2, x4[:, :1].contiguous()):
        with pytest.raises(RuntimeError, match='one channel count per'):
            tr.train_step(bad, bad)


# ---------------------------------------------------------------------------------------------- 3. narrow models = their padded image
def _padded(net):
    """(padded layout, padded flat parameters, boolean mask of the real entries) of a narrow module's node embedder."""
    lay = net._standard_layout()
    net._bind_flat()
    idx = net._pad['idx'].to(DEV)
    pflat = torch.zeros(lay.total, device=DEV)
    pflat[idx] = net._flat
    real = torch.zeros(lay.total, dtype=torch.bool, device=DEV)
    real[idx] = True
    return lay, pflat, idx, real


def _pad_x(x, c=32):
    out = torch.zeros(x.shape[0], c, *x.shape[2:])
    out[:, :x.shape[1]] = x
    return out


@pytest.mark.parametrize('c0,width,N', [(4, 32, 9), (3, 16, 33), (4, 24, 8)])
def test_narrow_half_models_equal_their_padded_image(c0, width, N):
    B = 2
    torch.manual_seed(c0 * 100 + width)
    model = Siamese_Node_Exp(c0, dict(NE, in_features=width, out_features=width)).to(DEV).half()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith('.bias') and p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    gen = torch.Generator().manual_seed(N)
    x1, x2 = torch.randn(B, c0, N, N, generator=gen), torch.randn(B, c0, N, N, generator=gen)
    net = model.node_embedder
    loss, scores = model.fused_step(x1.to(DEV), x2.to(DEV), capture=False)
    lay, pflat, idx, real = _padded(net)
    assert lay.c0 == 32 and net._pad['c0'] == c0
    narrow_grad = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
    pgrads = torch.full_like(pflat, float('nan'))
    eng = FgnnEngineBF16(lay, 2 * B, N, DEV)
    s_hand, l_hand = eng.step(pflat, pgrads, torch.cat([_pad_x(x1), _pad_x(x2)]).contiguous().to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(scores, s_hand) and torch.equal(loss.reshape(1), l_hand.reshape(1))
    assert torch.equal(narrow_grad, pgrads[idx])
    assert (pgrads[~real] == 0).all()
    # the eager module path runs the same engine: same embeddings, hence close scores, and the same parameter gradients
    model.zero_grad(set_to_none=True)
    s_mod = model(x1.to(DEV), x2.to(DEV))
    model.loss(s_mod).backward()
    assert l2rel(s_mod, s_hand) < 1e-5
    g_mod = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
    assert l2rel(g_mod, narrow_grad) < 1e-4
    sd = lay.unflatten(pflat.cpu())
    _gates(s_hand.cpu(), l_hand.item(), lay.unflatten(pgrads.cpu()), _pad_x(x1), _pad_x(x2), sd, 'narrow c0=%d w=%d' % (c0, width))


# ---------------------------------------------------------------------------------------------- 4. spectral pairs end to end
def _spectral_model(seed=5):
    torch.manual_seed(seed)
    return Siamese_Node_Exp(4, NE).to(DEV)


def test_spectral_pairs_train_and_decode_in_16_bit():
    gen = PairGenerator(20, 'ErdosRenyi', 'ErdosRenyi', 0.3, 0.05, seed=3, device=DEV)
    b1, b2 = gen.spectral(0, 4)
    x1, x2 = b1['input'], b2['input']
    assert x1.shape == (4, 4, 20, 20)
    model = _spectral_model().half()
    loss, scores = model.fused_step(b1, b2, capture=False)
    lay, pflat, idx, real = _padded(model.node_embedder)
    grads = torch.zeros(lay.total)
    grads[idx.cpu()] = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu()
    _gates(scores.cpu(), loss.item(), lay.unflatten(grads), _pad_x(x1.cpu()), _pad_x(x2.cpu()), lay.unflatten(pflat.cpu()), 'spectral N=20')
    # captured = eager, bit for bit
    g_eager = [p.grad.clone() for p in model.parameters()]
    loss_c, scores_c = model.fused_step(b1, b2, capture=True)
    assert torch.equal(loss_c, loss) and torch.equal(scores_c, scores)
    assert all(torch.equal(p.grad, g) for p, g in zip(model.parameters(), g_eager))
    # decode: the objective of the 16-bit model's own matching is what the fp32 decoder gives for that assignment
    out = model.match(b1, b2, weighted=True)
    assert out['assign'].shape == (4, 20) and torch.isfinite(out['qap']).all()
    assert torch.equal(out['qap'], qap.objective_weighted(x1, x2, out['assign'], None)['qap'])
    import qap_weighted_ref as R          # ... and the float64 objective of that matching, within the any-order fp32 summation bound
    for b in range(4):
        A, Bm, pi = x1[b, 0].double().cpu().numpy(), x2[b, 0].double().cpu().numpy(), out['assign'][b].cpu().numpy()
        assert sorted(pi) == list(range(20))
        assert abs(out['qap'][b].item() - R.objective(A, Bm, pi)[0]) <= R.objective_bounds(A, Bm, pi)[0]
    fp32 = _spectral_model()
    fp32.load_state_dict(model.state_dict())
    ref = fp32.match(b1, b2, weighted=True)
    assert l2rel(out['scores'], ref['scores']) < 5e-2          # the two precisions score the same pairs alike


def test_ragged_spectral_batch_equals_the_per_pair_dense_runs():
    gen = PairGenerator(20, 'ErdosRenyi', 'ErdosRenyi', 0.3, 0.05, vertex_proba=0.8, seed=4, device=DEV)
    m1, m2 = gen.spectral(0, 4)
    assert isinstance(m1, MaskedTensor)
    ns = [int(n) for n in m1.nvalid.cpu()]
    model = _spectral_model(6).half()
    loss, scores = model.fused_step(m1, m2, capture=False)
    s = scores.tensor.rename(None).cpu()
    lay, pflat, idx, real = _padded(model.node_embedder)
    sd = lay.unflatten(pflat.cpu())
    got = torch.zeros(lay.total)
    got[idx.cpu()] = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu()
    got = lay.unflatten(got)
    t1, t2 = m1.tensor.rename(None).cpu(), m2.tensor.rename(None).cpu()
    total = float(sum(ns))
    g16 = g32 = None
    for i, n in enumerate(ns):
        a, b = _pad_x(t1[i:i + 1, :, :n, :n]), _pad_x(t2[i:i + 1, :, :n, :n])
        si, _, g = OB.step_fwd_bwd(a, b, sd, total_nodes=total)
        _, _, gf = OB.step_fwd_bwd(a, b, sd, rounding=False, total_nodes=total)
        g16 = g if g16 is None else {k: g16[k] + g[k] for k in g}
        g32 = gf if g32 is None else {k: g32[k] + gf[k] for k in gf}
        assert s[i, n:, :].abs().sum() == 0 and s[i, :, n:].abs().sum() == 0
        assert l2rel(s[i, :n, :n], si[0]) < 2e-2, (i, n)
        # ... and the same pair as a dense batch of its own through the module
        alone = model.match(m1.tensor.rename(None)[i:i + 1, :, :n, :n].contiguous(), m2.tensor.rename(None)[i:i + 1, :, :n, :n].contiguous(),
                            weighted=True)['scores']
        assert l2rel(s[i, :n, :n], alone[0]) < 2e-2
    keys = [k for k in g16 if not is_zero_grad(k)]
    f = lambda g: flat_of(g, keys)
    print('ragged spectral: grads %.3e vs yard %.3e' % (l2rel(f(got), f(g16)), l2rel(f(g16), f(g32))))
    assert l2rel(f(got), f(g16)) <= SAME_POINT * l2rel(f(g16), f(g32))


# ---------------------------------------------------------------------------------------------- 5. trainer
def test_trainer_on_four_channel_batches():
    N, B = 20, 4
    gen = PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', 0.3, 0.05, seed=9, device=DEV)
    batches = [tuple(d['input'] for d in gen.spectral(4 * i, B)) for i in range(3)]
    runs = {}
    for name in ('eager16', 'graph16'):
        model = _spectral_model(7).half()
        tr = FgnnTrainer.from_module(model, lr=1e-3, capture=name == 'graph16')
        assert tr.precision == 'bf16' and tr.layout.c0 == 32
        losses = [tr.train_step(*batches[s])[0].item() for s in range(3)]
        runs[name] = (losses, tr.params.clone(), model)
        # the module sees the trained values
        assert torch.equal(model.node_embedder._flat, tr.params[model.node_embedder._pad['idx']])
    assert runs['eager16'][0] == runs['graph16'][0]
    assert torch.equal(runs['eager16'][1], runs['graph16'][1])
    # the fp32 trainer on the same data (its engine takes the 32-channel image of the batch)
    model = _spectral_model(7)
    lay, pflat, idx, real = _padded(model.half().node_embedder)
    tr32 = FgnnTrainer(lay, pflat.clone(), lr=1e-3)
    l32 = [tr32.train_step(_pad_x(batches[s][0].cpu()).to(DEV), _pad_x(batches[s][1].cpu()).to(DEV))[0].item() for s in range(3)]
    l16 = runs['eager16'][0]
    print('trainer: bf16 %s fp32 %s' % (l16, l32))
    for a, b in zip(l16, l32):                   # the gate of test_bf16_trainer_captured_equals_eager_and_tracks_fp32
        assert abs(a - b) < 5e-2 * abs(b), (l16, l32)
    assert abs(l16[0] - l32[0]) < 5e-3 * abs(l32[0])
    assert (runs['eager16'][1][~real] == 0).all()          # the padded entries stay exact zeros under Adam
    # eval_step: parameters, moments and gradients keep their bits
    tr = FgnnTrainer(lay, runs['eager16'][1].clone(), lr=1e-3, precision='bf16')
    tr.train_step(*batches[0])
    before = [t.clone() for t in (tr.params, tr.grads, tr.opt.exp_avg, tr.opt.exp_avg_sq)]
    out = tr.eval_step(*batches[1])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (tr.params, tr.grads, tr.opt.exp_avg, tr.opt.exp_avg_sq)))
    assert out['ce'].shape[0] == B and torch.isfinite(out['ce']).all()


# ---------------------------------------------------------------------------------------------- 6. unchanged paths
def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def c2_digests(pair_bwd=True):
    """{case: sha256 of (scores, loss, flat gradient)} of the 2-channel bf16 engine: tests/golden/make_bf16_c2_digest.py records them.
    pair_bwd=False: the dense cases with PAIR_BWD off on the engine, i.e. mlp1 and mlp2 of a block as two fgnn_mlp_bwd16 launches --
    the only way to the kernels mlp_bwd16<2,0,3> and <32,0,3> without tile ranges (a ragged batch runs their SKIP twins)."""
    from graph_neural_net_amd import synthetic
    out = {}
    lay = ParamLayout(2, 2, 32, 32, 3)
    params = lay.init_flat(3, DEV)
    cases = (('dense_n33_b2', 33, 2, None), ('dense_n8_b1', 8, 1, None), ('ragged_n24_b3', 24, 3, [24, 7, 15]))
    for name, N, B, nvalid in cases if pair_bwd else cases[:2]:
        x1, x2 = synthetic.make_batch(500 + N, B, N, 'ErdosRenyi', 0.3, 0.05)
        x = torch.cat([x1, x2]).contiguous().to(DEV)
        nv = None
        if nvalid is not None:
            for g, n in enumerate(nvalid * 2):
                x[g, :, n:, :] = 0
                x[g, :, :, n:] = 0
            nv = torch.tensor(nvalid * 2, dtype=torch.int32, device=DEV)
        grads = torch.zeros_like(params)
        eng = FgnnEngineBF16(lay, 2 * B, N, DEV, ragged=nvalid is not None)
        eng.PAIR_BWD = pair_bwd
        scores, loss = eng.step(params, grads, x, nvalid=nv)
        torch.cuda.synchronize()
        out[name] = _digest(scores, loss, grads)
    return out


def test_two_channel_engine_keeps_its_bits():
    """Recorded with the library of the commit before the 32-channel input slab existed."""
    want = json.load(open(os.path.join(GOLDEN, 'bf16_c2_digest.json')))
    assert c2_digests() == want


def test_two_channel_engine_keeps_its_bits_without_the_pair_launch():
    """The two dense cases with the single-MLP backward launches (mlp_bwd16<2,0,3>, <32,0,3> without tile ranges).  Recorded with the
    library of commit 0ebc75b, the last one before these two kernels and their pair twin took their common tile body from
    fgnn_bwd16.h as macros: tests/golden/make_bf16_c2_digest.py nopair.  (With 84 and 2 tiles for 256 workgroups no workgroup sums
    two tiles, so the order of the fp32 sums is the pair launch's and the recorded digests equal those of the test above.)"""
    want = json.load(open(os.path.join(GOLDEN, 'bf16_c2_nopair_digest.json')))
    assert sorted(want) == ['dense_n33_b2', 'dense_n8_b1']
    assert c2_digests(pair_bwd=False) == want


def test_refusals_keep_their_ground():
    lay32 = ParamLayout(32, 1, 32, 32, 3)
    eng = FgnnEngineBF16(lay32, 2, 8, DEV, block1='structured')
    assert not eng.struct1
    with pytest.raises(RuntimeError, match='2 input channels'):
        eng.embed(lay32.init_flat(0, DEV), None, bits=torch.zeros(2, 8, 1, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match='N <= 256'):
        FgnnEngineBF16(lay32, 2, 257, DEV)
    x = torch.randn(1, 4, 8, 8, device=DEV)
    for ne in (dict(NE, in_features=33, out_features=33), dict(NE, depth_of_mlp=2)):
        model = Siamese_Node_Exp(4, ne).to(DEV).half()
        with pytest.raises(RuntimeError, match='width above 32 or another depth'):
            model(x, x)
    with pytest.raises(RuntimeError, match='16-bit'):
        FgnnTrainer.from_module(Siamese_Node_Exp(4, NE).to(DEV))          # fp32 padded modules: not the trainer's
