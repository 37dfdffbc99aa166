"""GPU, end to end: training and validating on planted pairs -- EngineBase.step(labels=), the FgnnTrainer steps, epochs, evaluation
and fit with labels, triplet_loss(labels=) and Siamese_Node_Exp.fused_step(labels=).

Shapes of the section 11.2 end-to-end check: 2 blocks, B = 4, N = 20 and a ragged batch with n in [9, 20]; fp32 and bf16.
There is no tight bound on the end-to-end GRADIENT between a pair and its relabelled form: ReLU and arg-max near-ties may flip
under the other summation order.  The gradient is covered by the dE test of tests/test_gpu_ce_labels.py plus the wiring test
here (identity labels == no labels, bit for bit, through the whole step)."""
import numpy as np
import pytest
import torch

import ce_labels_ref as R
from eval_ref import CE_BOUND
from graph_neural_net_amd import planted, synthetic
from graph_neural_net_amd.engine import FgnnEngine, ParamLayout
from graph_neural_net_amd.engine16 import FgnnEngineBF16
from graph_neural_net_amd.evaluation import EvalMeter
from graph_neural_net_amd.losses import triplet_loss
from graph_neural_net_amd.masked import MaskedTensor
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.sampler import EpochSampler
from graph_neural_net_amd.siamese import Siamese_Node_Exp
from graph_neural_net_amd.trainer import FgnnTrainer
from oracle import fgnn_oracle as O
from test_gpu_parity import E2E_FWD_TOL
from util import rel

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LAY = ParamLayout(2, 2, 32, 32, 3)
B, N = 4, 20
RAGGED_SIZES = [9, 20, 14, 17]


def _engine(precision, ragged, block1=None):
    cls = FgnnEngineBF16 if precision == 'bf16' else FgnnEngine
    return cls(LAY, 2 * B, N, DEV, ragged=ragged, block1=block1)


def _batch(ragged, seed=77):
    """(x1, x2) dense (B, 2, N, N) on the GPU, zero-padded; nvalid (B,) int32 or None; the per-graph lists for the oracle"""
    rng = np.random.default_rng(seed)
    sizes = RAGGED_SIZES if ragged else [N] * B
    pairs = [synthetic.make_pair(rng, n, 'ErdosRenyi', 0.3, 0.1) for n in sizes]
    l1, l2 = [torch.from_numpy(p[0]) for p in pairs], [torch.from_numpy(p[1]) for p in pairs]
    x1, x2 = torch.zeros(B, 2, N, N), torch.zeros(B, 2, N, N)
    for b, n in enumerate(sizes):
        x1[b, :, :n, :n], x2[b, :, :n, :n] = l1[b], l2[b]
    nv = torch.tensor(sizes, dtype=torch.int32, device=DEV) if ragged else None
    return x1.to(DEV), x2.to(DEV), nv, sizes, l1, l2


def _labels(sizes, kind, seed=5):
    """(B, N) int32 on the GPU, -1 in the padding: 'identity', a random permutation, or a cyclic shift (no fixed point)"""
    rng = np.random.default_rng(seed)
    lab = np.full((B, N), -1, dtype=np.int32)
    for b, n in enumerate(sizes):
        lab[b, :n] = {'identity': np.arange(n), 'perm': rng.permutation(n), 'shift': (np.arange(n) + 1) % n}[kind]
    return torch.from_numpy(lab).to(DEV)


def _step(eng, params, x1, x2, nv, labels=None):
    grads = torch.full_like(params, float('nan'))
    nv2 = None if nv is None else torch.cat([nv, nv])
    kw = {} if labels is None else {'labels': labels}
    scores, loss = eng.step(params, grads, torch.cat([x1, x2]).contiguous(), nvalid=nv2, **kw)
    torch.cuda.synchronize()
    return scores.clone(), loss.clone(), grads


# ---- 1. wiring ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_identity_labels_are_the_label_less_step_eager(precision, ragged):
    x1, x2, nv, sizes, _, _ = _batch(ragged)
    params = LAY.init_flat(3, DEV)
    eng = _engine(precision, ragged)
    s0, l0, g0 = _step(eng, params, x1, x2, nv)
    s1, l1, g1 = _step(eng, params, x1, x2, nv, _labels(sizes, 'identity'))
    assert torch.equal(s0, s1) and torch.equal(l0, l1) and torch.equal(g0, g1) and not torch.isnan(g0).any()
    s2, l2, g2 = _step(eng, params, x1, x2, nv)                     # ... and the engine goes back to the label-less launches
    assert torch.equal(s0, s2) and torch.equal(l0, l2) and torch.equal(g0, g2)


@pytest.mark.parametrize('block1', ['structured', None])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_identity_labels_are_the_label_less_step_captured(precision, block1):
    """two trainers on the same batches, one with labels = arange: parameters, losses and scores bit for bit over three steps.
    structured block 1 takes the bit-packed batches, the generic kernels the dense ones."""
    gen = PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.05, seed=4, device=DEV)
    ident = _labels([N] * B, 'identity')
    a = FgnnTrainer(LAY, LAY.init_flat(5, DEV), lr=2e-3, capture=True, precision=precision, block1=block1)
    b = FgnnTrainer(LAY, LAY.init_flat(5, DEV), lr=2e-3, capture=True, precision=precision, block1=block1)
    for k in range(3):
        if block1 == 'structured':
            b1, b2, _ = gen.bits(B * k, B)
            la, sa = a.train_step_bits(b1, b2)
            lb, sb = b.train_step_bits(b1, b2, labels=ident)
        else:
            x1, x2 = gen.dense(B * k, B)
            la, sa = a.train_step(x1['input'], x2['input'])
            lb, sb = b.train_step(x1['input'], x2['input'], labels=ident)
        assert torch.equal(la, lb) and torch.equal(sa, sb) and torch.equal(a.grads, b.grads), k
    assert torch.equal(a.params, b.params) and a.opt.t == b.opt.t == 3
    assert any('labels' in key for key in b._graphs) and not any('labels' in key for key in a._graphs)


# ---- 2. the loss of a relabelled pair against its labels is the loss of the pair ----------------------------------------------------
def _oracle_losses(l1, l2, l2p, lab, sizes, sd):
    o_a, o_b = O.siamese_scores_ragged(l1, l2, sd), O.siamese_scores_ragged(l1, l2p, sd)
    ce = torch.nn.functional.cross_entropy
    a = sum(ce(s, torch.arange(n), reduction='sum') for s, n in zip(o_a, sizes)) / sum(sizes)
    b = sum(ce(s, lab[i, :n].long().cpu(), reduction='sum') for i, (s, n) in enumerate(zip(o_b, sizes))) / sum(sizes)
    return a.item(), b.item()


@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_loss_is_equivariant(precision, ragged):
    """loss(x1, relabel(x2, pi), labels=pi) against loss(x1, x2): the same function summed in another order.  Bound: 2 * E2E_FWD_TOL
    relative; if the fp32 CPU oracle's own difference between the two forms exceeds E2E_FWD_TOL, twice that difference (the rule
    of tests/test_gpu_planted.py for the scores)."""
    x1, x2, nv, sizes, l1, l2 = _batch(ragged)
    lab = _labels(sizes, 'perm')
    x2p = planted.relabel(x2, lab, nvalid=nv)
    params = LAY.init_flat(3, DEV)
    eng = _engine(precision, ragged)
    _, la, _ = _step(eng, params, x1, x2, nv)
    _, lb, gb = _step(eng, params, x1, x2p, nv, lab)
    assert bool(torch.isfinite(gb).all())
    sd = LAY.unflatten(params.cpu())
    l2p = [x2p[i, :, :n, :n].cpu() for i, n in enumerate(sizes)]
    oa, ob = _oracle_losses(l1, l2, l2p, lab, sizes, sd)
    own = abs(oa - ob) / abs(oa)
    tol = 2 * E2E_FWD_TOL if own <= E2E_FWD_TOL else 2 * own
    diff = abs(la.item() - lb.item()) / abs(la.item())
    print('%s ragged=%s: loss %.8f, relabelled with labels %.8f: differ by %.3g (oracle fp32 on the CPU: %.3g; bound %.3g)'
          % (precision, ragged, la.item(), lb.item(), diff, own, tol))
    assert diff < tol


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_the_labelled_step_is_not_the_identity_step(precision):
    """a permutation without a fixed point: against the identity the relabelled pair has the larger loss and another gradient"""
    x1, x2, nv, sizes, _, _ = _batch(False)
    lab = _labels(sizes, 'shift')
    x2p = planted.relabel(x2, lab)
    # a model a few steps into training (an untrained one scores every column alike and both losses sit at log n)
    tr = FgnnTrainer(LAY, LAY.init_flat(3, DEV), lr=2e-3, precision=precision)
    for _ in range(12):
        tr.train_step(x1, x2p, labels=lab)
    eng = _engine(precision, False)
    _, l_id, g_id = _step(eng, tr.params, x1, x2p, None)
    _, l_lab, g_lab = _step(eng, tr.params, x1, x2p, None, lab)
    print('%s: loss against the identity %.6f, against the labels %.6f' % (precision, l_id.item(), l_lab.item()))
    assert l_id.item() > l_lab.item()
    assert not torch.equal(g_id, g_lab) and rel(g_id, g_lab) > 1e-2


# ---- 3. the trainer -------------------------------------------------------------------------------------------------------------------
def _gen(seed=11, vp=1.0):
    return PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.05, vertex_proba=vp, seed=seed, device=DEV)


def _state(tr):
    return [t.clone() for t in (tr.params, tr.grads, tr.opt.exp_avg, tr.opt.exp_avg_sq, tr.opt._dev_state()[1][0:1])]


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_train_epoch_on_planted_pairs_lowers_the_labelled_loss(precision):
    """(the precedent: the 64-feature model trains, tests/test_gpu_widths.py)  Eight pairs, five epochs of two steps."""
    gen, M = _gen(1), 8
    tr = FgnnTrainer(LAY, LAY.init_flat(7, DEV), lr=2e-3, precision=precision, block1='structured' if precision == 'bf16' else None)
    val = lambda: tr.evaluate(gen, EpochSampler(M, shuffle=False), B, permute=True, loss_on_labels=True).result()
    before = val()
    for epoch in range(5):
        losses = tr.train_epoch(gen, EpochSampler(M, seed=1), epoch, B, permute=True)
        assert losses.shape == (2,) and bool(torch.isfinite(losses).all())
    after = val()
    print('%s: labelled validation loss %.5f -> %.5f (acc %.3f -> %.3f)' % (precision, before['loss'], after['loss'], before['acc'], after['acc']))
    assert after['loss'] < before['loss'] and tr.opt.t == 10


@pytest.mark.parametrize('vp', [1.0, 0.8])
def test_evaluate_loss_on_labels(vp):
    gen, M = _gen(3, vp), 4
    tr = FgnnTrainer(LAY, LAY.init_flat(7, DEV))
    tr.train_step_bits(*gen.bits(0, B))
    before = _state(tr)
    # one step holds the whole epoch: the scores it evaluated are still in the engine
    rec = tr.evaluate(gen, EpochSampler(M, shuffle=False), B, permute=True, loss_on_labels=True).record()
    b1, b2, nv, lab = gen.bits(0, B, permute=True)
    s = tr._engine(2 * B, N, nv is not None).scores.cpu().double().numpy()
    nvn = np.full(B, N) if nv is None else nv.cpu().numpy()
    labn = lab.cpu().numpy()
    lse, ce, _ = R.batch_ce(s, labn, nvn)
    scale = R.ce_scale(s, lse, labn, nvn).sum()
    err = abs(rec['ce_sum'] - ce.sum())
    print('vertex_proba %.1f: labelled loss %.8f (host %.8f), error / bound %.3g' % (vp, rec['ce_sum'] / rec['nodes'], ce.sum() / nvn.sum(),
                                                                                   err / (CE_BOUND * scale)))
    assert err <= CE_BOUND * scale and rec['nodes'] == int(nvn.sum()) and rec['pairs'] == M
    # the default keeps today's record: the loss against the identity, bit for bit
    plain = tr.evaluate(gen, EpochSampler(M, shuffle=False), B, permute=True).record()
    off = tr.evaluate(gen, EpochSampler(M, shuffle=False), B, permute=True, loss_on_labels=False).record()
    assert plain == off and plain['ce_sum'] != rec['ce_sum']
    assert all(plain[k] == rec[k] for k in ('nodes', 'correct_lsap', 'correct_max', 'pairs', 'steps'))
    _, ce_id, _ = R.batch_ce(s, np.where(np.arange(N)[None, :] < nvn[:, None], np.arange(N)[None, :], -1), nvn)
    assert abs(plain['ce_sum'] - ce_id.sum()) <= CE_BOUND * (np.abs(lse).sum() + np.abs(s).max() * nvn.sum())
    # without permute the keyword changes nothing (there are no labels)
    assert (tr.evaluate(gen, EpochSampler(M, shuffle=False), B, loss_on_labels=True).record()
            == tr.evaluate(gen, EpochSampler(M, shuffle=False), B).record())
    assert all(torch.equal(x, y) for x, y in zip(before, _state(tr)))


def test_fit_on_planted_pairs_hands_the_labelled_loss_to_the_scheduler():
    seen = []
    sched = type('S', (), {'step': lambda self, v: seen.append(v)})()
    tr = FgnnTrainer(LAY, LAY.init_flat(7, DEV), lr=1e-3)
    vgen, vs = _gen(2), EpochSampler(6, shuffle=False)
    hist = tr.fit(_gen(1), EpochSampler(8, seed=1), vgen, vs, epochs=2, batch_size=B, scheduler=sched, permute=True)
    assert [h['epoch'] for h in hist] == [0, 1] and all(h['train_losses'].shape == (2,) for h in hist) and tr.opt.t == 4
    assert seen == [h['val_loss'] for h in hist]
    lab = tr.evaluate(vgen, vs, B, epoch=1, permute=True, loss_on_labels=True).result()
    ident = tr.evaluate(vgen, vs, B, epoch=1, permute=True).result()
    assert seen[1] == lab['loss'] != ident['loss'] and hist[1]['val_acc'] == lab['acc'] and hist[1]['val_acc_max'] == lab['acc_max']


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_captured_labelled_step_is_the_eager_labelled_step(precision):
    """fresh labels on every call: the captured step copies them into its static buffer.  One trainer holds the labelled and the
    label-less graph and alternates them."""
    gen = _gen(9)
    kw = dict(lr=2e-3, precision=precision, block1='structured')
    a = FgnnTrainer(LAY, LAY.init_flat(5, DEV), capture=True, **kw)
    b = FgnnTrainer(LAY, LAY.init_flat(5, DEV), capture=False, **kw)
    for k in range(4):
        if k == 2:
            b1, b2, _ = gen.bits(B * k, B)
            la, sa = a.train_step_bits(b1, b2)
            lb, sb = b.train_step_bits(b1, b2)
        else:
            b1, b2, _, lab = gen.bits(B * k, B, permute=True)
            la, sa = a.train_step_bits(b1, b2, labels=lab)
            lb, sb = b.train_step_bits(b1, b2, labels=lab)
        assert torch.equal(la, lb) and torch.equal(sa, sb) and torch.equal(a.grads, b.grads), k
    assert torch.equal(a.params, b.params) and set(a._graphs) == {(B, N, 'bits'), (B, N, 'bits', 'labels')}


def test_train_step_ragged_takes_per_graph_labels():
    """the list API: every pair's label array follows it through the size buckets; with the identity it is the label-less step"""
    x1, x2, nv, sizes, l1, l2 = _batch(True)
    xs, ys = [t.to(DEV) for t in l1], [t.to(DEV) for t in l2]
    a = FgnnTrainer(LAY, LAY.init_flat(5, DEV))
    b = FgnnTrainer(LAY, LAY.init_flat(5, DEV))
    la, _ = a.train_step_ragged(xs, ys, granule=8)
    lb, _ = b.train_step_ragged(xs, ys, granule=8, labels=[np.arange(n) for n in sizes])
    assert torch.equal(la, lb) and torch.equal(a.params, b.params)
    lab = _labels(sizes, 'perm')
    yp = [planted.relabel(y[None], lab[i:i + 1, :n].contiguous())[0] for i, (y, n) in enumerate(zip(ys, sizes))]
    c = FgnnTrainer(LAY, LAY.init_flat(5, DEV))
    lc, _ = c.train_step_ragged(xs, yp, granule=8, labels=[lab[i, :n].cpu().numpy() for i, n in enumerate(sizes)])
    assert abs(lc.item() - la.item()) < 2 * E2E_FWD_TOL * abs(la.item()) * 4        # (several buckets: a loose sanity bound, the tight one is above)


# ---- 4. the module path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduction', ['mean', 'mean_of_mean'])
@pytest.mark.parametrize('Nn', [9, 65])
def test_triplet_loss_with_labels(reduction, Nn):
    """value and scores.grad against torch's cross-entropy (fp64, ignore_index=-1) on the same scores, tensor and MaskedTensor;
    the bounds of test_triplet_loss_module (tests/test_gpu_score_loss.py): 2e-6 on the value, 5e-6 on the gradient"""
    crit = triplet_loss(reduction)
    Bn = 7
    g = torch.Generator().manual_seed(Nn)
    rng = np.random.default_rng(Nn)
    tce = torch.nn.CrossEntropyLoss(reduction='sum', ignore_index=-1)
    for ragged in (False, True):
        nv = torch.randint(1, Nn + 1, (Bn,), generator=g, dtype=torch.int32) if ragged else torch.full((Bn,), Nn, dtype=torch.int32)
        nv[0] = Nn
        lab = R.label_cases(Bn, Nn, nv.numpy(), rng)['holes']
        ok = R.has_target(lab, nv.numpy())
        corner = (torch.arange(Nn)[None, :] < nv.long()[:, None])
        corner = corner[:, :, None] & corner[:, None, :]
        s = (torch.randn(Bn, Nn, Nn, generator=g) * 2).masked_fill(~corner, 0)
        sd = s.to(DEV).requires_grad_(True)
        labd = torch.from_numpy(lab).to(DEV)
        out = crit(MaskedTensor(sd, nv.to(DEV), (1, 2)) if ragged else sd, labels=labd)
        out.backward()
        s64 = s.double().requires_grad_(True)
        ce = torch.stack([tce(s64[b, :n, :n], torch.from_numpy(np.where(ok[b, :n], lab[b, :n], -1).astype(np.int64)))
                          for b, n in enumerate(nv.tolist())])
        n = nv.double()
        ref = ce.sum() / n.sum() if reduction == 'mean' else (ce / n).mean()
        ref.backward()
        assert rel(out.detach().cpu(), ref.detach()) < 2e-6, ragged
        assert rel(sd.grad.cpu(), s64.grad) < 5e-6, ragged
        assert torch.equal(sd.grad.cpu()[~corner], torch.zeros(int((~corner).sum())))
        # a list of per-graph arrays is the same argument
        out2 = crit(MaskedTensor(sd, nv.to(DEV), (1, 2)) if ragged else sd, labels=[lab[b, :n] for b, n in enumerate(nv.tolist())])
        assert torch.equal(out2.detach(), out.detach())


def _ne(ragged=False):
    ne = dict(type='node_embedding', block_init='block_emb', block_inside='block', num_blocks=2, in_features=32, out_features=32,
              depth_of_mlp=3)
    if ragged:
        ne['constant_n_vertices'] = False
    return ne


@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_fused_step_with_labels_is_the_module_path_with_labels(precision, ragged):
    """fused_step(labels=) against the module's eager forward, loss(labels=) and backward: the same function through two launch
    sequences.  Bounds of the label-less comparison of the two (tests/test_gpu_module_surface.py: 2e-5 fp32, 5e-2 bf16, on scores
    and loss); the flat gradient in the max norm to 1e-4 (the gradient bound of smoke()) resp. 5e-2."""
    torch.manual_seed(11)
    model = Siamese_Node_Exp(2, _ne(ragged), precision=precision).to(DEV)
    # (with the reference's zero conv biases many pre-activations are exactly 0 and a ReLU mask is anybody's choice: the two launch
    # sequences -- the ragged fused step pads to a multiple of 8 -- then differentiate different masks; as tests/test_gpu_module_surface.py)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith('.bias'):
                p.add_((torch.rand(p.shape, generator=g) * 0.2 - 0.1).to(p.device).view(p.shape))
    x1, x2, nv, sizes, _, _ = _batch(ragged)
    lab = _labels(sizes, 'perm')
    x2p = planted.relabel(x2, lab, nvalid=nv)
    if ragged:
        a1, a2 = MaskedTensor(x1, nv, (2, 3), 'N'), MaskedTensor(x2p, nv, (2, 3), 'M')
    else:
        a1, a2 = x1, x2p
    scores = model(a1, a2)
    loss = model.loss(scores, labels=lab)
    loss.backward()
    g_ref = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).clone()
    s_ref = (scores.tensor if ragged else scores).detach().rename(None)
    tol, gtol = (5e-2, 5e-2) if precision == 'bf16' else (2e-5, 1e-4)
    for cap in (False, True, True):
        for p in model.parameters():
            p.grad = None
        lf, sf, (acc, tot) = model.fused_step(a1, a2, capture=cap, metric=True, labels=lab)
        sf = (sf.tensor if ragged else sf).rename(None)
        flat = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
        assert abs(lf.item() - loss.item()) < tol * abs(loss.item()), cap
        print('%s ragged=%s capture=%s: scores %.3g loss %.3g gradient %.3g' % (precision, ragged, cap, rel(sf[:, :s_ref.shape[1], :s_ref.shape[2]], s_ref),
                                                                               abs(lf.item() - loss.item()) / abs(loss.item()), rel(flat, g_ref)))
        assert rel(sf[:, :s_ref.shape[1], :s_ref.shape[2]], s_ref) < tol and rel(flat, g_ref) < gtol, (cap, rel(flat, g_ref))
        assert int(tot) == sum(sizes) and 0 <= int(acc) <= int(tot)
    # the step methods take the labels as an optional third batch element
    assert abs(model.training_step((a1, a2, lab), 0).item() - loss.item()) < tol * abs(loss.item())
    assert model.training_step((a1, a2), 0).item() != model.training_step((a1, a2, lab), 0).item()
    model.validation_step((a1, a2, lab), 0)
