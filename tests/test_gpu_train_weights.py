"""GPU, end to end: per-pair loss weights in the fused step -- EngineBase.step(weights=), FgnnTrainer(
loss_reduction='mean_of_mean'), the train steps with weights= / live=, train_epoch(exact_last=True).

Shapes of tests/test_gpu_train_labels.py: 2 blocks, B = 4, N = 20 and a ragged batch with n in [9, 20]; fp32 and bf16, eager and
captured.  Bounds: those tests/test_gpu_train_labels.py holds the fused step to against the module path
(test_fused_step_with_labels_is_the_module_path_with_labels): scores and loss 2e-5 (fp32) / 5e-2 (bf16) relative, the flat gradient
1e-4 / 5e-2 in the max norm."""
import pytest
import torch

from graph_neural_net_amd.losses import triplet_loss
from graph_neural_net_amd.masked import MaskedTensor
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.sampler import EpochSampler
from graph_neural_net_amd.siamese import Siamese_Node_Exp
from graph_neural_net_amd.trainer import FgnnTrainer
from test_gpu_train_labels import B, DEV, LAY, N, _batch, _engine, _ne
from util import rel

pytestmark = pytest.mark.gpu
TOL = {'fp32': (2e-5, 1e-4), 'bf16': (5e-2, 5e-2)}        # (loss / scores, flat gradient)


def _gen(seed=11, vp=1.0):
    return PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.05, vertex_proba=vp, seed=seed, device=DEV)


# ---- 1. invariant 2 through the whole step -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_unit_weights_are_the_unweighted_step(precision, ragged):
    x1, x2, nv, sizes, _, _ = _batch(ragged)
    params = LAY.init_flat(3, DEV)
    eng = _engine(precision, ragged)
    nv2 = None if nv is None else torch.cat([nv, nv])
    x = torch.cat([x1, x2]).contiguous()

    def run(**kw):
        grads = torch.full_like(params, float('nan'))
        scores, loss = eng.step(params, grads, x, nvalid=nv2, total_nodes=1.0, **kw)
        torch.cuda.synchronize()
        return scores.clone(), loss.clone(), grads
    s0, l0, g0 = run()
    s1, l1, g1 = run(weights=torch.ones(B, device=DEV))
    assert torch.equal(s0, s1) and torch.equal(l0, l1) and torch.equal(g0, g1) and not torch.isnan(g0).any()
    s2, l2, g2 = run()                                          # ... and the engine goes back to the unweighted launches
    assert torch.equal(s0, s2) and torch.equal(l0, l2) and torch.equal(g0, g2)
    # the weights carry the reduction: a normaliser beside them is refused
    with pytest.raises(ValueError):
        eng.step(params, torch.empty_like(params), x, nvalid=nv2, total_nodes=5.0, weights=torch.ones(B, device=DEV))


# ---- 2. loss_reduction='mean_of_mean' against the module path -----------------------------------------------------------------------
@pytest.mark.parametrize('capture', [False, True])
@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_mean_of_mean_step_is_the_module_path(precision, ragged, capture):
    """FgnnTrainer.from_module on a module whose loss is triplet_loss('mean_of_mean'): loss and flat gradient of the fused step
    against the module's eager forward, loss and backward().  (A ragged step is eager whatever `capture` says.)
    This test fails without the feature: the trainer has no loss_reduction."""
    torch.manual_seed(11)
    model = Siamese_Node_Exp(2, _ne(ragged), precision=precision).to(DEV)
    model.loss = triplet_loss('mean_of_mean')
    g = torch.Generator().manual_seed(1)            # non-zero conv biases: no ReLU pre-activation sits exactly at 0 (test_gpu_train_labels.py)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith('.bias'):
                p.add_((torch.rand(p.shape, generator=g) * 0.2 - 0.1).to(p.device).view(p.shape))
    x1, x2, nv, sizes, _, _ = _batch(ragged)
    a1, a2 = (MaskedTensor(x1, nv, (2, 3), 'N'), MaskedTensor(x2, nv, (2, 3), 'M')) if ragged else (x1, x2)
    loss = model.loss(model(a1, a2))
    loss.backward()
    g_ref = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).clone()
    tr = FgnnTrainer.from_module(model, lr=1e-3, capture=capture)
    assert tr.loss_reduction == 'mean_of_mean'
    lf, sf = tr.train_step(x1, x2, nvalid=nv)
    torch.cuda.synchronize()
    D = tr._nodes.item()
    assert D == B                                                    # the number of non-empty pairs
    with torch.no_grad():
        l_mod = model.loss(MaskedTensor(sf.clone(), nv, (1, 2)) if ragged else sf.clone())
    tol, gtol = TOL[precision]
    flat = tr.grads / D
    print('%s ragged=%s capture=%s: loss %.8f (module on the step\'s scores %.8f, module path %.8f), gradient %.3g'
          % (precision, ragged, capture, lf.item(), l_mod.item(), loss.item(), rel(flat, g_ref)))
    assert abs(lf.item() - l_mod.item()) < tol * abs(l_mod.item())
    assert abs(lf.item() - loss.item()) < tol * abs(loss.item())
    assert rel(flat, g_ref) < gtol
    if ragged and precision == 'fp32':          # on ragged data 'mean' is another loss: the step above did not fall back to it
        with torch.no_grad():
            l_mean = triplet_loss('mean')(MaskedTensor(sf.clone(), nv, (1, 2)))
        assert abs(l_mean.item() - lf.item()) > 10 * tol * abs(lf.item())
    if capture and not ragged:
        assert set(tr._graphs) == {(B, N, 'weights')}


def test_trainer_refuses_an_unknown_reduction():
    with pytest.raises(ValueError):
        FgnnTrainer(LAY, LAY.init_flat(5, DEV), loss_reduction='median')


# ---- 3. live = 2 of 4 is the step over the first two pairs ----------------------------------------------------------------------------
@pytest.mark.parametrize('capture', [False, True])
@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_short_step_is_the_step_over_its_live_pairs(precision, ragged, capture):
    """Loss and gradient to the bounds above.  The Adam update: its state (the moments are m = 0.1 g and v = 0.001 g^2 after the first
    step) to the gradient's bound resp. twice that; the parameters to that bound on the entries whose gradient is safely away from
    zero (|g| >= 10 * bound * max |g|: the first update is lr * g / (|g| + 1e-8), a sign, which a gradient within the bound cannot
    flip there), and to 2 lr everywhere (the size of a flipped sign)."""
    gen = _gen(7, 0.8 if ragged else 1.0)
    b1, b2, nv = gen.bits(0, B)
    kw = dict(lr=1e-3, precision=precision, block1='structured', capture=capture)
    a = FgnnTrainer(LAY, LAY.init_flat(5, DEV), **kw)
    b = FgnnTrainer(LAY, LAY.init_flat(5, DEV), **kw)
    p0 = a.params.clone()
    la, sa = a.train_step_bits(b1, b2, nv, live=2)
    lb, sb = b.train_step_bits(b1[:2].contiguous(), b2[:2].contiguous(), None if nv is None else nv[:2].contiguous())
    torch.cuda.synchronize()
    want_D = 2.0 * N if nv is None else float(nv[:2].sum().item())
    assert a._nodes.item() == want_D == b._nodes.item()
    tol, gtol = TOL[precision]
    ga, gb = a.grads / want_D, b.grads / want_D
    print('%s ragged=%s capture=%s: loss %.8f / %.8f, gradient %.3g, parameters %.3g' % (precision, ragged, capture, la.item(), lb.item(),
                                                                                         rel(ga, gb), rel(a.params, b.params)))
    assert abs(la.item() - lb.item()) < tol * abs(lb.item())
    assert rel(sa[:2], sb) < tol
    assert rel(ga, gb) < gtol
    assert a.opt.t == b.opt.t == 1
    assert rel(a.opt.exp_avg, b.opt.exp_avg) < gtol and rel(a.opt.exp_avg_sq, b.opt.exp_avg_sq) < 2 * gtol + gtol ** 2
    safe = gb.abs() >= 10 * gtol * gb.abs().max()
    assert bool(safe.any()) and rel((a.params - p0)[safe], (b.params - p0)[safe]) < gtol
    assert float((a.params - b.params).abs().max()) <= 2 * 1e-3 * (1 + 1e-6)


@pytest.mark.parametrize('reduction', ['mean', 'mean_of_mean'])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_one_captured_graph_serves_every_live_count(precision, reduction):
    """live = 4, 2, 4 (and a step with user weights): one replayed graph against the eager weighted step, bit for bit"""
    gen = _gen(9)
    kw = dict(lr=2e-3, precision=precision, block1='structured', loss_reduction=reduction)
    a = FgnnTrainer(LAY, LAY.init_flat(5, DEV), capture=True, **kw)
    b = FgnnTrainer(LAY, LAY.init_flat(5, DEV), capture=False, **kw)
    user = torch.tensor([0.5, 2.0, 0.0, 1.0])
    for k, (live, u) in enumerate(((4, None), (2, None), (4, None), (torch.tensor([3], dtype=torch.int32, device=DEV), user))):
        b1, b2, _ = gen.bits(B * k, B)
        la, sa = a.train_step_bits(b1, b2, live=live, weights=u)
        lb, sb = b.train_step_bits(b1, b2, live=live, weights=u)
        assert torch.equal(la, lb) and torch.equal(sa, sb) and torch.equal(a.grads, b.grads) and torch.equal(a._nodes, b._nodes), k
        n_live = int(live) if not torch.is_tensor(live) else int(live.item())
        if u is None:
            assert a._nodes.item() == (n_live * N if reduction == 'mean' else n_live)
        else:
            assert a._nodes.item() == (2.5 * N if reduction == 'mean' else 2.5)
    assert torch.equal(a.params, b.params) and a.opt.t == b.opt.t == 4 and bool(torch.isfinite(a.params).all())
    assert set(a._graphs) == {(B, N, 'bits', 'weights')} and not b._graphs


# ---- 4. epochs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vp', [1.0, 0.8])
@pytest.mark.parametrize('capture', [False, True])
def test_exact_last_counts_every_example_once(vp, capture):
    """10 examples, B = 4: three steps with 4, 4 and 2 live pairs.  The per-step normalisers D (the device `_nodes` values) sum to the
    node count of the dataset; without exact_last the filled last step counts its two repeats as well."""
    gen, M = _gen(3, vp), 10
    sampler = EpochSampler(M, seed=2)
    nv_all = gen.bits(index=torch.arange(M, device=DEV))[2]
    total = M * N if nv_all is None else int(nv_all.sum().item())

    def epoch(**kw):
        tr = FgnnTrainer(LAY, LAY.init_flat(7, DEV), lr=1e-3, capture=capture)
        inner, seen = tr.train_step_bits, []

        def spy(*a, **k):
            out = inner(*a, **k)
            seen.append(tr._nodes.clone())
            return out
        tr.train_step_bits = spy
        losses = tr.train_epoch(gen, sampler, 0, B, **kw)
        torch.cuda.synchronize()
        return tr, losses, [float(d.item()) for d in seen]
    tr, losses, Ds = epoch(exact_last=True)
    assert losses.shape == (3,) and bool(torch.isfinite(losses).all()) and tr.opt.t == 3
    assert len(Ds) == 3 and sum(Ds) == total, (Ds, total)
    tr0, losses0, Ds0 = epoch()
    idx = sampler.batch_index(0, 2, B)
    last = B * N if nv_all is None else int(gen.bits(index=idx)[2].sum().item())
    assert Ds0[:2] == Ds[:2] and Ds0[2] == last and sum(Ds0) > total
    # exact_last=False is the behaviour before the argument existed: the same calls without the new arguments, bit for bit
    ref = FgnnTrainer(LAY, LAY.init_flat(7, DEV), lr=1e-3, capture=capture)
    want = torch.stack([ref.train_step_bits(*gen.bits(index=sampler.batch_index(0, s, B)))[0] for s in range(3)])
    assert torch.equal(losses0, want) and torch.equal(tr0.params, ref.params)
    assert torch.equal(losses[:2], losses0[:2])        # (full steps: w = 1 has the bits of the unweighted step)
    assert not any('weights' in k for k in tr0._graphs)


# ---- 5. the weighted step leaves nothing behind -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('capture', [False, True])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_weighted_step_leaks_no_state_into_the_unweighted_path(precision, capture):
    """a: unweighted, weighted with w = 1 (live = B, weights = ones), unweighted; b: three unweighted steps.  Bit for bit on every
    step -- the weighted step is the unweighted one under unit weights (invariant 2, through the flat gradient and the update), and the
    unweighted steps around it are those of a trainer that never ran a weighted step."""
    gen = _gen(13)
    kw = dict(lr=2e-3, precision=precision, block1='structured', capture=capture)
    a = FgnnTrainer(LAY, LAY.init_flat(5, DEV), **kw)
    b = FgnnTrainer(LAY, LAY.init_flat(5, DEV), **kw)
    for k in range(3):
        b1, b2, _ = gen.bits(B * k, B)
        la, sa = a.train_step_bits(b1, b2, **({'live': B, 'weights': torch.ones(B)} if k == 1 else {}))
        lb, sb = b.train_step_bits(b1, b2)
        assert torch.equal(la, lb) and torch.equal(sa, sb) and torch.equal(a.grads, b.grads) and torch.equal(a._nodes, b._nodes), k
        assert torch.equal(a.params, b.params), k
    if capture:
        assert set(a._graphs) == {(B, N, 'bits'), (B, N, 'bits', 'weights')} and set(b._graphs) == {(B, N, 'bits')}


def test_train_step_ragged_with_mean_of_mean():
    """the list API builds its weights on the host: against the padded ragged step (device weights) on the same pairs.  (Several
    buckets of other padded sizes: the loose sanity bound of test_train_step_ragged_takes_per_graph_labels, four times the loss bound.)"""
    x1, x2, nv, sizes, l1, l2 = _batch(True)
    xs, ys = [t.to(DEV) for t in l1], [t.to(DEV) for t in l2]
    a = FgnnTrainer(LAY, LAY.init_flat(5, DEV), loss_reduction='mean_of_mean')
    b = FgnnTrainer(LAY, LAY.init_flat(5, DEV), loss_reduction='mean_of_mean')
    la, _ = a.train_step_ragged(xs, ys, granule=8, live=3)
    lb, _ = b.train_step(x1, x2, nvalid=nv, live=3)
    assert a._nodes.item() == b._nodes.item() == 3
    tol, _ = TOL['fp32']
    print('ragged list step %.8f, padded step %.8f, gradient %.3g' % (la.item(), lb.item(), rel(a.grads, b.grads)))
    assert abs(la.item() - lb.item()) < 4 * tol * abs(lb.item()) and bool(torch.isfinite(a.params).all())
