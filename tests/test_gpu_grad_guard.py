"""GPU: the guarded optimizer step (csrc/grad_guard.hip, optim.FlatAdam(max_grad_norm, skip_nonfinite), FgnnTrainer) against the
numpy restatement tests/grad_guard_ref.py, against the unguarded step bit for bit, and under graph replay.

No non-finite value is ever fed to a model kernel here: gradients are poisoned only in buffers that the guard and the optimizer
read."""
import numpy as np
import pytest
import torch

import grad_guard_ref as R
from graph_neural_net_amd import checkpoint, optim
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.optim import FlatAdam, GradGuard
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.trainer import FgnnTrainer

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
LAY = ParamLayout(2, 2, 32, 32, 3)
SIZES = [1, 63, 64, 65, 255, 256, 257, 4097, LAY.total, 2 ** 20 + 3]
ADAM_PARITY = 1e-6


def _guard(g, scale=1.0, max_norm=None, skip=False, guard=None):
    guard = guard or GradGuard(DEV, max_norm, skip)
    guard.launch(g, torch.full((5,), float(scale), dtype=torch.float64, device=DEV))
    return guard


def _rand(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(n).astype(np.float32))


def _state(opt):
    return opt.params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_count()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


# ---------------------------------------------------------------------------------------------------------------- norm
@pytest.mark.parametrize('n', SIZES)
def test_norm_matches_restatement_to_one_ulp(n):
    """fp64 accumulation: n * 2^-53 relative, far below half an fp32 ulp, so after the cast to fp32 only a rounding-boundary case
    can differ from the restatement, and then by one ulp."""
    g = _rand(n, n)
    big = torch.full((n,), 1e30)
    for vec, scale in ((g, 1.0), (g, 1.0 / 96.0), (g, 1e-20), (big, 1.0)):
        d = vec.to(DEV)
        got = optim.grad_norm(d, scale)
        again = optim.grad_norm(d, scale)
        assert got.dtype == torch.float64 and got.dim() == 0 and torch.equal(got, again)
        ref, _, nonfinite = R.guard(vec.numpy(), scale)
        got32, ref32 = np.float32(got.item()), np.float32(ref)
        print('n %d scale %g: norm %.9g, restatement %.9g' % (n, scale, got.item(), ref))
        assert not nonfinite and np.isfinite(got32) and abs(got32 - ref32) <= np.spacing(ref32), (n, scale, got.item(), ref)
        gd = _guard(d, scale, max_norm=1e-3 * ref)
        assert torch.equal(gd.norm, got) and gd.flags.item() == 0 and gd.skipped.item() == 0
        assert abs(gd.coef.item() - 1e-3 * ref / (got.item() + 1e-6)) <= 1e-15 * gd.coef.item()
    assert torch.isinf(torch.tensor(1e30) * torch.tensor(1e30)).item()        # the squares of the last vector do overflow fp32


@pytest.mark.parametrize('n', [257, 4097, LAY.total, 2 ** 20 + 3])
def test_nonfinite_entries_raise_the_flag_and_finite_ones_clear_it(n):
    g = _rand(n, n + 1).to(DEV)
    gd = GradGuard(DEV, None, False)
    for idx in sorted({0, n - 1, 255, 256, n // 2 + 1}):
        for bad in (float('inf'), float('-inf'), float('nan')):
            keep = g[idx].clone()
            g[idx] = bad
            _guard(g, 1.0 / 96.0, guard=gd)
            assert gd.flags.item() == 1 and not torch.isfinite(gd.norm).item(), (n, idx, bad)
            g[idx] = keep
            _guard(g, 1.0 / 96.0, guard=gd)
            assert gd.flags.item() == 0 and torch.isfinite(gd.norm).item(), (n, idx, bad)
    assert gd.skipped.item() == 0               # not in skip mode: nothing is counted


# ------------------------------------------------------------------------------------------------------- optimizer
def _pair(max_grad_norm, skip_nonfinite, seed=3, scale=1.0 / 96.0):
    p0 = LAY.init_flat(seed, DEV)
    a = FlatAdam(p0.clone(), lr=2e-3, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
    b = FlatAdam(p0.clone(), lr=2e-3)
    a.sync_hyper_parameters(grad_scale=scale)
    b.sync_hyper_parameters(grad_scale=scale)
    return a, b


def test_guard_that_does_nothing_is_the_unguarded_step():
    a, b = _pair(1e9, True)
    for t in range(3):
        g = _rand(LAY.total, 10 + t).to(DEV)
        a.step_dev(g)
        b.step_dev(g)
        assert a.clip_coef.item() == 1.0 and a.grad_norm.item() < 1e9
    assert _same(_state(a), _state(b)) and a.step_count() == 3 and a.skipped_steps.item() == 0


def test_clipped_step_is_the_unguarded_step_with_the_scaled_gradient():
    scale = 1.0 / 96.0
    a, b = _pair(0.5, False, scale=scale)
    hp = b._dev_state()[0]
    for t in range(3):
        g = _rand(LAY.total, 20 + t).to(DEV)
        coef = _guard(g, scale, max_norm=0.5).coef
        assert coef.item() < 1.0
        a.step_dev(g)
        hp[4:5].fill_(scale).mul_(coef)           # grad_scale <- hp[4] * coef, formed in fp64 as the guarded kernel forms it
        b.step_dev(g)
        assert torch.equal(a.clip_coef, coef)
    assert _same(_state(a), _state(b))


@pytest.fixture(scope='module')
def clip_case():
    p0, grads = R.make_case(n=LAY.total)
    return p0, grads, R.torch_clip_adam(p0, grads, 1.0, 100.0, lr=1e-3)


def test_clipped_steps_match_torch_clip_and_adam(clip_case):
    p0, grads, ref = clip_case
    opt = FlatAdam(torch.from_numpy(p0).to(DEV), lr=1e-3, max_grad_norm=100.0)
    opt.sync_hyper_parameters(grad_scale=1.0)
    mine = R.GuardedAdam(p0, lr=1e-3, max_grad_norm=100.0)
    coefs = []
    for t, g in enumerate(grads):
        opt.step_dev(torch.from_numpy(g).to(DEV))
        mine.step(g)
        coefs.append(opt.clip_coef.item())
        errs = (R.rel(opt.params.cpu().numpy(), ref[t]['p']), R.rel(opt.exp_avg.cpu().numpy(), ref[t]['m']),
                R.rel(opt.exp_avg_sq.cpu().numpy(), ref[t]['v']))
        print('step %d: coef %.6g; against torch: p %.2e m %.2e v %.2e; against the restatement: p %.2e'
              % ((t, coefs[-1]) + errs + (R.rel(opt.params.cpu().numpy(), mine.p),)))
        assert max(errs) < ADAM_PARITY, (t, errs)
        assert R.rel(opt.params.cpu().numpy(), mine.p) < ADAM_PARITY and abs(coefs[-1] - mine.coef) <= 1e-12 * mine.coef
    assert coefs[0] == coefs[1] == 1.0 and all(c < 1.0 for c in coefs[2:]), coefs


def _nan_at(g, idx=1234):
    bad = g.clone()
    bad[idx] = float('nan')
    return bad


def test_nonfinite_step_is_skipped_and_does_not_count():
    a, b = _pair(5.0, True)
    g0, g1 = _rand(LAY.total, 30).to(DEV), _rand(LAY.total, 31).to(DEV)
    a.step_dev(g0)
    before = _state(a)
    a.step_dev(_nan_at(g1))
    assert _same(_state(a), before) and before[3] == 1 and a.skipped_steps.item() == 1
    assert not torch.isfinite(a.grad_norm).item()
    # a fresh unguarded optimizer started from the saved state takes the same next step (its gradient scaled by the clip coefficient)
    b.params.copy_(before[0]); b.exp_avg.copy_(before[1]); b.exp_avg_sq.copy_(before[2])
    b.t = before[3]
    hp, state = b._dev_state()
    state[0:1].fill_(before[3])
    a.step_dev(g1)
    hp[4:5].mul_(a.clip_coef)
    b.step_dev(g1)
    assert _same(_state(a), _state(b)) and a.step_count() == 2 and a.skipped_steps.item() == 1 and a.t == 3


def test_without_skip_a_nonfinite_gradient_propagates_as_in_torch():
    a, _ = _pair(5.0, False)
    a.step_dev(_nan_at(_rand(LAY.total, 32).to(DEV)))
    # clip_grad_norm_(error_if_nonfinite=False): the norm is NaN, the coefficient is NaN, every gradient entry becomes NaN
    assert torch.isnan(a.clip_coef).item() and torch.isnan(a.params).all().item() and a.step_count() == 1
    assert a.skipped_steps.item() == 0
    # with both options off there is no guard to read
    c = FlatAdam(LAY.init_flat(3, DEV), lr=2e-3, skip_nonfinite=False, max_grad_norm=None)
    with pytest.raises(RuntimeError, match='not guarded'):
        c.grad_norm


def test_replayed_guarded_step_equals_the_eager_sequence():
    """one captured step_dev replayed over finite, NaN, finite, finite: both arrival counters must have been reset by every launch,
    skipped or not"""
    gs = [_rand(LAY.total, 40 + t).to(DEV) for t in range(4)]
    gs[1] = _nan_at(gs[1])
    eager, _ = _pair(2.0, True)
    for g in gs:
        eager.step_dev(g)
    rep, _ = _pair(2.0, True)
    buf = torch.zeros_like(gs[0])
    rep._dev_state()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rep.step_dev(buf)
    for g in gs:
        buf.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    assert _same(_state(rep), _state(eager)) and rep.step_count() == 3
    assert rep.skipped_steps.item() == eager.skipped_steps.item() == 1
    assert torch.equal(rep.grad_norm, eager.grad_norm) and torch.equal(rep.clip_coef, eager.clip_coef)


# ---------------------------------------------------------------------------------------------------------- trainer
B, N = 4, 24


def _gen():
    return PairGenerator(N, 'Regular', 'ErdosRenyi', edge_density=0.25, noise=0.05, seed=4, device=DEV)


@pytest.fixture(scope='module')
def plain_params():
    """three plain train_step_bits steps, eager and captured"""
    out = {}
    gen = _gen()
    for capture in (False, True):
        tr = FgnnTrainer(LAY, LAY.init_flat(5, DEV), lr=2e-3, capture=capture)
        for s in range(3):
            tr.train_step_bits(*gen.bits(B * s, B)[:2])
        out[capture] = tr.params.clone()
    return out


@pytest.mark.parametrize('capture', [False, True])
def test_trainer_with_an_idle_guard_equals_the_plain_trainer(capture, plain_params):
    gen = _gen()
    tr = FgnnTrainer(LAY, LAY.init_flat(5, DEV), lr=2e-3, capture=capture, max_grad_norm=1e30, skip_nonfinite=True)
    for s in range(3):
        tr.train_step_bits(*gen.bits(B * s, B)[:2])
    assert torch.equal(tr.params, plain_params[capture]) and tr.skipped_steps.item() == 0
    assert tr.opt.step_count() == 3 and torch.isfinite(tr.grad_norm).item()


@pytest.mark.parametrize('capture', [False, True])
def test_trainer_clips_like_a_hand_applied_guarded_adam(capture):
    gen = _gen()
    p0 = LAY.init_flat(5, DEV)
    tr = FgnnTrainer(LAY, p0.clone(), lr=2e-3, capture=capture, max_grad_norm=1e-3)
    hand = FlatAdam(p0.clone(), lr=2e-3, max_grad_norm=1e-3)
    hand.sync_hyper_parameters(grad_scale=1.0 / (B * N))
    for s in range(3):
        tr.train_step_bits(*gen.bits(B * s, B)[:2])
        assert torch.equal(tr.grad_norm, optim.grad_norm(tr.grads, 1.0 / (B * N)))
        assert tr.opt.clip_coef.item() < 1.0
        hand.step_dev(tr.grads)             # the same gradients: the two parameter vectors are equal before every step
        assert torch.equal(tr.params, hand.params), s
    assert _same(_state(tr.opt), _state(hand))


def test_trainer_skips_a_poisoned_gradient():
    """the gradient buffer is poisoned between the model work and the update: no model kernel sees the NaN"""
    gen = _gen()
    d1, d2 = gen.dense(0, B)
    xs, ys = list(d1['input']), list(d2['input'])
    tr = FgnnTrainer(LAY, LAY.init_flat(5, DEV), lr=2e-3, max_grad_norm=1.0, skip_nonfinite=True)

    def step(poison):
        loss, _ = tr.model_step_ragged(xs, ys, None, total_nodes=1.0)
        tr._loss_sum.copy_(loss.reshape(1))
        tr._nodes.fill_(float(B * N))
        if poison:
            tr.grads[77] = float('nan')
        tr._reduce_and_update()
    step(False)
    before = _state(tr.opt)
    step(True)
    assert _same(_state(tr.opt), before) and tr.skipped_steps.item() == 1 and before[3] == 1
    step(False)
    assert tr.opt.step_count() == 2 and tr.skipped_steps.item() == 1 and torch.isfinite(tr.params).all().item()
    assert not torch.equal(tr.params, before[0])


def test_checkpoint_keeps_the_device_step_count(tmp_path):
    gen = _gen()
    tr = FgnnTrainer(LAY, LAY.init_flat(5, DEV), lr=2e-3, max_grad_norm=1.0, skip_nonfinite=True)
    tr.train_step_bits(*gen.bits(0, B)[:2])
    tr.opt.step_dev(_nan_at(tr.grads.clone()))          # a skipped step: issued (t = 2), not counted on the device
    tr.train_step_bits(*gen.bits(B, B)[:2])
    assert tr.opt.t == 3 and tr.opt.step_count() == 2 and tr.skipped_steps.item() == 1
    f = str(tmp_path / 'guarded.ckpt')
    tr.save_checkpoint(f, global_step=3)
    obj = torch.load(f, weights_only=True)
    assert obj['fgnn_adam']['step'] == 2 and set(obj['fgnn_adam']) == {'exp_avg', 'exp_avg_sq', 'step', 'lr'}
    layout, flat = checkpoint.load_checkpoint(obj, DEV)
    back = FgnnTrainer(layout, flat, lr=1.0, max_grad_norm=1.0, skip_nonfinite=True)
    assert checkpoint.restore_optimizer(obj, back.opt)
    assert back.opt.step_count() == 2 and back.opt.t == 2
    # and the resumed run takes the step the original takes
    tr.train_step_bits(*gen.bits(2 * B, B)[:2])
    back.train_step_bits(*gen.bits(2 * B, B)[:2])
    assert torch.equal(back.params, tr.params) and back.opt.step_count() == tr.opt.step_count() == 3
    # an unguarded optimizer's file is what it was: the host count
    plain = FgnnTrainer(LAY, LAY.init_flat(5, DEV), lr=2e-3)
    plain.train_step_bits(*gen.bits(0, B)[:2])
    assert plain.save_checkpoint(str(tmp_path / 'plain.ckpt'))['fgnn_adam']['step'] == plain.opt.t == 1
