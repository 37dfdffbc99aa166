"""CPU: oracle/fgnn_oracle_pinned.py (the op sequence of the reference with the ReLU / arg-max decisions as INPUTS) against the
committed vectors of tests/golden/pinned_decisions.npz and pinned_pin_er_n19_b2_3blk.npz -- the reference's own fp32 and fp64 runs
with the decisions its forward hooks saw (make_golden.py round5 / pins, where the comparison with the reference is torch.equal)."""
import numpy as np
import pytest
import torch

from oracle import fgnn_oracle as O
from oracle import fgnn_oracle_pinned as OP
from util import load_golden, rel, sub


def _case():
    d = load_golden('pinned_decisions.npz')
    return d, sub(d, 'sd/'), d['x1'], d['x2']


@pytest.mark.parametrize('tag,dtype,tol', [('f32', torch.float32, 1e-6), ('f64', torch.float64, 1e-13)])
def test_pinned_oracle_reproduces_the_reference_on_its_own_decisions(tag, dtype, tol):
    d, sd, x1, x2 = _case()
    masks, idx = OP.unpack_decisions({k: v.numpy() for k, v in d.items()}, prefix=tag + '/')
    s, l, g = OP.step_fwd_bwd_pinned(x1, x2, sd, masks, idx, dtype=dtype)
    assert rel(s, d[tag + '/scores']) <= tol and abs(l.item() - d[tag + '/loss'].item()) <= tol * abs(l.item())
    for k, v in sub(d, tag + '/grad/').items():
        assert rel(g[k], v) <= tol, (k, rel(g[k], v))
    # the decisions ARE those of the plain oracle in that precision (it is torch.equal to the reference, test_oracle_pinned.py)
    m2, i2 = OP.collect_decisions(torch.cat([x1, x2]).to(dtype), {k: v.to(dtype) for k, v in sd.items()})
    assert torch.equal(i2, idx) and all(torch.equal(m2[k], masks[k]) for k in masks)
    s0, l0, g0 = O.step_fwd_bwd(x1.to(dtype), x2.to(dtype), {k: v.to(dtype) for k, v in sd.items()})
    for k in g0:
        assert rel(g[k], g0[k]) <= tol


def test_fp64_arithmetic_on_the_fp32_branch():
    """What the GPU test computes: fp64 arithmetic, decisions of an fp32 evaluation.  On this fixture the fp32 and the fp64 run of
    the reference take the same decisions, so the cross evaluation equals the plain fp64 gradient; flipping ONE decision on a
    pixel that carries gradient moves the result by far more than rounding -- the pinned function follows its inputs."""
    d, sd, x1, x2 = _case()
    raw = {k: v.numpy() for k, v in d.items()}
    m32, i32 = OP.unpack_decisions(raw, prefix='f32/')
    s, l, g = OP.step_fwd_bwd_pinned(x1, x2, sd, m32, i32, dtype=torch.float64)
    for k, v in sub(d, 'x64on32/grad/').items():
        assert rel(g[k], v) <= 1e-13
        assert rel(g[k], d['f64/grad/' + k]) <= 1e-13
    # flip the decision of the largest hidden pre-activation... any live pixel: take one that is ON in the last block's mlp3
    key = (2, 3, 1)
    flipped = {k: v.clone() for k, v in m32.items()}
    on = flipped[key].nonzero()[0]
    flipped[key][tuple(on)] = False
    _, _, g2 = OP.step_fwd_bwd_pinned(x1, x2, sd, flipped, i32, dtype=torch.float64)
    moved = max(rel(g2[k], g[k]) for k in g if not k.endswith('convs.2.bias'))
    assert moved > 1e-7, moved
    # ... and another arg-max row moves it too
    i_f = i32.clone()
    i_f[0, 0, 0] = (i_f[0, 0, 0] + 1) % x1.shape[-1]
    _, _, g3 = OP.step_fwd_bwd_pinned(x1, x2, sd, m32, i_f, dtype=torch.float64)
    assert max(rel(g3[k], g[k]) for k in g if not k.endswith('convs.2.bias')) > 1e-7


def test_ragged_pinned_step_equals_the_per_graph_oracle():
    """step_fwd_bwd_pinned_ragged on a padded batch with the decisions of per-graph dense runs == oracle.step_fwd_bwd_ragged."""
    torch.manual_seed(3)
    sd = O.init_state_dict(num_blocks=2)
    g = torch.Generator().manual_seed(4)
    sd = {k: (v + 0.1 * torch.randn(v.shape, generator=g) if k.endswith('.bias') and v.dim() == 1 else v) for k, v in sd.items()}
    from graph_neural_net_amd import synthetic
    xs, ys = synthetic.make_ragged_batch(31, 3, 5, 11)
    sizes = [int(t.shape[-1]) for t in xs]
    nmax = max(sizes)
    pad = lambda lst: torch.stack([torch.nn.functional.pad(t, (0, nmax - t.shape[-1], 0, nmax - t.shape[-1])) for t in lst])
    x1, x2 = pad(xs), pad(ys)
    B = len(sizes)
    masks = {}
    idx = torch.zeros(2 * B, 32, nmax, dtype=torch.int64)
    for b, (a, c) in enumerate(zip(xs, ys)):
        for gi, t in ((b, a), (B + b, c)):
            m, i = OP.collect_decisions(t.unsqueeze(0), sd)
            n = sizes[b]
            for k, v in m.items():
                masks.setdefault(k, torch.zeros(2 * B, 32, nmax, nmax, dtype=torch.bool))[gi, :, :n, :n] = v[0]
            idx[gi, :, :n] = i[0]
    s, l, gr = OP.step_fwd_bwd_pinned_ragged(x1, x2, sizes, sd, masks, idx, dtype=torch.float32)
    s0, l0, g0 = O.step_fwd_bwd_ragged(xs, ys, sd)
    assert abs(l.item() - l0.item()) <= 1e-6 * abs(l0.item())
    for a, b in zip(s, s0):
        assert rel(a, b) <= 1e-6
    for k in g0:
        assert rel(gr[k], g0[k]) <= 1e-5, (k, rel(gr[k], g0[k]))


def test_pinned_oracle_bit_equal_to_reference_live():
    """A second case, on the reference's own results that `make_golden.py pins` stored after checking the same equalities against
    the imported reference (tests/golden/pinned_pin_er_n19_b2_3blk.npz: 3 blocks, 2 pairs, N = 19, fp32 and fp64): fed the
    reference's decisions the pinned oracle is torch.equal to it -- scores, loss, every gradient -- and the plain oracle's decision
    collector sees exactly those decisions."""
    d = load_golden('pinned_pin_er_n19_b2_3blk.npz')
    sd, x1, x2 = sub(d, 'sd/'), d['x1'], d['x2']
    threads = torch.get_num_threads()
    torch.set_num_threads(1)            # ATen's CPU gradients depend on the thread count: the fixture was made with one thread
    try:
        for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
            sdt = {k: v.to(dt) for k, v in sd.items()}
            masks, idx = OP.unpack_decisions({k: v.numpy() for k, v in d.items()}, prefix=tag + '/')
            s, l, g = OP.step_fwd_bwd_pinned(x1, x2, sdt, masks, idx, dtype=dt)
            assert torch.equal(s, d[tag + '/scores']), tag + ': pinned scores differ'
            assert torch.equal(l, d[tag + '/loss']), tag + ': pinned loss differs'
            ref = sub(d, tag + '/grad/')
            assert sorted(g) == sorted(ref)
            for k, v in ref.items():
                assert torch.equal(g[k], v), tag + ': pinned gradient %s differs' % k
            m2, i2 = OP.collect_decisions(torch.cat([x1, x2]).to(dt), sdt)
            assert torch.equal(i2, idx) and all(torch.equal(m2[k], masks[k]) for k in masks), tag + ': collect_decisions differs'
    finally:
        torch.set_num_threads(threads)


def _perturbed_model(num_blocks, depth, seed):
    torch.manual_seed(seed)
    sd = O.init_state_dict(num_blocks=num_blocks, depth_of_mlp=depth)
    g = torch.Generator().manual_seed(seed + 1)
    return {k: (v + 0.1 * torch.randn(v.shape, generator=g) if (k.endswith('bias') or k.endswith('gn.weight')) else v)
            for k, v in sd.items()}


# the configurations tests/test_gpu_pinned_shapes.py relies on that the committed fixtures (4 and 3 blocks, depth 3, N >= 19) do not cover
PLAIN_CASES = [(nb, depth, N) for nb, depth, N in ((2, 1, 17), (2, 2, 17), (1, 3, 33), (3, 3, 9), (2, 3, 1), (2, 3, 2), (2, 3, 65),
                                                   (1, 1, 2), (3, 2, 65))]


@pytest.mark.parametrize('tag,dtype,tol', [('f32', torch.float32, 1e-6), ('f64', torch.float64, 1e-13)])
@pytest.mark.parametrize('nb,depth,N', PLAIN_CASES, ids=['%dblk-depth%d-N%d' % c for c in PLAIN_CASES])
def test_pinned_oracle_on_the_plain_oracles_decisions(nb, depth, N, tag, dtype, tol):
    """Fed the plain oracle's own decisions (collect_decisions), the pinned oracle IS the plain oracle -- at depth 1 and 2 (no / one
    hidden ReLU per MLP), with 1 and 3 blocks, at N = 1, 2 (zero variance, gradients zero by symmetry) and 65, in both precisions."""
    from graph_neural_net_amd import synthetic
    sd = {k: v.to(dtype) for k, v in _perturbed_model(nb, depth, 10 * nb + depth).items()}
    x1, x2 = synthetic.make_batch(300 + N, 2, N, 'ErdosRenyi', 0.3, 0.1)
    x1, x2 = x1.to(dtype), x2.to(dtype)
    masks, idx = OP.collect_decisions(torch.cat([x1, x2]), sd)
    assert len(masks) == nb * 3 * (depth - 1)
    s, l, g = OP.step_fwd_bwd_pinned(x1, x2, sd, masks, idx, dtype=dtype)
    s0, l0, g0 = O.step_fwd_bwd(x1, x2, sd)
    assert rel(s, s0) <= tol and abs(l.item() - l0.item()) <= tol * abs(l0.item()) + tol ** 2
    assert sorted(g) == sorted(g0)
    for k in g0:
        assert rel(g[k], g0[k]) <= tol, (k, rel(g[k], g0[k]))


@pytest.mark.parametrize('tag,dtype,tol', [('f32', torch.float32, 1e-6), ('f64', torch.float64, 1e-13)])
@pytest.mark.parametrize('depth', [1, 2, 3])
def test_ragged_pinned_oracle_with_single_vertex_graphs(depth, tag, dtype, tol):
    """The ragged form on a batch with n = 1, n = Nmax and a size-0 filler pair (skipped: no scores, nothing in the loss), fed the
    per-graph decisions of the plain oracle: equal to the plain oracle's ragged step on the live pairs."""
    from graph_neural_net_amd import synthetic
    sd = {k: v.to(dtype) for k, v in _perturbed_model(2, depth, 50 + depth).items()}
    rng = np.random.default_rng(depth)
    sizes = [1, 12, 0, 5, 1]
    xs, ys = [], []
    for n in sizes:
        a, b = synthetic.make_pair(rng, max(n, 1), 'ErdosRenyi', 0.4, 0.1)
        xs.append(torch.from_numpy(a).to(dtype)[:, :n, :n])
        ys.append(torch.from_numpy(b).to(dtype)[:, :n, :n])
    nmax, B = max(sizes), len(sizes)
    pad = lambda lst: torch.stack([torch.nn.functional.pad(t, (0, nmax - t.shape[-1], 0, nmax - t.shape[-1])) for t in lst])
    x1, x2 = pad(xs), pad(ys)
    masks = {}
    idx = torch.zeros(2 * B, 32, nmax, dtype=torch.int64)
    for b, (a, c) in enumerate(zip(xs, ys)):
        n = sizes[b]
        if n == 0:
            continue
        for gi, t in ((b, a), (B + b, c)):
            m, i = OP.collect_decisions(t.unsqueeze(0), sd)
            for k, v in m.items():
                masks.setdefault(k, torch.zeros(2 * B, 32, nmax, nmax, dtype=torch.bool))[gi, :, :n, :n] = v[0]
            idx[gi, :, :n] = i[0]
    s, l, g = OP.step_fwd_bwd_pinned_ragged(x1, x2, sizes, sd, masks, idx, dtype=dtype)
    live = [b for b, n in enumerate(sizes) if n]
    s0, l0, g0 = O.step_fwd_bwd_ragged([xs[b] for b in live], [ys[b] for b in live], sd)
    assert s[2].shape == (0, 0)
    assert abs(l.item() - l0.item()) <= tol * abs(l0.item())
    for a, b in zip([s[b] for b in live], s0):
        assert rel(a, b) <= tol
    for k in g0:
        assert rel(g[k], g0[k]) <= tol, (k, rel(g[k], g0[k]))
