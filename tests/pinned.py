"""Decision-pinned runs of the fused engines: a plain helper module of the GPU tests (not a conftest).

run_pinned() runs one training step of FgnnEngine or FgnnEngineBF16 twice -- the product step, then the same step with the decision
export on, which must not change a bit of scores, loss or gradients -- and returns the engine's results with the ReLU masks and arg-max
indices it took.  pinned_oracle() evaluates the reference's op sequence on exactly that branch (oracle/fgnn_oracle_pinned.py;
oracle/fgnn_oracle_bf16.py with decisions= for the 16-bit engine) in a given precision and on a given device.  yardstick_errors()
compares the engine and an fp32 CPU evaluation of the same branch with the fp64 one, tensor by tensor.

Used by tests/test_gpu_grad_pinned.py (the benchmarked batches, against recorded reference errors) and tests/test_gpu_pinned_shapes.py
(the shape edges of every kernel form, against the fp32 CPU evaluation computed at test time).
"""
import numpy as np
import torch

from graph_neural_net_amd import synthetic
from graph_neural_net_amd.engine import FgnnEngine, ParamLayout
from oracle import fgnn_oracle as O
from oracle import fgnn_oracle_pinned as OP
from util import is_zero_grad

DEV = 'cuda:0'
SYM_ZERO = 1e-6          # a gradient tensor whose fp64 value stays below this is zero by symmetry (n <= 2): compared absolutely


def bits_of(x, device=DEV):
    """(G, 2, N, N) dense pairs -> (G, N, ceil(N/32)) int32 words of their bit-packed adjacency on the device."""
    return torch.from_numpy(synthetic.pack_adjacency(x[:, 0].numpy()).view(np.int32)).to(device)


def pad_pairs(xs, ys, nmax=None):
    """Lists of (2, n, n) graphs -> two zero-padded (B, 2, Nmax, Nmax) tensors and the sizes.  A None entry is a size-0 filler pair."""
    sizes = [0 if t is None else int(t.shape[-1]) for t in xs]
    N = max(sizes) if nmax is None else nmax
    pad = lambda t: torch.zeros(2, N, N) if t is None else torch.nn.functional.pad(t, (0, N - t.shape[-1], 0, N - t.shape[-1]))
    return torch.stack([pad(t) for t in xs]), torch.stack([pad(t) for t in ys]), sizes


class Run:
    """What run_pinned returns: the engine's scores (B, N, N), loss, gradients {name: tensor}, masks {(blk, mlp, layer): bool
    (G, 32, N, N)}, idx (G, 32, N) int64, and the entry points the product step called (in order)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def run_pinned(sd, x1, x2, sizes=None, num_blocks=None, depth=3, engine='f32', mfma='f32', block1='generic', bits=False,
               switches=None):
    """One step of the engine on the stacked batch cat(x1, x2) -- twice: the product step, then with the decision export on.
    engine: 'f32' (FgnnEngine) or 'bf16' (FgnnEngineBF16, constant-size batches and generic block 1);
    mfma, block1: FgnnEngine's arguments; bits: feed the bit-packed adjacency (embed(bits=...)) instead of the dense input;
    sizes: vertex counts of a ragged batch (x1, x2 zero-padded; 0 = filler pair); switches: {class attribute: value} of the engine
    class (T16, PAIR_BWD, ...) for this run only."""
    from graph_neural_net_amd import _lib
    B, N = x1.shape[0], x1.shape[-1]
    nb = O.num_blocks_of(sd) if num_blocks is None else num_blocks
    lay = ParamLayout(2, nb, 32, 32, depth)
    params = lay.flatten(sd, DEV)
    if engine == 'bf16':
        from graph_neural_net_amd.engine16 import FgnnEngineBF16
        cls = FgnnEngineBF16
        assert sizes is None and block1 == 'generic' and not bits, 'relu_decisions() of FgnnEngineBF16: constant size, generic block 1'
    else:
        cls = FgnnEngine
    saved = {k: cls.__dict__[k] for k in (switches or {}) if k in cls.__dict__}
    try:
        for k, v in (switches or {}).items():
            setattr(cls, k, v)
        if engine == 'bf16':
            eng = cls(lay, 2 * B, N, DEV, block1=block1)
        else:
            eng = cls(lay, 2 * B, N, DEV, ragged=sizes is not None, mfma=mfma, block1=block1)
        nv = torch.tensor(list(sizes) * 2, dtype=torch.int32, device=DEV) if sizes is not None else None
        x = torch.cat([x1, x2]).contiguous()
        kw = dict(bits=bits_of(x)) if bits else {}
        xin = None if bits else x.to(DEV)
        if nv is not None:
            kw['nvalid'] = nv
        # the product step (its entry points recorded), then the same step with the decision export on
        g0 = torch.zeros_like(params)
        prof = _lib.PROFILE
        _lib.PROFILE = []
        try:
            s0, l0 = eng.step(params, g0, xin, **kw)
            torch.cuda.synchronize()
            calls = [rec[3] for rec in _lib.PROFILE]
        finally:
            _lib.PROFILE = prof
        s0, l0 = s0.clone(), l0.clone()
        eng.export_decisions(True)
        grads = torch.zeros_like(params)
        scores, loss = eng.step(params, grads, xin, **kw)
        torch.cuda.synchronize()
    finally:
        for k in (switches or {}):
            if k in saved:
                setattr(cls, k, saved[k])
            else:
                delattr(cls, k)
    # the export does not change a bit of the step's results
    assert torch.equal(grads, g0) and torch.equal(scores, s0) and torch.equal(loss, l0), 'the decision export changed the results'
    masks = eng.relu_decisions()
    assert len(masks) == nb * 3 * (depth - 1)
    return Run(eng=eng, layout=lay, scores=scores.clone(), loss=loss.item(), grads=lay.unflatten(grads.clone()), masks=masks,
               idx=eng.idx.to(torch.int64), calls=calls, sizes=sizes, depth=depth, engine=engine)


def pinned_oracle(run, sd, x1, x2, dtype, device):
    """The reference's op sequence on the engine's branch, in `dtype` on `device`: (scores, loss, grads).  Ragged: scores is the list
    of the valid corners."""
    masks = {k: v.to(device) for k, v in run.masks.items()}
    idx = run.idx.to(device)
    if run.engine == 'bf16':
        from oracle import fgnn_oracle_bf16 as OB
        s, l, g = OB.step_fwd_bwd(x1, x2, sd, decisions=(masks, idx), dtype=dtype, device=device)
    elif run.sizes is None:
        s, l, g = OP.step_fwd_bwd_pinned(x1, x2, sd, masks, idx, dtype=dtype, device=device)
    else:
        s, l, g = OP.step_fwd_bwd_pinned_ragged(x1, x2, run.sizes, sd, masks, idx, dtype=dtype, device=device)
    cpu = lambda t: t.detach().double().cpu()
    s = [cpu(t) for t in s] if isinstance(s, list) else cpu(s)
    return s, l.item(), {k: cpu(v) for k, v in g.items()}


def _rel(a, b):
    s = b.abs().max().item() if b.numel() else 0.0
    d = (a - b).abs().max().item() if b.numel() else 0.0
    return d / s if s > 0 else d


def yardstick_errors(run, o64, o32):
    """Per gradient tensor, the engine's and the fp32 oracle's distance to the fp64 evaluation of the same branch.
    -> dict(live={name: (engine, fp32 oracle)} max-norm relative, sym={name: (engine, fp32 oracle)} absolute (zero by symmetry),
            zero={name: engine max |g|} (the analytically zero last-conv biases), scores=[(engine, fp32 oracle) per live pair],
            pad=[max |score| outside the valid corner of each pair], loss=(engine, fp32 oracle) relative)."""
    s64, l64, g64 = o64
    s32, l32, g32 = o32
    out = dict(live={}, sym={}, zero={}, scores=[], pad=[])
    for name, t in g64.items():
        a, b = run.grads[name].double().cpu().reshape(t.shape), g32[name].reshape(t.shape)
        if is_zero_grad(name, run.depth):
            out['zero'][name] = a.abs().max().item()
        elif t.abs().max().item() < SYM_ZERO:
            out['sym'][name] = ((a - t).abs().max().item(), (b - t).abs().max().item())
        else:
            out['live'][name] = (_rel(a, t), _rel(b, t))
    sc = run.scores.double().cpu()
    sizes = run.sizes if run.sizes is not None else [sc.shape[-1]] * sc.shape[0]
    for p, n in enumerate(sizes):
        ref64 = s64[p] if isinstance(s64, list) else s64[p]
        ref32 = s32[p] if isinstance(s32, list) else s32[p]
        if n:
            out['scores'].append((_rel(sc[p, :n, :n], ref64), _rel(ref32, ref64)))
        pad = sc[p].clone()
        pad[:n, :n] = 0
        out['pad'].append(pad.abs().max().item())
    den = abs(l64) if l64 != 0 else 1.0
    out['loss'] = (abs(run.loss - l64) / den, abs(l32 - l64) / den)
    return out


def argmax_gaps(run, sd, x1, x2, device=DEV):
    """The arg-max decisions themselves: for every valid (graph, channel, row), how far the value the engine's index picks lies below
    the row's maximum, both from an fp64 evaluation of the branch (the pooling's input, before the gather).  Relative to the largest
    |value| of that graph; a decision within rounding of a tie gives ~1e-7, a wrong column a gap of the order of the values.
    -> the largest gap over the batch."""
    depth = run.depth
    x = torch.cat([x1, x2])
    G = x.shape[0]
    sizes = run.sizes if run.sizes is not None else [x.shape[-1]] * (G // 2)
    params = {k: v.to(device=device, dtype=torch.float64) for k, v in O._strip(sd).items()}
    worst = 0.0
    for gi in range(G):
        n = sizes[gi % (G // 2)]
        if n == 0:
            continue
        h = x[gi:gi + 1, :, :n, :n].to(device=device, dtype=torch.float64)
        for blk in range(1, O.num_blocks_of(params) + 1):
            mk = lambda j: [run.masks[(blk, j, l)][gi:gi + 1, :, :n, :n].to(device) for l in range(depth - 1)]
            m1 = OP.mlp_block_real_pinned(h, *O.mlp_params(params, blk, 1), mk(1))
            m2 = OP.mlp_block_real_pinned(h, *O.mlp_params(params, blk, 2), mk(2))
            h = OP.mlp_block_real_pinned(torch.cat((torch.matmul(m1, m2), h), dim=1), *O.mlp_params(params, blk, 3), mk(3))
        picked = torch.gather(h, -1, run.idx[gi:gi + 1, :, :n].to(device).unsqueeze(-1)).squeeze(-1)
        gap = (h.max(-1)[0] - picked).max().item() / max(h.abs().max().item(), 1e-30)
        worst = max(worst, gap)
    return worst
