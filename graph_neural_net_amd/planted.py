"""Planted permutations: relabel the second graph of a pair and keep the ground truth (``csrc/planted.hip``).

``labels`` is a (B, N) int32 tensor with ``labels[b, i] = pi_b(i)``: vertex i of graph 1 is vertex pi_b(i) of graph 2; entries
``i >= n_b`` are -1, like ``assign`` of the decoders.  It is what the reference's metrics call ``labels``
(toolbox/metrics.py:92-141) and what ``metrics.accuracy_max`` / ``accuracy_linear_assignment``, ``qap.all_acc_qap`` / ``greedy_qap``
and ``Siamese_Node_Exp.match`` take as ``labels=``.

* ``planted_permutation``: one uniform permutation per pair, counter-based like ``pairgen``: pair k's permutation depends on
  (seed, k) only -- Fisher-Yates from the top on the identity, ``j = (u32_k * (k + 1)) >> 32`` for k = n - 1 .. 1 with ``u32_k`` draw
  k of Philox stream 7 of the pair (``pairgen``'s docstring lists the streams);
* ``relabel``: ``out[pi(i)][pi(j)] = in[i][j]`` on bit words, on dense (B, C, n, n) or (B, n, n) fp32 tensors (tensor
  representations, spectral channels, weighted graphs), on ``{'input': ...}`` dicts and on MaskedTensors; pure data movement,
  bit-exact, exact zeros outside every n_b x n_b corner.  No symmetry is assumed;
* ``inverse``: the inverse permutation, ``relabel(relabel(x, pi), inverse(pi)) == x`` (plain torch: it also runs on the host).

There is no CPU path for the first two (``_lib``); nothing here synchronises.
"""
import torch

from . import _lib
from .masked import MaskedTensor

MAX_N = _lib.FGNN_PLANTED_MAX_N
STREAM = 7                    # include/fgnn_hip.h: FGNN_PLANTED_STREAM
SEEDS_STREAM = 8              # include/fgnn_hip.h: FGNN_SEEDS_STREAM (reveal_seeds)


def check_labels(labels, B, N, what='labels'):
    """labels must be a (B, >= N) integer tensor; returns it unchanged."""
    if not torch.is_tensor(labels) or labels.is_floating_point() or labels.dtype == torch.bool or labels.is_complex():
        raise ValueError('%s must be an integer tensor, got %s' % (what, labels.dtype if torch.is_tensor(labels) else type(labels).__name__))
    if labels.dim() != 2 or labels.shape[0] != B or labels.shape[1] < N:
        raise ValueError('%s must have shape (%d, >= %d), got %s' % (what, B, N, tuple(labels.shape)))
    return labels


def _nv32(nvalid, B, dev):
    if nvalid is None:
        return None
    if not torch.is_tensor(nvalid) or nvalid.dim() != 1 or nvalid.shape[0] != B or nvalid.is_floating_point():
        raise ValueError('nvalid must be (%d,) integers, got %s' % (B, tuple(nvalid.shape) if torch.is_tensor(nvalid) else type(nvalid).__name__))
    return nvalid.to(device=dev, dtype=torch.int32).contiguous()


def planted_permutation(seed, N, first=None, count=None, index=None, nvalid=None, device=None):
    """The planted permutations of pairs first .. first + count - 1, or of the pairs index[0], index[1], ... (a 1-D int64 tensor or
    a list, any order, duplicates allowed; a negative entry gives the empty permutation) of dataset `seed` -> (count, N) int32 device
    tensor.  nvalid: the (count,) vertex counts the generator wrote for the same pairs (None: every pair has N vertices); row b is a
    permutation of [0, n_b) followed by -1.  Enqueued on the current stream."""
    N, seed = int(N), int(seed)
    if not 1 <= N <= MAX_N:
        raise ValueError('N must be in [1, %d], got %d' % (MAX_N, N))
    if not 0 <= seed < 1 << 64:
        raise ValueError('seed must be in [0, 2^64), got %r' % (seed,))
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if dev.type != 'cuda':
        raise RuntimeError('planted_permutation: device %s; the permutation is drawn on the GPU only (there is no CPU path)' % (dev,))
    if index is None:
        if first is None or count is None:
            raise ValueError('give either (first, count) or index=')
        first, count = int(first), int(count)
        if first < 0 or count < 0:
            raise ValueError('first and count must be >= 0, got %d, %d' % (first, count))
    else:
        if first is not None or count is not None:
            raise ValueError('give either (first, count) or index=, not both')
        if not torch.is_tensor(index):
            index = torch.tensor(index, dtype=torch.int64)
        if index.dim() != 1 or index.dtype != torch.int64:
            raise ValueError('index must be a 1-D int64 tensor, got shape %s, %s' % (tuple(index.shape), index.dtype))
        index = index.to(dev).contiguous()
        first, count = 0, index.numel()
    nv = _nv32(nvalid, count, dev)
    with torch.cuda.device(dev):
        labels = torch.empty(count, N, dtype=torch.int32, device=dev)
        if count:
            _lib.call('fgnn_planted_perm', seed, first, _lib.ptr(index), _lib.ptr(nv), count, N, _lib.ptr(labels), _lib.stream_ptr())
    return labels


def reveal_seeds(labels, nvalid, count, seed, first=0, index=None):
    """A seed vector for ``qap.faq`` / ``qap.two_opt`` / ``match`` (``seeds=``) from planted labels: per pair min(count, n_b) rows
    keep their label, chosen uniformly without replacement; every other entry is -1.  labels: (B, N) integer tensor on the GPU;
    nvalid: (B,) vertex counts or None.  The choice depends on (seed, pair index) only -- pair b is first + b, or index[b] -- and
    is drawn from Philox stream 8 of the pair (SEEDS_STREAM), next to the permutation's stream 7: the first `count` steps of
    `planted_permutation`'s Fisher-Yates.  -> (B, N) int32 device tensor.  Enqueued on the current stream."""
    if not torch.is_tensor(labels) or labels.dim() != 2:
        raise ValueError('reveal_seeds: labels must be a (B, N) integer tensor')
    B, N = labels.shape
    check_labels(labels, B, N)
    if not labels.is_cuda:
        raise RuntimeError('reveal_seeds: labels are on %s; the seeds are drawn on the GPU only (there is no CPU path)' % (labels.device,))
    if not 1 <= N <= MAX_N:
        raise ValueError('reveal_seeds: 1 to %d vertices per graph, got %d' % (MAX_N, N))
    count, seed, first = int(count), int(seed), int(first)
    if count < 0 or first < 0 or not 0 <= seed < 1 << 64:
        raise ValueError('reveal_seeds: count and first must be >= 0 and seed in [0, 2^64), got %d, %d, %d' % (count, first, seed))
    dev = labels.device
    if index is not None:
        if not torch.is_tensor(index):
            index = torch.tensor(index, dtype=torch.int64)
        if index.dim() != 1 or index.dtype != torch.int64 or index.numel() != B:
            raise ValueError('reveal_seeds: index must be a (%d,) int64 tensor' % B)
        index = index.to(dev).contiguous()
    lab = labels.to(dtype=torch.int32).contiguous()
    nv = _nv32(nvalid, B, dev)
    out = torch.empty(B, N, dtype=torch.int32, device=dev)
    if B:
        with torch.cuda.device(dev):
            _lib.call('fgnn_reveal_seeds', seed, first, _lib.ptr(index), _lib.ptr(lab), _lib.ptr(nv), B, N, min(count, N), _lib.ptr(out),
                      _lib.stream_ptr())
    return out


def relabel_bits(bits, labels, nvalid=None):
    """fgnn_relabel_bits: (B, N, ceil(N/32)) int32 words -> the relabelled words (a new tensor), zero outside every corner."""
    if not bits.is_cuda:
        raise RuntimeError('relabel: the input is on %s; relabelling runs on the GPU only (there is no CPU path)' % (bits.device,))
    if bits.dim() != 3 or bits.shape[2] != (bits.shape[1] + 31) // 32:
        raise ValueError('relabel: expected (B, N, ceil(N/32)) int32 bit words, got %s' % (tuple(bits.shape),))
    B, N, _ = bits.shape
    if not 1 <= N <= MAX_N:
        raise ValueError('relabel: 1 to %d vertices per graph, got %d' % (MAX_N, N))
    check_labels(labels, B, N)
    if labels.shape[1] != N:
        raise ValueError('relabel: labels of bit words must have shape (%d, %d), got %s' % (B, N, tuple(labels.shape)))
    lab = labels.to(device=bits.device, dtype=torch.int32).contiguous()
    nv = _nv32(nvalid, B, bits.device)
    out = torch.empty_like(bits, memory_format=torch.contiguous_format)
    if B:
        with torch.cuda.device(bits.device):
            _lib.call('fgnn_relabel_bits', _lib.ptr(bits.contiguous()), _lib.ptr(lab), _lib.ptr(nv), B, N, _lib.ptr(out), _lib.stream_ptr())
    return out


def relabel_dense(x, labels, nvalid=None):
    """fgnn_relabel_dense: (B, C, n, n) or (B, n, n) float tensor -> the relabelled tensor (fp32, same shape), exact zeros outside
    every corner.  labels may be wider than n (a ragged batch cropped to its largest graph)."""
    if not x.is_cuda:
        raise RuntimeError('relabel: the input is on %s; relabelling runs on the GPU only (there is no CPU path)' % (x.device,))
    if x.dim() not in (3, 4) or x.shape[-1] != x.shape[-2] or not x.is_floating_point():
        raise ValueError('relabel: expected int32 bit words or a (B, C, n, n) / (B, n, n) float tensor, got %s %s' % (tuple(x.shape), x.dtype))
    B, n = x.shape[0], x.shape[-1]
    C = x.shape[1] if x.dim() == 4 else 1
    if not 1 <= n <= MAX_N or C < 1:
        raise ValueError('relabel: 1 to %d vertices per graph and at least one channel, got %s' % (MAX_N, tuple(x.shape)))
    check_labels(labels, B, n)
    lab = labels.to(device=x.device, dtype=torch.int32).contiguous()
    nv = _nv32(nvalid, B, x.device)
    src = x.detach().float().contiguous()
    out = torch.empty_like(src)
    if B:
        with torch.cuda.device(x.device):
            _lib.call('fgnn_relabel_dense', _lib.ptr(src), _lib.ptr(lab), _lib.ptr(nv), B, C, n, lab.shape[1], _lib.ptr(out),
                      _lib.stream_ptr())
    return out


def relabel(x, labels, nvalid=None):
    """out[pi(i)][pi(j)] = x[i][j] per pair, with pi = labels (see the module docstring).  x: (B, N, ceil(N/32)) int32 bit words, a
    (B, C, n, n) or (B, n, n) float tensor, a {'input': tensor} dict or a MaskedTensor (whose vertex counts are used when nvalid is
    None); returns the same kind, a new object.  nvalid: (B,) vertex counts; everything outside the n_b x n_b corner of the result
    is zero.  Enqueued on the current stream."""
    if isinstance(x, dict):
        out = dict(x)
        out['input'] = relabel(x['input'], labels, nvalid)
        return out
    if isinstance(x, MaskedTensor):
        if tuple(x.masked_dims) != (2, 3) or x.tensor.dim() != 4:
            raise ValueError('relabel: a MaskedTensor must be a (B, C, n, n) batch masked along dims (2, 3), got dims %s' % (x.masked_dims,))
        t = relabel_dense(x.tensor.rename(None), labels, x.nvalid if nvalid is None else nvalid)
        return MaskedTensor(t, x.nvalid, x.masked_dims, x.base_name, x.names, x.masks)
    if not torch.is_tensor(x):
        raise ValueError('relabel: expected a tensor, a dict or a MaskedTensor, got %s' % type(x).__name__)
    if x.dtype == torch.int32:
        return relabel_bits(x, labels, nvalid)
    return relabel_dense(x, labels, nvalid)


def inverse(labels):
    """The inverse permutations: inv[b, labels[b, i]] = i for the n_b leading entries of row b (a permutation of [0, n_b)), -1 in the
    padding.  Plain torch on the labels' device, host included."""
    if not torch.is_tensor(labels) or labels.dim() != 2 or labels.is_floating_point():
        raise ValueError('inverse: labels must be a (B, N) integer tensor')
    B, N = labels.shape
    lab = labels.to(torch.int64)
    pos = torch.arange(N, device=labels.device).expand(B, N)
    valid = lab >= 0
    inv = torch.argsort(torch.where(valid, lab, N + pos), dim=1)              # the padding sorts behind every label, in place
    n = valid.sum(1, keepdim=True)
    return torch.where(pos < n, inv, torch.full_like(inv, -1)).to(labels.dtype)
