"""The spectral input of the reference's second dataset class (loaders/data_generator.py:221-232 ``make_laplacian`` /
``make_spectral_feature``, what ``QAP_spectralGenerator`` yields) on the device, through ``csrc/spectral.hip``.

Per graph the channels are ``L, L^2, ..., L^n_powers`` with ``L = D^-1/2 W D^-1/2`` (the reference uses 4):

* ``d_i`` = row sum of W over the valid ``n x n`` corner (bits outside it are masked, not trusted; W need not be symmetric);
* ``s_i = 1 / sqrt(d_i)`` in fp32, IEEE sqrt and division;
* ``F_1[i][j] = (s_i w_ij) s_j`` -- one correctly rounded product, bit-exact against the reference;
* ``F_{p+1} = F_p @ L``, the reference's left-to-right chain in fp32, computed as ``s_j sum_k (F_p[i][k] s_k) w_kj`` on the fp32
  matrix cores (within the reference's own fp32 error of the fp64 chain: tests/test_gpu_spectral.py);
* everything outside the ``n x n`` corner is exact zeros.

**Deviation.**  For a vertex of degree 0 the reference computes ``inf * 0 = NaN``, and every later power is then NaN in EVERY
entry: it is unusable on a graph with an isolated vertex.  Here ``s_i = 0`` where ``d_i = 0``, so the row and column of an isolated
vertex are zeros (an all-zero graph gives all zeros) and the rest of the graph is the reference's arithmetic.

Input is the engine's wire format -- (G, N, ceil(N/32)) int32 words, bit j of word row i = W[i][j] (``synthetic.pack_adjacency``,
``PairGenerator.bits``) -- and one launch writes all powers; nothing synchronises.  There is no CPU fallback (``_lib``).
"""
import torch

from . import _lib, qap

MAX_N = _lib.FGNN_SPECTRAL_MAX_N
MAX_POWERS = _lib.FGNN_SPECTRAL_MAX_POWERS


def spectral_features(bits, nvalid=None, n_powers=4, n_out=None, out=None):
    """bits (G, N, ceil(N/32)) int32 device tensor, nvalid optional (G,) vertex counts -> (G, n_powers, n_out, n_out) fp32, the
    top-left n_out x n_out corner (default n_out = N) of the zero-padded features: a ragged batch is written directly at its largest
    n.  `out`, if given, is that tensor (contiguous fp32 on the same device) and is returned.  Enqueued on the current stream, no
    synchronisation: the call can be captured."""
    if not isinstance(bits, torch.Tensor) or not bits.is_cuda:
        raise RuntimeError('spectral_features: the bit rows are on %s; the features are computed on the GPU only (there is no CPU '
                           'path)' % (getattr(bits, 'device', type(bits).__name__),))
    if bits.dim() != 3 or bits.dtype != torch.int32 or bits.shape[2] != (bits.shape[1] + 31) // 32:
        raise RuntimeError('spectral_features: expected (G, N, ceil(N/32)) int32 bit words, got %s %s' % (tuple(bits.shape), bits.dtype))
    G, N, _ = bits.shape
    if not 1 <= N <= MAX_N:
        raise RuntimeError('spectral_features: 1 to %d vertices per graph, got %d' % (MAX_N, N))
    n_powers = int(n_powers)
    if not 1 <= n_powers <= MAX_POWERS:
        raise ValueError('n_powers must be in [1, %d], got %d' % (MAX_POWERS, n_powers))
    n_out = N if n_out is None else int(n_out)
    if not 1 <= n_out <= N:
        raise ValueError('n_out must be in [1, N = %d], got %d' % (N, n_out))
    if nvalid is not None:
        if nvalid.dim() != 1 or nvalid.shape[0] != G or nvalid.is_floating_point():
            raise RuntimeError('spectral_features: nvalid must be (G = %d,) integers, got %s %s' % (G, tuple(nvalid.shape), nvalid.dtype))
        nvalid = nvalid.to(device=bits.device, dtype=torch.int32).contiguous()
    shape = (G, n_powers, n_out, n_out)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=bits.device)
    elif (not out.is_cuda or out.device != bits.device or out.dtype != torch.float32 or tuple(out.shape) != shape
          or not out.is_contiguous()):
        raise RuntimeError('spectral_features: out must be a contiguous fp32 %s tensor on %s' % (shape, bits.device))
    if G:
        with torch.cuda.device(bits.device):
            _lib.call('fgnn_spectral_features', _lib.ptr(bits.contiguous()), _lib.ptr(nvalid), G, N, n_powers, _lib.ptr(out), n_out,
                      _lib.stream_ptr())
    return out


def spectral_from_dense(x, nvalid=None, n_powers=4):
    """The same from what a dense loader holds: x is a (B, N, N) 0/1 adjacency or a (B, 2, N, N) tensor representation
    (loaders/data_generator.py:118-125) on the device -> (B, n_powers, N, N) fp32.  The batch is bit-packed on the device by
    fgnn_pack_adjacency_ld, which also verifies it (entries of W in {0, 1}); the one read of that verdict, after everything is
    queued, is the only synchronisation."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError('spectral_from_dense: the batch is on %s; there is no CPU path' % (getattr(x, 'device', type(x).__name__),))
    if not x.is_floating_point() or x.dim() not in (3, 4) or x.shape[-1] != x.shape[-2] or (x.dim() == 4 and x.shape[1] != 2):
        raise RuntimeError('spectral_from_dense: expected a (B, N, N) adjacency or a (B, 2, N, N) tensor representation, got %s %s'
                           % (tuple(x.shape), x.dtype))
    B, N = x.shape[0], x.shape[-1]
    if not 1 <= N <= MAX_N:
        raise RuntimeError('spectral_from_dense: 1 to %d vertices per graph, got %d' % (MAX_N, N))
    nv = nvalid.to(device=x.device, dtype=torch.int32).contiguous() if nvalid is not None else None
    if x.dim() == 3:                            # W alone: its tensor representation (channel 1 = diag(row sums over the corner))
        w = x.detach().float()
        if nv is not None:
            inside = torch.arange(N, device=x.device)[None, :] < nv[:, None]
            w = w * (inside[:, :, None] & inside[:, None, :])
        x = torch.stack([w, torch.diag_embed(w.sum(-1))], 1)
    flag = torch.zeros(1, dtype=torch.int32, device=x.device)
    bits = qap.to_bits(x, nv, flag)
    out = spectral_features(bits, nv, n_powers)
    if int(flag.item()) != 0:                   # (the one host synchronisation)
        raise RuntimeError('spectral_from_dense: ' + qap.NOT_A_REPRESENTATION)
    return out
