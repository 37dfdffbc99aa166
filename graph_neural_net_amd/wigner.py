"""Correlated Gaussian (Wigner) pairs generated on the device: the standard real-weighted model of graph alignment.

``A`` is symmetric with independent N(0, 1/n) entries above a zero diagonal and ``B = sqrt(1 - s^2) A + s Z`` with an independent
``Z`` of the same law, so every entry pair (A_ij, B_ij) has correlation ``sqrt(1 - s^2)``: `noise` = s = 0 is two equal graphs,
s = 1 two independent ones.  ``WignerGenerator.weighted`` writes both sides of a batch in ONE launch (``csrc/wigner.hip``,
``fgnn_wigner_pairs``) as the reference's tensor representation of a real ``W`` (loaders/data_generator.py:118-125: channel 0 = W,
channel 1 = diag(row sums)), (count, 2, N, N) fp32 padded to N = n_vertices -- what ``FgnnTrainer.train_step`` / ``eval_step`` and
``evaluation.decode_scores_weighted`` take, and what the epoch loops pull with ``features='weighted'``.

* vertex count: ``PairGenerator``'s -- stream 0 with its redraw rule, so a WignerGenerator and a PairGenerator of one
  (seed, n_vertices, vertex_proba) give the same ``nvalid``;
* normals: two pair streams of their own, 10 (parent) and 11 (noise) (``pairgen``'s docstring lists the streams).  The normal of the
  unordered entry {i, j}, i < j, has the linear index t = i N + j (N = n_vertices, so an entry does not move with the vertex count)
  and comes from Philox block t >> 3, 64-bit word (t & 7) >> 1 = (w0 low half, w1 high half), by Box-Muller on 24-bit uniforms:
  u = ((w0 >> 8) + 1) 2^-24, v = (w1 >> 8) 2^-24, z = sqrtf(-2 logf(u)) * (cospif(2 v) for even t, sinpif(2 v) for odd t);
* values: A_ij = c z10(t), B_ij = fmaf(rho, A_ij, sig (c z11(t))) with c = 1 / sqrtf(n_b) (``scale='wigner'``) or 1 (``scale=None``),
  rho = (float)sqrt(1 - s^2) and sig = (float)s computed in double and rounded once.  A draw does not depend on s: with
  ``levels = generator.levels(noises)`` and ``level=`` one launch holds pairs of several noise values, pair b being bit for bit
  the pair of a generator with ``noise=noises[level[b]]``;
* ``support=``: a ``PairSource`` (``PairGenerator``, ``PairStore``) whose words for the same pairs mask the two sides -- A_ij where
  bit (i, j) of its first graph is set, B_ij where that of its second graph is, zero elsewhere: correlated SPARSE weighted graphs on
  any family and noise model the library has.  The value at an entry is the dense generator's;
* ``permute=True``: side 2 is written relabelled by the pair's planted permutation (``planted.planted_permutation`` of the same
  seed: ``x2[pi(i)][pi(j)] = B_ij``) in the same launch, and the labels are appended to the return value;
* row sums (channel 1): fp32, per output row, in the fixed order of ``csrc/wigner.hip`` -- the partial sums of the columns
  l, l + 64, l + 128, l + 192 in ascending order for l < 64, then a butterfly over l with strides 32, 16, 8, 4, 2, 1.

There is no CPU path (``_lib``); nothing here reads the device except ``dense`` on a ragged batch (one size, as ``PairSource.dense``).
"""
import ctypes as C
import math

import torch

from . import _lib
from .masked import MaskedTensor
from .pairgen import MAX_N, PairSource, same_device, threshold
from .planted import planted_permutation

SCALES = ('wigner', None)
PARENT_STREAM, NOISE_STREAM = _lib.FGNN_WIGNER_PARENT_STREAM, _lib.FGNN_WIGNER_NOISE_STREAM


def coefficients(noise):
    """(rho, sig) = (sqrt(1 - s^2), s) in double; the launch rounds each to fp32 once"""
    s = float(noise)
    return math.sqrt(max(0.0, 1.0 - s * s)), s


class WignerLevels:
    """The noise levels of a mixed launch (``WignerGenerator.levels``): `noises`, the validated values as a tuple of floats; `table`,
    the (K, 2) float32 device tensor of their (rho, sig), built on the host."""

    def __init__(self, noises, owner):
        noises = tuple(float(v) for v in noises)
        if not 1 <= len(noises) <= _lib.FGNN_MAX_LEVELS:
            raise ValueError('between 1 and %d noise levels, got %d' % (_lib.FGNN_MAX_LEVELS, len(noises)))
        for v in noises:
            if not 0.0 <= v <= 1.0:
                raise ValueError('noise must be in [0, 1], got %r' % (v,))
        self.noises, self.owner = noises, owner
        self.table = torch.tensor([coefficients(v) for v in noises], dtype=torch.float64).to(torch.float32).to(owner.device)

    def __len__(self):
        return len(self.noises)


class WignerGenerator:
    """Correlated Gaussian pairs of `n_vertices` vertices at noise s = `noise` (see the module docstring); the `generator` of the
    epoch loops with ``features='weighted'``."""

    def __init__(self, n_vertices, noise=0.1, vertex_proba=1.0, seed=0, scale='wigner', support=None, device=None):
        N = int(n_vertices)
        noise, vertex_proba = float(noise), float(vertex_proba)
        if not 1 <= N <= MAX_N:
            raise ValueError('n_vertices must be in [1, %d], got %d' % (MAX_N, N))
        if not 0.0 <= noise <= 1.0:
            raise ValueError('noise must be in [0, 1], got %r' % (noise,))
        if not 0.0 < vertex_proba <= 1.0:
            raise ValueError('vertex_proba must be in (0, 1], got %r' % (vertex_proba,))
        if vertex_proba < 1.0 and N < 2:
            raise ValueError('a binomial vertex count needs n_vertices >= 2, got %d' % N)
        if scale not in SCALES:
            raise ValueError("scale must be 'wigner' or None, got %r" % (scale,))
        if not 0 <= int(seed) < 1 << 64:
            raise ValueError('seed must be in [0, 2^64), got %r' % (seed,))
        if support is not None:
            if not isinstance(support, PairSource):
                raise ValueError('support must be None or a PairSource (PairGenerator, PairStore), got %s' % type(support).__name__)
            if support.n_vertices != N:
                raise ValueError('support has n_vertices %d, the generator %d' % (support.n_vertices, N))
            if support.constant_n_vertices != (vertex_proba == 1.0):
                raise ValueError('support and generator must both have a constant or both a binomial vertex count')
            # a binomial count is drawn from (seed, pair, n_vertices, vertex_proba): the mask and the weights must share it
            if vertex_proba < 1.0 and (getattr(support, 'vertex_proba', None) != vertex_proba or support.seed != int(seed)):
                raise ValueError('a support with a binomial vertex count must have the seed and vertex_proba of the generator '
                                 '(both draw n from them)')
        self.n_vertices, self.noise, self.vertex_proba, self.seed, self.scale = N, noise, vertex_proba, int(seed), scale
        self.constant_n_vertices = vertex_proba == 1.0
        self.support = support
        self.device = torch.device(device) if device is not None else (
            support.device if support is not None else torch.device('cuda', torch.cuda.current_device()))
        if support is not None and not same_device(support.device, self.device):
            raise ValueError('support is on %s, the generator on %s' % (support.device, self.device))
        self._thr_vertex = threshold(vertex_proba)

    _selection = PairSource._selection

    def levels(self, noises):
        """The WignerLevels of `noises` (1 to 64 values in [0, 1]): the `levels=` of weighted / dense.  `self.noise` does not enter."""
        return WignerLevels(noises, self)

    def _need_gpu(self):
        if self.device.type != 'cuda':
            raise RuntimeError('WignerGenerator: device %s; the pairs are made on the GPU only (there is no CPU path)' % (self.device,))

    def _level(self, levels, level, count):
        if levels is None and level is None:
            return None
        if levels is None or level is None:
            raise ValueError('levels= (WignerGenerator.levels) and level= (one level number per pair) go together')
        if not isinstance(levels, WignerLevels) or levels.owner is not self:
            raise ValueError('levels must come from the levels() of this generator')
        if not torch.is_tensor(level):
            level = torch.tensor(level, dtype=torch.int32)
        if level.dim() != 1 or level.numel() != count or level.is_floating_point() or level.dtype == torch.bool:
            raise ValueError('level must be a (%d,) integer tensor, got shape %s, %s' % (count, tuple(level.shape), level.dtype))
        return level.to(device=self.device, dtype=torch.int32).contiguous()

    def bits(self, *args, **kw):
        raise RuntimeError('WignerGenerator makes real-weighted pairs: there are no bit words; use .weighted(...) '
                           "(the epoch loops: features='weighted')")

    def spectral(self, *args, **kw):
        raise RuntimeError('WignerGenerator makes real-weighted pairs: there are no spectral features of bit words; use '
                           ".weighted(...) (the epoch loops: features='weighted')")

    def _launch(self, first, count, index, level, levels, x1, x2, nv, sup=None, labels=None):
        a = _lib.WignerArgs()
        a.seed, a.first, a.B, a.N, a.thr_vertex = self.seed, first, count, self.n_vertices, self._thr_vertex
        a.rho, a.sig = coefficients(self.noise)
        a.scale = 1 if self.scale == 'wigner' else 0
        a.index = index.data_ptr() if index is not None else None
        if level is not None:
            a.level_coef, a.level, a.K = levels.table.data_ptr(), level.data_ptr(), len(levels)
        if sup is not None:
            a.bits1, a.bits2 = sup[0].data_ptr(), sup[1].data_ptr()
        a.labels = labels.data_ptr() if labels is not None else None
        a.x1 = x1.data_ptr() if x1 is not None else None
        a.x2 = x2.data_ptr() if x2 is not None else None
        a.nvalid = nv.data_ptr() if nv is not None else None
        _lib.call('fgnn_wigner_pairs', C.byref(a), _lib.stream_ptr())

    def weighted(self, first=None, count=None, index=None, permute=False, levels=None, level=None):
        """Pairs first .. first + count - 1, or the pairs index[0], index[1], ... (``PairGenerator.bits``' selection) ->
        (x1, x2, nvalid): two (count, 2, N, N) fp32 device tensors and, when the vertex count is binomial, the (count,) int32 vertex
        counts (else None).  One launch on the current stream; nothing is read on the host: a negative index, or a level outside
        [0, K), gives the empty graph and nvalid = 0.
        permute=True: x2 is written relabelled by the planted permutation of each pair, in the same launch, and (x1, x2, nvalid,
        labels) is returned; the permutation needs the vertex counts, so a binomial count costs one launch of a wave per pair first.
        levels, level: the WignerLevels of `levels()` and one level number per pair: pair b takes the noise levels.noises[level[b]].
        With a support, its ``bits`` of the same pairs (the same selection; its own noise, whatever the level) mask the two sides:
        one more launch."""
        first, count, index = self._selection(first, count, index)
        level = self._level(levels, level, count)
        self._need_gpu()
        N = self.n_vertices
        with torch.cuda.device(self.device):
            x1 = torch.empty(count, 2, N, N, dtype=torch.float32, device=self.device)
            x2 = torch.empty(count, 2, N, N, dtype=torch.float32, device=self.device)
            nv = None if self.constant_n_vertices else torch.empty(count, dtype=torch.int32, device=self.device)
            labels = None
            if count:
                sup = None
                if self.support is not None:
                    sup = self.support.bits(first, count) if index is None else self.support.bits(index=index)
                if permute:
                    if nv is not None:
                        self._launch(first, count, index, level, levels, None, None, nv)
                    if index is None:
                        labels = planted_permutation(self.seed, N, first, count, nvalid=nv, device=self.device)
                    else:
                        labels = planted_permutation(self.seed, N, index=index, nvalid=nv, device=self.device)
                self._launch(first, count, index, level, levels, x1, x2, nv, sup, labels)
            elif permute:
                labels = torch.empty(0, N, dtype=torch.int32, device=self.device)
        return (x1, x2, nv, labels) if permute else (x1, x2, nv)

    def dense(self, first=None, count=None, index=None, permute=False, levels=None, level=None):
        """The same call as the reference's collate structures, as ``PairSource.dense`` wraps its pairs: ({'input': x1},
        {'input': x2}) for a constant vertex count, else two MaskedTensors cropped to the largest n_i of the batch (one host sync
        for that size); the labels of permute=True are appended."""
        x1, x2, nv, *labels = self.weighted(first, count, index, permute, levels, level)
        if nv is None:
            return ({'input': x1}, {'input': x2}, *labels)
        n = int(nv.max().item()) if x1.shape[0] else 0
        x1, x2 = x1[:, :, :n, :n].contiguous(), x2[:, :, :n, :n].contiguous()
        return (MaskedTensor(x1, nv, (2, 3), 'N'), MaskedTensor(x2, nv, (2, 3), 'M'), *labels)
