"""QAP graph pairs generated on the device (loaders/data_generator.py:38-125,175-219, ``QAP_Generator``).

``PairGenerator`` writes (graph, noisy graph) pairs straight into the engine's wire format -- (B, N, ceil(N/32)) int32 words,
bit j of word row i = W[i][j] (``synthetic.pack_adjacency``) -- with ``csrc/pairgen.hip``; ``.bits`` feeds
``FgnnTrainer.train_step_bits``, ``.dense`` builds the reference's collate structures from the same words and ``.spectral`` those
of ``QAP_spectralGenerator`` (loaders/data_generator.py:221-277: the channels L, L^2, ... of ``spectral.py``).

Semantics follow the reference:

* vertex count: N, or n ~ Binomial(N, vertex_proba) as N Bernoulli draws, shared by both sides of a pair.  One deviation:
  a draw with n < 2 is redrawn from the next N positions of the size stream (at most 64 times, then n = 2), where the
  reference would build a graph on 0 or 1 vertices;
* families: ``ErdosRenyi`` (one draw per unordered pair), ``Regular`` (degree d = int(p n), +1 if n d is odd; circulant seed,
  ``swaps_per_edge`` * m degree-preserving double-edge swaps as in ``synthetic.random_regular``, random relabelling),
  ``BarabasiAlbert`` (m = int(p (n - 1) / 2); networkx 3.x's star + repeated-nodes attachment, no relabelling; constant N);
* noise models: ``ErdosRenyi`` (W' = W (1 - Z1) + (1 - W) Z2, Z1 ~ ER(noise), Z2 ~ ER(p noise / (1 - p))) and ``EdgeSwap``
  (the reference's nested loop over the parent's directed edges: the (u < v) edges in row-major order, then their reversals);
* by default the pair is not permuted: the ground truth is the identity, as ``triplet_loss`` and the reference's loaders have
  it.  ``permute=True`` on ``bits`` / ``dense`` / ``spectral`` relabels side 2 by the pair's planted permutation (``planted.py``:
  ``out[pi(i)][pi(j)] = in[i][j]``) and appends ``labels`` ((count, N) int32, ``labels[b, i] = pi_b(i)``, -1 past n_b) to the return
  value: the ground truth that ``metrics``, ``qap`` and ``Siamese_Node_Exp.match`` take as ``labels=``.  Training does not take it:
  the model is permutation-equivariant and the reference's loss has no label.

Randomness is counter-based (Philox4x64-10 keyed by ``seed``): every draw is addressed by (pair index, stream, position), so
pair k of a dataset is the same however a range is split into calls, devices or ranks.  Streams: 0 size, 1 parent, 2 noise-1,
3 noise-2, 4 relabel, 5 swap chain / attachment, 7 planted permutation (``planted.py``), 8 revealed seeds (``planted.reveal_seeds``),
9 restart starts (``qap.faq``), 10 Wigner parent and 11 Wigner noise (``wigner.py``: the normals of the correlated Gaussian pairs), all
with 0 in the fourth counter word; number 6 in that word belongs to the epoch permutation (``sampler.py``).  Probabilities are integer thresholds ``min(2^32, floor(prob * 2^32))`` compared with raw 32-bit
draws; integers in [0, k) are ``(u32 * k) >> 32`` (``tests/pairgen_ref.py`` restates it all in numpy, bit for bit).

Which pairs: a contiguous range ``(first, count)``, or any pairs by ``index=`` (an int64 tensor of dataset indices in any order,
duplicates allowed; one launch, ``fgnn_pairgen_indexed``).  The rank split: global step s of batch size B on w ranks covers positions
``[s * B * w, (s + 1) * B * w)`` of the epoch order and rank r takes ``r * B ... r * B + B - 1`` of them, with no communication.
For an endless dataset the order is the identity (``bits(step * B * w + r * B, B)``); for the reference's fixed dataset reshuffled
every epoch ``sampler.EpochSampler.batch_index`` gives the indices of those positions (``FgnnTrainer.train_epoch``).

Several noise levels in one launch: ``levels = generator.levels(noises)`` builds the threshold table of up to 64 noise values and
``bits`` / ``dense`` / ``spectral`` take ``levels=levels, level=`` (one level number per pair): pair b is the pair the same generator
with ``noise=noises[level[b]]`` makes for that index, bit for bit, because a draw does not depend on the threshold it is compared
with (``fgnn_pairgen_levels``; ``FgnnTrainer.noise_curve`` evaluates a model across noise levels with it).

There is no CPU fallback (``_lib``).
"""
import ctypes as C
import math

import torch

from . import _lib
from .inputs import expand_adjacency
from .masked import MaskedTensor
from .planted import planted_permutation, relabel_bits
from .spectral import spectral_features

FAMILIES = {'ErdosRenyi': 0, 'Regular': 1, 'BarabasiAlbert': 2}
NOISE_MODELS = {'ErdosRenyi': 0, 'EdgeSwap': 1}
MAX_N = 256                   # include/fgnn_hip.h: FGNN_PAIRGEN_MAX_N


def threshold(prob):
    """Integer threshold of an event of probability prob on a raw 32-bit draw (u32 < thr)."""
    return min(1 << 32, int(math.floor(prob * 4294967296.0)))


def same_device(a, b):
    """Do two torch devices name the same device?  A CUDA device without an index ('cuda') is the current one, as torch places
    tensors and as the launches here run; torch.device('cuda') == torch.device('cuda:0') is False even when 0 is current."""
    a, b = torch.device(a), torch.device(b)
    if a.type != b.type:
        return False
    if a.type != 'cuda' or a.index == b.index:
        return True
    cur = torch.cuda.current_device()
    return (cur if a.index is None else a.index) == (cur if b.index is None else b.index)


class NoiseLevels:
    """The noise levels of a mixed launch (``PairGenerator.levels``): `noises`, the validated values as a tuple of floats; `table`,
    the (K, 2) int64 device tensor of their thresholds (thr_noise1, thr_noise2 per level, as ``PairGenerator`` computes them for a
    single noise value), built on the host."""

    def __init__(self, noises, edge_density, device):
        noises = tuple(float(v) for v in noises)
        if not 1 <= len(noises) <= _lib.FGNN_MAX_LEVELS:
            raise ValueError('between 1 and %d noise levels, got %d' % (_lib.FGNN_MAX_LEVELS, len(noises)))
        for v in noises:
            if not 0.0 <= v <= 1.0:
                raise ValueError('noise must be in [0, 1], got %r' % (v,))
        p = float(edge_density)
        self.noises, self.edge_density = noises, p
        self.thresholds = [(threshold(v), threshold(p * v / (1 - p))) for v in noises]
        self.table = torch.tensor(self.thresholds, dtype=torch.int64).to(device)

    def __len__(self):
        return len(self.noises)


class PairSource:
    """What the epoch loops take as their `generator` (FgnnTrainer.train_epoch / evaluate / fit / noise_curve): the selection and
    level arguments, ``levels``, and ``dense`` / ``spectral`` over ``bits``.  A subclass has `n_vertices`, `edge_density`, `seed`,
    `device` and ``bits(first, count, index, permute, levels, level)``: ``PairGenerator`` below, ``pairstore.PairStore``."""

    def _selection(self, first, count, index):
        """(first, count, None) of a contiguous range, or (0, len(index), index as a contiguous int64 tensor on the device)."""
        if index is None:
            if first is None or count is None:
                raise ValueError('give either (first, count) or index=')
            first, count = int(first), int(count)
            if first < 0 or count < 0:
                raise ValueError('first and count must be >= 0, got %d, %d' % (first, count))
            return first, count, None
        if first is not None or count is not None:
            raise ValueError('give either (first, count) or index=, not both')
        if not torch.is_tensor(index):
            index = torch.tensor(index, dtype=torch.int64)
        if index.dim() != 1 or index.dtype != torch.int64:
            raise ValueError('index must be a 1-D int64 tensor, got shape %s, %s' % (tuple(index.shape), index.dtype))
        return 0, index.numel(), index.to(self.device).contiguous()

    def levels(self, noises):
        """The NoiseLevels of this generator's edge density for `noises` (1 to 64 values in [0, 1]): the `levels=` of bits / dense /
        spectral.  `self.noise` does not enter it."""
        return NoiseLevels(noises, self.edge_density, self.device)

    def _need_gpu(self):
        if self.device.type != 'cuda':
            raise RuntimeError('%s: device %s; the pairs are made on the GPU only (there is no CPU path)'
                               % (type(self).__name__, self.device))

    def _level(self, levels, level, count):
        """level= as a contiguous (count,) int32 tensor on the device (never read on the host), or None without levels"""
        if levels is None and level is None:
            return None
        if levels is None or level is None:
            raise ValueError('levels= (PairGenerator.levels) and level= (one level number per pair) go together')
        if not isinstance(levels, NoiseLevels) or levels.edge_density != self.edge_density or not same_device(levels.table.device, self.device):
            raise ValueError('levels must come from the levels() of this generator (edge density %r, device %s)'
                             % (self.edge_density, self.device))
        if not torch.is_tensor(level):
            level = torch.tensor(level, dtype=torch.int32)
        if level.dim() != 1 or level.numel() != count or level.is_floating_point() or level.dtype == torch.bool:
            raise ValueError('level must be a (%d,) integer tensor, got shape %s, %s' % (count, tuple(level.shape), level.dtype))
        return level.to(device=self.device, dtype=torch.int32).contiguous()

    def _planted(self, b1, b2, nv, first, count, index):
        """permute=True: side 2 relabelled by the planted permutation of each pair -> (bits1, bits2, nvalid, labels)"""
        N = self.n_vertices
        if index is None:
            labels = planted_permutation(self.seed, N, first, count, nvalid=nv, device=self.device)
        else:
            labels = planted_permutation(self.seed, N, index=index, nvalid=nv, device=self.device)
        return b1, relabel_bits(b2, labels, nv), nv, labels

    @staticmethod
    def _levels_kw(levels, level):
        return {} if levels is None and level is None else {'levels': levels, 'level': level}

    def dense(self, first=None, count=None, index=None, permute=False, levels=None, level=None):
        """The reference's collate structures for the same pairs: ({'input': x1}, {'input': x2}) with (count, 2, N, N) fp32
        tensor representations (collate_fn_pair_explore) for a constant vertex count, else two MaskedTensors padded to the
        largest n_i of the batch (collate_fn_pair; one host sync for that size).  permute=True: side 2 is the representation of
        the relabelled graph and the (count, N) labels are appended to the return value.  levels, level: as in `bits`."""
        b1, b2, nv, *labels = self.bits(first, count, index, permute, **self._levels_kw(levels, level))
        count = b1.shape[0]
        N = self.n_vertices
        x1, x2 = expand_adjacency(b1, N, nv), expand_adjacency(b2, N, nv)
        if nv is None:
            return ({'input': x1}, {'input': x2}, *labels)
        n = int(nv.max().item()) if count else 0
        x1, x2 = x1[:, :, :n, :n].contiguous(), x2[:, :, :n, :n].contiguous()
        return (MaskedTensor(x1, nv, (2, 3), 'N'), MaskedTensor(x2, nv, (2, 3), 'M'), *labels)

    def spectral(self, first=None, count=None, n_powers=4, index=None, permute=False, levels=None, level=None):
        """The twin of `dense` for the reference's ``QAP_spectralGenerator`` (loaders/data_generator.py:221-277): the same pairs as
        `bits`, each side as the n_powers channels L, L^2, ... of ``spectral.spectral_features`` (one launch per side, straight from
        the bit rows; an isolated vertex gives a zero row and column where the reference gives NaN).  ({'input': F1}, {'input': F2})
        with (count, n_powers, N, N) fp32 tensors for a constant vertex count, else two MaskedTensors written directly at the
        largest n_i of the batch (one host sync for that size), with the names and masked dims of `dense`.  permute=True: side 2 is
        computed from the relabelled bit rows and the (count, N) labels are appended to the return value.  levels, level: as in
        `bits`."""
        b1, b2, nv, *labels = self.bits(first, count, index, permute, **self._levels_kw(levels, level))
        count = b1.shape[0]
        if nv is None:
            return ({'input': spectral_features(b1, None, n_powers)}, {'input': spectral_features(b2, None, n_powers)}, *labels)
        n = max(int(nv.max().item()), 1) if count else 1
        f1, f2 = spectral_features(b1, nv, n_powers, n_out=n), spectral_features(b2, nv, n_powers, n_out=n)
        return (MaskedTensor(f1, nv, (2, 3), 'N'), MaskedTensor(f2, nv, (2, 3), 'M'), *labels)


class PairGenerator(PairSource):
    """On-device twin of the reference's ``QAP_Generator`` (the ``data.train`` / ``data.test`` parameters)."""

    def __init__(self, n_vertices, generative_model='Regular', noise_model='ErdosRenyi', edge_density=0.2, noise=0.1,
                 vertex_proba=1.0, seed=0, swaps_per_edge=10, device=None):
        N = int(n_vertices)
        p, noise, vertex_proba = float(edge_density), float(noise), float(vertex_proba)
        if not 1 <= N <= MAX_N:
            raise ValueError('n_vertices must be in [1, %d], got %d' % (MAX_N, N))
        if generative_model not in FAMILIES:
            raise ValueError('unknown graph family %r' % (generative_model,))
        if noise_model not in NOISE_MODELS:
            raise ValueError('unknown noise model %r' % (noise_model,))
        if not 0.0 <= p < 1.0:
            raise ValueError('edge_density must be in [0, 1), got %r' % (edge_density,))
        if not 0.0 <= noise <= 1.0:
            raise ValueError('noise must be in [0, 1], got %r' % (noise,))
        if not 0.0 < vertex_proba <= 1.0:
            raise ValueError('vertex_proba must be in (0, 1], got %r' % (vertex_proba,))
        if vertex_proba < 1.0 and N < 2:
            raise ValueError('a binomial vertex count needs n_vertices >= 2, got %d' % N)
        if not 0 <= int(swaps_per_edge) <= 10000:
            raise ValueError('swaps_per_edge must be in [0, 10000], got %r' % (swaps_per_edge,))
        if generative_model == 'BarabasiAlbert':
            m = int(p * (N - 1) / 2)
            if m < 1 or m >= N:
                raise ValueError('no Barabasi-Albert graph with m = %d attachments on %d vertices '
                                 '(m = int(edge_density * (n_vertices - 1) / 2) must be in [1, n_vertices))' % (m, N))
            if vertex_proba < 1.0:
                raise ValueError('BarabasiAlbert needs a constant vertex count (vertex_proba = 1), got vertex_proba %r'
                                 % (vertex_proba,))
        if not 0 <= int(seed) < 1 << 64:
            raise ValueError('seed must be in [0, 2^64), got %r' % (seed,))
        self.n_vertices, self.generative_model, self.noise_model = N, generative_model, noise_model
        self.edge_density, self.noise, self.vertex_proba = p, noise, vertex_proba
        self.seed, self.swaps_per_edge = int(seed), int(swaps_per_edge)
        self.constant_n_vertices = vertex_proba == 1.0
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self._thr = (threshold(p), threshold(noise), threshold(p * noise / (1 - p)), threshold(vertex_proba))

    @classmethod
    def from_config(cls, cfg, seed=0, **kw):
        """The reference's ``data.train`` / ``data.test`` dict as is (keys it does not use, num_examples_* among them, are ignored)."""
        return cls(cfg['n_vertices'], generative_model=cfg['generative_model'], noise_model=cfg['noise_model'],
                   edge_density=cfg['edge_density'], noise=cfg['noise'], vertex_proba=cfg.get('vertex_proba', 1.0),
                   seed=seed, **kw)

    def bits(self, first=None, count=None, index=None, permute=False, levels=None, level=None):
        """Pairs first .. first + count - 1, or the pairs index[0], index[1], ... (a 1-D int64 tensor, or a list; moved to the device
        if it is not there; any order, duplicates allowed) -> (bits1, bits2, nvalid): (count, N, ceil(N/32)) int32 device tensors
        and, when the vertex count is binomial, the (count,) int32 vertex counts (else None).  Enqueued on the current stream; the
        index is not read on the host: a negative entry (a caller error) gives the empty graph, all words zero and nvalid = 0.
        permute=True: bits2 is relabelled by the planted permutation of each pair and (bits1, bits2, nvalid, labels) is returned.
        levels, level: the NoiseLevels of `levels()` and one level number per pair ((count,) integer device tensor, or a list; not
        read on the host): pair b gets the noise levels.noises[level[b]] instead of self.noise and is otherwise the same pair (the
        planted permutation depends on (seed, index) only).  A level outside [0, K) is a caller error like a negative index."""
        mixed = levels is not None or level is not None
        if not mixed:       # (with levels every argument is checked before the device, so that the checks run anywhere)
            self._need_gpu()
        first, count, index = self._selection(first, count, index)
        level = self._level(levels, level, count)
        self._need_gpu()
        N = self.n_vertices
        W = (N + 31) // 32
        with torch.cuda.device(self.device):
            b1 = torch.empty(count, N, W, dtype=torch.int32, device=self.device)
            b2 = torch.empty(count, N, W, dtype=torch.int32, device=self.device)
            nv = None if self.constant_n_vertices else torch.empty(count, dtype=torch.int32, device=self.device)
            if count:
                a = _lib.PairgenArgs()
                a.seed, a.first, a.B, a.N = self.seed, first, count, N
                a.family, a.noise_model = FAMILIES[self.generative_model], NOISE_MODELS[self.noise_model]
                a.edge_density = self.edge_density
                a.thr_edge, a.thr_noise1, a.thr_noise2, a.thr_vertex = self._thr
                a.swaps_per_edge = self.swaps_per_edge
                a.bits1, a.bits2 = b1.data_ptr(), b2.data_ptr()
                a.nvalid = nv.data_ptr() if nv is not None else None
                if level is not None:
                    _lib.call('fgnn_pairgen_levels', C.byref(a), _lib.ptr(index), _lib.ptr(levels.table), len(levels), _lib.ptr(level),
                              _lib.stream_ptr())
                elif index is None:
                    _lib.call('fgnn_pairgen', C.byref(a), _lib.stream_ptr())
                else:
                    _lib.call('fgnn_pairgen_indexed', C.byref(a), _lib.ptr(index), _lib.stream_ptr())
            if permute:
                return self._planted(b1, b2, nv, first, count, index)
        return b1, b2, nv
