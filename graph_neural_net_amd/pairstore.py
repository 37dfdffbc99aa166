"""Pairs from stored graphs (loaders/data_generator.py:133-155, ``Base_Generator.load_dataset``: a dataset that is loaded, not
generated).

``PairStore`` holds M graphs in the engine's wire format -- (M, N, ceil(N/32)) int32 words, bit j of word row i = W[i][j]
(``synthetic.pack_adjacency``), an optional (M,) vertex count per graph, an optional stored second side -- resident in device
memory, and presents ``pairgen.PairGenerator``'s surface over them: ``bits`` / ``dense`` / ``spectral`` with the same arguments
and return values, ``levels``, `device`.  ``FgnnTrainer.train_epoch`` / ``evaluate`` / ``fit`` / ``noise_curve`` take it as their
`generator` unchanged, with an ``EpochSampler`` over `num_examples`.

Example k of a batch is side 1 = stored graph k and side 2 either

* the stored second side as it is (`paired`: the reference's (B, B_noise) datasets), or
* a noisy copy made on the device by the generator's own noise stage (``csrc/pairstore.hip``: one launch per batch,
  ``fgnn_pairstore_gather``): ``ErdosRenyi`` (W' = W (1 - Z1) + (1 - W) Z2) or ``EdgeSwap``, on the Philox streams, positions and
  thresholds ``PairGenerator`` uses for pair (seed, k) at this N and n_k.  A store filled with a generator's parents therefore
  returns that generator's pairs bit for bit, and ``tests/pairgen_ref.py`` restates both noise functions on any parent.

`seed` and `noise` are plain attributes: a loop that wants fresh noise every epoch changes `seed` between epochs.  `edge_density`
only feeds the ErdosRenyi noise (thr2 = threshold(p noise / (1 - p))) and the level tables; None takes the store's own density.

The constructors validate their input (symmetric, 0/1, zero diagonal; ``ValueError`` otherwise) and leave clean padding (rows,
columns and word bits past n_k zero).  They are not on the hot path and read sizes and edge counts on the host, once.  A store
may be built, saved and loaded with CPU tensors; only ``bits`` needs the GPU (there is no CPU path for it).
"""
import ctypes as C

import torch

from . import _lib
from .inputs import pack_tensor_representation
from .pairgen import MAX_N, NOISE_MODELS, PairSource, threshold

_CHUNK = 2048                 # graphs per validation / packing step of a constructor
_FORMAT = 'fgnn_pairstore/1'


def _as_words(t, what):
    """(M, N, ceil(N/32)) 32-bit words (torch int32, or a numpy uint32 / int32 array) -> int32 tensor"""
    if not torch.is_tensor(t):
        import numpy as np
        t = np.ascontiguousarray(t)
        if t.dtype not in (np.uint32, np.int32):
            raise ValueError('%s: expected 32-bit words, got %s' % (what, t.dtype))
        t = torch.from_numpy(t.view(np.int32))
    if t.dtype != torch.int32 or t.dim() != 3 or t.shape[0] < 1 or not 1 <= t.shape[1] <= MAX_N or t.shape[2] != (t.shape[1] + 31) // 32:
        raise ValueError('%s: expected (M >= 1, N <= %d, ceil(N/32)) int32 words, got %s %s' % (what, MAX_N, tuple(t.shape), t.dtype))
    return t.contiguous()


def _as_sizes(sizes, M, N):
    """vertex counts -> (M,) int32 CPU tensor with entries in [0, N] (one host read); None stays None: every graph has N vertices"""
    if sizes is None:
        return None
    s = torch.as_tensor(sizes).detach().cpu()
    if s.dim() != 1 or s.numel() != M or s.is_floating_point() or s.dtype == torch.bool:
        raise ValueError('sizes must be a (%d,) integer tensor, got shape %s, %s' % (M, tuple(s.shape), s.dtype))
    if int(s.min()) < 0 or int(s.max()) > N:
        raise ValueError('sizes must lie in [0, %d], got %d .. %d' % (N, int(s.min()), int(s.max())))
    return s.to(torch.int32)


def _unpack(bits):
    """(m, N, W) int32 words -> (m, N, 32 W) bool"""
    sh = torch.arange(32, dtype=torch.int32, device=bits.device)
    return ((bits.unsqueeze(-1) >> sh) & 1).bool().reshape(bits.shape[0], bits.shape[1], -1)


def _pack(w):
    """(m, N, N) bool -> (m, N, W) int32 words, bit j of word row i = w[i][j] (synthetic.pack_adjacency)"""
    m, N, _ = w.shape
    W = (N + 31) // 32
    u = torch.zeros(m, N, W * 32, dtype=torch.int64, device=w.device)
    u[:, :, :N] = w
    v = (u.reshape(m, N, W, 32) << torch.arange(32, dtype=torch.int64, device=w.device)).sum(-1)
    return torch.where(v >= 1 << 31, v - (1 << 32), v).to(torch.int32)


def _valid_corner(m, N, sizes, device):
    """(m, N, N) bool: entry (i, j) lies inside the n_k x n_k corner of graph k"""
    i = torch.arange(N, device=device)
    live = i.unsqueeze(0) < sizes.to(device).unsqueeze(1)
    return live.unsqueeze(2) & live.unsqueeze(1)


def _check_adjacency(w, sizes, what, first):
    """w: (m, N, N) bool adjacencies of graphs first ..; the ValueError of the first graph that is not symmetric with a zero diagonal
    and nothing outside its corner -> (m,) int64 edge counts"""
    m, N, _ = w.shape
    bad = (w != w.transpose(1, 2)).flatten(1).any(1) | torch.diagonal(w, dim1=1, dim2=2).any(1)
    if sizes is not None:
        bad |= (w & ~_valid_corner(m, N, sizes, w.device)).flatten(1).any(1)
    if bool(bad.any()):
        raise ValueError('%s: graph %d is not a symmetric 0/1 adjacency with a zero diagonal and zero padding past its vertex count'
                         % (what, first + int(bad.int().argmax())))
    return w.flatten(1).sum(1) // 2


def _check_words(bits, sizes, what):
    """Validate (M, N, W) words (where they are, in chunks) -> (M,) int64 CPU tensor of edge counts"""
    M, N, _ = bits.shape
    counts = []
    for a in range(0, M, _CHUNK):
        u = _unpack(bits[a:a + _CHUNK])
        if bool(u[:, :, N:].any()):
            raise ValueError('%s: word bits past column %d are set' % (what, N))
        counts.append(_check_adjacency(u[:, :, :N], None if sizes is None else sizes[a:a + _CHUNK], what, a))
    return torch.cat(counts).cpu()


def _pack_dense(w, sizes, what, first=0):
    """(m, N, N) numbers -> validated words.  Entries must be 0 or 1; those outside the n_k corner are not read."""
    m, N, _ = w.shape
    if sizes is not None:
        w = torch.where(_valid_corner(m, N, sizes, w.device), w, torch.zeros((), dtype=w.dtype, device=w.device))
    if not bool(((w == 0) | (w == 1)).all()):
        raise ValueError('%s: entries other than 0 and 1' % what)
    w = w != 0
    _check_adjacency(w, sizes, what, first)
    return _pack(w)


class PairStore(PairSource):
    """M stored graphs as a source of (graph, second graph) pairs with ``PairGenerator``'s surface; see the module docstring.
    Attributes: device, n_vertices, constant_n_vertices, edge_density, noise, noise_model, seed (as ``PairGenerator``'s),
    num_examples (M), paired (a second side is stored); the words themselves: parents, sizes (None for a constant-size store),
    seconds (None unless paired), and what one host read at construction gave: total_edges, total_slots, max_edges."""

    def __init__(self, parents, sizes, seconds, edge_counts, noise_model, noise, seed, edge_density, device):
        """Not for callers: `parents` / `seconds` validated words, `sizes` the (M,) int32 CPU tensor or None, `edge_counts` the
        (M,) int64 CPU tensor of the parents' edge counts.  Use from_bits / from_dense / from_list / from_reference_dataset / load."""
        M, N, _ = parents.shape
        if noise_model not in NOISE_MODELS:
            raise ValueError('unknown noise model %r' % (noise_model,))
        self.device = torch.device(device) if device is not None else parents.device
        self.n_vertices, self.num_examples, self.noise_model = N, M, noise_model
        self.constant_n_vertices, self.paired = sizes is None, seconds is not None
        self.noise, self.seed = float(noise), int(seed)
        self._check_noise()
        # the store's own density: total edges over total n (n - 1) / 2, in Python integers
        self.total_edges = int(edge_counts.sum())
        self.total_slots = M * N * (N - 1) // 2 if sizes is None else sum(n * (n - 1) // 2 for n in sizes.tolist())
        self.max_edges = int(edge_counts.max())
        if edge_density is None:
            if self.total_edges >= self.total_slots > 0:
                raise ValueError('every stored graph is complete (density 1): give edge_density in [0, 1)')
            edge_density = self.total_edges / self.total_slots if self.total_slots else 0.0
        p = float(edge_density)
        if not 0.0 <= p < 1.0:
            raise ValueError('edge_density must be in [0, 1), got %r' % (edge_density,))
        self.edge_density = p
        self.parents = parents.to(self.device)
        self.sizes = None if sizes is None else sizes.to(self.device)
        self.seconds = None if seconds is None else seconds.to(self.device)

    def _check_noise(self):
        if not 0.0 <= float(self.noise) <= 1.0:
            raise ValueError('noise must be in [0, 1], got %r' % (self.noise,))
        if not 0 <= int(self.seed) < 1 << 64:
            raise ValueError('seed must be in [0, 2^64), got %r' % (self.seed,))

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_bits(cls, parents, sizes=None, seconds=None, noise_model='ErdosRenyi', noise=0.1, seed=0, edge_density=None, device=None):
        """parents (and seconds): (M, N, ceil(N/32)) int32 words (a tensor on any device, or a numpy uint32 array), e.g. the bits1
        of ``PairGenerator.bits``; sizes: the (M,) vertex counts (its nvalid), None when every graph has N vertices (with sizes the
        store is a ragged one and `bits` returns vertex counts, whatever their values).  device: where
        the store lives (None: where `parents` is)."""
        parents = _as_words(parents, 'parents')
        M, N, _ = parents.shape
        sizes = _as_sizes(sizes, M, N)
        counts = _check_words(parents, sizes, 'parents')
        if seconds is not None:
            seconds = _as_words(seconds, 'seconds')
            if seconds.shape != parents.shape:
                raise ValueError('seconds: expected the shape of parents %s, got %s' % (tuple(parents.shape), tuple(seconds.shape)))
            _check_words(seconds, sizes, 'seconds')
        return cls(parents, sizes, seconds, counts, noise_model, noise, seed, edge_density, device)

    @classmethod
    def from_dense(cls, x1, x2=None, nvalid=None, **settings):
        """x1 (and x2, the stored second side): (M, 2, N, N) tensor representations (loaders/data_generator.py:118-125: channel 0 =
        W, channel 1 = diag(degree)); nvalid: the (M,) vertex counts of padded batches.  Device tensors go through
        ``pack_tensor_representation(check=True)``, CPU tensors through the host packer (channel 0).  settings: as from_bits."""
        def words(x, what):
            if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 2 or x.shape[2] != x.shape[3]:
                raise ValueError('%s: expected a (M, 2, N, N) tensor' % what)
            if x.is_cuda:
                try:
                    return pack_tensor_representation(x.float(), None if nvalid is None else torch.as_tensor(nvalid), check=True)
                except RuntimeError as exc:
                    raise ValueError('%s: %s' % (what, exc)) from None
            sizes = _as_sizes(nvalid, x.shape[0], x.shape[-1])
            return torch.cat([_pack_dense(x[a:a + _CHUNK, 0], None if sizes is None else sizes[a:a + _CHUNK], what, a)
                              for a in range(0, x.shape[0], _CHUNK)])
        return cls.from_bits(words(x1, 'x1'), nvalid, None if x2 is None else words(x2, 'x2'), **settings)

    @classmethod
    def from_list(cls, graphs, seconds=None, n_vertices=None, device=None, **settings):
        """graphs (and seconds, of the same sizes): a list of (n_i, n_i) adjacencies or (2, n_i, n_i) tensor representations
        (channel 0 is read), tensors or arrays, of differing sizes; padded to the largest n_i, or to n_vertices (a constant-size store when
        every graph fills it).  Packed in chunks
        of 2048 graphs on `device` (None: the CPU), where the store then lives."""
        dev = torch.device(device) if device is not None else torch.device('cpu')

        def adjacency(g, what, k):
            g = torch.as_tensor(g).detach().cpu()
            if g.dim() == 3 and g.shape[0] == 2:
                g = g[0]
            if g.dim() != 2 or g.shape[0] != g.shape[1]:
                raise ValueError('%s: graph %d is neither (n, n) nor (2, n, n), got %s' % (what, k, tuple(g.shape)))
            return g

        graphs = [adjacency(g, 'graphs', k) for k, g in enumerate(graphs)]
        if not graphs:
            raise ValueError('graphs: an empty list')
        sizes = [g.shape[0] for g in graphs]
        N = max(sizes) if n_vertices is None else int(n_vertices)
        if not 1 <= N <= MAX_N or max(sizes) > N:
            raise ValueError('n_vertices must be in [1, %d] and hold the largest graph (%d), got %d' % (MAX_N, max(sizes), N))

        def words(gs, what):
            out = []
            for a in range(0, len(gs), _CHUNK):
                pad = torch.zeros(len(gs[a:a + _CHUNK]), N, N, dtype=torch.float32)
                for k, g in enumerate(gs[a:a + _CHUNK]):
                    pad[k, :g.shape[0], :g.shape[0]] = g
                out.append(_pack_dense(pad.to(dev), torch.tensor(sizes[a:a + _CHUNK]), what, a))
            return torch.cat(out)

        if seconds is not None:
            seconds = [adjacency(g, 'seconds', k) for k, g in enumerate(seconds)]
            if [g.shape[0] for g in seconds] != sizes:
                raise ValueError('seconds: the second sides must have the sizes of the graphs')
            seconds = words(seconds, 'seconds')
        return cls.from_bits(words(graphs, 'graphs'), None if min(sizes) == N else sizes, seconds, device=dev, **settings)

    @classmethod
    def from_reference_dataset(cls, path_or_list, noisy=False, **settings):
        """The reference's dataset file (``Base_Generator.load_dataset``: the .pkl that torch.save wrote of a list of (B, B_noise)
        tensor representations; read with ``torch.load(weights_only=True)``), or such a list.  The pairs are stored as they are
        (paired); noisy=True keeps the parents only and the copies are made on the device.  settings: as from_list."""
        data = path_or_list
        if not isinstance(data, (list, tuple)):
            data = torch.load(data, map_location='cpu', weights_only=True)
        data = list(data)
        if not data or any(not isinstance(e, (list, tuple)) or len(e) != 2 for e in data):
            raise ValueError('a reference dataset is a non-empty list of (B, B_noise) pairs')
        return cls.from_list([e[0] for e in data], None if noisy else [e[1] for e in data], **settings)

    # ------------------------------------------------------------------ save / load
    def save(self, path):
        """Plain tensors and settings (read back by `load` with weights_only=True)."""
        torch.save({'format': _FORMAT, 'parents': self.parents.cpu(), 'sizes': None if self.sizes is None else self.sizes.cpu(),
                    'seconds': None if self.seconds is None else self.seconds.cpu(), 'noise_model': self.noise_model,
                    'noise': self.noise, 'seed': self.seed, 'edge_density': self.edge_density}, path)

    @classmethod
    def load(cls, path, device=None):
        """The store `save` wrote, on `device` (None: the CPU); its words are validated again."""
        d = torch.load(path, map_location='cpu', weights_only=True)
        if not isinstance(d, dict) or d.get('format') != _FORMAT:
            raise ValueError('%s is not a saved PairStore' % (path,))
        return cls.from_bits(d['parents'], d['sizes'], d['seconds'], noise_model=d['noise_model'], noise=d['noise'], seed=d['seed'],
                             edge_density=d['edge_density'], device=device if device is not None else 'cpu')

    def to(self, device):
        """The same store on another device (the words are shared when it is this one)."""
        other = object.__new__(type(self))
        other.__dict__.update(self.__dict__)
        other.device = torch.device(device)
        other.parents = self.parents.to(other.device)
        other.sizes = None if self.sizes is None else self.sizes.to(other.device)
        other.seconds = None if self.seconds is None else self.seconds.to(other.device)
        return other

    # ------------------------------------------------------------------ batches
    def gather_args(self, first, index, levels, level, bits1, bits2, nvalid):
        """The fgnn_pairstore_args of one launch into the given outputs (the tensors must outlive the launch)."""
        p, noise = self.edge_density, float(self.noise)
        a = _lib.PairstoreArgs()
        a.seed, a.first, a.M, a.B, a.N = int(self.seed), first, self.num_examples, bits1.shape[0], self.n_vertices
        a.noise_model, a.emax = NOISE_MODELS[self.noise_model], self.max_edges
        a.thr_noise1, a.thr_noise2 = threshold(noise), threshold(p * noise / (1 - p))
        a.parents = self.parents.data_ptr()
        a.sizes = self.sizes.data_ptr() if self.sizes is not None else None
        a.seconds = self.seconds.data_ptr() if self.seconds is not None else None
        a.index = index.data_ptr() if index is not None else None
        if level is not None:
            a.level_thr, a.level, a.K = levels.table.data_ptr(), level.data_ptr(), len(levels)
        a.bits1, a.bits2 = bits1.data_ptr(), bits2.data_ptr()
        a.nvalid = nvalid.data_ptr() if nvalid is not None else None
        return a

    def bits(self, first=None, count=None, index=None, permute=False, levels=None, level=None):
        """``PairGenerator.bits`` over the stored examples: first .. first + count - 1 (inside the store), or index[0], index[1], ...
        (never read on the host) -> (bits1, bits2, nvalid): (count, N, ceil(N/32)) int32 device tensors and the (count,) int32
        vertex counts (None for a constant-size store); one launch on the current stream.  An index outside [0, num_examples)
        or a level outside the table is a caller error that gives the empty graph and nvalid = 0.  permute=True: bits2 is
        relabelled by the planted permutation of (seed, example) and (bits1, bits2, nvalid, labels) is returned.  levels, level:
        as in ``PairGenerator.bits``; refused by a paired store, whose second sides are not made here.  Every argument is checked
        before the device is."""
        first, count, index = self._selection(first, count, index)
        if self.paired and (levels is not None or level is not None):
            raise ValueError('levels= on a paired store: its second sides are stored, not made at a noise level')
        level = self._level(levels, level, count)
        if index is None and first + count > self.num_examples:
            raise ValueError('examples %d .. %d lie outside the store (num_examples %d)' % (first, first + count - 1, self.num_examples))
        self._check_noise()
        self._need_gpu()
        N = self.n_vertices
        W = (N + 31) // 32
        with torch.cuda.device(self.device):
            b1 = torch.empty(count, N, W, dtype=torch.int32, device=self.device)
            b2 = torch.empty(count, N, W, dtype=torch.int32, device=self.device)
            nv = None if self.constant_n_vertices else torch.empty(count, dtype=torch.int32, device=self.device)
            if count:
                _lib.call('fgnn_pairstore_gather', C.byref(self.gather_args(first, index, levels, level, b1, b2, nv)), _lib.stream_ptr())
            if permute:
                return self._planted(b1, b2, nv, first, count, index)
        return b1, b2, nv
