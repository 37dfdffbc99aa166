"""What the two fused engines share: the host bookkeeping around their launch sequences.

``engine.FgnnEngine`` (fp32 storage) and ``engine16.FgnnEngineBF16`` (bf16 storage) run the same step with two kernel sets.
The kernels, their argument records and the order of the launches belong to each engine; the state of a step, the scoring /
loss launches on the fp32 embeddings, the operand packing jobs, the backward workspace and the ONE gradient reduction at the
end are the same code for both and live here.  Nothing in this module asks which engine it serves: where the two differ by
a name, the subclass states it as an attribute; where they differ by an argument list, the subclass keeps its own method.
"""
import ctypes as C

import torch

from . import _lib


class EngineBase:
    """State and precision-independent methods of an engine for a fixed (G, N) problem on the current device.

    A subclass provides: ``ldp`` and ``tpg`` (its slab geometry), ``_act()`` (a new activation slab in its storage type),
    ``_packs`` (the operand images of its kernel set), ``_pack_entry`` (the packing entry point), ``GN_FINALIZE`` /
    ``_gn_args`` (its GraphNorm finalize launches), ``embed()`` and ``backward_from_dE()`` (its two launch sequences)."""

    def __init__(self, layout, G, N, device, ragged):
        self.layout = layout
        self.G, self.N = G, N
        self.B = G // 2
        self.device = device
        f32 = dict(dtype=torch.float32, device=device)
        self.nrm = {(k, j): torch.empty(G * 32 * 4, **f32) for k in range(1, layout.num_blocks + 1) for j in (1, 2, 3)}
        self.E = torch.empty(G, 32, N, **f32)
        self.idx = torch.empty(G, 32, N, dtype=torch.int32, device=device)
        self.scores = torch.empty(self.B, N, N, **f32)
        self.lse = torch.empty(self.B, N, **f32)
        self.score_blocks = _lib.load().fgnn_score_row_blocks(self.B, N)      # row blocks per pair of the scoring kernel
        self.pair_loss = torch.empty(self.B * self.score_blocks, **f32)
        self.loss = torch.empty(1, **f32)
        self.nvalid = torch.empty(G, dtype=torch.int32, device=device) if ragged else None
        self._nvalid_own = self.nvalid      # the engine's own buffer; an int32 device tensor handed in is used in place (no copy launch)
        # ragged batches: work-balanced tile ranges of the MLP kernels (padding-only tiles are stepped over)
        self.ranges = (torch.empty(_lib.FGNN_RANGE_WG + 1, dtype=torch.int32, device=device)
                       if ragged and self.SKIP_PADDING_TILES else None)
        # backward workspace (allocated lazily)
        self._bwd = None
        self._struct = None
        self.xbits = None         # bit-packed adjacency input (embed(..., bits=...))
        self.decisions = None       # test-only, see export_decisions()
        # the state of a step: set by forward(), read by backward() and grad_finalize()
        self.total_nodes = None
        self._loss_pending = False
        self._loss_target = None
        self._loss_scale_dev = None      # 1 / sum(n) as a device scalar: assigned by the caller that keeps the normaliser on the device
        self.labels = None               # (B, N) int32 targets of the cross-entropy (forward(labels=...)); None: the identity
        self.weights = None              # (B,) fp32 per-pair loss weights (forward(weights=...)); None: the unweighted launches

    # ------------------------------------------------------------------ helpers
    def _nv(self):
        return _lib.ptr(self.nvalid) if self.nvalid is not None else None

    def _w(self, params, off):
        return params.data_ptr() + 4 * off

    def _pack_jobs(self, params, chunk):
        L = self.layout
        jobs = (_lib.PackJob * len(chunk))()
        for i, ((kind, k, which), (knd, ca, cb, nmlp, buf)) in enumerate(chunk):
            jobs[i].kind, jobs[i].ca, jobs[i].cb, jobs[i].depth, jobs[i].nmlp = knd, ca, cb, L.depth, nmlp
            js = (1, 2) if which == 12 else (which,)
            for m, j in enumerate(js):
                rec = L.mlp[(k, j)]
                for l in range(L.depth):
                    jobs[i].W[m][l] = self._w(params, rec['w'][l])
                    jobs[i].bias[m][l] = self._w(params, rec['b'][l])
            jobs[i].out = buf.data_ptr()
        return jobs

    def pack_operands(self, params):
        """Pack the LDS operand images of all MLP launches of one step (one small launch)."""
        items = list(self._packs.items())
        for lo in range(0, len(items), _lib.MAX_PACK_JOBS):
            chunk = items[lo:lo + _lib.MAX_PACK_JOBS]
            _lib.call(self._pack_entry, self._pack_jobs(params, chunk), len(chunk), _lib.stream_ptr())

    def _gn_finalize(self, params, k, js):
        """GraphNorm records of the MLPs `js` of block k from the tile statistics their forward launch left in part / cnt."""
        L = self.layout
        st = _lib.stream_ptr()
        if len(js) == 2:
            r0, r1 = L.mlp[(k, js[0])], L.mlp[(k, js[1])]
            _lib.call(self.GN_FINALIZE[1], _lib.ptr(self.part[0]), _lib.ptr(self.part[1]), _lib.ptr(self.cnt),
                      C.c_void_p(self._w(params, r0['gn_w'])), C.c_void_p(self._w(params, r1['gn_w'])), self._nv(),
                      self.G, 32, self.N, *self._gn_args, _lib.ptr(self.nrm[(k, js[0])]), _lib.ptr(self.nrm[(k, js[1])]), st)
        else:
            rec = L.mlp[(k, js[0])]
            _lib.call(self.GN_FINALIZE[0], _lib.ptr(self.part[0]), _lib.ptr(self.cnt),
                      C.c_void_p(self._w(params, rec['gn_w'])), self._nv(), self.G, 32, self.N, *self._gn_args,
                      _lib.ptr(self.nrm[(k, js[0])]), st)

    def _adopt_nvalid(self, nvalid):
        """The vertex counts of a ragged batch: an int32 device tensor of G entries is read in place, anything else is copied."""
        if (nvalid is None) != (self.nvalid is None):
            raise RuntimeError('%s: ragged flag and nvalid argument disagree' % type(self).__name__)
        if nvalid is not None:
            if nvalid.dtype == torch.int32 and nvalid.is_cuda and nvalid.is_contiguous() and nvalid.numel() == self.G:
                self.nvalid = nvalid            # read in place by every kernel of the step (a copy node costs 4.6 + 8.6 us of gap in a replayed graph)
            else:
                self._nvalid_own.copy_(nvalid.to(torch.int32))
                self.nvalid = self._nvalid_own

    def _adopt_labels(self, labels):
        """labels= of forward / step: None (the identity: the label-less launches), or what metrics.labels_tensor takes.  A (B, N)
        int32 contiguous tensor on the engine's device is read in place by the two score launches, like nvalid."""
        if labels is not None:
            from .metrics import labels_tensor
            labels = labels_tensor(labels, self.B, self.N, self.device)
        self.labels = labels

    def _adopt_weights(self, weights):
        """weights= of forward / step: None (the unweighted launches), or (B,) per-pair weights w_b >= 0.  A contiguous fp32 tensor
        on the engine's device is read in place by the weighted loss sum and the weighted score backward, like nvalid and labels."""
        if weights is not None:
            if not torch.is_tensor(weights):
                weights = torch.as_tensor(weights, dtype=torch.float32)
            if tuple(weights.shape) != (self.B,):
                raise ValueError('%s: weights must have shape (%d,), got %s' % (type(self).__name__, self.B, tuple(weights.shape)))
            if weights.dtype != torch.float32 or weights.device != torch.device(self.device) or not weights.is_contiguous():
                weights = weights.to(device=self.device, dtype=torch.float32).contiguous()
        self.weights = weights

    def _check_bits(self, bits):
        """bits: (G, N, ceil(N/32)) contiguous 32-bit words of the bit-packed adjacency on the GPU."""
        words = (self.N + 31) // 32
        if tuple(bits.shape) != (self.G, self.N, words) or bits.dtype not in (torch.int32, torch.uint32) \
                or not bits.is_contiguous() or bits.device.type != 'cuda':
            raise RuntimeError('%s.embed: expected contiguous 32-bit words %s on the GPU, got %s %s'
                               % (type(self).__name__, (self.G, self.N, words), tuple(bits.shape), bits.dtype))

    def _check_spectral(self, x, bits, spectral):
        """spectral=(bits, n_powers) of embed / forward / step: the stacked (G, N, ceil(N/32)) bit words whose spectral features
        L, L^2, ..., L^n_powers are block 1's input (csrc/spectral.hip) -> (bits, n_powers), checked.  Replaces x and bits=."""
        who = type(self).__name__
        if x is not None or bits is not None:
            raise RuntimeError('%s.embed: pass x, bits= or spectral=, not two of them' % who)
        try:
            sbits, n_powers = spectral
            n_powers = int(n_powers)
        except (TypeError, ValueError):
            raise RuntimeError('%s.embed: spectral= takes (bits, n_powers), got %r' % (who, spectral)) from None
        if self.struct1:
            raise RuntimeError("%s.embed: spectral= runs the generic block 1; this engine was built with block1='structured', which "
                               'serves the 2-channel tensor representation of bits= only' % who)
        if not 1 <= n_powers <= _lib.FGNN_SPECTRAL_MAX_POWERS:
            raise RuntimeError('%s.embed: spectral= takes 1 to %d powers, got %d' % (who, _lib.FGNN_SPECTRAL_MAX_POWERS, n_powers))
        if self.N > _lib.FGNN_SPECTRAL_MAX_N:
            raise RuntimeError('%s.embed: spectral= handles N <= %d (got %d)' % (who, _lib.FGNN_SPECTRAL_MAX_N, self.N))
        self._check_spectral_channels(n_powers)
        self._check_bits(sbits)
        return sbits, n_powers

    # ------------------------------------------------------------------ block 1 on its structured input (csrc/block1_struct.hip)
    def _struct_ws(self):
        if self._struct is None:
            lib = _lib.load()
            f32 = dict(dtype=torch.float32, device=self.device)
            self._struct = {'tab': torch.empty(lib.fgnn_block1_struct_table_floats(self.N), **f32),
                            'ws': torch.empty(lib.fgnn_block1_struct_ws_floats(self.G, self.N), **f32)}
        return self._struct

    def _w3(self, params, j):
        rec = self.layout.mlp[(1, j)]
        return ((C.c_void_p * 3)(*[self._w(params, o) for o in rec['w']]), (C.c_void_p * 3)(*[self._w(params, o) for o in rec['b']]))

    # ------------------------------------------------------------------ forward
    def forward(self, params, x=None, nvalid=None, total_nodes=None, defer_loss=False, loss_out=None, bits=None, labels=None, weights=None,
                spectral=None, **embed_kw):
        """Siamese forward on the stacked batch x = cat(x1, x2) (or its bit-packed adjacency, see embed): returns
        (scores, loss).
        labels: (B, N) integer tensor, labels[b, i] = the column row i of pair b should match (planted.py; -1 in the padding):
        the cross-entropy is taken against them instead of the identity, and the following backward()
        differentiates that loss.  A live row whose label lies outside [0, n_b) has no target: no loss, no gradient.  The
        normaliser stays the node count.  None: the label-less launches, as before.
        weights: (B,) fp32 per-pair loss weights w_b >= 0: loss = sum over the pairs with w_b != 0 of
        w_b * CE_b, one fgnn_pair_loss_w launch right after the scoring (the gradient-finalize launch carries no loss job then,
        whatever defer_loss says), and the following backward() differentiates that loss.  A pair with w_b == 0 is switched off by a
        select: NaN or inf in its scores reach neither loss nor gradient.  The weights carry the reduction, so total_nodes must be
        left out or 1: the normaliser D of a reduction (fgnn_pair_weights) is applied by the caller (FgnnTrainer: as Adam's gradient
        scale, after the all-reduce).  None: the launches of the unweighted step, unchanged.
        spectral: (bits, n_powers) -- block 1's input is the spectral features L, ..., L^n_powers of the stacked bit words, computed
        by the engine (see embed); replaces x and bits=.  None: the launches of a forward without it, unchanged.
        defer_loss: leave the final sum of the per-pair losses to the gradient-finalize launch of the
        following backward() (one launch less per training step); `loss` is valid after that.
        embed_kw: keywords of the engine's own embed()."""
        self._adopt_labels(labels)
        self._adopt_weights(weights)
        if self.weights is not None:
            if total_nodes is not None and float(total_nodes) != 1.0:
                raise ValueError('%s.forward: weights carry the reduction; total_nodes must be None or 1 (got %r)'
                                 % (type(self).__name__, total_nodes))
            total_nodes = 1.0
        if spectral is not None:
            embed_kw['spectral'] = spectral
        self.embed(params, x, nvalid, bits=bits, **embed_kw)
        B, N = self.B, self.N
        st = _lib.stream_ptr()
        e1, e2 = self.E[:B], self.E[B:]
        if total_nodes is None:
            total_nodes = B * N if nvalid is None else int(nvalid[:B].sum().item())
        self.total_nodes = float(total_nodes)
        if self.labels is None:
            _lib.call('fgnn_score_ce_fwd_blocks', _lib.ptr(e1), _lib.ptr(e2), self._nv(), B, 32, N, self.score_blocks,
                      _lib.ptr(self.scores), _lib.ptr(self.lse), _lib.ptr(self.pair_loss), st)
        else:
            _lib.call('fgnn_score_ce_fwd_blocks_labels', _lib.ptr(e1), _lib.ptr(e2), self._nv(), _lib.ptr(self.labels), B, 32, N,
                      self.score_blocks, _lib.ptr(self.scores), _lib.ptr(self.lse), _lib.ptr(self.pair_loss), st)
        self._loss_pending = bool(defer_loss) and self.weights is None
        self._loss_target = self.loss if loss_out is None else loss_out     # 1-element fp32 device tensor
        if self.weights is not None:
            _lib.call('fgnn_pair_loss_w', _lib.ptr(self.pair_loss), self.score_blocks, _lib.ptr(self.weights), B,
                      _lib.ptr(self._loss_target), st)
        elif not defer_loss:
            _lib.call('fgnn_sum_scale', _lib.ptr(self.pair_loss), B * self.score_blocks, 1, 1.0 / self.total_nodes,
                      _lib.ptr(self._loss_target), st)
        return self.scores, self._loss_target

    # ------------------------------------------------------------------ backward
    def _partial_rows(self):
        """Rows of every weight-gradient partial buffer: one per workgroup of the MLP backward kernels."""
        return _lib.load().fgnn_mlp_bwd_num_workgroups()

    def _alloc_bwd(self):
        if self._bwd is not None:
            return self._bwd
        f32 = dict(dtype=torch.float32, device=self.device)
        act, nwg = self._act, self._partial_rows()
        L = self.layout
        keys = [(k, j) for k in range(1, L.num_blocks + 1) for j in (1, 2, 3)]
        self._bwd = {
            'dE': torch.empty(self.G, 32, self.N, **f32),
            'dy': [act(), act()],
            'dmult': act(), 'dy1': act(), 'dy2': act(),
            # per-MLP GraphNorm-backward sums and workgroup partials live until the final
            # fgnn_grad_finalize launch
            's12': {kj: torch.empty(self.G * 32 * 2, **f32) for kj in keys},
            # (the structured block 1 writes one row per graph: the other rows of its two buffers stay zero)
            'wpart': {kj: torch.empty(nwg * L.mlp[kj]['count'], **f32)
                      for kj in keys},
            's12part': torch.empty(self.G * self.tpg * 32 * 2, **f32),
            'coef': [torch.empty(self.G * 32 * 4, **f32) for _ in range(3)],
            'nwg': nwg,
            'gscale': torch.empty(1, **f32),
        }
        return self._bwd

    def backward(self, params, grads, grad_scale=1.0, gscale_dev=None, **kw):
        """Backward of loss*grad_scale after forward(); fills the flat `grads` buffer (the fp32 engine's finalize=False: everything
        but the last launch, see its backward_from_dE).
        After forward(labels=...) the gradient is that of the labelled loss (the labels are read again, in place); after
        forward(weights=...) that of the weighted loss (fgnn_score_ce_bwd_w, labelled or not; the weights are read again, in place).
        gscale_dev: a 1-element fp32 DEVICE tensor that holds grad_scale / total_nodes (replaces both): the normaliser of a ragged
        batch then never visits the host, and a captured step stays valid when the next batch has another node count.
        kw: keywords of the engine's own backward_from_dE() (finalize=, hook=)."""
        W = self._alloc_bwd()
        B, N = self.B, self.N
        st = _lib.stream_ptr()
        gs_t = W['gscale']
        if gscale_dev is not None:
            gs_t = gscale_dev                  # read in place (a 1-element fp32 device tensor; no copy launch)
        else:
            self._set_gscale(grad_scale / self.total_nodes)
        e1, e2 = self.E[:B], self.E[B:]
        if self.weights is not None:
            _lib.call('fgnn_score_ce_bwd_w', _lib.ptr(e1), _lib.ptr(e2), _lib.ptr(self.scores), _lib.ptr(self.lse), self._nv(),
                      _lib.ptr(self.labels), _lib.ptr(self.weights), _lib.ptr(gs_t), B, 32, N, _lib.ptr(W['dE'][:B]),
                      _lib.ptr(W['dE'][B:]), st)
        elif self.labels is None:
            _lib.call('fgnn_score_ce_bwd', _lib.ptr(e1), _lib.ptr(e2), _lib.ptr(self.scores), _lib.ptr(self.lse),
                      self._nv(), _lib.ptr(gs_t), B, 32, N, _lib.ptr(W['dE'][:B]), _lib.ptr(W['dE'][B:]), st)
        else:
            _lib.call('fgnn_score_ce_bwd_labels', _lib.ptr(e1), _lib.ptr(e2), _lib.ptr(self.scores), _lib.ptr(self.lse),
                      self._nv(), _lib.ptr(self.labels), _lib.ptr(gs_t), B, 32, N, _lib.ptr(W['dE'][:B]), _lib.ptr(W['dE'][B:]), st)
        return self.backward_from_dE(params, grads, W['dE'], **kw)

    def _set_gscale(self, gs):
        W = self._bwd
        if W.get('gscale_value') != gs:        # a 1-element fill kernel per step otherwise
            W['gscale'].fill_(gs)
            W['gscale_value'] = gs

    def grad_finalize(self, grads, rows=None, graphs=None, pair_rows=None):
        """ONE launch: reduce the workgroup partials + GraphNorm affine gradients of all MLPs (and the deferred loss sum).
        rows / graphs / pair_rows: FgnnEngineDual reduces the partials of both of its engines at once -- their wpart, s12,
        nrm and pair_loss buffers are consecutive halves of one allocation, this engine holding the first."""
        L = self.layout
        W = self._bwd
        K = L.num_blocks
        st = _lib.stream_ptr()
        keys = [(k, j) for k in range(1, K + 1) for j in (1, 2, 3)]
        if self._loss_pending:
            keys.append('loss')
            self._loss_pending = False
        for lo in range(0, len(keys), _lib.MAX_GRAD_JOBS):
            chunk = keys[lo:lo + _lib.MAX_GRAD_JOBS]
            jobs = (_lib.GradJob * len(chunk))()
            for i, kj in enumerate(chunk):
                if kj == 'loss':        # loss = sum(pair_loss) / nodes rides along as one more reduction job
                    jobs[i].wpart = self.pair_loss.data_ptr()
                    jobs[i].count = 1
                    jobs[i].out = self._loss_target.data_ptr()
                    jobs[i].rows = self.B * self.score_blocks if pair_rows is None else pair_rows
                    jobs[i].scale = 1.0 / self.total_nodes
                    if self._loss_scale_dev is not None:       # 1 / sum(n) as a device scalar (forward(inv_nodes_dev=...))
                        jobs[i].scale_dev = self._loss_scale_dev.data_ptr()
                    continue
                rec = L.mlp[kj]
                jobs[i].wpart = W['wpart'][kj].data_ptr()
                jobs[i].count = rec['count']
                if kj in ((1, 1), (1, 2)) and W.get('struct_rows', 0):
                    jobs[i].rows = W['struct_rows']         # block 1 on its structured input: the rows its backward wrote
                jobs[i].out = grads.data_ptr() + 4 * rec['off']
                jobs[i].s12 = W['s12'][kj].data_ptr()
                jobs[i].nrm = self.nrm[kj].data_ptr()
                jobs[i].dgn_w = grads.data_ptr() + 4 * rec['gn_w']
                jobs[i].dgn_b = grads.data_ptr() + 4 * rec['gn_b']
            _lib.call('fgnn_grad_finalize', jobs, len(chunk), W['nwg'] if rows is None else rows,
                      self.G if graphs is None else graphs, 32, st)
        return grads

    def step(self, params, grads, x=None, nvalid=None, total_nodes=None, loss_out=None, bits=None, labels=None, weights=None,
             spectral=None):
        """One training step's model work: forward + loss + backward.  (x / bits / the bit words of spectral= / an int32 device nvalid /
        int32 device labels / fp32 device weights are read in place by both passes: see embed() and forward().)"""
        wkw = {} if weights is None else {'weights': weights}
        if spectral is not None:
            wkw['spectral'] = spectral
        scores, loss = self.forward(params, x, nvalid, total_nodes, defer_loss=True, loss_out=loss_out, bits=bits, labels=labels, **wkw)
        self.backward(params, grads)
        return scores, loss

    # ------------------------------------------------------------------ inspection (tests / module API)
    def export_decisions(self, on=True):
        """Test-only (tests/test_gpu_grad_pinned.py): from the next forward on, every fgnn_mlp_fwd / fgnn_mlp_fwd16 launch is followed
        by its decision-exporting twin (fgnn_debug_mlp_fwd_masks / fgnn_debug_mlp_fwd16_masks) and `relu_decisions()` returns the ReLU
        masks the step took; together with self.idx (the arg-max of the pooling) these are ALL the discrete decisions of a step
        (the 16-bit engine: constant-size batches, generic block 1)."""
        self.decisions = {} if on else None
