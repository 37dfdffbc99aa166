"""Minimal data-parallel training step around the fused engine (the Lightning shell of the reference,
models/trainers.py:70-104, is out of scope): forward + loss + backward (HIP), ONE all-reduce (RCCL) of the flat
gradient buffer with the loss sum and the node count riding in its last two floats, fused Adam.

No step reads anything back to the host: the loss normaliser of the concatenated global batch
(toolbox/losses.py:27-34) arrives with the all-reduce and is applied on the device as Adam's gradient scale.
"""
import torch

from . import dp
from .engine import EngineCache, FgnnEngine
from .optim import FlatAdam


class FgnnTrainer:
    ENGINE_CACHE_BYTES = 8 << 30      # workspace budget of the per-shape engine cache (LRU); 288 GB HBM leave room to raise it

    INPUT_CHECK_EVERY = 128     # input_form='tensor_representation': the device verdict is read back on every k-th train_step (0: never)

    def __init__(self, layout, params_flat, lr=1e-3, capture=False, precision='fp32', collective='auto', block1=None,
                 input_form='dense', max_grad_norm=None, skip_nonfinite=False, loss_reduction='mean'):
        """capture=True: constant-shape steps are captured in a HIP graph and replayed -- the launch overhead of ~40 kernels
        per step disappears.  With more than one rank the gradient all-reduce is recorded INSIDE that graph when the backend
        can be captured (RCCL: model work -> all-reduce -> fused Adam is one replay, no host launch on the critical path;
        `allreduce_in_graph` says which form is in use); with gloo it stays an eager call between two captured halves.
        collective='always': issue the all-reduce with a single rank as well (exercises the RCCL path on a one-GPU box).
        precision='bf16': the model work runs on the bf16 kernel set (engine16; the reference's
        pl.Trainer(precision=16), commander_explore.py:120-122); parameters, gradients, Adam state and the collective
        stay fp32.
        block1='structured': batches handed over as bit-packed adjacency (train_step_bits) run block 1 on its structured form
        (csrc/block1_struct.hip); None = the engines' default (FGNN_BLOCK1, 'generic').
        input_form='tensor_representation': the caller states that the dense (B, 2, N, N) batches handed to train_step ARE what the
        reference's loaders yield (loaders/data_generator.py:118-125); train_step then bit-packs them on the device
        (fgnn_pack_adjacency, which also verifies the statement: the verdict is read on the first step of a shape and on every
        INPUT_CHECK_EVERY-th step, and a batch that is not a tensor representation raises) and runs train_step_bits with the structured
        block 1.  'dense' (default): dense batches run the generic kernels, whatever block1 says.
        max_grad_norm / skip_nonfinite: the guarded optimizer step (optim.FlatAdam) -- clip the global L2 norm of the normalised
        gradient with clip_grad_norm_ semantics (Lightning's gradient_clip_val), and drop the whole update when the gradient holds
        an inf or a NaN (what the AMP GradScaler behind pl.Trainer(precision=16) does).  The guard is part of every optimizer
        step: the eager one, the one-graph captured step and the optimizer graph of the gloo fallback; `grad_norm` and
        `skipped_steps` stay on the device and no step reads them.  It runs AFTER the all-reduce, on a buffer that is bit-identical
        on every rank, and its sums have a fixed order, so every rank takes the same clip and skip decision without another
        collective.  The defaults (None, False) leave every launch sequence and captured graph as it was.
        loss_reduction: 'mean' (the sum of the cross-entropies over the node count, toolbox/losses.py:27-34) or 'mean_of_mean' (the
        average over the graphs of the per-graph mean, toolbox/losses.py:14-15; on ragged batches another loss).  'mean_of_mean'
        runs every step as a weighted step: w_b = 1 / n_b, normalised by the number of non-empty pairs of the
        global batch.  With 'mean', a step without weights= and live= issues the launches it always did."""
        if loss_reduction not in ('mean', 'mean_of_mean'):
            raise ValueError('Unknown loss_reduction parameters {}'.format(loss_reduction))
        self.loss_reduction = loss_reduction
        self._pw = {}               # B -> buffers of the eager weighted step
        if input_form not in ('dense', 'tensor_representation'):
            raise ValueError('input_form must be "dense" or "tensor_representation" (got %r)' % (input_form,))
        self.input_form = input_form
        if input_form == 'tensor_representation' and block1 is None:
            block1 = 'structured'
        self._tr = {}               # (B, N) -> staging words of the packed batch
        self._tr_flag = None
        self._tr_calls = 0
        if precision not in ('fp32', 'bf16'):
            raise ValueError('precision must be "fp32" or "bf16" (got %r)' % (precision,))
        self.precision = precision
        self.block1 = block1
        self.layout = layout
        self.params = params_flat
        n = params_flat.numel()
        # [gradients (n) | sum of the pair losses | node count]: the unit of the one all-reduce per step
        self.comm = torch.zeros(n + 2, dtype=torch.float32, device=params_flat.device)
        self.grads = self.comm[:n]
        self._loss_sum = self.comm[n:n + 1]
        self._nodes = self.comm[n + 1:n + 2]
        self.opt = FlatAdam(params_flat, lr=lr, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
        self.capture = capture
        self._engines = EngineCache(self.ENGINE_CACHE_BYTES)
        self._graphs = {}
        if collective not in ('auto', 'always'):
            raise ValueError("collective must be 'auto' or 'always' (got %r)" % (collective,))
        self._force_collective = collective == 'always'
        self.allreduce_in_graph = False
        if dp.world_size() > 1 or self._force_collective:
            # communicator set-up (RCCL: rings over xGMI) happens at the first collective: here, not inside a step or a capture.
            # NOTE: this IS a collective -- with more than one rank every rank must construct its trainers in the same order (a
            # trainer built on rank 0 only, e.g. for evaluation, would wait here for the others: build it before init_process_group
            # or on every rank)
            dp.warm_up_collective(params_flat.device, force=self._force_collective)
            self.allreduce_in_graph = bool(capture) and dp.collective_captures()

    @classmethod
    def from_module(cls, model, lr=None, capture=True, max_grad_norm=None, skip_nonfinite=False):
        """The fused training step for a `Siamese_Node_Exp` built through the reference's own surface
        (models/trainers.py:20-58): the trainer works IN PLACE on the module's flat parameter buffer (a padded 16-bit module: on its
        padded image, see below), so the module (its `state_dict`, its eager forward) always sees the trained weights, and `capture=True` gives a reference user the
        replayed-graph step instead of ~40 host launches per step.  Standard node_embedding graphs only.
        A 16-bit module narrower than the engine (`model.half()` with original_features_num 1 or 3..31, widths below 32) trains on its
        zero-padded image (Network._padded_layout): layout, parameters, Adam moments and checkpoints of the trainer are the padded
        ones -- the padded entries get exact zero gradients and stay zero -- and every step ends with one gather of the trained
        values back into the module's flat buffer (one eager launch after the step, outside a captured graph).  `tr.params` then IS
        the module's padded image (Network._pad['pflat']), which every forward of the module rewrites from the module's own
        parameters: the two agree after every train_step, but a value written into `tr.params` by anything else than a step is lost
        at the module's next forward (load a checkpoint into the MODULE, not into such a trainer).  train_step / eval_step take the
        module's own (B, c, N, N) batches."""
        net = model.node_embedder
        lay = net._standard_layout()
        precision = getattr(net, 'precision', 'fp32')
        pad = net._pad
        if lay is None or (pad is not None and precision != 'bf16'):
            raise RuntimeError('FgnnTrainer.from_module: the module is not a node_embedding graph the fused trainer runs: fp32 needs '
                               'original_features_num 2 or 32 and in_features = out_features = 32; 16-bit (model.half()) takes '
                               'original_features_num, in_features and out_features up to 32; depth_of_mlp = 3 in 16-bit')
        net._bind_flat()
        from .losses import triplet_loss
        loss = getattr(model, 'loss', None)
        rkw = {'loss_reduction': loss.loss_reduction} if isinstance(loss, triplet_loss) else {}
        tr = cls(lay, net._flat if pad is None else net._engine_params(), lr=model.lr if lr is None else lr, capture=capture,
                 precision=precision, input_form=getattr(net, 'input_form', 'dense'), max_grad_norm=max_grad_norm,
                 skip_nonfinite=skip_nonfinite, **rkw)
        if pad is not None:
            tr._module = net
        return tr

    def _sync_module(self):
        """from_module on a padded module: the trained values back into the module's own flat buffer (one gather launch)."""
        net = getattr(self, '_module', None)
        if net is not None:
            torch.index_select(self.params, 0, net._pad['idx'], out=net._flat)

    @property
    def grad_norm(self):
        """0-dim fp64 device tensor: global L2 norm of the last step's normalised gradient, before clipping (guarded trainers)"""
        return self.opt.grad_norm

    @property
    def skipped_steps(self):
        """0-dim int32 device tensor: updates dropped so far because their gradient was not finite (guarded trainers)"""
        return self.opt.skipped_steps

    # ------------------------------------------------------------------ engines: bounded cache keyed on padded shapes
    def _engine(self, G, N, ragged):
        """Engine for (G, N).  Ragged engines are shared between nearby shapes: G is rounded up to a multiple of 4
        graphs (the surplus graphs get nvalid = 0 and cost nothing but their padding tiles), so a stream of ragged
        batches re-uses a handful of workspaces instead of allocating one per (count, nmax); least recently used
        engines are dropped beyond ENGINE_CACHE_BYTES (engine.EngineCache)."""
        def make():
            if self.precision == 'bf16':
                from .engine16 import FgnnEngineBF16
                return FgnnEngineBF16(self.layout, G, N, self.params.device, ragged=ragged, block1=self.block1)
            return FgnnEngine(self.layout, G, N, self.params.device, ragged=ragged, block1=self.block1)
        self._engines.budget = self.ENGINE_CACHE_BYTES
        eng, evicted = self._engines.get((G, N, ragged), make, EngineCache.engine_bytes(G, N, self.layout.num_blocks))
        for g, n, r in evicted:
            self._graphs = {k: v for k, v in self._graphs.items() if not (2 * k[0] == g and k[1] == n and not r)}
        return eng

    # ------------------------------------------------------------------ the one collective + optimizer
    def _reduce_and_update(self, opt_graph=None):
        """all-reduce [grads | loss sum | nodes], then Adam with grad_scale = 1 / global nodes (device side).
        Returns the loss of the global batch as a fresh device scalar."""
        dp.allreduce_sum_(self.comm, force=self._force_collective)
        self.opt.sync_hyper_parameters(grad_scale=None)
        self.opt.set_grad_scale_reciprocal(self._nodes)
        if opt_graph is not None:
            opt_graph.replay()
            self.opt.t += 1
        else:
            self.opt.step_dev(self.grads)
        self._sync_module()
        return (self._loss_sum / self._nodes).reshape(())

    # ------------------------------------------------------------------ per-pair loss weights
    def _weighted(self, weights, live):
        """does this step run the weighted launches?  ('mean' without weights= and live=: no, the step is the one it always was)"""
        return self.loss_reduction != 'mean' or weights is not None or live is not None

    def _user_weights(self, weights, B):
        """weights= of the train steps -> None or a (B,) fp32 device tensor"""
        if weights is None:
            return None
        w = torch.as_tensor(weights, dtype=torch.float32).to(self.params.device).contiguous()
        if tuple(w.shape) != (B,):
            raise ValueError('FgnnTrainer: weights must have shape (%d,), got %s' % (B, tuple(w.shape)))
        return w

    def _set_live(self, buf, live, B):
        """live= of the train steps into the int32[1] device buffer the weight kernel reads: an int (host) or a 1-element device
        tensor; None: B"""
        if torch.is_tensor(live):
            buf.copy_(live.reshape(1))
        else:
            buf.fill_(B if live is None else max(0, min(B, int(live))))

    def _launch_pair_weights(self, nvalid, live_buf, user, B, N, w_out):
        """ONE launch: w_out <- the weights of self.loss_reduction on this rank's pairs, self._nodes <- their normaliser D (the
        all-reduce sums it over the ranks, set_grad_scale_reciprocal applies 1 / D: no further collective)"""
        from . import _lib
        _lib.call('fgnn_pair_weights', _lib.ptr(nvalid), _lib.ptr(live_buf), 1 if self.loss_reduction == 'mean_of_mean' else 0,
                  _lib.ptr(user), B, N, _lib.ptr(w_out), _lib.ptr(self._nodes), _lib.stream_ptr())
        return w_out

    def _pair_weights(self, B, N, nvalid, live, weights):
        """the eager weighted step's weights: (B,) fp32 device tensor; self._nodes holds D afterwards.  nvalid: (B,) or None."""
        pw = self._pw.get(B)
        if pw is None:
            dev = self.params.device
            pw = self._pw[B] = {'w': torch.empty(B, dtype=torch.float32, device=dev), 'live': torch.empty(1, dtype=torch.int32, device=dev)}
        self._set_live(pw['live'], live, B)
        nv = None if nvalid is None else nvalid.to(device=self.params.device, dtype=torch.int32).contiguous()
        return self._launch_pair_weights(nv, pw['live'], self._user_weights(weights, B), B, N, pw['w'])

    # ------------------------------------------------------------------ ragged batches, bucketed by size
    @staticmethod
    def bucket_by_size(sizes, granule=16):
        """Group graph indices by padded size ceil(n / granule) * granule (a batch
        padded to its global Nmax wastes up to (Nmax / n)^2 of the work on the small graphs).
        -> list of (padded_n, [indices]) in increasing size."""
        buckets = {}
        for i, n in enumerate(sizes):
            buckets.setdefault(-(-int(n) // granule) * granule, []).append(i)
        return sorted(buckets.items())

    def prepare_ragged(self, xs, ys, granule=None, labels=None, weights=None):
        """Stage a ragged list of pairs (xs[i], ys[i]: (c0, n_i, n_i) tensors): one stacked, zero-padded
        (2 * pairs, c0, npad, npad) device tensor + vertex counts per size bucket.  This is loader work (pad / stack / copy):
        done once per batch, off the step's critical path.  -> dict for model_step_prepared.
        granule=None: ONE batch padded to its largest graph (rounded up to a multiple of 16) -- since the MLP kernels step over padding tiles this is the
        fastest schedule up to a size spread of about 4x (measured, 8 and 64 pairs with n in [30, 120]: 1.13 / 5.96 ms against
        1.77 / 6.09 ms with buckets of 32); granule=g: one engine pass per size class ceil(n / g) * g (bounded workspace for
        very mixed batches).
        labels: None, or one integer array per pair (labels[i][r] = the vertex of ys[i] that vertex r of xs[i] matches, at most n_i
        entries): they follow their pairs into the buckets as (pairs, npad) int32 tensors, -1 in the padding.
        weights: None, or one loss weight per pair: they follow their pairs as (pairs,) fp32 tensors, 0 for the
        pairs a bucket is filled up with; every bucket then runs the weighted launches."""
        dev = self.params.device
        sizes = [int(x.shape[-1]) for x in xs]
        if labels is not None and len(labels) != len(xs):
            raise ValueError('FgnnTrainer.prepare_ragged: %d label arrays for %d pairs' % (len(labels), len(xs)))
        if weights is not None and len(weights) != len(xs):
            raise ValueError('FgnnTrainer.prepare_ragged: %d weights for %d pairs' % (len(weights), len(xs)))
        if granule is None:
            granule = -(-max(sizes) // 16) * 16        # one bucket; rounded up so that engines are shared between batches
        buckets = []
        for npad, idx in self.bucket_by_size(sizes, granule):
            cnt = -(-len(idx) // 2) * 2                     # pairs rounded up to a multiple of 2 (G to a multiple of 4)
            x = torch.zeros(2 * cnt, xs[0].shape[0], npad, npad, dtype=torch.float32, device=dev)
            for k, i in enumerate(idx):
                n = sizes[i]
                x[k, :, :n, :n] = xs[i]
                x[cnt + k, :, :n, :n] = ys[i]
            ns = [sizes[i] for i in idx] + [0] * (cnt - len(idx))
            nv = torch.tensor(ns * 2, dtype=torch.int32, device=dev)
            buckets.append({'npad': npad, 'idx': idx, 'pairs': cnt, 'x': x, 'nvalid': nv})
            if weights is not None:
                buckets[-1]['weights'] = torch.tensor([float(weights[i]) for i in idx] + [0.0] * (cnt - len(idx)), dtype=torch.float32,
                                                      device=dev)
            if labels is not None:
                import numpy as np
                from .metrics import labels_tensor
                buckets[-1]['labels'] = labels_tensor([labels[i] for i in idx] + [np.zeros(0, dtype=np.int64)] * (cnt - len(idx)), cnt, npad, dev)
        return {'sizes': sizes, 'buckets': buckets}

    def model_step_prepared(self, batch, total_nodes=None, want_scores=True):
        """Forward + loss + backward of a batch staged by prepare_ragged: one fused-engine pass per size bucket;
        gradients and losses of the buckets are summed.
        total_nodes=None: normalised by this batch's own node count (the single-process result);
        total_nodes=1.0: the UN-normalised sums (the data-parallel step normalises after its all-reduce).
        A batch staged with weights: every bucket's loss and gradient are the weighted sums (the weights carry the reduction, so
        total_nodes is not applied to them).
        Returns (loss, [scores_i of shape (n_i, n_i)] or None); self.grads holds the gradient sum."""
        sizes = batch['sizes']
        total = float(sum(sizes)) if total_nodes is None else float(total_nodes)
        loss = torch.zeros(1, dtype=torch.float32, device=self.params.device)
        scores = [None] * len(sizes) if want_scores else None
        first = True
        for b in batch['buckets']:
            eng = self._engine(2 * b['pairs'], b['npad'], True)
            # the first bucket writes self.grads, the others go through the scratch vector and are added
            dst = self.grads if first else self._grad_tmp()
            kw = {'labels': b['labels']} if b.get('labels') is not None else {}
            if b.get('weights') is not None:
                kw['weights'] = b['weights']
            sc, l = eng.step(self.params, dst, b['x'], nvalid=b['nvalid'], total_nodes=1.0 if 'weights' in kw else total, **kw)
            if not first:
                self.grads += dst
            first = False
            loss = loss + l
            if want_scores:
                for k, i in enumerate(b['idx']):
                    scores[i] = sc[k, :sizes[i], :sizes[i]].clone()
        return loss.reshape(()), scores

    def _grad_tmp(self):
        if getattr(self, '_gtmp', None) is None:
            self._gtmp = torch.empty_like(self.grads)
        return self._gtmp

    def model_step_ragged(self, xs, ys, granule=None, total_nodes=None, labels=None, weights=None):
        """prepare_ragged + model_step_prepared in one call.  Returns (loss, [scores_i of shape (n_i, n_i)])."""
        return self.model_step_prepared(self.prepare_ragged(xs, ys, granule, labels, weights), total_nodes)

    def ragged_weights(self, sizes, weights=None, live=None):
        """The per-pair weights and the normaliser D of self.loss_reduction for a list of pairs of the given sizes, on the host (where
        the sizes already are): what fgnn_pair_weights computes on the device.  weights: optional per-pair factors; live: the pairs
        from position `live` on are switched off (None: all count).  -> ([w_i], D)"""
        import numpy as np
        n = len(sizes)
        live = n if live is None else max(0, min(n, int(live)))
        u = np.ones(n, dtype=np.float32) if weights is None else np.asarray(weights, dtype=np.float32).reshape(n)
        w, D = np.zeros(n, dtype=np.float32), 0.0
        for i, size in enumerate(sizes):
            if i >= live or (self.loss_reduction == 'mean_of_mean' and size <= 0):
                continue
            if self.loss_reduction == 'mean_of_mean':
                w[i] = np.float32(1.0 / size) * u[i]
                D += float(u[i])
            else:
                w[i] = u[i]
                D += float(size) * float(u[i])
        return [float(v) for v in w], D

    def train_step_ragged(self, xs, ys, granule=None, labels=None, weights=None, live=None):
        """labels: per-pair integer arrays (prepare_ragged): the loss is the cross-entropy against them (train_step).
        weights, live: see train_step; the per-bucket weights are built on the host (ragged_weights)."""
        sizes = [int(x.shape[-1]) for x in xs]
        if self._weighted(weights, live):
            w, D = self.ragged_weights(sizes, weights, live)
            loss, scores = self.model_step_ragged(xs, ys, granule, total_nodes=1.0, labels=labels, weights=w)
        else:
            D = float(sum(sizes))
            loss, scores = self.model_step_ragged(xs, ys, granule, total_nodes=1.0, labels=labels)
        self._loss_sum.copy_(loss.reshape(1))
        self._nodes.fill_(D)
        return self._reduce_and_update(), scores

    # ------------------------------------------------------------------ captured constant-shape step
    def _captured_step(self, x1, x2, bits=False, labels=None, weights=None, live=None, weighted=False, spectral=None):
        """bits: x1, x2 are (B, N, ceil(N / 32)) int32 words of bit-packed adjacency instead of (B, c0, N, N) tensors.
        spectral: None, or n_powers -- x1, x2 are bit words as well, and the step takes their spectral features as its input
        (engine.step(spectral=...)): a graph of its own, key (B, N, 'spectral', n_powers); its static input is the stacked words, as
        for 'bits', and the feature launch rides inside the graph.
        labels: (B, N) int32 device tensor or None.  A labelled step is a graph of its own (the key says which): its labels live in
        a static buffer that every call copies into, like xs, so one trainer can hold and alternate both.
        weighted (weights: (B,) fp32 device tensor or None; live: int, 1-element device tensor or None): the weighted step is a graph
        of its own as well (key: 'weights').  It holds the fgnn_pair_weights launch; the caller's weights (None: ones) and live
        (None: B) live in static device buffers, so ONE graph serves every step of an epoch, the short last one included."""
        B, N = x1.shape[0], x1.shape[-2 if (bits or spectral is not None) else -1]
        world = dp.world_size()
        key = (B, N, 'spectral', spectral) if spectral is not None else (B, N, 'bits') if bits else (B, N)
        if labels is not None:
            key = key + ('labels',)
        if weighted:
            key = key + ('weights',)
        st = self._graphs.get(key)
        if st is None:
            eng = self._engine(2 * B, N, False)
            xs = torch.cat([x1, x2]).contiguous().clone()
            lab = None if labels is None else labels.clone()
            lkw = {} if lab is None else {'labels': lab}
            wst = None
            if weighted:
                dev = self.params.device
                wst = {'user': torch.ones(B, dtype=torch.float32, device=dev), 'live': torch.full((1,), B, dtype=torch.int32, device=dev),
                       'w': torch.zeros(B, dtype=torch.float32, device=dev)}
                lkw['weights'] = wst['w']
            if spectral is not None:
                lkw['spectral'] = (xs, spectral)
            model = ((lambda: eng.step(self.params, self.grads, None, total_nodes=1.0, loss_out=self._loss_sum, **lkw)) if spectral is not None else
                     (lambda: eng.step(self.params, self.grads, None, total_nodes=1.0, loss_out=self._loss_sum, bits=xs, **lkw)) if bits else
                     (lambda: eng.step(self.params, self.grads, xs, total_nodes=1.0, loss_out=self._loss_sum, **lkw)))
            if weighted:
                def step():
                    self._launch_pair_weights(None, wst['live'], wst['user'], B, N, wst['w'])
                    return model()
            else:
                step = model
            self.opt.sync_hyper_parameters(grad_scale=None)
            # two eager steps on a side stream (allocations, kernel attributes); they do not touch the optimizer
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            t0 = self.opt.t
            g_opt = None
            exchange = world > 1 or self._force_collective

            def capture_model():
                g = torch.cuda.CUDAGraph()
                # (a collective inside the capture: 'thread_local', so that the process group's watchdog thread cannot invalidate it)
                with torch.cuda.graph(g, capture_error_mode='thread_local' if (exchange and self.allreduce_in_graph) else 'global'):
                    sc, _ = step()
                    if not exchange or self.allreduce_in_graph:
                        # nothing to exchange, or the ONE collective rides in the graph: the whole step is one replay
                        if exchange:
                            dp.allreduce_sum_(self.comm, force=self._force_collective)
                        self.opt.set_grad_scale_reciprocal(self._nodes)
                        self.opt.step_dev(self.grads)
                return g, sc
            if exchange and self.allreduce_in_graph:
                # The collective may fail to capture on ONE rank only (a torch / RCCL build that cannot record it, a watchdog event
                # query at the wrong moment); a rank that fell back alone would then wait in an eager all-reduce that the others never
                # issue.  So the ranks AGREE: one eager flag all-reduce per captured shape (set-up, not a step collective); if any
                # rank failed, all of them use the two-graph form (model work | eager all-reduce | optimizer).
                try:
                    g_model, scores = capture_model()
                    failed = 0.0
                except RuntimeError as e:    # a capture failure takes the fallback; anything else (argument errors, OOM, ...) is a real error
                    msg = str(e).lower()
                    if not any(w in msg for w in ('captur', 'graph', 'nccl', 'rccl')):
                        raise
                    import warnings
                    warnings.warn('FgnnTrainer: the gradient all-reduce could not be recorded into the step graph on rank %d (%s); every '
                                  'rank falls back to model graph | eager all-reduce | optimizer graph' % (torch.distributed.get_rank() if torch.distributed.is_initialized() else 0, e))
                    self.capture_fallback_reason = str(e)
                    torch.cuda.synchronize()
                    g_model, failed = None, 1.0
                flag = torch.tensor([failed], dtype=torch.float32, device=self.params.device)
                dp.allreduce_sum_(flag, force=self._force_collective)
                if flag.item() > 0:
                    self.allreduce_in_graph = False
                    g_model = None
            else:
                g_model = None
            if g_model is None:
                g_model, scores = capture_model()
            if exchange and not self.allreduce_in_graph:
                g_opt = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g_opt):
                    self.opt.step_dev(self.grads)
            self.opt.t = t0                               # a capture does not execute an update
            st = self._graphs[key] = (xs, g_model, g_opt, scores, B, lab, wst)
        xs, g_model, g_opt, scores, B, lab, wst = st
        if tuple(x1.shape[1:]) != tuple(xs.shape[1:]) or tuple(x2.shape) != tuple(x1.shape):
            raise RuntimeError('FgnnTrainer: the captured step of (B, N) = (%d, %d) was recorded for batches of shape %s per side, got %s / '
                               '%s; a trainer captures one channel count per (B, N)' % (B, N, (B,) + tuple(xs.shape[1:]),
                                                                                         tuple(x1.shape), tuple(x2.shape)))
        if x1.data_ptr() != xs.data_ptr():              # (train_step(input_form='tensor_representation') packs straight into xs)
            xs[:B].copy_(x1)
            xs[B:].copy_(x2)
        if lab is not None and labels.data_ptr() != lab.data_ptr():
            lab.copy_(labels)
        if wst is not None:
            if weights is None:
                wst['user'].fill_(1.0)
            else:
                wst['user'].copy_(weights)
            self._set_live(wst['live'], live, B)
        self._nodes.fill_(float(B * N))
        if g_opt is None:
            self.opt.sync_hyper_parameters(grad_scale=None)
            g_model.replay()
            self.opt.t += 1
            self._sync_module()
            return (self._loss_sum / self._nodes).reshape(()), scores
        g_model.replay()
        return self._reduce_and_update(opt_graph=g_opt), scores

    def check_input_form(self):
        """input_form='tensor_representation': read the device verdict of every train_step since the last check (one host
        synchronisation); raises if one of those batches was not a tensor representation."""
        if self._tr_flag is None:
            return
        if dp.world_size() > 1 or self._force_collective:
            # every rank reads the SUM of the flags (the check runs at the same step on all of them): the rank that saw the bad batch
            # does not raise alone while the others wait in the next gradient all-reduce
            dp.allreduce_sum_(self._tr_flag, force=self._force_collective)
        if int(self._tr_flag.item()) != 0:
            self._tr_flag.zero_()
            raise RuntimeError("FgnnTrainer(input_form='tensor_representation'): a batch since the last check is NOT the tensor "
                               'representation of a 0/1 adjacency (channel 0 in {0, 1}, channel 1 = diag(row sums), '
                               'loaders/data_generator.py:118-125); the updates of those steps are invalid -- run it through the dense '
                               "path (input_form='dense')")

    def save_checkpoint(self, path, **kw):
        """checkpoint.save_checkpoint of this trainer's parameters (+ optimizer) AFTER the pending input verdicts have been read: a run
        that ends fewer than INPUT_CHECK_EVERY steps after the last check must not persist parameters a bad batch has touched."""
        from .checkpoint import save_checkpoint
        self.check_input_form()
        return save_checkpoint(path, self.layout, self.params, optimizer=self.opt, **kw)

    def _labels(self, labels, B, N):
        """labels= of the train steps -> None or a (B, N) int32 device tensor (metrics.labels_tensor does the checking)"""
        if labels is None:
            return None
        from .metrics import labels_tensor
        return labels_tensor(labels, B, N, self.params.device)

    @staticmethod
    def _bits_shape(who, bits1, bits2):
        """The shape check of a bit-packed pair of batches (who: the calling method, for the message) -> (B, N)"""
        if bits1.dim() != 3 or bits1.shape != bits2.shape or bits1.dtype not in (torch.int32, torch.uint32) or not bits1.is_cuda:
            raise RuntimeError('FgnnTrainer.%s: expected two (B, N, ceil(N/32)) int32 device tensors, got %s %s / %s %s'
                               % (who, tuple(bits1.shape), bits1.dtype, tuple(bits2.shape), bits2.dtype))
        B, N = bits1.shape[0], bits1.shape[1]
        if bits1.shape[2] != (N + 31) // 32:
            raise RuntimeError('FgnnTrainer.%s: %d words per row for N = %d (expected %d)' % (who, bits1.shape[2], N, (N + 31) // 32))
        return B, N

    def train_step_bits(self, bits1, bits2, nvalid=None, labels=None, weights=None, live=None):
        """The same step with the local shard handed over as bit-packed adjacency: bits1, bits2
        (B, N, ceil(N / 32)) int32 device tensors, bit j of row i = W[i][j] (synthetic.pack_adjacency / the loader's packing); the
        tensor representation of loaders/data_generator.py:118-125 is built inside block 1's kernels, and with block1='structured'
        block 1 runs on the class tables of csrc/block1_struct.hip.  nvalid: (B,) int32 for ragged batches (padded to N).
        labels, weights, live: see train_step."""
        return self._train_step_words('train_step_bits', bits1, bits2, nvalid, labels, weights, live, None)

    def _check_features(self, who, n_powers):
        """The layout checks of the spectral steps and loops (before any launch) -> n_powers"""
        from . import _lib
        n_powers = int(n_powers)
        if not 1 <= n_powers <= _lib.FGNN_SPECTRAL_MAX_POWERS:
            raise ValueError('FgnnTrainer.%s: n_powers must be in [1, %d], got %d' % (who, _lib.FGNN_SPECTRAL_MAX_POWERS, n_powers))
        c0 = self.layout.c0
        if n_powers > c0 or (self.precision == 'fp32' and n_powers != c0 and c0 != 32):
            raise RuntimeError('FgnnTrainer.%s: %d spectral channels do not fit this layout (original_features_num = %d: n_powers <= '
                               'it; an fp32 2-channel layout takes exactly 2)' % (who, n_powers, c0))
        if self.block1 == 'structured':
            raise RuntimeError("FgnnTrainer.%s: spectral features run the generic block 1; this trainer was built with "
                               "block1='structured' (the 2-channel tensor representation only)" % who)
        return n_powers

    def train_step_spectral(self, bits1, bits2, nvalid=None, n_powers=4, labels=None, weights=None, live=None):
        """The twin of train_step_bits for the reference's second dataset class (QAP_spectralGenerator): the same bit words, but the
        step's input is their spectral features L, L^2, ..., L^n_powers (spectral.spectral_features), computed by the engine
        (engine.step(spectral=...)) -- bf16: one fgnn_spectral_slab16 launch straight into block 1's input slab; fp32: one
        fgnn_spectral_features launch into the engine's own buffer.  Bit-identical to train_step on the features of
        ``generator.spectral`` (fp32 on the 32-channel layout: zero-padded to its 32 channels, the input a narrow model runs on).  The
        layout needs original_features_num >= n_powers (an fp32 2-channel layout: exactly 2 powers) and the generic block 1.
        With capture=True the step is a graph of its own, keyed (B, N, 'spectral', n_powers) (+ 'labels' / 'weights'): its static
        input is the stacked words, the feature launch rides inside the graph.  nvalid, labels, weights, live: see train_step_bits."""
        n_powers = self._check_features('train_step_spectral', n_powers)
        return self._train_step_words('train_step_spectral', bits1, bits2, nvalid, labels, weights, live, n_powers)

    def _train_step_words(self, who, bits1, bits2, nvalid, labels, weights, live, n_powers):
        """train_step_bits (n_powers None) / train_step_spectral: one body, the engine keyword differs"""
        B, N = self._bits_shape(who, bits1, bits2)
        labels = self._labels(labels, B, N)
        weighted = self._weighted(weights, live)
        if self.capture and nvalid is None:
            if weighted:
                return self._captured_step(bits1, bits2, bits=True, labels=labels, weights=self._user_weights(weights, B), live=live,
                                           weighted=True, spectral=n_powers)
            return self._captured_step(bits1, bits2, bits=True, labels=labels, spectral=n_powers)
        eng = self._engine(2 * B, N, nvalid is not None)
        b = torch.cat([bits1, bits2]).contiguous()
        nv = None if nvalid is None else torch.cat([nvalid, nvalid]).to(torch.int32)
        lkw = {} if labels is None else {'labels': labels}
        lkw.update({'bits': b} if n_powers is None else {'spectral': (b, n_powers)})
        if weighted:
            lkw['weights'] = self._pair_weights(B, N, nvalid, live, weights)        # (self._nodes <- D)
        elif nvalid is None:
            self._nodes.fill_(float(B * N))
        else:
            self._nodes.copy_(nvalid.sum().to(torch.float32).reshape(1))
        scores, _ = eng.step(self.params, self.grads, None, nvalid=nv, total_nodes=1.0, loss_out=self._loss_sum, **lkw)
        return self._reduce_and_update(), scores

    def _features(self, who, features, n_powers, generators=()):
        """features= / n_powers= of the epoch loops -> None (the tensor representation: the bits steps), the checked n_powers
        ('spectral'), or 'weighted' (the dense steps on ``generator.weighted``; generators: the loop's generators, checked for it)"""
        if features is None:
            return None
        if features == 'weighted':
            return self._check_weighted(who, generators)
        if features != 'spectral':
            raise ValueError("FgnnTrainer.%s: features must be None or 'spectral', or 'weighted' for real-weighted pairs (got %r)" % (who, features))
        return self._check_features(who, n_powers)

    def _check_weighted(self, who, generators):
        """The refusals of features='weighted' (before any launch) -> 'weighted'"""
        for g in generators:
            if not callable(getattr(g, 'weighted', None)):
                raise ValueError("FgnnTrainer.%s: features='weighted' needs a generator with .weighted(...) (wigner.WignerGenerator), "
                                 'got %s' % (who, type(g).__name__))
        if self.input_form == 'tensor_representation':
            raise ValueError("FgnnTrainer.%s: features='weighted' feeds real weights; this trainer was built with "
                             "input_form='tensor_representation', whose 0/1 check would reject them (build it with input_form='dense')"
                             % who)
        c0 = self.layout.c0
        if c0 != 2 and not (self.precision == 'bf16' and c0 == 32):
            raise ValueError("FgnnTrainer.%s: features='weighted' feeds 2-channel tensor representations; a layout with "
                             'original_features_num = %d does not take them (2; bf16 also 32, zero-filled)' % (who, c0))
        return 'weighted'

    def train_epoch(self, generator, sampler, epoch, batch_size, permute=False, exact_last=False, features=None, n_powers=4):
        """One epoch over a fixed dataset of on-device pairs, in the sampler's order (the reference's shuffled DataLoader over
        num_examples_train pairs): per step ``train_step_bits(*generator.bits(index=sampler.batch_index(epoch, step, batch_size)))``.
        generator: pairgen.PairGenerator or pairstore.PairStore; sampler: sampler.EpochSampler (its rank and world size are this process's).  The loop reads
        nothing back (a ragged generator's vertex counts stay on the device as well).  Returns the (steps,) device tensor of the
        per-step losses of the global batch.
        permute=True: the pairs come relabelled (``generator.bits(index=..., permute=True)``) and the step trains on the
        cross-entropy against their planted labels (train_step_bits(labels=...)).
        exact_last=True: every example trains exactly once per epoch -- the positions with which a short last step is filled (they
        wrap to examples the epoch has already shown) are switched off (train_step_bits(live=sampler.live_count(...)), DESIGN.md
        section 14); every step then runs the weighted launches.  A rank whose last step has no live pair still takes part in the
        all-reduce, with a zero gradient.  False (default): the filled step trains its repeats, as before.
        features='spectral' (the reference's QAP_spectralGenerator): the same ``generator.bits(...)`` words go to
        train_step_spectral(n_powers=n_powers) -- the hand-written loop over ``generator.spectral(index=...)`` and train_step, bit
        for bit, without the fp32 features between two launches.  None (default): the loop above, launch for launch.
        features='weighted' (real-weighted pairs; generator: wigner.WignerGenerator): per step
        ``train_step(*generator.weighted(index=..., permute=permute))`` on the (B, 2, N, N) tensors, with the same labels and live --
        the hand-written loop, launch for launch.  ValueError for a generator without ``.weighted``, a trainer with
        input_form='tensor_representation' and a layout that does not take 2 channels."""
        spec = self._features('train_epoch', features, n_powers, (generator,))
        steps = sampler.steps_per_epoch(batch_size)
        losses = torch.empty(steps, dtype=torch.float32, device=self.params.device)
        pull = generator.weighted if spec == 'weighted' else generator.bits
        for step in range(steps):
            b1, b2, nv, *lab = pull(index=sampler.batch_index(epoch, step, batch_size), permute=permute)
            kw = {'labels': lab[0] if lab else None, 'live': sampler.live_count(step, batch_size) if exact_last else None}
            if spec == 'weighted':
                loss, _ = self.train_step(b1, b2, nv, **kw)
            else:
                loss, _ = self.train_step_bits(b1, b2, nv, **kw) if spec is None else self.train_step_spectral(b1, b2, nv, spec, **kw)
            losses[step].copy_(loss)
        return losses

    # ------------------------------------------------------------------ validation / test epochs (evaluation.py)
    def _eval_forward(self, B, N, nvalid, x=None, bits=None, spectral=None):
        """EngineBase.forward of the training engine for (B, N) on the stacked batch: raw scores only.  Its loss sum goes to a buffer
        of this method's own; gradients, the collective's buffer, the optimizer and the captured graphs are not touched."""
        if getattr(self, '_eval_loss', None) is None:
            self._eval_loss = torch.zeros(1, dtype=torch.float32, device=self.params.device)
        eng = self._engine(2 * B, N, nvalid is not None)
        nv = None if nvalid is None else torch.cat([nvalid, nvalid]).to(torch.int32)
        skw = {} if spectral is None else {'spectral': spectral}
        scores, _ = eng.forward(self.params, x, nvalid=nv, total_nodes=1.0, defer_loss=False, loss_out=self._eval_loss, bits=bits, **skw)
        return scores

    def _eval_tail(self, B, N, nvalid, x=None, bits=None, pair_bits=None, spectral=None, **options):
        """The stacked batch -> its scores -> evaluation.evaluate_scores with the step's options (pair_bits: its bits=, the two
        graphs' bit words for a qap_meter)"""
        from .evaluation import evaluate_scores
        if pair_bits is not None:
            options['bits'] = pair_bits
        return evaluate_scores(self._eval_forward(B, N, nvalid, x=x, bits=bits, spectral=spectral), nvalid=nvalid, **options)

    def eval_step_bits(self, bits1, bits2, nvalid=None, labels=None, meter=None, live=None, hungarian=True, loss_on_labels=False,
                       bins=None, rank_meter=None, qap_meter=None, refine=0, two_opt=False, faq=None, seeds=None, seed_meter=None):
        """Forward-only evaluation of a batch handed over as train_step_bits takes it: the training engine's forward pass (a third of
        a step's work), then evaluation.evaluate_scores on its scores -- see there for labels, meter, live, hungarian,
        loss_on_labels, bins, rank_meter and the returned per-pair device tensors.  Nothing is read back; parameters, gradients and optimizer state keep their bits.
        qap_meter (a QapMeter; with bins= a BinnedQapMeter), refine: the decode chain of evaluation.decode_scores on the bit words
        handed in here and the solver's assignment (0/1 graphs only; needs hungarian=True).  None: nothing of it is launched.
        two_opt=True (with a qap_meter): the chain ends in the pairwise-exchange search of qap.two_opt_bits, one more launch, and the
        meter's refined figures describe its matching.
        faq (with a qap_meter): None, True or the dict of evaluation.decode_scores -- the Fast Approximate QAP stage between the
        Hungarian matching and the refinement, started from the Sinkhorn projection of this step's scores or from the barycenter.
        seeds, seed_meter (with a qap_meter and faq): a (B, N) seed tensor or the spec of evaluation.decode_scores -- 'scores' draws
        the seeds from this step's scores (qap.confident_seeds) -- and a SeedMeter (with bins= a BinnedSeedMeter); both go to the
        decode, which refuses seeds without faq= and with refine > 0."""
        return self._eval_step_words('eval_step_bits', bits1, bits2, nvalid, None, labels=labels, meter=meter, live=live,
                                     hungarian=hungarian, loss_on_labels=loss_on_labels, bins=bins, rank_meter=rank_meter,
                                     qap_meter=qap_meter, refine=refine, two_opt=two_opt, faq=faq, seeds=seeds, seed_meter=seed_meter)

    def eval_step_spectral(self, bits1, bits2, nvalid=None, n_powers=4, labels=None, meter=None, live=None, hungarian=True,
                           loss_on_labels=False, bins=None, rank_meter=None, qap_meter=None, refine=0, two_opt=False, faq=None,
                           seeds=None, seed_meter=None):
        """The twin of eval_step_bits for spectral input: the forward pass runs on the features L, ..., L^n_powers of the bit words
        (engine.forward(spectral=...), as train_step_spectral), everything after the scores is eval_step_bits'.
        qap_meter, refine, two_opt, faq, seeds, seed_meter: the decode runs on the BIT WORDS handed in here -- the QAP objective on the adjacency W, not on the
        normalised L the model sees.  On regular graphs L = W / d, so the ratio to the planted objective is the one the reference
        reports for its spectral pairs; the reference's literal decode on channel 0 of the features stays what
        ``match(..., weighted=True)`` computes per batch."""
        n_powers = self._check_features('eval_step_spectral', n_powers)
        return self._eval_step_words('eval_step_spectral', bits1, bits2, nvalid, n_powers, labels=labels, meter=meter, live=live,
                                     hungarian=hungarian, loss_on_labels=loss_on_labels, bins=bins, rank_meter=rank_meter,
                                     qap_meter=qap_meter, refine=refine, two_opt=two_opt, faq=faq, seeds=seeds, seed_meter=seed_meter)

    def _eval_step_words(self, who, bits1, bits2, nvalid, n_powers, qap_meter=None, refine=0, two_opt=False, faq=None, seeds=None,
                         seed_meter=None, **options):
        """eval_step_bits (n_powers None) / eval_step_spectral: one body, the engine keyword differs"""
        B, N = self._bits_shape(who, bits1, bits2)
        decode = {} if qap_meter is None and not refine else {'qap_meter': qap_meter, 'pair_bits': (bits1, bits2), 'refine': refine}
        if two_opt is not False:
            decode = dict(decode, qap_meter=qap_meter, two_opt=two_opt)
        if faq is not None:
            decode = dict(decode, qap_meter=qap_meter, faq=faq)
        if seeds is not None:
            decode = dict(decode, qap_meter=qap_meter, seeds=seeds)
        if seed_meter is not None:
            decode = dict(decode, qap_meter=qap_meter, seed_meter=seed_meter)
        b = torch.cat([bits1, bits2]).contiguous()
        src = {'bits': b} if n_powers is None else {'spectral': (b, n_powers)}
        return self._eval_tail(B, N, nvalid, **src, **options, **decode)

    def eval_step(self, x1, x2, nvalid=None, labels=None, meter=None, live=None, hungarian=True, loss_on_labels=False, bins=None,
                  rank_meter=None, qap_meter=None, refine=0, two_opt=False, faq=None, seeds=None, seed_meter=None):
        """eval_step_bits for dense batches: x1, x2 (B, c0, N, N) fp32 on the GPU, through the generic kernels (precision='bf16' with
        a 32-channel layout: any 1..32 channels, as train_step).
        qap_meter (a WeightedQapMeter; with bins= a BinnedWeightedQapMeter), refine, two_opt, faq, seeds, seed_meter: the decode chain
        of evaluation.decode_scores_weighted on channel 0 of x1 and x2, read in place (evaluate_scores(adj=(x1, x2))), on the
        solver's assignment -- real-weighted pairs (WignerGenerator.weighted) and any tensor representation.  Without these keywords
        nothing of it is launched and the step is the one it always was."""
        if x1.dim() != 4 or x1.shape != x2.shape or not x1.is_cuda:
            raise RuntimeError('FgnnTrainer.eval_step: expected two (B, c0, N, N) device tensors, got %s / %s'
                               % (tuple(x1.shape), tuple(x2.shape)))
        decode = {} if qap_meter is None and not refine else {'qap_meter': qap_meter, 'adj': (x1, x2), 'refine': refine}
        if two_opt is not False:
            decode = dict(decode, qap_meter=qap_meter, two_opt=two_opt)
        if faq is not None:
            decode = dict(decode, qap_meter=qap_meter, faq=faq)
        if seeds is not None:
            decode = dict(decode, qap_meter=qap_meter, seeds=seeds)
        if seed_meter is not None:
            decode = dict(decode, qap_meter=qap_meter, seed_meter=seed_meter)
        return self._eval_tail(x1.shape[0], x1.shape[-1], nvalid, x=torch.cat([x1, x2]).contiguous(), labels=labels, meter=meter, live=live,
                               hungarian=hungarian, loss_on_labels=loss_on_labels, bins=bins, rank_meter=rank_meter, **decode)

    def evaluate(self, generator, sampler, batch_size, epoch=0, hungarian=True, meter=None, permute=False, loss_on_labels=False,
                 rank_meter=None, qap_meter=None, refine=0, features=None, n_powers=4, two_opt=False, faq=None, seeds=None,
                 seed_meter=None):
        """One pass over this rank's examples of `sampler` (sampler.EpochSampler; shuffle=False is the reference's validation
        loader): per step ``eval_step_bits(*generator.bits(index=sampler.batch_index(epoch, step, batch_size)))`` with the generator's
        vertex counts and, with permute=True, its planted labels.  Every example counts exactly once: the positions with which a
        short last step is filled are masked out (live=sampler.live_count(...)).  With more than one rank the record is summed
        over the ranks at the end (one all-reduce of 6 values).  Reads nothing back; returns the meter (EvalMeter).
        loss_on_labels=True (with permute=True): the record's loss is the cross-entropy against the planted labels -- the model's
        loss on those pairs, the one ReduceLROnPlateau should watch -- instead of the one against the identity.
        rank_meter: a RankMeter that takes the rank of every example's true match (the planted labels with permute=True) from the
        same steps (evaluation.rank_scores; two more launches per step) and is summed over the ranks like the meter.
        qap_meter: a QapMeter that takes the decode of every example from the same steps -- the accuracy of the Hungarian
        matching, its QAP objective against the planted one and, with refine = T > 0, the same after T rounds of greedy refinement
        (evaluation.decode_scores on the steps' bit words and the solver's assignment; the reference's all_acc_qap(val_loader, ...)
        and all_greedy_losses_acc; 0/1 graphs only) -- and is summed over the ranks like the meter.  Needs hungarian=True.
        two_opt=True (with a qap_meter): every step's chain ends in the pairwise-exchange search (evaluation.decode_scores), and the
        meter's 'refined_acc', 'refined_qap_ratio' and 'improved' describe the matching it leaves.
        faq (with a qap_meter): None, True or the dict of evaluation.decode_scores -- every step's chain runs the Fast Approximate
        QAP stage after the Hungarian matching; the refined figures describe the last stage of the chain that ran.
        seeds (with a qap_meter and faq): what eval_step_bits takes -- 'scores' or the spec dict: every step's seeds come from its own
        scores -- or an integer k: every step reveals k rows of the planted labels,
        ``planted.reveal_seeds(labels, nvalid, k, generator.seed, index=...)`` with the step's example indices (needs permute=True,
        ValueError otherwise).  seed_meter: a SeedMeter that takes every step's seed fold and is summed over the ranks like the meter.
        features='spectral', n_powers: the steps are eval_step_spectral on the same words (the decode of a qap_meter stays on the
        adjacency, see there).  None: eval_step_bits, as before.
        features='weighted' (generator: wigner.WignerGenerator): per step ``eval_step(*generator.weighted(index=..., permute=permute))``;
        the qap_meter is then a WeightedQapMeter and its decode the fp32 chain of evaluation.decode_scores_weighted on channel 0 of
        the step's tensors.  The refusals of train_epoch hold."""
        from .evaluation import EvalMeter, QapMeter, RankMeter, SeedMeter, WeightedQapMeter
        spec = self._features('evaluate', features, n_powers, (generator,))
        qap_class = WeightedQapMeter if spec == 'weighted' else QapMeter
        B = int(batch_size)
        if meter is None:
            meter = EvalMeter(self.params.device)
        elif not isinstance(meter, EvalMeter):
            raise ValueError('FgnnTrainer.evaluate: meter must be an EvalMeter or None (got %s)' % type(meter).__name__)
        if rank_meter is not None and not isinstance(rank_meter, RankMeter):
            raise ValueError('FgnnTrainer.evaluate: rank_meter must be a RankMeter or None (got %s)' % type(rank_meter).__name__)
        if qap_meter is not None and not isinstance(qap_meter, qap_class):
            raise ValueError('FgnnTrainer.evaluate: qap_meter must be a %s or None (got %s)' % (qap_class.__name__, type(qap_meter).__name__))
        if seed_meter is not None and not isinstance(seed_meter, SeedMeter):
            raise ValueError('FgnnTrainer.evaluate: seed_meter must be a SeedMeter or None (got %s)' % type(seed_meter).__name__)
        def batches():
            for step in range(sampler.steps_per_epoch(B)):
                live = sampler.live_count(step, B)
                if live:        # (0: a rank past the end of the data in the last global step; its index is never made)
                    yield live, None, {'index': sampler.batch_index(epoch, step, B), 'permute': permute}
        return self._eval_epoch(generator, batches(), meter, rank_meter, dp.world_size() > 1, hungarian, loss_on_labels, qap_meter,
                                refine, spec, two_opt, faq, seeds, seed_meter)

    def _eval_epoch(self, generator, batches, meter, rank_meter, reduce, hungarian, loss_on_labels, qap_meter=None, refine=0, spec=None,
                    two_opt=False, faq=None, seeds=None, seed_meter=None):
        """The loop of evaluate and noise_curve.  batches: per step that has a live pair (live, bins, the keyword arguments of
        generator.bits); reduce: sum the meters over the ranks at the end; spec: None, the n_powers of spectral steps, or 'weighted' (the
        keyword arguments go to generator.weighted, the steps are eval_step).  -> meter"""
        if qap_meter is None and refine:
            raise ValueError('FgnnTrainer: refine= belongs to a qap_meter')
        if qap_meter is None and two_opt:
            raise ValueError('FgnnTrainer: two_opt= belongs to a qap_meter')
        if qap_meter is None and faq is not None:
            raise ValueError('FgnnTrainer: faq= belongs to a qap_meter')
        decode = {} if qap_meter is None else {'qap_meter': qap_meter, 'refine': refine}
        if two_opt is not False:
            decode['two_opt'] = two_opt
        if faq is not None:
            decode['faq'] = faq
        if qap_meter is None and (seeds is not None or seed_meter is not None):
            raise ValueError('FgnnTrainer: seeds= and seed_meter= belong to a qap_meter')
        reveal = None
        if seeds is not None and not isinstance(seeds, (str, dict)) and not torch.is_tensor(seeds):
            if isinstance(seeds, bool) or not hasattr(seeds, '__index__') or seeds < 0:
                raise ValueError("FgnnTrainer: seeds must be a seed tensor, 'scores', a spec dict or an integer >= 0, got %r" % (seeds,))
            reveal = int(seeds)
        elif seeds is not None:
            decode['seeds'] = seeds
        if seed_meter is not None:
            decode['seed_meter'] = seed_meter
        # restarts draw from (seed, pair index, k): hand the step's dataset indices over, so the record does not depend on the batching
        restart_index = isinstance(faq, dict) and faq.get('restarts', 1) != 1 and faq.get('index') is None
        for live, bins, bits_kw in batches:
            if restart_index:
                decode['faq'] = dict(faq, index=bits_kw['index'])
            if reveal is not None and not bits_kw.get('permute'):
                raise ValueError('FgnnTrainer: an integer seeds= reveals rows of the planted labels; it needs permute=True')
            b1, b2, nv, *labels = generator.weighted(**bits_kw) if spec == 'weighted' else generator.bits(**bits_kw)
            if reveal is not None:
                from .planted import reveal_seeds
                decode['seeds'] = reveal_seeds(labels[0], nv, reveal, generator.seed, index=bits_kw['index'])
            kw = dict(nvalid=nv, labels=labels[0] if labels else None, meter=meter, live=live, hungarian=hungarian,
                      loss_on_labels=loss_on_labels, bins=bins, rank_meter=rank_meter, **decode)
            if spec is None:
                self.eval_step_bits(b1, b2, **kw)
            elif spec == 'weighted':
                self.eval_step(b1, b2, **kw)
            else:
                self.eval_step_spectral(b1, b2, n_powers=spec, **kw)
        if reduce:
            meter.allreduce_()
            if rank_meter is not None:
                rank_meter.allreduce_()
            if qap_meter is not None:
                qap_meter.allreduce_()
            if seed_meter is not None:
                seed_meter.allreduce_()
        return meter

    @staticmethod
    def noise_curve_batch(sampler, step, batch_size, num_examples):
        """This rank's batch at `step` of a noise curve over num_examples pairs per level: (pair, level, live).  The K * M examples
        lie level-major -- example e is dataset pair e % M at level e // M -- and `sampler` is the unshuffled EpochSampler over
        them; pair and level are (batch_size,) int64 tensors on the sampler's device (two integer ops, nothing is read), live the
        number of leading positions that are examples of their own (the filling of a short last step wraps to example 0)."""
        M = int(num_examples)
        e = sampler.batch_index(0, step, batch_size)
        return e % M, e // M, sampler.live_count(step, batch_size)

    def noise_curve(self, generator, noises, num_examples, batch_size, hungarian=True, permute=False, loss_on_labels=False,
                    rank=None, world_size=None, meter=None, rank_meter=None, qap_meter=None, refine=0, features=None, n_powers=4,
                    two_opt=False, faq=None, seeds=None, seed_meter=None):
        """The reference's result figure (README.md, "Results": a trained model evaluated across noise levels; per level
        toolbox/metrics.py:144-166) in one pass: the first num_examples pairs of `generator` at each of the K = len(noises) noise
        levels -- the SAME parent graphs at every level, a paired design -- through full batches of mixed levels
        (``generator.bits(index=pair, levels=generator.levels(noises), level=level)``) and ``eval_step_bits(..., bins=level)`` into
        a BinnedEvalMeter with one record per level.  `generator.noise` is ignored here: every pair takes the noise of its level.
        The K * num_examples examples are cut by an unshuffled EpochSampler (rank, world_size: None is this process's rank and
        the number of ranks of torch.distributed); every example counts once, a step with no live pair on this rank is skipped.
        When the split is the one of torch.distributed (world_size left at None, or equal to its number of ranks, above 1) the
        records are summed over the ranks at the end (one all-reduce of K x 6 values); with any other world_size -- 1 on every
        rank for a whole curve each, or the parts of a split walked in one process -- the records stay this call's own.
        hungarian, permute, loss_on_labels: as in `evaluate`.  meter: a BinnedEvalMeter of K records to accumulate into (None: a
        fresh one whose values are the noises).  Reads nothing back: ``meter.result()``, K dicts with 'noise', 'loss', 'acc',
        'acc_max', is the one host read.  Returns the meter.
        rank_meter: a BinnedRankMeter of K records that takes the rank metrics of every level from the same steps; it is summed
        over the ranks where the meter is.
        qap_meter: a BinnedQapMeter of K records that takes the decode of every level (see `evaluate`; refine: its rounds of
        greedy refinement; two_opt: the pairwise-exchange search at its end; faq: the Fast Approximate QAP stage before them) from the same steps -- the QAP ratio across noise
        levels; it is summed over the ranks where the meter is.
        seeds: as in `evaluate` (an integer k reveals the same rows of a pair at every level: the choice depends on the pair's index
        alone); seed_meter: a BinnedSeedMeter of K records, summed over the ranks where the meter is.
        features='spectral', n_powers: as in `evaluate`.  features='weighted': as in `evaluate`, the levels being the generator's own
        (``WignerGenerator.levels``: one (rho, sig) per level) and the qap_meter a BinnedWeightedQapMeter."""
        from .evaluation import BinnedEvalMeter, BinnedQapMeter, BinnedRankMeter, BinnedSeedMeter, BinnedWeightedQapMeter
        spec = self._features('noise_curve', features, n_powers, (generator,))
        qap_class = BinnedWeightedQapMeter if spec == 'weighted' else BinnedQapMeter
        from .sampler import EpochSampler
        levels = generator.levels(noises)
        K, M, B = len(levels), int(num_examples), int(batch_size)
        if M < 1:
            raise ValueError('FgnnTrainer.noise_curve: num_examples must be >= 1, got %d' % M)
        if meter is None:
            meter = BinnedEvalMeter(self.params.device, K, values=levels.noises)
        elif not isinstance(meter, BinnedEvalMeter) or meter.K != K:
            raise ValueError('FgnnTrainer.noise_curve: meter must be a BinnedEvalMeter of %d records or None' % K)
        if rank_meter is not None and (not isinstance(rank_meter, BinnedRankMeter) or rank_meter.K != K):
            raise ValueError('FgnnTrainer.noise_curve: rank_meter must be a BinnedRankMeter of %d records or None' % K)
        if qap_meter is not None and (not isinstance(qap_meter, qap_class) or qap_meter.K != K):
            raise ValueError('FgnnTrainer.noise_curve: qap_meter must be a %s of %d records or None' % (qap_class.__name__, K))
        if seed_meter is not None and (not isinstance(seed_meter, BinnedSeedMeter) or seed_meter.K != K):
            raise ValueError('FgnnTrainer.noise_curve: seed_meter must be a BinnedSeedMeter of %d records or None' % K)
        if world_size is None:
            world_size = dp.world_size()
        if rank is None:        # (this process's rank in the split of torch.distributed; any other split has to name it)
            rank = torch.distributed.get_rank() if world_size == dp.world_size() > 1 else 0
        sampler = EpochSampler(K * M, shuffle=False, rank=rank, world_size=world_size, drop_last=False, device=generator.device)
        def batches():
            for step in range(sampler.steps_per_epoch(B)):
                pair, level, live = self.noise_curve_batch(sampler, step, B, M)
                if live:        # (0: a rank past the end of the examples in the last global step)
                    yield live, level, {'index': pair, 'levels': levels, 'level': level, 'permute': permute}
        return self._eval_epoch(generator, batches(), meter, rank_meter, dp.world_size() > 1 and sampler.world_size == dp.world_size(),
                                hungarian, loss_on_labels, qap_meter, refine, spec, two_opt, faq, seeds, seed_meter)

    def fit(self, train_gen, train_sampler, val_gen, val_sampler, epochs, batch_size, scheduler=None, permute=False, exact_last=False,
            rank_ks=None, decode_refine=None, features=None, n_powers=4, decode_two_opt=False, decode_faq=None, decode_seeds=None):
        """The reference's training loop around its scheduler (models/trainers.py:92-104): per epoch train_epoch, evaluate, ONE host
        read (the validation record), scheduler.step(val_loss).  scheduler=None: optim.ReduceLROnPlateau with the reference's
        settings, driving self.opt.lr (the next step pushes a changed rate to the device).  Returns the per-epoch history: dicts
        with 'epoch', 'train_losses' (the (steps,) device tensor of train_epoch), 'val_loss', 'val_acc', 'val_acc_max', 'lr' (the
        rate the NEXT epoch runs with).
        permute=True: training and validation run on planted pairs (train_epoch(permute=True), evaluate(permute=True,
        loss_on_labels=True)): 'val_loss' (what the scheduler sees), 'val_acc' and 'val_acc_max' all refer to the labels, and the
        Hungarian accuracy is free of the identity tie bias.
        exact_last: handed to train_epoch.
        rank_ks: a tuple of thresholds (evaluation.RankMeter): every epoch's dict gains 'val_hits' ({k: Hits@k}) and 'val_mrr' of the
        validation pairs, taken by the same validation steps and read with the validation record in the same single host copy.
        decode_refine: an integer T >= 0 (evaluation.QapMeter; 0/1 graphs only): every epoch's dict gains 'val_qap_ratio' (the
        objective of the Hungarian matching over the planted one, summed over the validation pairs), 'val_recovered' (the fraction
        of pairs whose matching reaches the planted objective) and, for T > 0, 'val_refined_acc' (the accuracy after T rounds of
        greedy refinement), taken by the same validation steps and read in the same single host copy.
        decode_two_opt=True (with decode_refine, which may be 0): the validation decode ends in the pairwise-exchange search
        (evaluate(two_opt=True)); 'val_refined_acc' is then reported for every T and describes the matching the search leaves, and
        'val_refined_qap_ratio' is its objective over the planted one.
        decode_faq (with decode_refine, which may be 0): None, True or the dict of evaluation.decode_scores -- the validation decode
        runs the Fast Approximate QAP stage (evaluate(faq=...)); 'val_refined_acc' and 'val_refined_qap_ratio' are then reported
        for every T, as with decode_two_opt, and describe the last stage of the chain.
        decode_seeds (with decode_faq; decode_refine may be left out and is then 0): what evaluate(seeds=...) takes -- 'scores', the spec dict, or an integer
        k with permute=True -- the validation decode is seeded, and every epoch's dict gains 'val_seed_precision' (the seeds that
        are right over the seeds) and 'val_free_acc' (the rows without a seed the seeded stage got right over those rows), from a
        SeedMeter read in the same single host copy.
        features='spectral', n_powers: training and validation run on the spectral features of the generators' pairs (train_epoch /
        evaluate with the same arguments).  features='weighted': on the real-weighted pairs of two wigner.WignerGenerators;
        decode_refine then builds a WeightedQapMeter and the same 'val_*' keys are reported."""
        spec = self._features('fit', features, n_powers, (train_gen, val_gen))
        fkw = {} if features is None else {'features': features} if spec == 'weighted' else {'features': features, 'n_powers': spec}
        from .evaluation import (EvalMeter, QapMeter, RankMeter, SeedMeter, WeightedQapMeter, _check_faq, _check_refine, qap_result,
                                 rank_result, read_records, record_result, seed_result)
        if scheduler is None:
            from .optim import ReduceLROnPlateau
            scheduler = ReduceLROnPlateau(self.opt)
        history = []
        rank_meter = None if rank_ks is None else RankMeter(self.params.device, ks=rank_ks)
        if decode_seeds is not None and decode_refine is None:       # (seeds exclude refine > 0: theirs is the decode without rounds)
            decode_refine = 0
        if decode_refine is not None:
            decode_refine = _check_refine('FgnnTrainer.fit', decode_refine)
        if decode_two_opt and decode_refine is None:
            raise ValueError('FgnnTrainer.fit: decode_two_opt= belongs to a decode_refine (which may be 0)')
        if decode_faq is not None and decode_refine is None:
            raise ValueError('FgnnTrainer.fit: decode_faq= belongs to a decode_refine (which may be 0)')
        decode_faq = _check_faq('FgnnTrainer.fit', decode_faq)
        if decode_seeds is not None and decode_faq is None:
            raise ValueError('FgnnTrainer.fit: decode_seeds= needs decode_faq= (seeds need the faq stage of the decode)')
        qap_meter = None if decode_refine is None else (WeightedQapMeter if spec == 'weighted' else QapMeter)(self.params.device)
        seed_meter = None if decode_seeds is None else SeedMeter(self.params.device)
        extra = [m for m in (rank_meter, qap_meter, seed_meter) if m is not None]
        own = EvalMeter(self.params.device) if extra else None                       # (read together with the other meters)
        decode = {} if qap_meter is None else {'qap_meter': qap_meter, 'refine': decode_refine}
        if decode_two_opt is not False:
            decode['two_opt'] = decode_two_opt
        if decode_faq is not None:
            decode['faq'] = decode_faq
        if decode_seeds is not None:
            decode.update(seeds=decode_seeds, seed_meter=seed_meter)
        for epoch in range(int(epochs)):
            for m in extra + [own] * bool(extra):
                m.reset()
            losses = self.train_epoch(train_gen, train_sampler, epoch, batch_size, permute=permute, exact_last=exact_last, **fkw)
            meter = self.evaluate(val_gen, val_sampler, batch_size, epoch=epoch, meter=own, permute=permute, loss_on_labels=permute,
                                  rank_meter=rank_meter, **decode, **fkw)
            if not extra:
                res = meter.result()
            else:
                rec, *others = read_records(meter, *extra)
                res, others = record_result(rec), dict(zip(map(id, extra), others))
            scheduler.step(res['loss'])
            history.append({'epoch': epoch, 'train_losses': losses, 'val_loss': res['loss'], 'val_acc': res['acc'],
                            'val_acc_max': res['acc_max'], 'lr': self.opt.lr})
            if rank_meter is not None:
                rres = rank_result(others[id(rank_meter)])
                history[-1]['val_hits'] = {k: rres['hits@%d' % k] for k in rank_meter.ks}
                history[-1]['val_mrr'] = rres['mrr']
            if qap_meter is not None:
                qres = qap_result(others[id(qap_meter)])
                history[-1]['val_qap_ratio'], history[-1]['val_recovered'] = qres['qap_ratio'], qres['recovered']
                if decode_refine > 0 or decode_two_opt or decode_faq is not None:
                    history[-1]['val_refined_acc'] = qres['refined_acc']
                if decode_two_opt or decode_faq is not None:
                    history[-1]['val_refined_qap_ratio'] = qres['refined_qap_ratio']
            if seed_meter is not None:
                sres = seed_result(others[id(seed_meter)])
                history[-1]['val_seed_precision'], history[-1]['val_free_acc'] = sres['seed_precision'], sres['free_acc']
        return history

    def train_step(self, x1, x2, nvalid=None, labels=None, weights=None, live=None):
        """x1, x2: (B, c0, N, N) local shard on the GPU (precision='bf16' with a 32-channel layout: any 1..32 channels, e.g. the four
        spectral ones; the engine's input conversion zero-fills the rest).  Returns (loss of the global batch as a device
        scalar, scores of the local shard).
        labels: None (the identity, the reference's target), or what metrics.labels_tensor takes -- a (B, N) integer tensor with
        labels[b, i] = the vertex of x2[b] that vertex i of x1[b] matches (-1: no target), or a list of B integer arrays: the loss is
        the cross-entropy against them (normalised by the node count as before).  An int32 device tensor is
        read in place by the eager step and copied into the captured step's static buffer.
        weights: None, or (B,) per-pair factors u_b >= 0 multiplied into the weights of the reduction.  live: None, or the number of
        leading pairs of the shard that count (an int, or a 1-element int32 device tensor): the others are fillers, switched off by
        a select -- they add nothing to loss, gradient and normaliser, whatever their scores hold (EpochSampler.live_count; a rank
        may pass 0).  With either, or with loss_reduction='mean_of_mean', the step runs the weighted launches (DESIGN.md section
        15): the loss returned is sum_b w_b CE_b / D over the global batch.  A global step must have a pair that counts (D > 0)."""
        if self.input_form == 'tensor_representation' and x1.dim() == 4 and x1.shape[1] == 2 and self.layout.c0 == 2 \
                and x1.dtype == torch.float32 and x1.shape == x2.shape:
            from . import _lib
            B, N = x1.shape[0], x1.shape[-1]
            if bool(_lib.load().fgnn_block1_struct_supported(N, self.layout.depth, self.layout.c0)):
                w = self._tr.get((B, N))
                first = w is None
                if first:
                    w = self._tr[(B, N)] = torch.zeros(2 * B, N, (N + 31) // 32, dtype=torch.int32, device=x1.device)
                if self._tr_flag is None:
                    self._tr_flag = torch.zeros(1, dtype=torch.int32, device=x1.device)
                nv = None if nvalid is None else nvalid.to(device=x1.device, dtype=torch.int32)
                nvp = _lib.ptr(nv) if nv is not None else None      # (both sides of a pair share their vertex counts)
                _lib.call('fgnn_pack_adjacency_pair', _lib.ptr(x1.contiguous()), _lib.ptr(x2.contiguous()), nvp, nvp, B, N, N, _lib.ptr(w),
                          None, None, _lib.ptr(self._tr_flag), _lib.stream_ptr())         # one launch for both sides
                self._tr_calls += 1
                if first or (self.INPUT_CHECK_EVERY and self._tr_calls % self.INPUT_CHECK_EVERY == 0):
                    self.check_input_form()
                out = self.train_step_bits(w[:B], w[B:], nvalid=nv, labels=labels, weights=weights, live=live)
                if first and (B, N, 'bits') in self._graphs:        # from now on pack straight into the captured step's input words
                    self._tr[(B, N)] = self._graphs[(B, N, 'bits')][0]
                return out
        labels = self._labels(labels, x1.shape[0], x1.shape[-1])
        weighted = self._weighted(weights, live)
        if self.capture and nvalid is None:
            if weighted:
                return self._captured_step(x1, x2, labels=labels, weights=self._user_weights(weights, x1.shape[0]), live=live, weighted=True)
            return self._captured_step(x1, x2, labels=labels)
        B, _, N, _ = x1.shape
        eng = self._engine(2 * B, N, nvalid is not None)
        x = torch.cat([x1, x2]).contiguous()
        nv = None if nvalid is None else torch.cat([nvalid, nvalid])
        lkw = {} if labels is None else {'labels': labels}
        if weighted:
            lkw['weights'] = self._pair_weights(B, N, nvalid, live, weights)        # (self._nodes <- D)
        elif nvalid is None:
            self._nodes.fill_(float(B * N))
        else:
            self._nodes.copy_(nvalid.sum().to(torch.float32).reshape(1))     # device-side, no host sync
        scores, _ = eng.step(self.params, self.grads, x, nvalid=nv, total_nodes=1.0, loss_out=self._loss_sum, **lkw)
        return self._reduce_and_update(), scores
