"""``Siamese_Node_Exp`` (models/trainers.py:20-68) without the Lightning shell: shared node
embedder on both graphs of a pair, scores[b,i,j] = <E1[b,:,i], E2[b,:,j]>.

The two branches share weights, so they are embedded as ONE stacked batch of 2B graphs
through the fused engine; the outer-product scoring and its backward are HIP kernels too.
Inputs arrive as the reference's loaders produce them: ``{'input': T}`` dicts
(loaders/loaders.py:12-15) or bare tensors / MaskedTensors.
"""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib, qap
from .blocks import block, block_emb, node_embedding
from .losses import triplet_loss
from .metrics import accuracy_linear_assignment, accuracy_max, count_matches, labels_tensor, lsap_device
from .masked import MaskedTensor
from .network import Network

get_node_emb = {'node_embedding': node_embedding}
get_block_init = {'block_emb': block_emb}
get_block_inside = {'block': block}


class _ScoreFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e1, e2, nvalid):
        e1, e2 = e1.contiguous(), e2.contiguous()
        B, Cc, N = e1.shape
        scores = torch.empty(B, N, N, dtype=torch.float32, device=e1.device)
        _lib.call('fgnn_score_ce_fwd', _lib.ptr(e1), _lib.ptr(e2), _lib.ptr(nvalid) if nvalid is not None else None,
                  B, Cc, N, _lib.ptr(scores), None, None, _lib.stream_ptr())
        ctx.save_for_backward(e1, e2, nvalid)
        return scores

    @staticmethod
    def backward(ctx, ds):
        e1, e2, nvalid = ctx.saved_tensors
        B, Cc, N = e1.shape
        d1, d2 = torch.empty_like(e1), torch.empty_like(e2)
        _lib.call('fgnn_score_bwd', _lib.ptr(e1), _lib.ptr(e2), _lib.ptr(ds.contiguous()),
                  _lib.ptr(nvalid) if nvalid is not None else None, B, Cc, N, _lib.ptr(d1), _lib.ptr(d2),
                  _lib.stream_ptr())
        return d1, d2, None


def _unwrap_input(x):
    return x['input'] if isinstance(x, dict) else x


class Siamese_Node_Exp(nn.Module):
    MODULE_STEPS_MAX = 8        # captured module steps kept per model (fused_step through the module surface), LRU

    # MaskedTensor batches run padded to a multiple of this (batches whose largest graphs fall in the same granule replay ONE graph; cfg5
    # through fused_step: 0.861 ms at 8, 0.876 at 16, engine on the exact size 0.846 -- profiles/archive/r05_cfg5_surface.txt)
    RAGGED_GRANULE = int(__import__('os').environ.get('FGNN_RAGGED_GRANULE', '8'))
    INPUT_CHECK_EVERY = 128     # input_form='tensor_representation': the device verdict is read back on every k-th fused_step (0: never)

    def __init__(self, original_features_num, node_emb, lr=1e-3, scheduler_decay=0.5, scheduler_step=3, lr_stop=1e-5,
                 metric=None, precision='fp32', input_form='dense'):
        """Same positional signature as the reference (models/trainers.py:21).  Three keyword-only extras:
        input_form: 'dense' (default) -- block 1 makes no assumption about the input tensor; 'tensor_representation' -- the caller
                states that every batch is what the reference's loaders yield (loaders/data_generator.py:118-125: channel 0 a 0/1
                adjacency, channel 1 = diag(row sums)), and `fused_step` / `FgnnTrainer.from_module` then run block 1 on that structure
                (csrc/block1_struct.hip: the batch is bit-packed on the device, mlp1 / mlp2 become class tables, the per-channel
                product a closed form; same function, results equal to fp32 rounding).  The statement is VERIFIED on the device by
                the packing kernel of every step; the verdict is read on the first step of each batch shape, on every
                INPUT_CHECK_EVERY-th step and by `check_input_form()`, and a batch that is not a tensor representation raises.
                Also settable later: `model.node_embedder.input_form = 'tensor_representation'`.
        metric: None -> the reference's default, the Hungarian matching accuracy (`accuracy_linear_assignment`: trainers.py:52,
                metrics.py:92-116; SciPy's assignment computed on the device, csrc/lsap.hip); 'max' -> the arg-max accuracy
                (`accuracy_max`, metrics.py:118-141); or any callable.  Neither copies the scores to the host.
        precision: 'fp32' (default) or 'bf16' (the bf16 engine; what `node_embedder.half()` also selects)."""
        super().__init__()
        node_emb = dict(node_emb)
        try:
            node_emb_type = get_node_emb[node_emb['type']]
        except KeyError:
            raise NotImplementedError(f"node embedding {node_emb['type']} is not implemented")
        try:
            node_emb['block_inside'] = get_block_inside[node_emb['block_inside']]
        except KeyError:
            raise NotImplementedError(f"block inside {node_emb['block_inside']} is not implemented")
        try:
            node_emb['block_init'] = get_block_init[node_emb['block_init']]
        except KeyError:
            raise NotImplementedError(f"block init {node_emb['block_init']} is not implemented")
        self.out_features = node_emb['out_features']
        self.node_embedder_dic = {'input': (None, []), 'ne': node_emb_type(original_features_num, **node_emb)}
        self.node_embedder = Network(self.node_embedder_dic)
        self.loss = triplet_loss()
        if metric is None or metric == 'linear_assignment':
            self.metric = accuracy_linear_assignment
        elif metric == 'max':
            self.metric = accuracy_max
        elif callable(metric):
            self.metric = metric
        else:
            raise ValueError('metric must be None, "linear_assignment", "max" or a callable (got %r)' % (metric,))
        if precision not in ('fp32', 'bf16'):
            raise ValueError('precision must be "fp32" or "bf16" (got %r)' % (precision,))
        if precision == 'bf16':
            self.node_embedder.half()
        if input_form not in ('dense', 'tensor_representation'):
            raise ValueError('input_form must be "dense" or "tensor_representation" (got %r)' % (input_form,))
        self.node_embedder.input_form = input_form
        self.lr, self.scheduler_decay, self.scheduler_step, self.lr_stop = lr, scheduler_decay, scheduler_step, lr_stop

    def half(self):
        """The reference's 16-bit switch on the whole model (pl.Trainer(precision=16), commander_explore.py:120-122): selects the bf16
        engine of the node embedder (Network.half) and returns self.  The parameters stay fp32 masters; nothing is cast."""
        self.node_embedder.half()
        return self

    def forward(self, x1, x2):
        """x1, x2: (bs, features, n, n) (or MaskedTensors of ragged graphs, both sides sharing the
        per-pair vertex counts) -> raw scores (bs, n, n)."""
        x1, x2 = _unwrap_input(x1), _unwrap_input(x2)
        ragged = isinstance(x1, MaskedTensor)
        if ragged:
            t = torch.cat([x1.tensor, x2.tensor])
            stacked = MaskedTensor(t, torch.cat([x1.nvalid, x2.nvalid]), x1.masked_dims, x1.base_name)
            nvalid = x1.nvalid
        else:
            stacked = torch.cat([x1, x2])
            nvalid = None
        e = self.node_embedder.fused_embedding(stacked)
        et = e.tensor if ragged else e
        B = et.shape[0] // 2
        scores = _ScoreFn.apply(et[:B], et[B:], nvalid)
        if ragged:
            return MaskedTensor(scores, nvalid, (1, 2), x1.base_name)
        return scores

    def _match_inputs(self, who, x1, x2, refine, labels, faq, seeds, seed_meter):
        """What `match` and `match_weighted` (who, in the messages) do before they decode: the refusals of faq, seeds and seed_meter,
        the eager forward under no_grad, the ragged batch unwrapped, labels and seeds cut to n and checked.
        -> (faq checked, scores as the model returned them, s / t1 / t2 their and the two sides' plain tensors, nv (B,) int32 or None,
        labels, seeds: a (B, n) int32 tensor, None, or the checked spec of evaluation.seed_spec, which the caller launches)"""
        from .evaluation import SeedMeter, _check_faq, seed_spec
        faq = _check_faq(who, faq)
        spec = seed_spec(who, seeds)
        if seed_meter is not None and (not isinstance(seed_meter, SeedMeter) or faq is None):
            raise ValueError('%s: seed_meter must be a SeedMeter and needs the faq= stage' % who)
        if seeds is not None and faq is None:
            raise ValueError('%s: seeds= needs the faq= stage (the Hungarian matching knows no fixed rows)' % who)
        if seeds is not None and refine:
            raise ValueError("%s: seeds= and refine > 0 do not go together (the reference's greedy_qap knows no fixed rows)" % who)
        a1, a2 = _unwrap_input(x1), _unwrap_input(x2)
        with torch.no_grad():
            scores = self(a1, a2)
            ragged = isinstance(scores, MaskedTensor)
            t1, t2 = (a1.tensor.rename(None), a2.tensor.rename(None)) if ragged else (a1, a2)
            s = scores.tensor.rename(None) if ragged else scores
            dev, B, N = s.device, s.shape[0], s.shape[-1]
            nv = a1.nvalid.to(device=dev, dtype=torch.int32).contiguous() if ragged else None
            if torch.is_tensor(labels) and labels.dim() == 2 and labels.shape[1] > N:
                labels = labels[:, :N]
            labels = labels_tensor(labels, B, N, dev)
            if torch.is_tensor(seeds) and seeds.dim() == 2 and seeds.shape[1] > N:
                seeds = seeds[:, :N]
            if spec is None:
                seeds = qap.check_seeds(who, seeds, B, N, dev)
            else:
                if N > qap._lib.FGNN_SEED_MAX_N:
                    raise RuntimeError('%s: seeds from the scores take at most %d vertices per graph (got %d)'
                                       % (who, qap._lib.FGNN_SEED_MAX_N, N))
                seeds = spec
        return faq, scores, s, t1, t2, nv, labels, seeds

    def match(self, x1, x2, refine=0, weighted=False, labels=None, two_opt=False, faq=None, seeds=None, seed_meter=None):
        """Decode a batch: the eager forward under no_grad (no `.grad` is touched), the Hungarian matching of -log_softmax(scores)
        and the reference's evaluation of it (toolbox/metrics.py:168-193 all_acc_qap), all on the device (qap.py).  Takes what
        `forward` takes.  Returns a dict: scores ((bs, n, n) tensor or MaskedTensor), assign ((bs, n) int32: the matched column of
        every row, -1 in the padding), and per pair acc (fixed points of the matching), qap, planted (int64).  refine=T > 0 adds the
        outputs of qap.greedy_qap(T) started from `assign`: s_best, na, nb, acc_best, T_best, perm (see its docstring for the
        reference's quirk: acc_best need not describe perm).  The batch must be a tensor representation -- channel 0 the 0/1
        adjacency -- whatever input_form the model was built with; it is verified on the device, and the one read of that verdict,
        after everything is queued, is the only host synchronisation.

        weighted=True decodes real-weighted batches -- the output of PairGenerator.spectral goes straight in: channel 0 of the batch
        is used as the matrices, as the reference's all_acc_qap does (qap.py, csrc/qap_weighted.hip).  No verdict is taken and nothing
        synchronises; the keys are the same, with qap, planted, s_best, na, nb as float32.

        labels (planted.py; a (bs, n) integer tensor, labels[b, i] = the vertex of x2 that vertex i of x1 is, or the reference's list
        of per-graph arrays; wider rows, such as a generator's (bs, N) labels beside a ragged batch cropped to its largest graph, are
        cut to n): acc and acc_best count the matches with the labels instead of the fixed points, and planted is the objective of
        the labels' matching.  None: the identity, as before.

        two_opt=True ends the decode in the pairwise-exchange search of qap.two_opt (one launch), started from the refinement's perm,
        or from assign when refine = 0: the dict gains -- as qap.two_opt names them -- perm (the polished matching, in place of the
        refinement's), qap_2opt (its objective, in the unit of qap), acc_2opt (its rows that meet the labels, or the identity), swaps,
        nit and status.  0/1 batches only: with weighted=True it is refused.

        faq (None, True or the dict evaluation.decode_scores takes) runs the Fast Approximate QAP stage after the Hungarian matching
        and before refine and two_opt, which then start from its matching: the Sinkhorn projection of the scores (or the barycenter)
        as the start, the chain of qap.faq, and where that chain reports status 2 the stage keeps assign.  The dict gains perm (the
        stage's matching, until a later stage replaces it), qap_faq and acc_faq (int64: its objective in the unit of qap, its rows
        that meet the labels or the identity), faq_perm, faq_nit, faq_status (as the chain left them) and sinkhorn_err (None with the
        barycenter).  0/1 batches only: with weighted=True it is refused.  With {'restarts': R, 'seed': ..} (and 'polish', 'index':
        qap.faq's random restarts, as evaluation.decode_scores takes them) the chain runs from R starts per pair -- the stage's own
        start and R - 1 perturbations of it -- and the best matching is kept on the device; the pair index is the position in the
        batch unless 'index' says otherwise.  The dict gains faq_restart ((bs,) int32, the winner's restart; None without restarts).

        seeds (None or a (bs, n) integer tensor of known matches: seeds[b, i] = j fixes vertex i of x1 to vertex j of x2, -1 leaves
        it free; wider rows are cut to n like labels; planted.reveal_seeds draws one): the anchors of seeded graph matching.  They
        need the faq= stage and exclude refine > 0 (ValueError otherwise).  Sinkhorn then runs on the free block of the scores, the
        seeded chain of qap.faq(seeds=) follows and two_opt=True runs the seeded exchange search, so faq_perm and perm hold every
        seed; assign and acc, the Hungarian stage, stay unseeded.  The dict gains seeded (int32: the seeds per pair).
        seeds may also be a spec -- 'scores', or {'from': 'scores', 'count': k, 'min_margin': x} -- the seeds the model's own scores
        give (qap.confident_seeds: rows whose best column picks them back with margin >= x, the k clearest; one launch on the scores
        the solver saw), under the same rules.  With any seeds the dict gains seeds ((bs, n) int32) and nseeds ((bs,) int32).
        seed_meter (an evaluation.SeedMeter, with faq=): the seeds that are right and the rows without a seed that the faq stage's
        and the final matching got right are added to it (fgnn_seed_fold, against the labels or the identity)."""
        if two_opt and weighted:
            raise NotImplementedError('match: two_opt=True runs on 0/1 adjacency only, not with weighted=True')
        if faq is not None and weighted:
            raise NotImplementedError('match: faq= runs on 0/1 adjacency only, not with weighted=True')
        from .evaluation import _BitPairs, _faq_launches, seed_fold
        faq, scores, s, t1, t2, nv, labels, seeds = self._match_inputs('match', x1, x2, refine, labels, faq, seeds, seed_meter)
        dev = s.device
        with torch.no_grad():
            nseeds = None
            if isinstance(seeds, dict):     # a spec: the seeds come from the scores the solver will see
                picked = qap.confident_seeds_device(s.detach().float(), nv, seeds['count'], seeds['min_margin'])
                seeds, nseeds = picked['seeds'], picked['nseeds']
            if weighted:
                correct, assign = lsap_device(s, nv, want_assign=True)
                obj = qap.objective_weighted(t1, t2, assign, nv)
                if labels is not None:
                    correct, obj['planted'] = count_matches(assign, labels, nv), qap.objective_weighted(t1, t2, labels, nv)['qap']
                out = {'scores': scores, 'assign': assign, 'acc': correct.to(torch.int64), 'qap': obj['qap'], 'planted': obj['planted']}
                if refine:
                    out.update(qap.greedy_weighted(t1, t2, assign, int(refine), nv, labels))
                return out
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            b1, b2 = qap.to_bits(t1, nv, flag), qap.to_bits(t2, nv, flag)
            correct, assign = lsap_device(s, nv, want_assign=True)
            obj = qap.objective_bits(b1, b2, assign, nv)
            if labels is not None:
                correct, obj['planted'] = count_matches(assign, labels, nv), qap.objective_bits(b1, b2, labels, nv)['qap']
            out = {'scores': scores, 'assign': assign, 'acc': correct.to(torch.int64), 'qap': obj['qap'], 'planted': obj['planted']}
            if faq is not None or two_opt:
                target = labels if labels is not None else torch.arange(s.shape[-1], dtype=torch.int32, device=dev).expand_as(assign).contiguous()
            if faq is not None:
                st = _faq_launches(_BitPairs(b1, b2), s.detach().float(), assign, obj['qap'].to(torch.int32), nv, s.shape[0], s.shape[-1],
                                   faq, seeds)
                if seeds is not None:
                    out['seeded'] = st['seeded']
                    out['seeds'], out['nseeds'] = seeds, st['seeded'] if nseeds is None else nseeds
                out.update({'perm': st['perm'], 'qap_faq': st['qap'].to(torch.int64),
                            'acc_faq': count_matches(st['perm'], target, nv).to(torch.int64), 'faq_perm': st['faq_perm'],
                            'faq_nit': st['faq_nit'], 'faq_status': st['faq_status'], 'sinkhorn_err': st['sinkhorn_err'],
                            'faq_restart': st['faq_restart']})
            if refine:
                out.update(qap.greedy_bits(b1, b2, out.get('perm', assign), int(refine), nv, labels))
            if two_opt:
                t = qap.two_opt_bits(b1, b2, out.get('perm', assign), nv, seeds=seeds)
                out.update({'perm': t['perm'], 'qap_2opt': t['qap'], 'acc_2opt': count_matches(t['perm'], target, nv).to(torch.int64),
                            'swaps': t['swaps'], 'nit': t['nit'], 'status': t['status']})
            if seed_meter is not None:
                seed_fold(seed_meter, seeds, st['perm'], out['perm'], nv, labels, None, s.shape[0], s.shape[-1], s.shape[0])
        self._raise_if_not_representation({'flag': flag})
        return out

    def match_weighted(self, x1, x2, refine=0, labels=None, two_opt=False, faq=None, seeds=None, seed_meter=None):
        """What `match` does for 0/1 batches, on REAL-weighted batches (the output of PairGenerator.spectral goes straight in: channel
        0 of the batch is used as the matrices, in place): the eager forward under no_grad, the Hungarian matching, and the chain of
        evaluation.decode_scores_weighted without a meter -- the faq= stage on fp32 (Sinkhorn start, seeds, restarts, polish), refine
        rounds of qap.greedy_weighted, and with two_opt=True the exchange search fgnn_qapw_2opt (fgnn_qapw_2opt_seeded with seeds).
        refine, labels, two_opt, faq, seeds, seed_meter: as `match` takes them, with its rules and messages (seeds need faq= and
        exclude refine > 0; 'scores' and dict specs are accepted).  Returns `match`'s keys -- scores, assign, acc, qap, planted; with
        faq perm, qap_faq, acc_faq, faq_perm, faq_nit, faq_status, sinkhorn_err, faq_restart (and seeded, seeds, nseeds); with refine
        the outputs of qap.greedy_weighted; with two_opt perm, qap_2opt, acc_2opt, swaps, nit, status -- the objectives as float32.
        With only refine the outputs equal ``match(weighted=True, refine=)`` bit for bit.  No verdict is taken and nothing
        synchronises.  `match` itself is unchanged, its refusals of weighted=True with two_opt / faq included."""
        from .evaluation import _WeightedPairs, _check_refine, _check_two_opt, _decode_launches
        who = 'match_weighted'
        refine, two_opt = _check_refine(who, refine), _check_two_opt(who, two_opt)
        faq, scores, s, t1, t2, nv, labels, seeds = self._match_inputs(who, x1, x2, refine, labels, faq, seeds, seed_meter)
        dev, B, N = s.device, s.shape[0], s.shape[-1]
        with torch.no_grad():
            pairs = _WeightedPairs.checked(who, t1, t2, B, N, dev)
            with torch.cuda.device(dev):
                correct, assign = lsap_device(s, nv, want_assign=True)
                if labels is not None:
                    correct = count_matches(assign, labels, nv)
                d = _decode_launches(pairs, assign, nv, labels, None, B, N, B, None, refine, two_opt, faq, s.detach().float(), seeds,
                                     seed_meter)
                out = {'scores': scores, 'assign': assign, 'acc': correct.to(torch.int64), 'qap': d['qap'], 'planted': d['planted']}
                if faq is not None or two_opt:
                    target = labels if labels is not None else torch.arange(N, dtype=torch.int32, device=dev).expand_as(assign).contiguous()
                if faq is not None:
                    if seeds is not None:
                        out.update({'seeded': d['seeded'], 'seeds': d['seeds'], 'nseeds': d['nseeds']})
                    failed = d['faq_status'] == 2
                    stage_perm = torch.where(failed[:, None], assign, d['faq_perm'])
                    out.update({'perm': stage_perm, 'qap_faq': torch.where(failed, d['qap'], d['faq_qap']),
                                'acc_faq': count_matches(stage_perm, target, nv).to(torch.int64), 'faq_perm': d['faq_perm'],
                                'faq_nit': d['faq_nit'], 'faq_status': d['faq_status'], 'sinkhorn_err': d['sinkhorn_err'],
                                'faq_restart': d['faq_restart']})
                if refine:
                    out.update(d['greedy'])
                if two_opt:
                    out.update({'perm': d['perm'], 'qap_2opt': d['refined'], 'acc_2opt': count_matches(d['perm'], target, nv).to(torch.int64),
                                'swaps': d['swaps'].to(torch.int64), 'nit': d['nit'], 'status': d['status'].to(torch.int64)})
        return out

    def fused_step(self, x1, x2, capture=True, metric=False, labels=None):
        """Forward of both branches + scoring + `triplet_loss` + the full backward (+ the step's metric, models/trainers.py:70-76)
        as the fused launch sequence of engine.FgnnEngine -- with capture=True ONE replayed HIP graph per (padded) batch shape,
        the step `bench.py` measures (the eager module path `loss = model.loss(model(x1, x2)); loss.backward()` of
        models/trainers.py:60-76 issues the same kernels but pays ~40 host launches and the autograd bookkeeping per step).
        Afterwards every trainable parameter's `.grad` is the gradient of this batch (views of one flat buffer, OVERWRITTEN
        per call like after `zero_grad()`), so any torch optimizer / scheduler steps as usual.

        Takes whatever the reference's loaders yield (loaders/loaders.py:5-15): tensors or {'input': T} dicts of constant-size
        batches, and MaskedTensor batches (both sides sharing the per-pair vertex counts).  A ragged batch runs zero-padded to its
        largest graph rounded up to a multiple of RAGGED_GRANULE = 8 (so batches of nearby sizes replay the same graph); the vertex counts and
        the loss normaliser 1 / sum(n) (toolbox/losses.py:27-34) live in device buffers that each call overwrites -- nothing
        about a batch is baked into the captured graph but its padded shape.  Models narrower than the engine (widths below 32,
        1 or 3..31 input channels) run on zero-padded parameters (Network._padded_layout): the scatter of the parameters and the
        gather of their gradients are part of the graph.  Widths / depths the engine is not built for (in_features > 32,
        depth_of_mlp > 3 ...) run the module path's own per-layer launch sequence, captured the same way.

        metric=True appends the model's matching accuracy (the default Hungarian accuracy or 'max', both device kernels) to the
        step: returns (loss, scores, (n_correct, n_vertices)) with the counts as DEVICE tensors -- no host synchronisation
        unless the caller reads them.  Returns (loss, raw scores) otherwise; scores are (bs, n, n) or a MaskedTensor; all outputs
        are device tensors that the NEXT call of the same shape overwrites.

        labels (an extension: the reference's target is always the identity): what metrics.labels_tensor takes, (bs, n) with
        labels[b, i] = the vertex of x2[b] that vertex i of x1[b] matches, -1 for none (wider rows are cut to n).  Loss and gradient
        are those of the cross-entropy against them and the metric counts matches with them; a labelled step
        is a captured graph of its own whose labels live in a static buffer each call overwrites.  On the module path's own launch
        sequence (non-standard widths) a labelled step runs eagerly."""
        x1, x2 = _unwrap_input(x1), _unwrap_input(x2)
        net = self.node_embedder
        lay = net._standard_layout()
        ragged = isinstance(x1, MaskedTensor)
        t1, t2 = (x1.tensor.rename(None), x2.tensor.rename(None)) if ragged else (x1, x2)
        if not t1.is_cuda:
            raise RuntimeError('graph_neural_net_amd only runs on the GPU (input is on %s)' % (t1.device,))
        builtin_metric = self.metric is accuracy_linear_assignment or self.metric is accuracy_max
        if labels is not None:
            if torch.is_tensor(labels) and labels.dim() == 2 and labels.shape[1] > t1.shape[-1]:
                labels = labels[:, :t1.shape[-1]]
            labels = labels_tensor(labels, t1.shape[0], t1.shape[-1], t1.device)
        mkw = {} if labels is None else {'labels': labels}
        if lay is None or (ragged and self.loss.loss_reduction != 'mean'):
            # widths / depths the fused engine is not built for (or a per-graph loss weighting the engine's scoring kernel does not
            # have): the module path's own launch sequence, captured once per batch shape and replayed (constant-size batches)
            if ragged:
                raise RuntimeError('fused_step: MaskedTensor batches need the standard node_embedding graph and loss_reduction="mean"; '
                                   'use the module path `loss = model.loss(model(x1, x2)); loss.backward()`')
            out = self._captured_module_step(t1, t2, capture and labels is None, labels)
            if metric:
                acc, n = self.metric(out[1], **mkw)
                return out + ((acc, n),)
            return out
        net._bind_flat()
        dev = t1.device
        B, nmax = t1.shape[0], t1.shape[-1]
        gran = max(1, int(self.RAGGED_GRANULE))
        N = -(-nmax // gran) * gran if ragged else nmax
        pad = net._pad
        # (the bf16 engine takes the batch's own channels: its input conversion writes the padded slab, fgnn_to_bf16_pad)
        c0e = pad['c0p'] if pad is not None and getattr(net, 'precision', 'fp32') != 'bf16' else t1.shape[1]
        if tuple(t1.shape) != tuple(t2.shape):
            raise RuntimeError('fused_step: the two sides of the batch have different (padded) shapes %s / %s; use the module path '
                               '`loss = model.loss(model(x1, x2)); loss.backward()`' % (tuple(t1.shape), tuple(t2.shape)))
        # input_form='tensor_representation': the loader's dense batch is bit-packed (and verified) on the device and block 1 runs on
        # its structured form -- where the kernels are built for the shape (2 input channels, depth 3, N <= 256); else the dense path
        want_tr = getattr(net, 'input_form', 'dense') == 'tensor_representation' and t1.shape[1] == 2 and lay.c0 == 2 \
            and t1.dtype == torch.float32
        eng = net._engine_for_shape(2 * B, N, ragged, dev, 'step', block1='structured' if want_tr else None)
        tr = want_tr and bool(getattr(eng, 'struct1', False))
        st = getattr(eng, '_step_state', None)
        if st is None:
            st = eng._step_state = {'x': None if tr else torch.zeros(2 * B, c0e, N, N, dtype=torch.float32, device=dev), 'graph': {},
                                    'nv': torch.zeros(2 * B, dtype=torch.int32, device=dev) if ragged else None,
                                    'inv': torch.ones(1, dtype=torch.float32, device=dev),
                                    'correct': torch.zeros(B, dtype=torch.int32, device=dev), 'nmax': N, 'calls': 0}
            if tr:      # (the verdict flag is the model's, shared by all batch shapes: check_input_form() reads one word)
                st['bits'] = torch.zeros(2 * B, N, (N + 31) // 32, dtype=torch.int32, device=dev)
                st['flag'] = self.__dict__.setdefault('_tr_flags', {}).setdefault(dev, torch.zeros(1, dtype=torch.int32, device=dev))
        c0 = t1.shape[1]
        lkw = {}
        if labels is not None:
            if st.get('labels') is None:
                st['labels'] = torch.full((B, N), -1, dtype=torch.int32, device=dev)
            st['labels'][:, :nmax].copy_(labels)
            if nmax < N:
                st['labels'][:, nmax:].fill_(-1)
            lkw = mkw = {'labels': st['labels']}        # (the metric sees the padded scores: it takes the padded labels)
        if getattr(net, 'precision', 'fp32') == 'bf16':
            net._check_channels(t1)
        first_of_shape = st['calls'] == 0
        st['calls'] += 1
        if ragged:
            if first_of_shape or (self.INPUT_CHECK_EVERY and st['calls'] % self.INPUT_CHECK_EVERY == 0):
                # both sides must share the per-pair vertex counts (the loss has target arange(n): toolbox/losses.py:27-34)
                if not torch.equal(x1.nvalid, x2.nvalid):
                    raise RuntimeError('fused_step: the two sides of a MaskedTensor batch must share the per-pair vertex counts; use '
                                       'the module path `loss = model.loss(model(x1, x2)); loss.backward()`')
            # Between those checks side 2 runs with side 1's counts (as FgnnTrainer does): a batch whose sides differ then still has the
            # reference's target / normaliser semantics for side 1 instead of silently mixing two sets of counts
            if not tr:
                st['nv'][:B].copy_(x1.nvalid)
                st['nv'][B:].copy_(x1.nvalid)
        if tr:
            # ONE launch straight from the loader's tensors, both sides: rows of ballots -> (2 B, N, ceil(N/32)) words of the engine's padded
            # size, with the verdict (channel 0 in {0, 1}, channel 1 = diag(row sums), counts within the padded size) OR-ed into a flag;
            # ragged batches: the same launch copies the vertex counts into the engine's buffer and leaves 1 / sum(n) in st['inv']
            nv1 = nv2 = None
            if ragged:
                nv1, nv2 = x1.nvalid, x1.nvalid            # (side 2 with side 1's counts, see above)
                if nv1.dtype != torch.int32 or not nv1.is_cuda or not nv1.is_contiguous() or nv2.dtype != torch.int32 \
                        or not nv2.is_cuda or not nv2.is_contiguous():
                    nv1, nv2 = nv1.to(device=dev, dtype=torch.int32).contiguous(), nv2.to(device=dev, dtype=torch.int32).contiguous()
            _lib.call('fgnn_pack_adjacency_pair', _lib.ptr(t1.contiguous()), _lib.ptr(t2.contiguous()),
                      _lib.ptr(nv1) if ragged else None, _lib.ptr(nv2) if ragged else None, B, nmax, N, _lib.ptr(st['bits']),
                      _lib.ptr(st['nv']) if ragged else None, _lib.ptr(st['inv']) if ragged else None, _lib.ptr(st['flag']),
                      _lib.stream_ptr())
            if first_of_shape or (self.INPUT_CHECK_EVERY and st['calls'] % self.INPUT_CHECK_EVERY == 0):
                self._raise_if_not_representation(st)
        elif ragged:
            if nmax < st['nmax']:                        # a smaller batch in the same workspace: the old values are padding now
                st['x'].zero_()
            st['x'][:B, :c0, :nmax, :nmax].copy_(t1)
            st['x'][B:, :c0, :nmax, :nmax].copy_(t2)
        else:
            st['x'][:B, :c0].copy_(t1)
            st['x'][B:, :c0].copy_(t2)
        st['nmax'] = nmax
        if st.get('flat') is not net._flat:             # (re)bound parameters: a captured graph holds the old addresses
            st['graph'], st['flat'] = {}, net._flat
        xin, bits = (None, st['bits']) if tr else (st['x'], None)

        def work():
            params = net._engine_params()                # the bound flat buffer, or its zero-padded image (an index_copy_)
            grads = net._flat_grad if pad is None else pad['pgrad']
            if ragged:
                # 1 / sum(n) on the device (one tiny launch): the scoring backward reads it as its gradient scale and the loss job of
                # the gradient-finalize launch multiplies it in -- no copy, no host round trip, nothing of the batch in the graph
                if not tr:      # (input_form='tensor_representation': the packing launch in front of the graph has written st['inv'])
                    _lib.call('fgnn_inv_node_count', _lib.ptr(st['nv']), B, _lib.ptr(st['inv']), _lib.stream_ptr())
                eng._loss_scale_dev = st['inv']
                scores, loss = eng.forward(params, xin, nvalid=st['nv'], total_nodes=1.0, defer_loss=True, bits=bits, **lkw)
                eng.backward(params, grads, gscale_dev=st['inv'])
            else:
                scores, loss = eng.step(params, grads, xin, bits=bits, **lkw)
            if pad is not None:
                torch.index_select(pad['pgrad'], 0, pad['idx'], out=net._flat_grad)
            if metric and in_graph_metric:
                nvp = _lib.ptr(st['nv']) if ragged else None
                if self.metric is accuracy_max:
                    _lib.call('fgnn_accuracy_max', _lib.ptr(scores), nvp, B, N, _lib.ptr(st['correct']), _lib.stream_ptr())
                else:               # -log_softmax over the valid columns, then SciPy's assignment on the device (metrics.py)
                    s = scores
                    if ragged:
                        col = torch.arange(N, device=dev)[None, None, :] < st['nv'][:B, None, None]
                        s = s.masked_fill(~col, float('-inf'))
                    cost = (-torch.log_softmax(s, -1)).contiguous()
                    _lib.call('fgnn_lsap_accuracy', _lib.ptr(cost), N * N, N, nvp, B, N, _lib.ptr(st['correct']), None, _lib.stream_ptr())
            return scores, loss

        in_graph_metric = builtin_metric and labels is None       # (with labels the metric is the module's own call after the step)
        key = bool(metric and in_graph_metric)                    # (the label-less graphs keep their keys: False / True)
        if labels is not None:
            key = (key, 'labels')
        if capture and st['graph'].get(key) is None:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):               # allocations, kernel attributes
                for _ in range(2):
                    work()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                st['out', key] = work()
            st['graph'][key] = g
        if capture:
            st['graph'][key].replay()
            scores, loss = st['out', key]
        else:
            scores, loss = work()
        for p, v in zip(net._param_list, net._grad_views):
            if p.requires_grad:
                p.grad = v
        if ragged:
            scores = MaskedTensor(scores, x1.nvalid, (1, 2), x1.base_name)
        if not metric:
            return loss.reshape(()), scores
        if in_graph_metric:
            total = st['nv'][:B].sum() if ragged else torch.tensor(B * N, device=dev)
            return loss.reshape(()), scores, (st['correct'].sum(), total)
        acc, n = self.metric(scores, **mkw)
        return loss.reshape(()), scores, (acc, n)

    @staticmethod
    def _raise_if_not_representation(st):
        if int(st['flag'].item()) != 0:             # (one host synchronisation)
            st['flag'].zero_()
            raise RuntimeError("fused_step(input_form='tensor_representation'): a batch since the last check is NOT the tensor "
                               'representation of a 0/1 adjacency (channel 0 in {0, 1}, channel 1 = diag(row sums), '
                               'loaders/data_generator.py:118-125) -- the structured block 1 does not apply and the results of those '
                               "steps are invalid; run it through the dense path (input_form='dense')")

    def check_input_form(self):
        """input_form='tensor_representation': read the device verdict of every fused_step since the last check now (one host
        synchronisation); raises if one of those batches was not a tensor representation.  True if there was something to check."""
        flags = self.__dict__.get('_tr_flags', {})
        for flag in flags.values():
            self._raise_if_not_representation({'flag': flag})
        return bool(flags)

    def _captured_module_step(self, x1, x2, capture, labels=None):
        """forward + loss + backward of the eager module path (models/trainers.py:60-76) as ONE replayed HIP graph per batch
        shape: the ~400 launches of a non-standard model cost the host nothing on replay.  Same contract as fused_step:
        every p.grad is overwritten per call, the returned tensors are overwritten by the next call of the same shape."""
        named = [(n, p) for n, p in self.named_parameters() if p.requires_grad]
        params = [p for _, p in named]

        def run(a, b):
            # The step differentiates fresh leaves that alias the parameters' storage, not the parameters themselves: a
            # parameter's AccumulateGrad node lives as long as ANY autograd graph that reached it (e.g. the caller's previous
            # `loss`), belongs to the stream it was created on, and the autograd engine synchronises with that stream --
            # which is not allowed inside a capture (the capture then dies in hipStreamEndCapture).
            leaves = {n: p.detach().requires_grad_(True) for n, p in named}
            scores = torch.func.functional_call(self, leaves, (a, b))
            loss = self.loss(scores) if labels is None else self.loss(scores, labels=labels)
            grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
            return loss.detach().reshape(()), scores.detach(), grads

        if not capture:
            loss, scores, grads = run(x1, x2)
            for p, gr in zip(params, grads):
                p.grad = gr
            return loss, scores
        steps = self.__dict__.setdefault('_module_steps', {})
        key = (tuple(x1.shape), tuple(x2.shape), x1.dtype, x1.device, tuple(id(p) for p in params))
        st = steps.pop(key, None)
        if st is None:
            # a handful of batch shapes, least recently used first out (each holds a graph's private memory pool; a loader that
            # cycles through more shapes than MODULE_STEPS_MAX re-captures -- ~400 launches x 4 -- on every miss: raise the bound)
            while len(steps) >= max(1, int(self.MODULE_STEPS_MAX)):
                steps.pop(next(iter(steps)))
            st = {'x1': torch.empty_like(x1), 'x2': torch.empty_like(x2), 'graph': None}
        steps[key] = st                                 # (re-)inserted last = most recently used
        st['x1'].copy_(x1)
        st['x2'].copy_(x2)
        if st['graph'] is None:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):               # allocations, kernel attributes, autograd's first-use set-up
                for _ in range(3):
                    run(st['x1'], st['x2'])
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                loss, scores, grads = run(st['x1'], st['x2'])
            if all(gr is None for gr in grads):
                raise RuntimeError('fused_step: no parameter received a gradient from the captured module step')
            st['out'], st['grads'], st['graph'] = (loss, scores), grads, g
        st['graph'].replay()
        for p, gr in zip(params, st['grads']):
            p.grad = gr
        return st['out']

    # -- the step methods of the reference's LightningModule (models/trainers.py:70-90); `log` is a no-op
    #    here and is overridden by whatever training shell wraps the module
    def log(self, name, value, **kwargs):
        pass

    def _shared_step(self, batch, prefix):
        """batch: (data1, data2) as the reference's loaders yield it, or (data1, data2, labels) -- an extension: loss and metric
        are then taken against the labels (PairGenerator.dense(permute=True) yields such batches)."""
        raw_scores = self(batch[0], batch[1])
        lkw = {'labels': batch[2]} if len(batch) > 2 and batch[2] is not None else {}
        if lkw:
            n = (raw_scores.tensor if isinstance(raw_scores, MaskedTensor) else raw_scores).shape[-1]
            if torch.is_tensor(batch[2]) and batch[2].dim() == 2 and batch[2].shape[1] > n:
                lkw = {'labels': batch[2][:, :n]}
        loss = self.loss(raw_scores, **lkw)
        self.log(prefix + '_loss', loss)
        acc, n = self.metric(raw_scores, **lkw)
        self.log(prefix + '_acc', acc / n)
        return loss

    def training_step(self, batch, batch_idx):
        return self._shared_step(batch, 'train')

    def validation_step(self, batch, batch_idx):
        self._shared_step(batch, 'val')

    def test_step(self, batch, batch_idx):
        self._shared_step(batch, 'test')

    def configure_optimizers(self):
        optimizer = torch.optim.Adam(self.parameters(), lr=self.lr, amsgrad=False)
        scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, factor=self.scheduler_decay,
                                                               patience=self.scheduler_step, min_lr=self.lr_stop)
        return {'optimizer': optimizer, 'lr_scheduler': {'scheduler': scheduler, 'monitor': 'val_loss', 'frequency': 1}}
