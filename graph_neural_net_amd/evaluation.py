"""Validation and test epochs on the device: the number the reference's ReduceLROnPlateau watches (val_loss,
models/trainers.py:78-104) and its evaluation of a trained model (all_losses_acc, toolbox/metrics.py:144-166).

``evaluate_scores`` turns a batch of raw scores into per-pair loss sums, arg-max hits and Hungarian matches with four launches
(csrc/eval.hip: fgnn_eval_pairs -- one pass that also writes the cost matrix of the solver; fgnn_lsap_accuracy;
fgnn_count_matches when there are labels; fgnn_eval_fold) and adds them to an ``EvalMeter``, a record in device memory whose sums
have a fixed order.  Nothing is read back until ``EvalMeter.result()``.  There is no CPU path (``_lib``).

``BinnedEvalMeter`` is K such records side by side and ``evaluate_scores(..., bins=)`` adds every pair to the record of its bin
(fgnn_eval_fold_bins in place of the fourth launch): the accuracy of a model across K noise levels from one pass
(``FgnnTrainer.noise_curve``), each record with the bits ``fgnn_eval_fold`` gives for its pairs alone.
"""
import ctypes

import numpy as np
import torch

from . import _lib, dp
from .masked import MaskedTensor
from .metrics import labels_tensor


class EvalMeter:
    """The device record of an evaluation epoch (fgnn_eval_record, include/fgnn_hip.h).  `ce_sum` (fp64), `nodes`, `correct_lsap`,
    `correct_max`, `pairs`, `steps` (int64) are 0-dim views of the record; `loss`, `acc`, `acc_max` are 0-dim fp64 device tensors
    formed from them on the device.  `result()` is the only host synchronisation."""

    FIELDS = ('ce_sum', 'nodes', 'correct_lsap', 'correct_max', 'pairs', 'steps')

    def __init__(self, device, buf=None):
        """buf: the record's bytes when they belong to a larger buffer (a record of a BinnedEvalMeter)"""
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('EvalMeter: device %s; the epoch record lives on the GPU (there is no CPU path)' % (device,))
        R = _lib.EvalRecord
        self.buf = torch.zeros(ctypes.sizeof(R), dtype=torch.uint8, device=device) if buf is None else buf
        self.ce_sum = self.buf[R.ce_sum.offset:R.ce_sum.offset + 8].view(torch.float64).reshape(())
        for name in self.FIELDS[1:]:
            off = getattr(R, name).offset
            setattr(self, name, self.buf[off:off + 8].view(torch.int64).reshape(()))

    def reset(self):
        self.buf.zero_()
        return self

    @property
    def loss(self):
        """ce_sum / nodes: triplet_loss('mean') of everything folded so far (NaN before the first node)"""
        return self.ce_sum / self.nodes.to(torch.float64)

    @property
    def acc(self):
        return self.correct_lsap.to(torch.float64) / self.nodes.to(torch.float64)

    @property
    def acc_max(self):
        return self.correct_max.to(torch.float64) / self.nodes.to(torch.float64)

    def record(self):
        """The record as a dict of Python numbers (one device-to-host copy)."""
        raw = self.buf.cpu().numpy().tobytes()
        rec = _lib.EvalRecord.from_buffer_copy(raw)
        return {name: getattr(rec, name) for name in self.FIELDS}

    def result(self):
        """{'loss', 'acc', 'acc_max', 'nodes', 'pairs'} of the epoch (one device-to-host copy: the one synchronisation)."""
        return record_result(self.record())

    def allreduce_(self):
        """Sum the record over the ranks: one all-reduce of 6 fp64 values (the counts are exact below 2^53)."""
        t = torch.stack([self.ce_sum] + [getattr(self, n).to(torch.float64) for n in self.FIELDS[1:]])
        dp.allreduce_sum_(t)
        self.ce_sum.copy_(t[0])
        for k, name in enumerate(self.FIELDS[1:], 1):
            getattr(self, name).copy_(t[k].round().to(torch.int64))
        return self


class BinnedEvalMeter:
    """K epoch records in one device buffer, one per bin (the noise levels of FgnnTrainer.noise_curve): `meter[k]` is an EvalMeter
    on record k's bytes (`loss`, `acc`, `acc_max` as device tensors, `record()`, `result()`).  values: K labels of the bins, carried
    as 'noise' in the dicts of `record()` / `result()`."""

    def __init__(self, device, K, values=None):
        K = int(K)
        if not 1 <= K <= _lib.FGNN_MAX_LEVELS:
            raise ValueError('BinnedEvalMeter: between 1 and %d records, got %d' % (_lib.FGNN_MAX_LEVELS, K))
        if values is not None and len(values) != K:
            raise ValueError('BinnedEvalMeter: %d values for %d records' % (len(values), K))
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('BinnedEvalMeter: device %s; the epoch records live on the GPU (there is no CPU path)' % (device,))
        size = ctypes.sizeof(_lib.EvalRecord)
        self.K, self.values = K, None if values is None else tuple(values)
        self.buf = torch.zeros(K * size, dtype=torch.uint8, device=device)
        self.meters = [EvalMeter(device, buf=self.buf[k * size:(k + 1) * size]) for k in range(K)]

    def __len__(self):
        return self.K

    def __getitem__(self, k):
        return self.meters[k]

    def reset(self):
        self.buf.zero_()
        return self

    def record(self):
        """The K records as dicts of Python numbers, with 'noise' when values were given (one device-to-host copy)."""
        raw = self.buf.cpu().numpy().tobytes()
        recs = (_lib.EvalRecord * self.K).from_buffer_copy(raw)
        out = [{name: getattr(r, name) for name in EvalMeter.FIELDS} for r in recs]
        if self.values is not None:
            for r, v in zip(out, self.values):
                r['noise'] = v
        return out

    def result(self):
        """record_result of every record, with 'noise' when values were given (one device-to-host copy: the one synchronisation)."""
        out = []
        for rec in self.record():
            res = record_result(rec)
            if 'noise' in rec:
                res['noise'] = rec['noise']
            out.append(res)
        return out

    def allreduce_(self):
        """Sum the records over the ranks: one all-reduce of K x 6 fp64 values (the counts are exact below 2^53)."""
        words = self.buf.view(torch.int64).view(self.K, len(EvalMeter.FIELDS))
        ce = self.buf.view(torch.float64).view(self.K, len(EvalMeter.FIELDS))[:, :1]
        t = torch.cat([ce, words[:, 1:].to(torch.float64)], dim=1).contiguous()
        dp.allreduce_sum_(t)
        ce.copy_(t[:, :1])
        words[:, 1:].copy_(t[:, 1:].round().to(torch.int64))
        return self


def record_result(rec):
    """The reference's figures from a record: loss = ce_sum / nodes (toolbox/losses.py:27-34), acc = matches / nodes
    (toolbox/metrics.py:107-114).  An empty record gives NaN, the 0 / 0 of the reference."""
    nodes = rec['nodes']
    div = (lambda a: a / nodes) if nodes else (lambda a: float('nan'))
    return {'loss': div(rec['ce_sum']), 'acc': div(rec['correct_lsap']), 'acc_max': div(rec['correct_max']),
            'nodes': nodes, 'pairs': rec['pairs']}


def evaluate_scores(scores, nvalid=None, labels=None, meter=None, live=None, hungarian=True, loss_on_labels=False, bins=None):
    """scores: (B, N, N) fp32 raw scores on the GPU, or a MaskedTensor of them (its vertex counts are used unless nvalid is given).
    nvalid: (B,) vertex counts in [0, N]; labels: see metrics.py (None: the identity; they enter the accuracies, never the loss).
    live: the first `live` pairs count (None: all B) -- the others, the filling of a short last step, are ignored entirely.
    loss_on_labels=True: the labels enter the loss as well -- 'ce' and the meter's ce_sum are the cross-entropy against labels[b, i]
    (fgnn_eval_pairs_labels; a row whose label lies outside [0, n_b) adds nothing; the node count still counts it), the loss of a
    model trained with train_step(labels=...).  Without labels it changes nothing.
    hungarian=False leaves the solver out (correct_lsap stays 0, assign is None).
    Adds the live pairs to `meter` (an EvalMeter; None: a fresh one, returned under 'meter') and returns the per-pair device
    tensors {'ce': (B,) fp64 CE sums, 'n': (B,) int32 vertex counts, 'correct_max', 'correct_lsap': (B,) int32, 'assign': (B, N) int32
    matched columns, -1 in the padding}; entries of pairs >= live are zero in ce / correct_max and not meaningful elsewhere.
    bins: a (B,) integer device tensor with a BinnedEvalMeter as `meter` (the two go together): live pair b is added to record
    bins[b] of the meter, a pair whose bin lies outside [0, K) to none (fgnn_eval_fold_bins as the fourth launch; the other three
    and everything returned are the same).
    Four launches, nothing is read back."""
    if isinstance(meter, BinnedEvalMeter) != (bins is not None):
        raise ValueError('evaluate_scores: bins= and a BinnedEvalMeter as meter go together')
    if isinstance(scores, MaskedTensor):
        if nvalid is None:
            nvalid = scores.nvalid
        scores = scores.tensor
    if not torch.is_tensor(scores) or scores.dim() != 3 or scores.shape[1] != scores.shape[2] or not scores.is_floating_point():
        raise ValueError('evaluate_scores: expected (B, N, N) floating-point scores, got %s'
                         % (tuple(scores.shape) if torch.is_tensor(scores) else type(scores).__name__,))
    if not scores.is_cuda:
        raise RuntimeError('evaluate_scores: scores on %s; the evaluation runs on the GPU only (there is no CPU path)' % (scores.device,))
    B, N, _ = scores.shape
    if B < 1 or N < 1:
        raise ValueError('evaluate_scores: empty batch %s' % (tuple(scores.shape),))
    if N > _lib.FGNN_LSAP_MAX_N:
        raise RuntimeError('evaluate_scores: at most %d vertices per graph (got %d)' % (_lib.FGNN_LSAP_MAX_N, N))
    live = B if live is None else int(live)
    if not 0 <= live <= B:
        raise ValueError('evaluate_scores: live = %d outside [0, %d]' % (live, B))
    dev = scores.device
    if nvalid is not None:
        if not torch.is_tensor(nvalid) or tuple(nvalid.shape) != (B,) or nvalid.is_floating_point():
            raise ValueError('evaluate_scores: nvalid must be a (%d,) integer tensor' % B)
        nvalid = nvalid.to(device=dev, dtype=torch.int32).contiguous()
    labels = labels_tensor(labels, B, N, dev)
    if bins is not None:
        if not torch.is_tensor(bins) or tuple(bins.shape) != (B,) or bins.is_floating_point() or bins.dtype == torch.bool:
            raise ValueError('evaluate_scores: bins must be a (%d,) integer tensor' % B)
        if meter.buf.device != dev:
            raise ValueError('evaluate_scores: meter must be a BinnedEvalMeter on %s' % (dev,))
        bins = bins.to(device=dev, dtype=torch.int32).contiguous()
    elif meter is None:
        meter = EvalMeter(dev)
    elif not isinstance(meter, EvalMeter) or meter.buf.device != dev:
        raise ValueError('evaluate_scores: meter must be an EvalMeter on %s' % (dev,))
    s = scores.detach().to(torch.float32).contiguous()
    with torch.cuda.device(dev):
        i32 = dict(dtype=torch.int32, device=dev)
        cost = torch.empty(B, N, N, dtype=torch.float32, device=dev)
        row_ce = torch.empty(B, N, dtype=torch.float32, device=dev)
        row_hit = torch.empty(B, N, **i32)
        pair_ce = torch.zeros(B, dtype=torch.float64, device=dev)
        pair_max = torch.zeros(B, **i32)
        correct = torch.zeros(B, **i32)
        assign = None
        st = _lib.stream_ptr()
        _lib.call('fgnn_eval_pairs_labels' if loss_on_labels and labels is not None else 'fgnn_eval_pairs', _lib.ptr(s), _lib.ptr(nvalid), _lib.ptr(labels), B, N, _lib.ptr(cost), N * N, N,
                  _lib.ptr(row_ce), _lib.ptr(row_hit), st)
        if hungarian:
            assign = torch.empty(B, N, **i32)
            _lib.call('fgnn_lsap_accuracy', _lib.ptr(cost), N * N, N, _lib.ptr(nvalid), B, N, _lib.ptr(correct), _lib.ptr(assign), st)
            if labels is not None:
                _lib.call('fgnn_count_matches', _lib.ptr(assign), _lib.ptr(labels), _lib.ptr(nvalid), B, N, _lib.ptr(correct), st)
        if bins is None:
            _lib.call('fgnn_eval_fold', _lib.ptr(row_ce), _lib.ptr(row_hit), _lib.ptr(correct) if hungarian else None, _lib.ptr(nvalid),
                      B, N, live, _lib.ptr(pair_ce), _lib.ptr(pair_max), _lib.ptr(meter.buf), st)
        else:
            _lib.call('fgnn_eval_fold_bins', _lib.ptr(row_ce), _lib.ptr(row_hit), _lib.ptr(correct) if hungarian else None,
                      _lib.ptr(nvalid), B, N, live, _lib.ptr(bins), meter.K, _lib.ptr(pair_ce), _lib.ptr(pair_max), _lib.ptr(meter.buf), st)
    n = nvalid if nvalid is not None else torch.full((B,), N, **i32)
    return {'ce': pair_ce, 'n': n, 'correct_max': pair_max, 'correct_lsap': correct, 'assign': assign, 'meter': meter}


def all_losses_acc(batches, model, eval_score='linear_assignment', labels=None):
    """The reference's all_losses_acc (toolbox/metrics.py:144-166) over an iterable of (data1, data2) batches as `model` takes
    them: -> (np.array of the per-batch losses ce_sum_batch / nodes_batch, np.array of the per-pair accuracies).
    eval_score: 'linear_assignment' (the Hungarian accuracy), 'max' (arg-max) or None (losses only, an empty accuracy array).
    labels: None, or one labels argument (metrics.py) per batch.  The model's eager forward runs under no_grad, evaluate_scores
    per batch; the ONE host copy comes at the end."""
    if eval_score not in ('linear_assignment', 'max', None):
        raise ValueError("eval_score must be 'linear_assignment', 'max' or None (got %r)" % (eval_score,))
    batches = list(batches)
    if labels is not None and len(labels) != len(batches):
        raise ValueError('all_losses_acc: %d labels entries for %d batches' % (len(labels), len(batches)))
    losses, accs = [], []
    with torch.no_grad():
        for k, (d1, d2) in enumerate(batches):
            out = evaluate_scores(model(d1, d2), labels=None if labels is None else labels[k],
                                  hungarian=eval_score == 'linear_assignment')
            losses.append(out['meter'].loss.reshape(1))
            if eval_score is not None:
                hits = out['correct_lsap'] if eval_score == 'linear_assignment' else out['correct_max']
                accs.append(hits.to(torch.float64) / out['n'].to(torch.float64))
    if not batches:
        return np.zeros(0), np.zeros(0)
    flat = torch.cat(losses + accs).cpu().numpy()
    return flat[:len(losses)].copy(), flat[len(losses):].copy()
