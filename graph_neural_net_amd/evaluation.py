"""Validation and test epochs on the device: the number the reference's ReduceLROnPlateau watches (val_loss,
models/trainers.py:78-104) and its evaluation of a trained model (all_losses_acc, toolbox/metrics.py:144-166).

``evaluate_scores`` turns a batch of raw scores into per-pair loss sums, arg-max hits and Hungarian matches with four launches
(csrc/eval.hip: fgnn_eval_pairs -- one pass that also writes the cost matrix of the solver; fgnn_lsap_accuracy;
fgnn_count_matches when there are labels; fgnn_eval_fold) and adds them to an ``EvalMeter``, a record in device memory whose sums
have a fixed order.  Nothing is read back until ``EvalMeter.result()``.  There is no CPU path (``_lib``).

``BinnedEvalMeter`` is K such records side by side and ``evaluate_scores(..., bins=)`` adds every pair to the record of its bin
(fgnn_eval_fold_bins, the same kernel, as the fourth launch): the accuracy of a model across K noise levels from one pass
(``FgnnTrainer.noise_curve``), each record with the bits ``fgnn_eval_fold`` gives for its pairs alone.

``rank_scores`` gives the rank of every row's true match and the Hits@k / reciprocal-rank sums with two launches (csrc/rank.hip:
fgnn_eval_ranks, fgnn_rank_fold) into a ``RankMeter`` or, with ``bins=``, a ``BinnedRankMeter``; ``evaluate_scores(...,
rank_meter=)`` issues them after its own four, on the same scores, labels, ``live`` and bins.

``decode_scores`` is the epoch form of the reference's ``all_acc_qap(val_loader, ...)`` / ``all_greedy_losses_acc``
(toolbox/metrics.py:168-223): the Hungarian matching, its QAP objective and the planted one on the pairs' bit words (csrc/qap.hip),
optionally the greedy refinement and, with ``two_opt=True``, the pairwise-exchange search after it (csrc/qap_2opt.hip), and
fgnn_qap_fold (csrc/qap_fold.hip) into a ``QapMeter`` or, with ``bins=``, a ``BinnedQapMeter``; ``evaluate_scores(..., qap_meter=,
bits=, refine=, two_opt=)`` issues it after its own launches on the assignment its solver launch wrote.  0/1 graphs only; the
real-weighted decode is ``decode_scores_weighted`` (a ``WeightedQapMeter``; ``evaluate_scores(..., adj=)``).  The two are ONE chain
(``_decode_launches``, ``_faq_launches``) over a pair operand, ``_BitPairs`` or ``_WeightedPairs``, which holds what differs: the
objective, the matrices of the FAQ chain, the refinement and search wrappers, the fold entry point and the meter classes.  ``faq=`` puts the Fast Approximate QAP chain
(csrc/qap_faq.hip) between the Hungarian matching and the refinement, started from the Sinkhorn projection of the scores
(csrc/sinkhorn.hip) or from the barycenter.

``seeds=`` of the decode takes known matches -- a tensor, or a spec that draws them from the scores themselves (csrc/seed_select.hip:
fgnn_confident_seeds) -- and ``seed_meter=`` a ``SeedMeter`` / ``BinnedSeedMeter`` that says what the seeds were worth.

The eight meters are one thing -- records of one ctypes struct in one device buffer (``_Records``) -- with four record types.
"""
import ctypes

import numpy as np
import torch

from . import _lib, dp, qap
from .masked import MaskedTensor
from .metrics import labels_tensor


def pack_records(buf, K, words, head=1):
    """The bytes of K records of `words` 8-byte words each (a uint8 tensor on any device) -> the (K, words) fp64 tensor of their
    all-reduce: the first `head` words, fp64 sums (one, word 0, in every record but fgnn_qapw_record, which has four), as they are,
    the int64 counts converted (exact below 2^53).  A pure function of tensors."""
    counts = buf.view(torch.int64).view(K, words)[:, head:]
    return torch.cat([buf.view(torch.float64).view(K, words)[:, :head], counts.to(torch.float64)], dim=1).contiguous()


def unpack_records_(buf, K, t, head=1):
    """The inverse of pack_records: writes the (K, words) fp64 tensor t into the records' bytes, in place."""
    words = t.shape[1]
    buf.view(torch.float64).view(K, words)[:, :head].copy_(t[:, :head])
    buf.view(torch.int64).view(K, words)[:, head:].copy_(t[:, head:].round().to(torch.int64))
    return buf


def _read(*meters):
    """ONE device-to-host copy of several meters' bytes -> per meter the ctypes array of its records"""
    bufs = [m.buf for m in meters]
    raw = (bufs[0] if len(bufs) == 1 else torch.cat(bufs)).cpu().numpy().tobytes()
    out, at = [], 0
    for m in meters:
        n = m.buf.numel()
        out.append((m.RECORD * (n // ctypes.sizeof(m.RECORD))).from_buffer_copy(raw[at:at + n]))
        at += n
    return out


class _Records:
    """What the four meters share: records of one ctypes struct (RECORD: word 0 an fp64 sum, every other word an int64 count) in one
    device buffer `buf`, read with one device-to-host copy and summed over the ranks with one all-reduce.  A plain meter is one
    record, its FIELDS 0-dim views of `buf`; a binned meter (_BinnedRecords) is K of them side by side.  A record type adds
    `_dict` (a ctypes record -> a dict of Python numbers) and `_result` (that dict -> the epoch's figures)."""
    RECORD, FIELDS, NOUN = None, (), 'record lives'
    HEAD_FP64 = True            # word 0 is an fp64 sum (False: every word is an int64 count)
    HEAD_WORDS = 1              # with HEAD_FP64: how many leading words are fp64 sums

    def _open(self, device, K=1, buf=None):
        """The device refusal, then K zeroed records -- or `buf`, the bytes of one record of a binned meter.  -> the device"""
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('%s: device %s; the epoch %s on the GPU (there is no CPU path)' % (type(self).__name__, device, self.NOUN))
        self.buf = torch.zeros(K * ctypes.sizeof(self.RECORD), dtype=torch.uint8, device=device) if buf is None else buf
        for j, name in enumerate(self.FIELDS):              # (a binned meter has none: its records' fields are its meters')
            off = getattr(self.RECORD, name).offset
            fp64 = self.HEAD_FP64 and j < self.HEAD_WORDS
            setattr(self, name, self.buf[off:off + 8].view(torch.float64 if fp64 else torch.int64).reshape(()))
        return device

    def reset(self):
        self.buf.zero_()
        return self

    def record(self):
        """The record as a dict of Python numbers (one device-to-host copy)."""
        return self._dict(_read(self)[0][0])

    def result(self):
        """The figures of the epoch (one device-to-host copy: the one synchronisation)."""
        return self._result(self.record())

    def allreduce_(self):
        """Sum the records over the ranks: one all-reduce of one fp64 value per 8-byte word (the counts are exact below 2^53)."""
        words = ctypes.sizeof(self.RECORD) // 8
        K = self.buf.numel() // (8 * words)
        if not self.HEAD_FP64:
            t = self.buf.view(torch.int64).to(torch.float64)
            dp.allreduce_sum_(t)
            self.buf.view(torch.int64).copy_(t.round().to(torch.int64))
            return self
        t = pack_records(self.buf, K, words, self.HEAD_WORDS)
        dp.allreduce_sum_(t)
        unpack_records_(self.buf, K, t, self.HEAD_WORDS)
        return self


class _BinnedRecords(_Records):
    """K records in one device buffer, one per bin (the noise levels of FgnnTrainer.noise_curve): `meter[k]` is a plain meter of
    class PLAIN on record k's bytes.  values: K labels of the bins, carried as 'noise' in the dicts of `record()` / `result()`."""
    PLAIN, FIELDS, NOUN = None, (), 'records live'

    @classmethod
    def _check_bins(cls, K, values):
        K = int(K)
        if not 1 <= K <= _lib.FGNN_MAX_LEVELS:
            raise ValueError('%s: between 1 and %d records, got %d' % (cls.__name__, _lib.FGNN_MAX_LEVELS, K))
        if values is not None and len(values) != K:
            raise ValueError('%s: %d values for %d records' % (cls.__name__, len(values), K))
        return K

    def _open_bins(self, device, K, values, **own):
        device = self._open(device, K)
        size = ctypes.sizeof(self.RECORD)
        self.K, self.values = K, None if values is None else tuple(values)
        self.meters = [self.PLAIN(device, buf=self.buf[k * size:(k + 1) * size], **own) for k in range(K)]

    def __len__(self):
        return self.K

    def __getitem__(self, k):
        return self.meters[k]

    def record(self):
        """The K records as dicts of Python numbers, with 'noise' when values were given (one device-to-host copy)."""
        out = [m._dict(r) for m, r in zip(self.meters, _read(self)[0])]
        for rec, v in zip(out, self.values or ()):
            rec['noise'] = v
        return out

    def result(self):
        """The figures of every record, with 'noise' when values were given (one device-to-host copy: the one synchronisation)."""
        out = [m._result(rec) for m, rec in zip(self.meters, self.record())]
        for res, v in zip(out, self.values or ()):
            res['noise'] = v
        return out


def record_result(rec):
    """The reference's figures from a record: loss = ce_sum / nodes (toolbox/losses.py:27-34), acc = matches / nodes
    (toolbox/metrics.py:107-114).  An empty record gives NaN, the 0 / 0 of the reference."""
    nodes = rec['nodes']
    div = (lambda a: a / nodes) if nodes else (lambda a: float('nan'))
    return {'loss': div(rec['ce_sum']), 'acc': div(rec['correct_lsap']), 'acc_max': div(rec['correct_max']),
            'nodes': nodes, 'pairs': rec['pairs']}


class EvalMeter(_Records):
    """The device record of an evaluation epoch (fgnn_eval_record, include/fgnn_hip.h).  `ce_sum` (fp64), `nodes`, `correct_lsap`,
    `correct_max`, `pairs`, `steps` (int64) are 0-dim views of the record; `loss`, `acc`, `acc_max` are 0-dim fp64 device tensors
    formed from them on the device.  `result()`, {'loss', 'acc', 'acc_max', 'nodes', 'pairs'}, is the only host synchronisation."""
    RECORD, FIELDS = _lib.EvalRecord, ('ce_sum', 'nodes', 'correct_lsap', 'correct_max', 'pairs', 'steps')
    _result = staticmethod(record_result)

    def __init__(self, device, buf=None):
        """buf: the record's bytes when they belong to a larger buffer (a record of a BinnedEvalMeter)"""
        self._open(device, buf=buf)

    def _dict(self, rec):
        return {name: getattr(rec, name) for name in self.FIELDS}

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


class BinnedEvalMeter(_BinnedRecords):
    """K epoch records, one per bin: `meter[k]` is an EvalMeter (`loss`, `acc`, `acc_max` as device tensors, `record()`,
    `result()`); see _BinnedRecords."""
    PLAIN, RECORD = EvalMeter, _lib.EvalRecord

    def __init__(self, device, K, values=None):
        self._open_bins(device, self._check_bins(K, values), values)


def check_ks(ks):
    """The thresholds of a rank meter as a tuple of ints: 1 to FGNN_RANK_MAX_K of them, positive, strictly increasing."""
    try:
        ks = tuple(ks)
    except TypeError:
        raise ValueError('ks must be a sequence of integers, got %r' % (ks,))
    if not 1 <= len(ks) <= _lib.FGNN_RANK_MAX_K:
        raise ValueError('ks: between 1 and %d thresholds, got %d' % (_lib.FGNN_RANK_MAX_K, len(ks)))
    if any(isinstance(k, bool) or int(k) != k for k in ks):
        raise ValueError('ks must be integers, got %r' % (ks,))
    ks = tuple(int(k) for k in ks)
    if ks[0] < 1 or any(b <= a for a, b in zip(ks, ks[1:])) or ks[-1] > 0x7fffffff:
        raise ValueError('ks must be positive and strictly increasing, got %r' % (ks,))
    return ks


def rank_record_dict(rec, ks):
    out = {name: getattr(rec, name) for name in RankMeter.FIELDS}
    out['hits'] = {k: rec.hits[q] for q, k in enumerate(ks)}
    return out


def rank_result(rec):
    """Hits@k = hits[k] / targets, MRR = rr_sum / targets, the mean rank = rank_sum / targets: ratios over the rows that have a
    target.  An empty record gives NaN."""
    targets = rec['targets']
    div = (lambda a: a / targets) if targets else (lambda a: float('nan'))
    out = {'hits@%d' % k: div(h) for k, h in rec['hits'].items()}
    out.update({'mrr': div(rec['rr_sum']), 'mean_rank': div(rec['rank_sum']), 'targets': targets, 'nodes': rec['nodes'],
                'pairs': rec['pairs']})
    return out


class RankMeter(_Records):
    """The device record of the rank metrics of an evaluation epoch (fgnn_rank_record, include/fgnn_hip.h) for the thresholds `ks`
    (1 to FGNN_RANK_MAX_K positive, strictly increasing integers).  `rr_sum` (fp64), `rank_sum`, `targets`, `nodes`, `pairs`, `steps`
    (int64) are 0-dim views of the record, `hits[q]` the view of the count for ks[q]; `mrr`, `mean_rank` and `hits_at(k)` are 0-dim
    fp64 device tensors formed from them on the device.  `record()` has 'hits' as {k: count}; `result()`, {'hits@k' for every k,
    'mrr', 'mean_rank', 'targets', 'nodes', 'pairs'}, is the only host synchronisation."""
    RECORD, FIELDS = _lib.RankRecord, ('rr_sum', 'rank_sum', 'targets', 'nodes', 'pairs', 'steps')
    _result = staticmethod(rank_result)

    def __init__(self, device, ks=(1, 5, 10), buf=None):
        """buf: the record's bytes when they belong to a larger buffer (a record of a BinnedRankMeter)"""
        self.ks = check_ks(ks)
        self._open(device, buf=buf)
        off = _lib.RankRecord.hits.offset
        self.hits = [self.buf[off + 8 * q:off + 8 * q + 8].view(torch.int64).reshape(()) for q in range(len(self.ks))]

    def _dict(self, rec):
        return rank_record_dict(rec, self.ks)

    @property
    def mrr(self):
        """rr_sum / targets: the mean reciprocal rank of everything folded so far (NaN before the first target)"""
        return self.rr_sum / self.targets.to(torch.float64)

    @property
    def mean_rank(self):
        return self.rank_sum.to(torch.float64) / self.targets.to(torch.float64)

    def hits_at(self, k):
        return self.hits[self.ks.index(int(k))].to(torch.float64) / self.targets.to(torch.float64)


class BinnedRankMeter(_BinnedRecords):
    """K rank records, one per bin: `meter[k]` is a RankMeter of the same `ks`; see _BinnedRecords."""
    PLAIN, RECORD = RankMeter, _lib.RankRecord

    def __init__(self, device, K, ks=(1, 5, 10), values=None):
        K = self._check_bins(K, values)
        self.ks = check_ks(ks)
        self._open_bins(device, K, values, ks=self.ks)


def qap_result(rec):
    """The decode figures of an epoch from a QapRecord dict: 'acc' = correct / nodes (the accuracy of all_acc_qap's matching),
    'qap_ratio' = qap_sum / planted_sum (the recovered objective over the planted one, the figure quoted across noise levels),
    'mean_ratio' = ratio_sum / ratio_pairs (the mean of the per-pair ratios), 'recovered' and 'exact' as fractions of the pairs,
    'unmatched', 'nodes', 'pairs'; and, when a refinement was folded (rec['refined'], which a meter's record carries):
    'refined_acc' = refined_correct / nodes, 'refined_qap_ratio' = refined_sum / planted_sum, 'improved' as a fraction of the
    pairs.  An empty denominator gives NaN."""
    div = lambda a, b: a / b if b else float('nan')
    out = {'acc': div(rec['correct'], rec['nodes']), 'qap_ratio': div(rec['qap_sum'], rec['planted_sum']),
           'mean_ratio': div(rec['ratio_sum'], rec['ratio_pairs']), 'recovered': div(rec['recovered'], rec['pairs']),
           'exact': div(rec['exact'], rec['pairs']), 'unmatched': rec['unmatched'], 'nodes': rec['nodes'], 'pairs': rec['pairs']}
    if rec.get('refined'):
        out.update({'refined_acc': div(rec['refined_correct'], rec['nodes']),
                    'refined_qap_ratio': div(rec['refined_sum'], rec['planted_sum']), 'improved': div(rec['improved'], rec['pairs'])})
    return out


class _QapRecords(_Records):
    """What the 0/1 and the real-weighted decode record share: `refined` (host: whether a refinement was folded since the last
    reset, carried by `record()`), the derived device tensors and `result()` (qap_result).  A subclass names its RECORD, FIELDS and
    HEAD_WORDS."""
    _result = staticmethod(qap_result)

    def __init__(self, device, buf=None):
        """buf: the record's bytes when they belong to a larger buffer (a record of the binned meter)"""
        self.refined = False
        self._open(device, buf=buf)

    def reset(self):
        self.refined = False
        return super().reset()

    def _mark_refined(self):
        self.refined = True

    def _dict(self, rec):
        out = {name: getattr(rec, name) for name in self.FIELDS}
        out['refined'] = self.refined
        return out

    def _over(self, a, b):
        return a.to(torch.float64) / b.to(torch.float64)

    @property
    def acc(self):
        """correct / nodes of everything folded so far (NaN before the first node)"""
        return self._over(self.correct, self.nodes)

    @property
    def qap_ratio(self):
        return self._over(self.qap_sum, self.planted_sum)

    @property
    def mean_ratio(self):
        return self.ratio_sum / self.ratio_pairs.to(torch.float64)

    @property
    def refined_acc(self):
        return self._over(self.refined_correct, self.nodes)

    @property
    def refined_qap_ratio(self):
        return self._over(self.refined_sum, self.planted_sum)


class _BinnedQapRecords(_BinnedRecords):
    """K decode records, one per bin, with the `refined` of _QapRecords kept on every one of them; see _BinnedRecords."""

    def __init__(self, device, K, values=None):
        self._open_bins(device, self._check_bins(K, values), values)

    @property
    def refined(self):
        return self.meters[0].refined

    def reset(self):
        for m in self.meters:
            m.refined = False
        return super().reset()

    def _mark_refined(self):
        for m in self.meters:
            m.refined = True


class QapMeter(_QapRecords):
    """The device record of a decode epoch (fgnn_qap_record, include/fgnn_hip.h): the reference's all_acc_qap(val_loader, ...) and
    all_greedy_losses_acc (toolbox/metrics.py:168-223) over a whole loader, for 0/1 graphs on the bit-word path (the real-weighted
    decode, qap.py's weighted=True, has its own meter, WeightedQapMeter).  Every field of the record is a 0-dim view of it
    (`ratio_sum` fp64, the others int64); `acc`, `qap_ratio`, `mean_ratio`, `refined_acc`, `refined_qap_ratio` are 0-dim fp64 device tensors formed from
    them on the device.  `refined` (host) says whether a refinement was folded since the last reset; `record()` carries it and
    `result()` (qap_result) is the only host synchronisation."""
    RECORD, FIELDS = _lib.QapRecord, tuple(name for name, _ in _lib.QapRecord._fields_)


class BinnedQapMeter(_BinnedQapRecords):
    """K decode records, one per bin: `meter[k]` is a QapMeter; see _BinnedRecords."""
    PLAIN, RECORD = QapMeter, _lib.QapRecord


class WeightedQapMeter(_QapRecords):
    """The device record of a decode epoch on REAL-weighted pairs (fgnn_qapw_record, include/fgnn_hip.h; csrc/qap_fold_weighted.hip):
    what QapMeter is for 0/1 graphs, over the fp32 objectives of csrc/qap_weighted.hip.  `ratio_sum`, `qap_sum`, `planted_sum`,
    `refined_sum` are 0-dim fp64 views of the record, the ten counts int64; `unmatched` counts the pairs whose matching leaves the
    corner (a weighted objective may be negative, so its sign marks nothing).  The derived tensors, `refined`, `record()` and
    `result()` (qap_result: the same keys) are QapMeter's (_QapRecords).  A class of its own: decode_scores refuses it, decode_scores_weighted
    refuses a QapMeter."""
    RECORD, FIELDS, HEAD_WORDS = _lib.QapwRecord, tuple(name for name, _ in _lib.QapwRecord._fields_), 4


class BinnedWeightedQapMeter(_BinnedQapRecords):
    """K weighted decode records, one per bin: `meter[k]` is a WeightedQapMeter; see _BinnedRecords."""
    PLAIN, RECORD, HEAD_WORDS = WeightedQapMeter, _lib.QapwRecord, 4


def seed_result(rec):
    """The seed figures of an epoch from a SeedRecord dict: 'seed_precision' = seed_correct / seeds, 'seeds_per_pair' = seeds / pairs,
    'free_acc' = free_correct / free_nodes and 'free_refined_acc' = free_refined_correct / free_nodes (the rows WITHOUT a seed that
    the first and the final matching handed to the fold got right), 'clean' (pairs whose every seed is right) and 'exact_free'
    (pairs whose every free row of the final matching is right) as fractions of the pairs, 'seeds', 'free_nodes', 'nodes', 'pairs'.
    An empty denominator gives NaN."""
    div = lambda a, b: a / b if b else float('nan')
    return {'seed_precision': div(rec['seed_correct'], rec['seeds']), 'seeds_per_pair': div(rec['seeds'], rec['pairs']),
            'free_acc': div(rec['free_correct'], rec['free_nodes']),
            'free_refined_acc': div(rec['free_refined_correct'], rec['free_nodes']), 'clean': div(rec['clean_pairs'], rec['pairs']),
            'exact_free': div(rec['exact_free'], rec['pairs']), 'seeds': rec['seeds'], 'free_nodes': rec['free_nodes'],
            'nodes': rec['nodes'], 'pairs': rec['pairs']}


class SeedMeter(_Records):
    """The device record of the seeds of a decode epoch (fgnn_seed_record, include/fgnn_hip.h): how many rows were seeded, how many
    of the seeds were right, and what the matchings recovered on the rows that were NOT given -- the figure the QapMeter cannot
    give, because fgnn_qap_fold counts a seeded row as a hit.  Every field is a 0-dim int64 view of the record; `seed_precision`,
    `free_acc` and `free_refined_acc` are 0-dim fp64 device tensors formed from them on the device.  `result()` (seed_result) is
    the only host synchronisation."""
    RECORD, FIELDS, HEAD_FP64 = _lib.SeedRecord, tuple(name for name, _ in _lib.SeedRecord._fields_), False
    _result = staticmethod(seed_result)

    def __init__(self, device, buf=None):
        """buf: the record's bytes when they belong to a larger buffer (a record of a BinnedSeedMeter)"""
        self._open(device, buf=buf)

    def _dict(self, rec):
        return {name: getattr(rec, name) for name in self.FIELDS}

    @property
    def seed_precision(self):
        """seed_correct / seeds of everything folded so far (NaN before the first seed)"""
        return self.seed_correct.to(torch.float64) / self.seeds.to(torch.float64)

    @property
    def free_acc(self):
        return self.free_correct.to(torch.float64) / self.free_nodes.to(torch.float64)

    @property
    def free_refined_acc(self):
        return self.free_refined_correct.to(torch.float64) / self.free_nodes.to(torch.float64)


class BinnedSeedMeter(_BinnedRecords):
    """K seed records, one per bin: `meter[k]` is a SeedMeter; see _BinnedRecords."""
    PLAIN, RECORD, HEAD_FP64 = SeedMeter, _lib.SeedRecord, False

    def __init__(self, device, K, values=None):
        self._open_bins(device, self._check_bins(K, values), values)


RANK_WORDS = ctypes.sizeof(_lib.RankRecord) // 8
unpack_rank_records_ = unpack_records_


def pack_rank_records(buf, K):
    """pack_records of K rank records -> (K, 14) fp64"""
    return pack_records(buf, K, RANK_WORDS)


def read_records(*meters):
    """(meter.record(), rank_meter.record(), ...) of plain meters -- an EvalMeter, a RankMeter, a QapMeter -- from ONE device-to-host
    copy."""
    return tuple(m._dict(recs[0]) for m, recs in zip(meters, _read(*meters)))


def _score_args(who, scores, nvalid, labels, live, bins):
    """The argument forms and refusals evaluate_scores and rank_scores share -> (s fp32 contiguous, nvalid, labels, bins int32 on the
    scores' device, B, N, live)."""
    if isinstance(scores, MaskedTensor):
        if nvalid is None:
            nvalid = scores.nvalid
        scores = scores.tensor
    if not torch.is_tensor(scores) or scores.dim() != 3 or scores.shape[1] != scores.shape[2] or not scores.is_floating_point():
        raise ValueError('%s: expected (B, N, N) floating-point scores, got %s'
                         % (who, tuple(scores.shape) if torch.is_tensor(scores) else type(scores).__name__,))
    if not scores.is_cuda:
        raise RuntimeError('%s: scores on %s; the evaluation runs on the GPU only (there is no CPU path)' % (who, scores.device))
    B, N, _ = scores.shape
    if B < 1 or N < 1:
        raise ValueError('%s: empty batch %s' % (who, tuple(scores.shape),))
    if N > _lib.FGNN_LSAP_MAX_N:
        raise RuntimeError('%s: at most %d vertices per graph (got %d)' % (who, _lib.FGNN_LSAP_MAX_N, N))
    live = B if live is None else int(live)
    if not 0 <= live <= B:
        raise ValueError('%s: live = %d outside [0, %d]' % (who, live, B))
    dev = scores.device
    if nvalid is not None:
        if not torch.is_tensor(nvalid) or tuple(nvalid.shape) != (B,) or nvalid.is_floating_point():
            raise ValueError('%s: nvalid must be a (%d,) integer tensor' % (who, B))
        nvalid = nvalid.to(device=dev, dtype=torch.int32).contiguous()
    labels = labels_tensor(labels, B, N, dev)
    if bins is not None:
        if not torch.is_tensor(bins) or tuple(bins.shape) != (B,) or bins.is_floating_point() or bins.dtype == torch.bool:
            raise ValueError('%s: bins must be a (%d,) integer tensor' % (who, B))
        bins = bins.to(device=dev, dtype=torch.int32).contiguous()
    return scores.detach().to(torch.float32).contiguous(), nvalid, labels, bins, B, N, live


def _check_meter(who, what, binned, meter, bins, dev, ks=None):
    """meter: a `binned` meter with bins=, else one of its PLAIN class, on dev (what: 'meter' or 'rank meter' in the messages)"""
    if isinstance(meter, binned) != (bins is not None):
        raise ValueError('%s: bins= and a %s as %s go together' % (who, binned.__name__, what))
    if not isinstance(meter, (binned.PLAIN, binned)) or meter.buf.device != dev:
        raise ValueError('%s: the %s must be of class %s (with bins=: %s) on %s' % (who, what, binned.PLAIN.__name__, binned.__name__, dev))
    if ks is not None and check_ks(ks) != meter.ks:
        raise ValueError('%s: ks = %r differ from the meter\'s %r' % (who, tuple(ks), meter.ks))


def _rank_launches(s, nvalid, labels, bins, B, N, live, meter):
    """fgnn_eval_ranks, fgnn_rank_fold on checked arguments (on the current stream of s's device) -> the dict of rank_scores"""
    dev = s.device
    nk = len(meter.ks)
    # one zero-filled allocation for the five outputs (one fill launch instead of five): the 8-byte words first
    words = torch.zeros(2 * B + (B * (N + nk + 1) + 1) // 2, dtype=torch.int64, device=dev)
    rr, rank_sum = words[:B].view(torch.float64), words[B:2 * B]
    ints = words[2 * B:].view(torch.int32)
    rank = ints[:B * N].view(B, N)
    hits = ints[B * N:B * (N + nk)].view(B, nk)
    targets = ints[B * (N + nk):B * (N + nk + 1)]
    st = _lib.stream_ptr()
    _lib.call('fgnn_eval_ranks', _lib.ptr(s), N * N, N, _lib.ptr(nvalid), _lib.ptr(labels), B, N, _lib.ptr(rank), st)
    _lib.call('fgnn_rank_fold', _lib.ptr(rank), _lib.ptr(nvalid), B, N, live, (ctypes.c_int * nk)(*meter.ks), nk, _lib.ptr(bins),
              meter.K if bins is not None else 1, _lib.ptr(hits), _lib.ptr(rr), _lib.ptr(rank_sum), _lib.ptr(targets),
              _lib.ptr(meter.buf), st)
    return {'rank': rank, 'hits': hits, 'rr': rr, 'rank_sum': rank_sum, 'targets': targets, 'meter': meter}


def rank_scores(scores, nvalid=None, labels=None, meter=None, live=None, bins=None, ks=None):
    """The rank of every row's true match and its sums: scores, nvalid, labels, live, bins as evaluate_scores takes them (a
    MaskedTensor included), with the same refusals.  rank[b, i] = 1 + the number of columns j < n_b that beat the target column
    t = labels[b, i] (None: i) in the order of the arg-max of accuracy_max -- a larger score, NaN above every number, the smaller
    index on ties -- so rank 1 is an arg-max hit; 0 for a row whose label lies outside [0, n_b).
    Adds the live pairs to `meter` (a RankMeter; with bins= a BinnedRankMeter, pair b to record bins[b]; None: a fresh RankMeter of
    ks, default (1, 5, 10)); ks, when given next to a meter, must be the meter's.  Returns the device tensors {'rank': (B, N) int32, 0
    in the padding rows, 'hits': (B, nk) int32 rows with 1 <= rank <= ks[q], 'rr': (B,) fp64 sums of 1 / rank, 'rank_sum': (B,) int64,
    'targets': (B,) int32 rows with a target, 'meter'}; the sums of pairs >= live are zero.
    Two launches (fgnn_eval_ranks, fgnn_rank_fold), nothing is read back."""
    if meter is None and bins is not None:
        raise ValueError('rank_scores: bins= and a BinnedRankMeter as rank meter go together')
    s, nvalid, labels, bins, B, N, live = _score_args('rank_scores', scores, nvalid, labels, live, bins)
    if meter is None:
        meter = RankMeter(s.device, ks=(1, 5, 10) if ks is None else ks)
    else:
        _check_meter('rank_scores', 'rank meter', BinnedRankMeter, meter, bins, s.device, ks)
    with torch.cuda.device(s.device):
        return _rank_launches(s, nvalid, labels, bins, B, N, live, meter)


def _check_refine(who, refine):
    if isinstance(refine, bool) or int(refine) != refine or refine < 0:
        raise ValueError('%s: refine must be an integer >= 0 (rounds of greedy_qap), got %r' % (who, refine))
    return int(refine)


def _bits_args(who, bits, B, N, dev):
    """bits: (bits1, bits2), each (B, N, ceil(N/32)) int32 bit words on dev -> the two, contiguous"""
    if bits is None or len(bits) != 2:
        raise ValueError('%s: the decode needs bits=(bits1, bits2), the two graphs as bit words' % who)
    want = (B, N, (N + 31) // 32)
    for t in bits:
        if not torch.is_tensor(t) or t.dtype != torch.int32 or tuple(t.shape) != want or t.device != dev:
            raise ValueError('%s: bit words must be %s int32 tensors on %s, got %s'
                             % (who, want, dev, (tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__))
    if N > _lib.FGNN_QAP_MAX_N:
        raise RuntimeError('%s: at most %d vertices per graph (got %d)' % (who, _lib.FGNN_QAP_MAX_N, N))
    return bits[0].contiguous(), bits[1].contiguous()


FAQ_DEFAULTS = {'P0': 'scores', 'maxiter': 30, 'tol': 0.03, 'tau': 1.0, 'iters': 20}
FAQ_RESTART_DEFAULTS = {'restarts': 1, 'seed': 0, 'polish': False, 'index': None}      # qap.faq's restarts=, seed=, polish=, pair_index=


def _check_faq(who, faq):
    """faq= of the decode: None (off), True (FAQ_DEFAULTS) or a dict of some of its keys and of FAQ_RESTART_DEFAULTS' -> None or
    the full dict, checked"""
    if faq is None:
        return None
    if faq is True:
        faq = {}
    keys = dict(FAQ_DEFAULTS, **FAQ_RESTART_DEFAULTS)
    if not isinstance(faq, dict):
        raise ValueError('%s: faq must be None, True or a dict with keys from %s, got %r' % (who, sorted(keys), faq))
    unknown = sorted(set(faq) - set(keys), key=str)
    if unknown:
        raise ValueError('%s: faq has unknown key(s) %s; the keys are %s' % (who, unknown, sorted(keys)))
    from .qap import _check_restarts, check_sinkhorn
    o = dict(keys, **faq)
    o['restarts'], o['seed'] = _check_restarts('%s: faq' % who, o['restarts'], o['seed'])
    if not isinstance(o['polish'], bool):
        raise ValueError("%s: faq['polish'] must be True or False, got %r" % (who, o['polish']))
    if o['index'] is not None and (not torch.is_tensor(o['index']) or o['index'].dim() != 1 or o['index'].is_floating_point()
                                   or not o['index'].is_cuda):
        raise ValueError("%s: faq['index'] must be a (B,) integer device tensor of pair indices" % who)
    if o['P0'] not in ('scores', 'barycenter'):
        raise ValueError("%s: faq['P0'] is 'scores' or 'barycenter', got %r" % (who, o['P0']))
    if isinstance(o['maxiter'], bool) or not isinstance(o['maxiter'], (int, np.integer)) or o['maxiter'] <= 0:
        raise ValueError("%s: faq['maxiter'] must be a positive integer, got %r" % (who, o['maxiter']))
    if isinstance(o['tol'], bool) or not isinstance(o['tol'], (int, float, np.floating, np.integer)) or not o['tol'] > 0:
        raise ValueError("%s: faq['tol'] must be a positive float, got %r" % (who, o['tol']))
    o['tau'], o['iters'] = check_sinkhorn('%s: faq' % who, o['tau'], o['iters'])
    o['maxiter'], o['tol'] = int(o['maxiter']), float(o['tol'])
    return o


class _BitPairs:
    """The 0/1 pairs of a decode as bit words: what the chain (_decode_launches, _faq_launches) needs from the graphs, on checked
    arguments.  Objectives are int32, as fgnn_qap_fold reads them.  _WeightedPairs is the same surface on fp32 matrices."""
    FOLD, BINNED, EXTRA = 'fgnn_qap_fold', BinnedQapMeter, ()       # the fold entry point, the meters, the route's own keys

    def __init__(self, b1, b2):
        self.b1, self.b2 = b1, b2

    @classmethod
    def checked(cls, who, bits1, bits2, B, N, dev):
        return cls(*_bits_args(who, (bits1, bits2), B, N, dev))

    def objective(self, matching, nvalid):
        """-> (qap of `matching`, planted), as the fold reads them"""
        obj = qap.objective_bits(self.b1, self.b2, matching, nvalid, raw=True)
        return obj[0], obj[1]

    def faq_buffer(self, B, N):
        """what faq_matrices fills (the stage allocates before its first launch)"""
        return torch.empty(2, B, 2, N, N, dtype=torch.float32, device=self.b1.device)

    def faq_matrices(self, x, nvalid):
        """-> the two sides as the fp32 matrices the FAQ chain runs on: fgnn_expand_adjacency on both sides' words"""
        B, N = self.b1.shape[:2]
        for side, bits in enumerate((self.b1, self.b2)):
            _lib.call('fgnn_expand_adjacency', _lib.ptr(bits), _lib.ptr(nvalid), B, N, _lib.ptr(x[side]), _lib.stream_ptr())
        return x[0, :, 0], x[1, :, 0]

    def repeated(self, rep, m1, m2):
        """-> (the operand of the B R restart problems, its two FAQ matrices); rep: a tensor R-fold, pair-major"""
        return _BitPairs(rep(self.b1), rep(self.b2)), rep(m1), rep(m2)

    def candidates(self, perms, nvalid, seeds, polish):
        """The restart candidates as the best-of choice takes them -> (their objectives, their matchings, veto): with polish the
        exchange search on all of them, its own objective and its status as veto"""
        if not polish:
            return qap.objective_bits(self.b1, self.b2, perms, nvalid)['qap'], perms, None
        t = qap.two_opt_bits(self.b1, self.b2, perms, nvalid, seeds=seeds)
        return t['qap'], t['perm'], t['status'].to(torch.int32)

    def greedy(self, matching, T, nvalid, labels):
        """-> (perm, refined = 2 s_best, the route's 'greedy' entry)"""
        g = qap.greedy_bits(self.b1, self.b2, matching, T, nvalid, labels, raw=True)
        return g['perm'], g['s_best2'], None

    def two_opt(self, matching, nvalid, seeds):
        """-> (perm, refined, swaps, status, nit); the search's objective IS qap's sum, whatever the symmetry"""
        t = qap.two_opt_bits(self.b1, self.b2, matching, nvalid, raw=True, seeds=seeds)
        return t['perm'], t['qap'], t['swaps'], t['status'], t['nit']


class _WeightedPairs:
    """The real-weighted pairs of a decode as the fp32 views of qap.weighted_views: the surface of _BitPairs, objectives fp32 as
    fgnn_qapw_fold reads them.  The FAQ chain runs on the views themselves."""
    FOLD, BINNED, EXTRA = 'fgnn_qapw_fold', BinnedWeightedQapMeter, ('nit', 'greedy')

    def __init__(self, x1, x2, gs, ld):
        self.x1, self.x2, self.gs, self.ld = x1, x2, gs, ld

    @classmethod
    def checked(cls, who, adj1, adj2, B, N, dev):
        return cls(*_weighted_args(who, adj1, adj2, B, N, dev))

    def objective(self, matching, nvalid):
        obj = qap.objective_weighted(self.x1, self.x2, matching, nvalid)
        return obj['qap'], obj['planted']

    def faq_buffer(self, B, N):
        return None

    def faq_matrices(self, x, nvalid):
        return self.x1, self.x2

    def repeated(self, rep, m1, m2):
        N = self.x1.shape[-1]
        r = _WeightedPairs(rep(m1), rep(m2), N * N, N)
        return r, r.x1, r.x2

    def candidates(self, perms, nvalid, seeds, polish):
        veto = None
        if polish:
            t = qap.two_opt_weighted_device(self.x1, self.x2, self.gs, self.ld, perms, nvalid, -1, seeds)
            perms, veto = t['perm'], t['status']
        return self.objective(perms, nvalid)[0], perms, veto

    def greedy(self, matching, T, nvalid, labels):
        g = qap.greedy_weighted(self.x1, self.x2, matching, T, nvalid, labels)
        return g['perm'], g['s_best'] * 2, g                     # (an exact doubling: trace(A P B P^T), the unit of qap)

    def two_opt(self, matching, nvalid, seeds):
        """(the search returns no objective: a fresh launch on its perm)"""
        t = qap.two_opt_weighted_device(self.x1, self.x2, self.gs, self.ld, matching, nvalid, -1, seeds)
        return t['perm'], self.objective(t['perm'], nvalid)[0], t['swaps'], t['status'], t['nit']


def _faq_launches(pairs, s, assign, q, nvalid, B, N, faq, seeds=None):
    """The FAQ stage of the decode, on checked arguments and the operand `pairs` (_BitPairs or _WeightedPairs): fgnn_sinkhorn on the
    scores (P0 'scores'), the operand's FAQ matrices (0/1: fgnn_expand_adjacency on both sides; weighted: the views themselves), the
    fgnn_qapw_faq chain, the objective of its perm, and the select -- where the chain reports status 2 the stage keeps `assign` and
    its objective `q`.  Every buffer is allocated before the first launch; nothing is read back.
    With seeds: fgnn_seed_index and fgnn_seed_gather first, so that Sinkhorn runs on the free block of the scores with n_b := u_b,
    and the fgnn_qapw_faq_seeded chain from that start, already in free coordinates.
    With faq['restarts'] = R > 1 or faq['polish'] (qap.faq's restarts): that start -- the Sinkhorn matrix or the barycenter -- is the
    base of fgnn_faq_restart_starts (pair indices faq['index'], else the position in the batch), the operand is replicated R-fold,
    the chain runs once on the B R problems, the operand scores them (its objective; with polish after its exchange search, seeded
    with seeds, on all of them) and fgnn_qap_best_of picks; the select then works on the winner.  Restart 0 is the start the stage
    always had.
    -> {'perm', 'qap', 'faq_perm', 'faq_qap', 'faq_nit', 'faq_status', 'sinkhorn_err', 'faq_restart'} (+ 'seeded' with seeds), 'qap'
    and 'faq_qap' in q's dtype; faq_restart is None without restarts"""
    dev = assign.device
    R = faq['restarts']
    restarted = R > 1 or faq['polish']
    if restarted and B * R > _lib.FGNN_RESTART_MAX_STARTS:
        raise ValueError('decode: at most %d starts per call (got %d pairs x %d restarts)' % (_lib.FGNN_RESTART_MAX_STARTS, B, R))
    if faq['index'] is not None and tuple(faq['index'].shape) != (B,):
        raise ValueError("decode: faq['index'] must hold %d pair indices, got %s" % (B, tuple(faq['index'].shape)))
    x = pairs.faq_buffer(B, N)
    p0 = err = u = restart = None
    if seeds is not None and (restarted or faq['P0'] == 'scores'):
        ix = qap.seed_index_device(seeds, nvalid)
        u = torch.where(ix['valid'] != 0, ix['nfree'], torch.zeros_like(ix['nfree']))
    if faq['P0'] == 'scores':
        if seeds is None:
            sk = qap.sinkhorn_device(s, nvalid, faq['tau'], faq['iters'])
        else:
            sk = qap.sinkhorn_device(qap.seed_gather_device(s, ix['free_a'], ix['free_b'], u), u, faq['tau'], faq['iters'])
        p0, err = sk['P'], sk['err']
    m1, m2 = pairs.faq_matrices(x, nvalid)
    if restarted:
        def rep(t):
            return t.repeat_interleave(R, 0) if t is not None else None
        index = faq['index'].to(torch.int64).contiguous() if faq['index'] is not None else None
        starts = qap.random_starts_device(p0, nvalid if seeds is None else u, index, faq['seed'], B, N, R, dev)
        pairs_r, m1, m2 = pairs.repeated(rep, m1, m2)
        nvr, sdr = rep(nvalid), rep(seeds)
        run = qap.faq_weighted(m1, m2, nvr, starts, None, faq['maxiter'], faq['tol'], seeds=sdr, p0_free=seeds is not None)
        score, perms, veto = pairs_r.candidates(run['perm'], nvr, sdr, faq['polish'])
        best = qap.best_of_device(score, run['status'], run['nit'], perms, R, veto)
        out = {'perm': best['perm'], 'nit': best['nit'], 'status': best['status']}
        if seeds is not None:
            out['seeded'] = run['seeded'].view(B, R)[:, 0].contiguous()
        fq, restart = best['qap'].to(q.dtype), best['restart']
    else:
        out = qap.faq_weighted(m1, m2, nvalid, p0, None, faq['maxiter'], faq['tol'], seeds=seeds, p0_free=seeds is not None)
        fq = pairs.objective(out['perm'], nvalid)[0]
    failed = out['status'] == 2
    res = {'perm': torch.where(failed[:, None], assign, out['perm']), 'qap': torch.where(failed, q, fq), 'faq_perm': out['perm'],
           'faq_qap': fq, 'faq_nit': out['nit'], 'faq_status': out['status'], 'sinkhorn_err': err, 'faq_restart': restart}
    if seeds is not None:
        res['seeded'] = out['seeded']
    return res


def seed_fold(seed_meter, seeds, first, final, nvalid, labels, bins, B, N, live):
    """fgnn_seed_fold(_bins) on checked (B, N) int32 device tensors: seeds (None: every row free), `first` (the matching the seeds
    went into) and `final` (the last matching of the chain, or None) against labels (None: the identity) into seed_meter"""
    pairs = (_lib.ptr(seeds), _lib.ptr(first), _lib.ptr(final), _lib.ptr(labels), _lib.ptr(nvalid), B, N, live)
    if bins is None:
        _lib.call('fgnn_seed_fold', *pairs, _lib.ptr(seed_meter.buf), _lib.stream_ptr())
    else:
        _lib.call('fgnn_seed_fold_bins', *pairs, _lib.ptr(bins), seed_meter.K, _lib.ptr(seed_meter.buf), _lib.stream_ptr())


def _decode_launches(pairs, assign, nvalid, labels, bins, B, N, live, meter, refine, two_opt=False, faq=None, scores=None, seeds=None,
                     seed_meter=None):
    """The decode chain on checked arguments and the operand `pairs` (_BitPairs or _WeightedPairs), on the current stream of its
    device: the operand's objective of `assign` (once more on the labels), fgnn_confident_seeds on `scores` when seeds is a spec,
    _faq_launches with faq (on `scores`), the operand's greedy refinement with refine > 0, its exchange search with two_opt (the
    weighted one with a fresh objective of its perm), then the operand's fold entry point (fgnn_qap_fold(_bins) /
    fgnn_qapw_fold(_bins)) and, with a seed_meter, fgnn_seed_fold(_bins), which reads integer matchings only.  meter None: no fold
    (Siamese_Node_Exp.match_weighted).  -> the dict of decode_scores / decode_scores_weighted"""
    nseeds = None
    if isinstance(seeds, dict):     # a spec: the seeds come from the scores the solver saw
        picked = qap.confident_seeds_device(scores, nvalid, seeds['count'], seeds['min_margin'])
        seeds, nseeds = picked['seeds'], picked['nseeds']
    q, planted = pairs.objective(assign, nvalid)
    if labels is not None:          # (as all_acc_qap: planted is the objective of the labels' matching)
        planted = pairs.objective(labels, nvalid)[0]
    perm = refined = greedy = None
    first = assign
    mark = meter._mark_refined if meter is not None else (lambda: None)
    stage = dict.fromkeys(('faq_perm', 'faq_qap', 'faq_nit', 'faq_status', 'sinkhorn_err', 'faq_restart'))
    if faq is not None:
        stage = _faq_launches(pairs, scores, assign, q, nvalid, B, N, faq, seeds)
        perm, refined = stage.pop('perm'), stage.pop('qap')
        first = perm
        mark()
    if refine > 0:
        perm, refined, greedy = pairs.greedy(assign if perm is None else perm, refine, nvalid, labels)
        mark()
    swaps = status = nit = None
    if two_opt:                     # from the last matching of the chain
        perm, refined, swaps, status, nit = pairs.two_opt(assign if perm is None else perm, nvalid, seeds)
        mark()
    correct = refined_correct = ratio = None
    if meter is not None:
        # one zero-filled allocation for the three per-pair outputs: the 8-byte words first
        words = torch.zeros(2 * B, dtype=torch.int64, device=assign.device)
        ratio, ints = words[:B].view(torch.float64), words[B:].view(torch.int32)
        correct, refined_correct = ints[:B], ints[B:]
        per_pair = (_lib.ptr(assign), _lib.ptr(perm), _lib.ptr(labels), _lib.ptr(q), _lib.ptr(planted), _lib.ptr(refined),
                    _lib.ptr(nvalid), B, N, live)
        outs = (_lib.ptr(correct), _lib.ptr(refined_correct), _lib.ptr(ratio), _lib.ptr(meter.buf), _lib.stream_ptr())
        if bins is None:
            _lib.call(pairs.FOLD, *per_pair, *outs)
        else:
            _lib.call(pairs.FOLD + '_bins', *per_pair, _lib.ptr(bins), meter.K, *outs)
    if seed_meter is not None:
        seed_fold(seed_meter, seeds, first, perm, nvalid, labels, bins, B, N, live)
        stage['seed_meter'] = seed_meter
    if seeds is not None:
        stage['seeds'], stage['nseeds'] = seeds, stage['seeded'] if nseeds is None else nseeds
    return {'assign': assign, 'qap': q, 'planted': planted, 'correct': correct, 'ratio': ratio, 'perm': perm, 'refined': refined,
            'refined_correct': None if perm is None else refined_correct, 'meter': meter, 'swaps': swaps, 'status': status,
            **dict(zip(pairs.EXTRA, (nit, greedy))), **stage}           # (EXTRA: 'nit' and 'greedy' on the weighted route only)


def _check_two_opt(who, two_opt):
    if not isinstance(two_opt, bool):
        raise ValueError('%s: two_opt must be True or False, got %r' % (who, two_opt))
    return two_opt


SEED_SPEC_DEFAULTS = {'from': 'scores', 'count': None, 'min_margin': 0.0}


def seed_spec(who, seeds):
    """seeds= as a spec -- 'scores' or a dict with keys from {'from': 'scores', 'count': None, 'min_margin': 0.0} -> the checked
    {'count': int (-1: no cap), 'min_margin': float} of qap.confident_seeds_device; None when seeds is neither (a tensor, None)"""
    if isinstance(seeds, str):
        seeds = {'from': seeds}
    elif not isinstance(seeds, dict):
        return None
    unknown = sorted(set(seeds) - set(SEED_SPEC_DEFAULTS), key=str)
    if unknown:
        raise ValueError('%s: seeds has unknown key(s) %s; the keys are %s' % (who, unknown, sorted(SEED_SPEC_DEFAULTS)))
    o = dict(SEED_SPEC_DEFAULTS, **seeds)
    if o['from'] != 'scores':
        raise ValueError("%s: seeds['from'] is 'scores', got %r" % (who, o['from']))
    from .qap import check_confident
    count, min_margin = check_confident('%s: seeds' % who, o['count'], o['min_margin'])
    return {'count': count, 'min_margin': min_margin}


def _check_seed_meter(who, seed_meter, bins, dev, K=None):
    if seed_meter is None:
        return
    _check_meter(who, 'seed meter', BinnedSeedMeter, seed_meter, bins, dev)
    if bins is not None and K is not None and seed_meter.K != K:
        raise ValueError('%s: the seed meter has %d records, the meter %d' % (who, seed_meter.K, K))


def _check_decode_seeds(who, seeds, B, N, dev, faq, refine):
    """seeds= of the decode -> (B, N) int32 on dev, the checked spec of seed_spec, or None; seeds need the faq= stage and exclude
    refine"""
    if seeds is None:
        return None
    from . import qap
    spec = seed_spec(who, seeds)
    if spec is not None and N > _lib.FGNN_SEED_MAX_N:
        raise RuntimeError('%s: seeds from the scores take at most %d vertices per graph (got %d)' % (who, _lib.FGNN_SEED_MAX_N, N))
    seeds = qap.check_seeds(who, seeds, B, N, dev) if spec is None else spec
    if faq is None:
        raise ValueError('%s: seeds= needs the faq= stage (the Hungarian matching knows no fixed rows)' % who)
    if refine > 0:
        raise ValueError("%s: seeds= and refine > 0 do not go together (the reference's greedy_qap knows no fixed rows)" % who)
    return seeds


def _decode(who, operand, g1, g2, scores, nvalid, labels, meter, live, bins, refine, assign, two_opt, faq, seeds, seed_meter):
    """The body decode_scores (operand _BitPairs, the graphs as bit words) and decode_scores_weighted (_WeightedPairs, as float
    matrices) share: the checks, the meter of the operand's class, the Hungarian matching unless `assign`, _decode_launches"""
    if meter is None and bins is not None:
        raise ValueError('%s: bins= and a %s as meter go together' % (who, operand.BINNED.__name__))
    refine = _check_refine(who, refine)
    two_opt = _check_two_opt(who, two_opt)
    faq = _check_faq(who, faq)
    s, nvalid, labels, bins, B, N, live = _score_args(who, scores, nvalid, labels, live, bins)
    dev = s.device
    pairs = operand.checked(who, g1, g2, B, N, dev)
    seeds = _check_decode_seeds(who, seeds, B, N, dev, faq, refine)
    if meter is None:
        meter = operand.BINNED.PLAIN(dev)
    else:
        _check_meter(who, 'meter', operand.BINNED, meter, bins, dev)
    _check_seed_meter(who, seed_meter, bins, dev, meter.K if bins is not None else None)
    if assign is not None:
        if not torch.is_tensor(assign) or tuple(assign.shape) != (B, N) or assign.is_floating_point() or assign.device != dev:
            raise ValueError('%s: assign must be a (%d, %d) integer tensor on %s' % (who, B, N, dev))
        assign = assign.to(torch.int32).contiguous()
    with torch.cuda.device(dev):
        if assign is None:
            from .metrics import lsap_device
            assign = lsap_device(s, nvalid, want_assign=True)[1]
        return _decode_launches(pairs, assign, nvalid, labels, bins, B, N, live, meter, refine, two_opt, faq, s, seeds, seed_meter)


def decode_scores(scores, bits1, bits2, nvalid=None, labels=None, meter=None, live=None, bins=None, refine=0, assign=None,
                  two_opt=False, faq=None, seeds=None, seed_meter=None):
    """The reference's all_acc_qap / all_greedy_losses_acc (toolbox/metrics.py:168-223) of a batch, added to an epoch record.
    scores, nvalid, labels, live, bins: as evaluate_scores takes them, with the same refusals; bits1, bits2: the two graphs as
    (B, N, ceil(N/32)) int32 bit words on the scores' device (PairGenerator.bits, synthetic.pack_adjacency).  0/1 graphs only: the
    real-weighted decode (qap.all_acc_qap / greedy_qap with weighted=True, fp32 objectives) is decode_scores_weighted, with a
    WeightedQapMeter.
    The chain: the Hungarian matching of the scores (metrics.lsap_device, the route of qap.all_acc_qap) unless `assign`, a (B, N)
    int32 device tensor of matched columns, is handed in; qap.objective_bits for qap and planted, once more on the labels when
    there are any (planted is then the objective of the labels' matching); with refine = T > 0 the T rounds of qap.greedy_bits
    from that matching; with two_opt=True the pairwise-exchange search of qap.two_opt_bits (one launch, no limit on its exchanges)
    from the refinement's matching, or from the first one when refine = 0; then fgnn_qap_fold, which adds the live pairs to `meter`
    (a QapMeter; with bins= a BinnedQapMeter, pair b to record bins[b]; None: a fresh QapMeter).  The fold takes the matching and
    objective of the LAST stage that ran as perm / refined, so 'refined_acc', 'refined_qap_ratio' and 'improved' of the meter
    describe the final matching of the chain.
    Returns the device tensors {'assign': (B, N) int32, 'qap', 'planted': (B,) int32, 'correct': (B,) int32 rows where assign is the
    row's target, 'ratio': (B,) fp64 qap / planted (0 for an unmatched pair or planted <= 0), 'perm': (B, N) int32 and 'refined':
    (B,) int32 of the refinement (None without) -- refined is 2 s_best, trace(A P B P^T) of perm, the unit of qap; after two_opt it
    is the qap of perm itself, sum_{i,k} A[i,k] B[perm(i),perm(k)], -1 where the search was handed no permutation --
    'refined_correct': (B,) int32 (None without), 'meter', 'swaps', 'status': (B,) int32 of qap.two_opt_bits (None without
    two_opt)}; correct, ratio and refined_correct of pairs >= live are zero.
    faq: None (off), True or a dict with keys from {'P0': 'scores' | 'barycenter', 'maxiter': 30, 'tol': 0.03, 'tau': 1.0,
    'iters': 20} (True: these defaults with P0 'scores'; an unknown key raises ValueError) -- the Fast Approximate QAP stage, after
    the Hungarian matching and before refine and two_opt: with 'scores' the Sinkhorn projection of the scores the solver saw
    (qap.sinkhorn: tau, iters; one launch) is the start P0, else the barycenter; fgnn_expand_adjacency on both sides' words; the
    chain of qap.faq (maxiter, tol); qap.objective_bits of its perm; and a select on the device: where the chain reports status 2
    the stage's matching and objective are `assign` and its qap.  refine and two_opt then start from the stage's matching, and the
    fold takes the last stage that ran, as above.  The dict gains 'faq_perm' (B, N) int32, 'faq_qap', 'faq_nit', 'faq_status' (B,)
    int32 as the chain left them (faq_qap: the objective of faq_perm, -1 where it holds no matching) and 'sinkhorn_err' (B,) fp32
    (None with the barycenter); all None without faq.  With {'P0': 'barycenter'} and `assign` handed in the scores do not enter
    the stage's matching: the classical-baseline epoch.
    The faq dict also takes qap.faq's restarts: 'restarts': R in [1, 64], 'seed', 'polish': True / False, and 'index', a (B,) integer
    device tensor of pair indices (default: the position in the batch).  With R > 1 (or polish) the stage's start -- the Sinkhorn
    matrix of the scores or the barycenter -- is the base of R starts per pair (fgnn_faq_restart_starts: restart 0 is that start,
    the others its mean with a random doubly stochastic matrix drawn from (seed, index[b], k)), the chain runs once on the B R
    problems, and fgnn_qap_best_of keeps each pair's best matching -- by qap.objective_bits, with polish by qap.two_opt_bits'
    objective after the exchange search on all of them -- before the select; 'faq_perm', 'faq_qap', 'faq_nit', 'faq_status' are the
    winner's and the dict gains 'faq_restart' (B,) int32, its k (None without restarts).  {'restarts': 1} issues the launches it
    always did.  {'P0': 'randomized'} stays refused.
    seeds: None or a (B, N) integer tensor of known matches (qap.faq: seeds[b, i] = j fixes row i, -1 leaves it free;
    planted.reveal_seeds draws one from labels).  Seeds need the faq= stage and exclude refine > 0 (ValueError otherwise): with P0
    'scores' Sinkhorn runs on the free block of the scores (fgnn_seed_index, fgnn_seed_gather, n_b := u_b), the seeded chain
    fgnn_qapw_faq_seeded follows, and two_opt=True runs fgnn_qap_2opt_seeded, so 'faq_perm' and 'perm' hold every seed.  The
    Hungarian stage ('assign', 'correct') stays unseeded; the fold and the meters are unchanged.  The dict gains 'seeded' (B,) int32
    = m_b.  seeds=None issues the launches and returns the keys it always did.
    seeds may also be a spec -- 'scores', or {'from': 'scores', 'count': k, 'min_margin': x} (an unknown key or 'from' raises
    ValueError) -- the seeds the model's own scores give: one fgnn_confident_seeds launch (qap.confident_seeds: rows whose best
    column picks them back with margin >= x, the k clearest of them) on the scores the solver saw, its output going where a seed
    tensor goes.  The rules are the same: the faq= stage, no refine.  With any seeds the dict gains 'seeds' (B, N) int32 and
    'nseeds' (B,) int32.
    seed_meter: a SeedMeter (with bins= a BinnedSeedMeter of the meter's K) -- fgnn_seed_fold(_bins) runs after fgnn_qap_fold with
    the same labels, live and bins and adds, per live pair, the seeds that are right and the rows WITHOUT a seed that the faq stage's
    matching (without faq: assign) and the final `perm` of the chain got right; it comes back under 'seed_meter'.  The QapMeter and
    its fold are untouched: they count a seeded row as a hit.
    Nothing is read back."""
    return _decode('decode_scores', _BitPairs, bits1, bits2, scores, nvalid, labels, meter, live, bins, refine, assign, two_opt, faq,
                   seeds, seed_meter)


def _weighted_args(who, adj1, adj2, B, N, dev):
    """adj1, adj2 of the weighted decode -> (x1, x2, gstride, ld) of qap.weighted_views, checked against the scores' (B, N) and
    device"""
    from . import qap
    for a in (adj1, adj2):
        if not torch.is_tensor(a) or a.device != dev or a.dim() not in (3, 4) or a.shape[0] != B or tuple(a.shape[-2:]) != (N, N):
            raise ValueError('%s: the graphs are (%d, %d, %d) or (%d, C, %d, %d) float tensors on %s, got %s'
                             % (who, B, N, N, B, N, N, dev, (tuple(a.shape), a.device) if torch.is_tensor(a) else type(a).__name__))
    if N > _lib.FGNN_QAPW_MAX_N:
        raise RuntimeError('%s: at most %d vertices per graph (got %d)' % (who, _lib.FGNN_QAPW_MAX_N, N))
    return qap.weighted_views(adj1, adj2)


def decode_scores_weighted(scores, adj1, adj2, nvalid=None, labels=None, meter=None, live=None, bins=None, refine=0, assign=None,
                           two_opt=False, faq=None, seeds=None, seed_meter=None):
    """`decode_scores` on REAL-weighted pairs: the same chain, arguments, rules and messages, on what qap.weighted_views takes --
    adj1, adj2 are (B, N, N) float matrices or (B, C, N, N) batches on the scores' device whose channel 0 is used in place (a
    spectral L of PairGenerator.spectral, any weighted graph).  No representation check, no host read: capturable.
    The chain: metrics.lsap_device unless `assign` is handed in; qap.objective_weighted for qap and planted, once more on the labels
    when there are any; with faq the stage of decode_scores on fp32 -- Sinkhorn on the scores (on their free block with seeds),
    qap.faq_weighted directly on the views, restarts through fgnn_faq_restart_starts, qap.objective_weighted, fgnn_qap_best_of_f32,
    with 'polish' the exchange search fgnn_qapw_2opt (fgnn_qapw_2opt_seeded with seeds) on every restart, and the select on status
    2; with refine = T > 0 qap.greedy_weighted, refined = 2 s_best, an exact doubling, the unit of qap; with two_opt=True
    fgnn_qapw_2opt (seeded with seeds) from the last matching, refined = the fresh qap.objective_weighted of its perm; then
    fgnn_qapw_fold(_bins) into `meter` (a WeightedQapMeter; with bins= a BinnedWeightedQapMeter; None: a fresh WeightedQapMeter) and,
    with a seed_meter, fgnn_seed_fold(_bins), which reads integer matchings only.  Seeds need faq= and exclude refine > 0; seed
    specs ('scores', a dict) are accepted.
    Returns decode_scores' keys with 'qap', 'planted', 'refined', 'faq_qap' as float32 (plus 'nit', (B,) int64 of the exchange
    search, and 'greedy', the dict of qap.greedy_weighted; None without).  A pair whose `assign` leaves its corner has the
    sentinel qap = -1 of fgnn_qapw_objective and counts as unmatched in the fold.  Nothing is read back."""
    return _decode('decode_scores_weighted', _WeightedPairs, adj1, adj2, scores, nvalid, labels, meter, live, bins, refine, assign,
                   two_opt, faq, seeds, seed_meter)


def evaluate_scores(scores, nvalid=None, labels=None, meter=None, live=None, hungarian=True, loss_on_labels=False, bins=None,
                    rank_meter=None, qap_meter=None, bits=None, refine=0, two_opt=False, faq=None, seeds=None, seed_meter=None,
                    adj=None):
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
    rank_meter: a RankMeter (with bins=: a BinnedRankMeter) -- the two launches of rank_scores follow on the same scores, labels,
    live and bins and add to it; their per-pair tensors come back under 'ranks'.  None: nothing of this is launched.
    qap_meter: a QapMeter (with bins=: a BinnedQapMeter of the meter's K) with bits=(bits1, bits2), the two graphs as bit words --
    the chain of decode_scores follows on the assignment of the solver launch made here (the solver does not run twice, so
    hungarian=False is refused), with refine rounds of greedy refinement and, with two_opt=True, the pairwise-exchange search
    after them, on the same labels, live and bins; its per-pair tensors come back under 'decode'.  0/1 graphs only (see decode_scores).  None: nothing of this is launched.
    faq (with a qap_meter): the Fast Approximate QAP stage of decode_scores, started from these scores or from the barycenter.
    seeds, seed_meter (with a qap_meter): a (B, N) seed tensor or the spec of decode_scores ('scores', or a dict), and a SeedMeter
    (with bins=: a BinnedSeedMeter) -- both are handed to the decode, with its refusals: seeds need faq= and exclude refine > 0.
    adj=(x1, x2) instead of bits= (REAL-weighted pairs; the two together raise ValueError): the two graphs as (B, N, N) float
    matrices or (B, C, N, N) batches whose channel 0 is read in place (qap.weighted_views; WignerGenerator.weighted's tensors) with a
    WeightedQapMeter as qap_meter (with bins=: a BinnedWeightedQapMeter; a QapMeter is refused, as a WeightedQapMeter is with bits=)
    -- the chain of decode_scores_weighted follows on the assignment of the solver launch made here, with its rules and messages
    for refine, two_opt, faq, seeds and seed_meter; its per-pair tensors come back under 'decode'.
    Four launches, nothing is read back."""
    if isinstance(meter, BinnedEvalMeter) != (bins is not None):
        raise ValueError('evaluate_scores: bins= and a BinnedEvalMeter as meter go together')
    if qap_meter is None:
        if bits is not None or refine:
            raise ValueError('evaluate_scores: bits= and refine= belong to a qap_meter')
        if adj is not None:
            raise ValueError('evaluate_scores: adj= belongs to a qap_meter')
        if two_opt:
            raise ValueError('evaluate_scores: two_opt= belongs to a qap_meter')
        if faq is not None:
            raise ValueError('evaluate_scores: faq= belongs to a qap_meter')
        if seeds is not None or seed_meter is not None:
            raise ValueError('evaluate_scores: seeds= and seed_meter= belong to a qap_meter')
    else:
        if not hungarian:
            raise ValueError('evaluate_scores: a qap_meter decodes the matching of the Hungarian solver; it needs hungarian=True')
        if bits is not None and adj is not None:
            raise ValueError('evaluate_scores: give the graphs as bits= (0/1, a QapMeter) or as adj= (real weights, a '
                             'WeightedQapMeter), not both')
        refine = _check_refine('evaluate_scores', refine)
        two_opt = _check_two_opt('evaluate_scores', two_opt)
        faq = _check_faq('evaluate_scores', faq)
    s, nvalid, labels, bins, B, N, live = _score_args('evaluate_scores', scores, nvalid, labels, live, bins)
    dev = s.device
    if meter is None:
        meter = EvalMeter(dev)
    else:
        _check_meter('evaluate_scores', 'meter', BinnedEvalMeter, meter, bins, dev)
    if rank_meter is not None:
        _check_meter('evaluate_scores', 'rank meter', BinnedRankMeter, rank_meter, bins, dev)
    if qap_meter is not None:
        _check_meter('evaluate_scores', 'qap meter', BinnedQapMeter if adj is None else BinnedWeightedQapMeter, qap_meter, bins, dev)
        if bins is not None and qap_meter.K != meter.K:
            raise ValueError('evaluate_scores: the qap meter has %d records, the meter %d' % (qap_meter.K, meter.K))
        if adj is None:
            pairs = _BitPairs(*_bits_args('evaluate_scores', bits, B, N, dev))
        else:
            if not isinstance(adj, (tuple, list)) or len(adj) != 2:
                raise ValueError('evaluate_scores: adj must be the pair (x1, x2) of the two graphs')
            pairs = _WeightedPairs.checked('evaluate_scores', adj[0], adj[1], B, N, dev)
        seeds = _check_decode_seeds('evaluate_scores', seeds, B, N, dev, faq, refine)
        _check_seed_meter('evaluate_scores', seed_meter, bins, dev, meter.K if bins is not None else None)
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
        _lib.call('fgnn_eval_pairs_labels' if loss_on_labels and labels is not None else 'fgnn_eval_pairs', _lib.ptr(s), _lib.ptr(nvalid),
                  _lib.ptr(labels), B, N, _lib.ptr(cost), N * N, N, _lib.ptr(row_ce), _lib.ptr(row_hit), st)
        if hungarian:
            assign = torch.empty(B, N, **i32)
            _lib.call('fgnn_lsap_accuracy', _lib.ptr(cost), N * N, N, _lib.ptr(nvalid), B, N, _lib.ptr(correct), _lib.ptr(assign), st)
            if labels is not None:
                _lib.call('fgnn_count_matches', _lib.ptr(assign), _lib.ptr(labels), _lib.ptr(nvalid), B, N, _lib.ptr(correct), st)
        rows = (_lib.ptr(row_ce), _lib.ptr(row_hit), _lib.ptr(correct) if hungarian else None, _lib.ptr(nvalid), B, N, live)
        sums = (_lib.ptr(pair_ce), _lib.ptr(pair_max), _lib.ptr(meter.buf), st)
        if bins is None:
            _lib.call('fgnn_eval_fold', *rows, *sums)
        else:
            _lib.call('fgnn_eval_fold_bins', *rows, _lib.ptr(bins), meter.K, *sums)
        ranks = None if rank_meter is None else _rank_launches(s, nvalid, labels, bins, B, N, live, rank_meter)
        decode = None
        if qap_meter is not None:
            decode = _decode_launches(pairs, assign, nvalid, labels, bins, B, N, live, qap_meter, refine, two_opt, faq, s, seeds, seed_meter)
    n = nvalid if nvalid is not None else torch.full((B,), N, **i32)
    out = {'ce': pair_ce, 'n': n, 'correct_max': pair_max, 'correct_lsap': correct, 'assign': assign, 'meter': meter}
    if ranks is not None:
        out['ranks'] = ranks
    if decode is not None:
        out['decode'] = decode
    return out


BASELINE_METHODS = ('grampa', 'degree_profile')
# the keywords baseline_curve hands on to a method's function (qap.grampa, qap.degree_profile); the pairs, nvalid=, labels= and
# weighted= are the curve's own
_BASELINE_KWARGS = {'grampa': ('eta', 'maxiter', 'tol', 'standardize', 'rhs'), 'degree_profile': ()}


def baseline_curve(generator, noises, num_examples, batch_size, method='grampa', features=None, permute=True, meter=None,
                   rank_meter=None, qap_meter=None, seed_meter=None, refine=0, two_opt=False, faq=None, seeds=None, **kwargs):
    """The model-free twin of ``FgnnTrainer.noise_curve``: the curve of a model-free baseline across K = len(noises) noise levels, in
    one pass, with the same paired design and the same cut -- the K * num_examples examples lie level-major (example e is dataset
    pair e % num_examples at level e // num_examples) and an unshuffled EpochSampler cuts them into full batches of mixed levels;
    the filling of a short last batch is masked out (live=).  Per batch the pairs come from ``generator.bits(index=, levels=, level=,
    permute=)`` (features=None: a PairSource, 0/1 graphs) or ``generator.weighted(...)`` (features='weighted': a WignerGenerator),
    the scores from ``qap.grampa(x1, x2, nvalid=, labels=, weighted=, **kwargs)`` (method='grampa') or ``qap.degree_profile(x1, x2,
    nvalid=, labels=, weighted=)`` (method='degree_profile', which takes no further keyword; one the method does not take raises
    ValueError before any launch), and
    ``evaluate_scores(X, nvalid=, labels=, meter=, bins=level, live=, rank_meter=, qap_meter=, bits= / adj=, refine=, two_opt=, faq=,
    seeds=, seed_meter=)`` folds them: the records are bit for bit those of that loop written by hand.
    meter: a BinnedEvalMeter of K records (None: a fresh one whose values are the noises); rank_meter, qap_meter (a BinnedQapMeter,
    with features='weighted' a BinnedWeightedQapMeter), seed_meter: binned meters of K records, with the rules of evaluate_scores
    for refine, two_opt, faq and seeds (a tensor of seeds makes no sense across batches: 'scores' or the spec dict).
    Nothing is read until the end: ONE device-to-host copy of all the meters' records.  -> {'meter', 'records' (K dicts with 'noise',
    'loss', 'acc', 'acc_max', ...)} plus, for each meter given, 'rank_records' / 'qap_records' / 'seed_records', the meters' result()
    dicts.  One process: there is no split over ranks here."""
    from . import qap
    from .sampler import EpochSampler
    if method not in BASELINE_METHODS:
        raise ValueError("baseline_curve: method must be 'grampa' or 'degree_profile', got %r" % (method,))
    stray = sorted(k for k in kwargs if k not in _BASELINE_KWARGS[method])
    if stray:
        raise ValueError('baseline_curve: method %r takes no keyword %s' % (method, ', '.join(repr(k) for k in stray)))
    score_fn = qap.grampa if method == 'grampa' else qap.degree_profile
    if features not in (None, 'weighted'):
        raise ValueError("baseline_curve: features must be None or 'weighted', got %r" % (features,))
    if torch.is_tensor(seeds):
        raise ValueError("baseline_curve: seeds must be None, 'scores' or a spec dict (one seed tensor cannot serve every batch)")
    weighted = features == 'weighted'
    levels = generator.levels(noises)
    K, M, B = len(levels), int(num_examples), int(batch_size)
    if M < 1 or B < 1:
        raise ValueError('baseline_curve: num_examples and batch_size must be >= 1, got %d, %d' % (M, B))
    dev = generator.device
    if meter is None:
        meter = BinnedEvalMeter(dev, K, values=levels.noises)
    elif not isinstance(meter, BinnedEvalMeter) or meter.K != K:
        raise ValueError('baseline_curve: meter must be a BinnedEvalMeter of %d records or None' % K)
    qap_class = BinnedWeightedQapMeter if weighted else BinnedQapMeter
    for what, m, cls in (('rank_meter', rank_meter, BinnedRankMeter), ('qap_meter', qap_meter, qap_class),
                         ('seed_meter', seed_meter, BinnedSeedMeter)):
        if m is not None and (not isinstance(m, cls) or m.K != K):
            raise ValueError('baseline_curve: %s must be a %s of %d records or None' % (what, cls.__name__, K))
    decode = {}
    if qap_meter is not None:
        decode = {'qap_meter': qap_meter, 'refine': refine, 'two_opt': two_opt, 'faq': faq, 'seeds': seeds, 'seed_meter': seed_meter}
    elif refine or two_opt or faq is not None or seeds is not None or seed_meter is not None:
        raise ValueError('baseline_curve: refine=, two_opt=, faq=, seeds= and seed_meter= belong to a qap_meter')
    sampler = EpochSampler(K * M, shuffle=False, rank=0, world_size=1, drop_last=False, device=dev)
    for step in range(sampler.steps_per_epoch(B)):
        e = sampler.batch_index(0, step, B)
        pair, level, live = e % M, e // M, sampler.live_count(step, B)
        if not live:
            continue
        kw = {'index': pair, 'levels': levels, 'level': level, 'permute': permute}
        x1, x2, nv, *labels = generator.weighted(**kw) if weighted else generator.bits(**kw)
        labels = labels[0] if labels else None
        X = score_fn(x1, x2, nvalid=nv, labels=labels, weighted=weighted, **kwargs)['X']
        if qap_meter is not None:
            decode['adj' if weighted else 'bits'] = (x1, x2)
        evaluate_scores(X, nvalid=nv, labels=labels, meter=meter, live=live, bins=level, rank_meter=rank_meter, **decode)
    extra = [(k, m) for k, m in (('rank_records', rank_meter), ('qap_records', qap_meter), ('seed_records', seed_meter)) if m is not None]
    raws = _read(meter, *(m for _, m in extra))
    out = {'meter': meter}
    for key, m, recs in zip(['records'] + [k for k, _ in extra], [meter] + [m for _, m in extra], raws):
        rows = [pm._result(pm._dict(r)) for pm, r in zip(m.meters, recs)]
        for row, v in zip(rows, m.values or ()):
            row['noise'] = v
        out[key] = rows
    return out


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
