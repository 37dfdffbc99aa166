"""CPU: the host side of the decode epochs (no launch): the ctypes mirror of fgnn_qap_record against include/fgnn_hip.h, qap_result on
hand-made records, the all-reduce packing of a QapRecord buffer, the restatement tests/qap_fold_ref.py on a hand-made batch, and the
argument errors of evaluate_scores / FgnnTrainer."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import qap_fold_ref as QR
from graph_neural_net_amd import _lib
from graph_neural_net_amd.evaluation import (BinnedEvalMeter, BinnedQapMeter, EvalMeter, QapMeter, decode_scores, evaluate_scores, pack_records,
                                             qap_result, unpack_records_)
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.sampler import EpochSampler
from graph_neural_net_amd.trainer import FgnnTrainer
from util import ROOT

FIELDS = ('ratio_sum', 'ratio_pairs', 'qap_sum', 'planted_sum', 'correct', 'refined_sum', 'refined_correct', 'recovered', 'exact',
          'improved', 'unmatched', 'nodes', 'pairs', 'steps')


def test_qap_record_mirror_and_declarations():
    """the ctypes mirror gives the offsets the Python side views: it must be the struct of include/fgnn_hip.h"""
    hdr = open(os.path.join(ROOT, 'include', 'fgnn_hip.h')).read()
    body = re.search(r'typedef struct \{([^}]*)\} fgnn_qap_record;', hdr).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = [(m.group(2), m.group(1)) for m in re.finditer(r'(double|long long)\s+(\w+);', body)]
    ctype = {'double': C.c_double, 'long long': C.c_longlong}
    assert [(n, t) for n, t in _lib.QapRecord._fields_] == [(n, ctype[t]) for n, t in fields]
    assert tuple(n for n, _ in fields) == FIELDS == QapMeter.FIELDS == QR.FIELDS
    assert fields[0][1] == 'double' and all(t == 'long long' for _, t in fields[1:])          # (what pack_records relies on)
    assert C.sizeof(_lib.QapRecord) == 112 == QR.REC
    assert [getattr(_lib.QapRecord, n).offset for n in FIELDS] == list(range(0, 112, 8))
    lib = _lib.load()
    for name in ('fgnn_qap_fold', 'fgnn_qap_fold_bins'):
        m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, hdr)
        assert m, '%s is not declared in include/fgnn_hip.h' % name
        args = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
        assert name in _lib.EXPORTS and hasattr(lib, name) and len(_lib._SIGNATURES[name]) == len(args.split(',')), name


def test_qap_result_on_hand_made_records():
    rec = dict(zip(FIELDS, (1.75, 2, 30, 40, 11, 36, 13, 1, 1, 2, 1, 20, 4, 2)))
    res = qap_result(rec)
    assert res == {'acc': 11 / 20, 'qap_ratio': 30 / 40, 'mean_ratio': 1.75 / 2, 'recovered': 1 / 4, 'exact': 1 / 4, 'unmatched': 1,
                   'nodes': 20, 'pairs': 4}
    res = qap_result(dict(rec, refined=True))
    assert res['refined_acc'] == 13 / 20 and res['refined_qap_ratio'] == 36 / 40 and res['improved'] == 2 / 4 and res['acc'] == 11 / 20
    assert set(res) == {'acc', 'qap_ratio', 'mean_ratio', 'recovered', 'exact', 'unmatched', 'nodes', 'pairs', 'refined_acc',
                        'refined_qap_ratio', 'improved'}
    empty = qap_result(dict(QR.empty(), refined=True))
    for key in ('acc', 'qap_ratio', 'mean_ratio', 'recovered', 'exact', 'refined_acc', 'refined_qap_ratio', 'improved'):
        assert np.isnan(empty[key]), key
    assert empty['unmatched'] == empty['nodes'] == empty['pairs'] == 0
    # pairs without a planted objective: the ratios are NaN, the accuracies are not
    res = qap_result(dict(QR.empty(), correct=3, nodes=4, pairs=1, recovered=1))
    assert res['acc'] == 0.75 and res['recovered'] == 1.0 and np.isnan(res['qap_ratio']) and np.isnan(res['mean_ratio'])


def test_restatement_on_a_hand_made_batch():
    """four pairs of N = 3 by hand: an exact one, an unmatched one, one without a planted objective, one beyond `live`"""
    assign = np.array([[0, 1, 2], [-1, 0, -1], [1, 0, -1], [0, 1, 2]], dtype=np.int32)
    perm = np.array([[0, 2, 1], [0, 1, 2], [0, 1, -1], [0, 1, 2]], dtype=np.int32)
    qap, planted, refined = [6, -1, 4, 9], [8, 5, 0, 9], [10, -1, 4, 9]
    nv = [3, 3, 2, 3]
    recs, correct, rcorrect, ratio = QR.fold(assign, perm, None, qap, planted, refined, nv, 3)
    assert correct.tolist() == [3, 0, 0, 0] and rcorrect.tolist() == [1, 3, 2, 0] and ratio.tolist() == [0.75, 0.0, 0.0, 0.0]
    assert recs == [dict(zip(FIELDS, (0.75, 1, 10, 8, 3, 14, 6, 1, 1, 1, 1, 8, 3, 1)))]
    # without a refinement its three fields stay; live = 0 changes nothing, the step count included
    plain = QR.fold(assign, None, None, qap, planted, None, nv, 3)[0]
    assert plain == [dict(recs[0], refined_sum=0, refined_correct=0, improved=0)]
    assert QR.fold(assign, perm, None, qap, planted, refined, nv, 0, start=recs)[0] == recs
    # labels: -1 and an entry >= n_b are no targets
    lab = np.array([[0, -1, 2], [0, 1, 2], [1, 2, 0], [0, 1, 2]], dtype=np.int32)
    assert QR.pair_counts(assign, perm, lab, nv, 4)[0].tolist() == [2, 0, 1, 3]
    # bins: K = 3, bin 1 stays empty, a bin outside [0, K) is dropped; the bytes round-trip
    binned = QR.fold(assign, perm, None, qap, planted, refined, nv, 4, bin=[2, 0, 7, 2], K=3)[0]
    assert [r['pairs'] for r in binned] == [1, 0, 2] and [r['steps'] for r in binned] == [1, 0, 1] and binned[1] == QR.empty()
    assert binned[2]['ratio_sum'] == 0.75 + 1.0 and binned[0]['unmatched'] == 1
    assert QR.from_bytes(QR.to_bytes(binned)) == binned


def test_pack_and_unpack_round_trip_a_qap_record_buffer():
    """the all-reduce form of K records: word 0 as it is, the counts through fp64 and back"""
    recs = [dict(zip(FIELDS, (0.1 + k, 3 + k, 10 ** 12 + k, 7, 5, 2 ** 40, 1, 0, 2, 3, 4, 50, 6, 7))) for k in range(3)]
    buf = torch.from_numpy(QR.to_bytes(recs))
    t = pack_records(buf, 3, 14)
    assert t.shape == (3, 14) and t.dtype == torch.float64 and t[1, 0].item() == 1.1 and t[2, 2].item() == 10 ** 12 + 2
    out = unpack_records_(torch.zeros_like(buf), 3, t)
    assert torch.equal(out, buf)
    assert QR.from_bytes(unpack_records_(torch.zeros_like(buf), 3, 2 * t).numpy())[1]['refined_sum'] == 2 ** 41


class _Stub(FgnnTrainer):
    def __init__(self):
        self.params = torch.zeros(1)


class _CurveGenerator:
    device = torch.device('cpu')

    def levels(self, noises):
        return PairGenerator(20, 'ErdosRenyi', device='cpu').levels(noises)


def _binned(cls, K):
    meter = cls.__new__(cls)
    meter.K = K
    return meter


def test_argument_errors_are_raised_before_anything_is_launched():
    s = torch.zeros(2, 4, 4)
    with pytest.raises(RuntimeError, match='GPU'):
        QapMeter('cpu')
    with pytest.raises(RuntimeError, match='GPU'):
        BinnedQapMeter('cpu', 3)
    with pytest.raises(ValueError, match='records'):
        BinnedQapMeter('cpu', _lib.FGNN_MAX_LEVELS + 1)
    with pytest.raises(ValueError, match='values'):
        BinnedQapMeter('cpu', 3, values=(0.0, 0.1))
    # the solver's assignment is what a qap_meter decodes
    with pytest.raises(ValueError, match='hungarian=True'):
        evaluate_scores(s, qap_meter=object(), bits=(None, None), hungarian=False)
    with pytest.raises(ValueError, match='belong to a qap_meter'):
        evaluate_scores(s, refine=3)
    with pytest.raises(ValueError, match='refine'):
        evaluate_scores(s, qap_meter=object(), bits=(None, None), refine=-1)
    with pytest.raises(ValueError, match='refine'):
        decode_scores(s, None, None, refine=1.5)
    with pytest.raises(ValueError, match='go together'):
        decode_scores(s, None, None, bins=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='GPU only'):
        decode_scores(s, None, None)
    # a meter of the wrong kind, a K mismatch
    tr = _Stub()
    with pytest.raises(ValueError, match='qap_meter must be a QapMeter'):
        tr.evaluate(None, EpochSampler(4), 2, meter=EvalMeter.__new__(EvalMeter), qap_meter={})
    with pytest.raises(ValueError, match='qap_meter must be a QapMeter'):
        tr.evaluate(None, EpochSampler(4), 2, meter=EvalMeter.__new__(EvalMeter), qap_meter=_binned(BinnedQapMeter, 3))
    args = (_CurveGenerator(), (0.0, 0.2, 0.5), 5, 4)
    with pytest.raises(ValueError, match='BinnedQapMeter of 3 records'):
        tr.noise_curve(*args, meter=_binned(BinnedEvalMeter, 3), qap_meter=_binned(BinnedQapMeter, 2))
    with pytest.raises(ValueError, match='BinnedQapMeter of 3 records'):
        tr.noise_curve(*args, meter=_binned(BinnedEvalMeter, 3), qap_meter=QapMeter.__new__(QapMeter))
    with pytest.raises(ValueError, match='refine'):
        tr.fit(None, None, None, None, 1, 4, scheduler=object(), decode_refine=-2)
