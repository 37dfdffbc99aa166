"""CPU: the reference and the host side of the device evaluation (no launch): tests/eval_ref.py against the oracle's loss, the
ctypes mirror of the epoch record against include/fgnn_hip.h, argument validation, the sampler's live-count arithmetic and the
scheduler wiring of FgnnTrainer.fit against torch's ReduceLROnPlateau."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import eval_ref as R
from graph_neural_net_amd import _lib
from graph_neural_net_amd.evaluation import EvalMeter, all_losses_acc, evaluate_scores, record_result
from graph_neural_net_amd.sampler import EpochSampler
from graph_neural_net_amd.trainer import FgnnTrainer
from oracle import fgnn_oracle as O
from util import ROOT


@pytest.mark.parametrize('N', [1, 2, 17, 50])
def test_reference_loss_equals_the_oracle_loss(N):
    """the helper's ce_sum / nodes is triplet_loss('mean') of the reference on stacked equal-size scores"""
    B = 5
    g = torch.Generator().manual_seed(N)
    s = R.make_scores(B, N, torch.full((B,), N, dtype=torch.int32), g).double()
    mine = R.loss_of([s[b].numpy() for b in range(B)])
    ref = O.triplet_loss_mean(s).item()
    assert abs(mine - ref) <= 1e-12 * max(abs(ref), 1.0), (mine, ref)
    # ... and the cost corner is -log_softmax
    ls = -torch.log_softmax(s[0], -1).numpy()
    assert np.abs(R.cost_corner(s[0].numpy()) - ls).max() <= 1e-12 * max(np.abs(ls).max(), 1.0)


def test_reference_meets_the_stability_cap():
    bad, tot = R.unstable_fraction()
    print('unstable pairs: %d of %d' % (bad, tot))
    assert tot == 2 * len(R.SIZES) * sum(R.BATCHES) and bad <= R.UNSTABLE_CAP * tot, (bad, tot)


def test_record_arithmetic():
    rec = R.fold_record([1.5, 2.25, 100.0], [3, 0, 7], [2, 0, 7], [1, 0, 6], live=2)
    assert rec == {'ce_sum': 3.75, 'nodes': 3, 'correct_lsap': 2, 'correct_max': 1, 'pairs': 2, 'steps': 1}
    assert R.fold_record([1.0], [1], [1], [1], live=0, start=rec) == rec
    res = record_result(rec)
    assert res == {'loss': 1.25, 'acc': 2 / 3, 'acc_max': 1 / 3, 'nodes': 3, 'pairs': 2}
    empty = record_result(R.fold_record([], [], [], [], live=0))
    assert np.isnan(empty['loss']) and np.isnan(empty['acc']) and empty['nodes'] == 0 and empty['pairs'] == 0


def test_eval_record_mirror_and_declarations():
    """the ctypes mirror gives the offsets the Python side views: it must be the struct of include/fgnn_hip.h"""
    hdr = open(os.path.join(ROOT, 'include', 'fgnn_hip.h')).read()
    body = re.search(r'typedef struct \{([^}]*)\} fgnn_eval_record;', hdr).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = [(m.group(2), m.group(1)) for m in re.finditer(r'(double|long long)\s+(\w+);', body)]
    ctype = {'double': C.c_double, 'long long': C.c_longlong}
    assert [(n, t) for n, t in _lib.EvalRecord._fields_] == [(n, ctype[t]) for n, t in fields]
    assert tuple(n for n, _ in fields) == EvalMeter.FIELDS
    assert C.sizeof(_lib.EvalRecord) == 48 and [getattr(_lib.EvalRecord, n).offset for n in EvalMeter.FIELDS] == [0, 8, 16, 24, 32, 40]
    assert int(re.search(r'#define FGNN_LSAP_MAX_N (\d+)', hdr).group(1)) == _lib.FGNN_LSAP_MAX_N
    lib = _lib.load()
    for name in ('fgnn_eval_pairs', 'fgnn_eval_fold'):
        m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, hdr)
        assert m, '%s is not declared in include/fgnn_hip.h' % name
        args = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
        assert hasattr(lib, name) and len(_lib._SIGNATURES[name]) == len(args.split(',')), name


def test_evaluate_scores_validates_before_anything_is_launched():
    with pytest.raises(RuntimeError, match='GPU'):
        evaluate_scores(torch.zeros(2, 4, 4))
    with pytest.raises(RuntimeError, match='GPU'):
        EvalMeter('cpu')
    for bad in (torch.zeros(4, 4), torch.zeros(2, 4, 5), torch.zeros(2, 4, 4, dtype=torch.int32), [[1.0]]):
        with pytest.raises(ValueError, match='scores'):
            evaluate_scores(bad)
    with pytest.raises(ValueError, match='eval_score'):
        all_losses_acc([], None, eval_score='hungarian')
    with pytest.raises(ValueError, match='labels'):
        all_losses_acc([(None, None)], None, labels=[None, None])
    losses, accs = all_losses_acc([], None)
    assert losses.shape == (0,) and accs.shape == (0,)


class _StubTrainer(FgnnTrainer):
    """fit() and evaluate() without a device: the optimizer is a bare learning rate, the epochs are scripted"""

    class _Opt:
        lr = 1e-3

    class _Meter:
        def __init__(self, loss):
            self.loss = loss

        def result(self):
            return {'loss': self.loss, 'acc': 0.5, 'acc_max': 0.25, 'nodes': 1, 'pairs': 1}

    def __init__(self, val_losses):
        self.opt = self._Opt()
        self.val_losses = list(val_losses)
        self.calls = []

    def train_epoch(self, generator, sampler, epoch, batch_size, permute=False, exact_last=False):
        self.calls.append(('train', generator, sampler, epoch, batch_size, self.opt.lr))
        return 'losses%d' % epoch

    def evaluate(self, generator, sampler, batch_size, epoch=0, hungarian=True, meter=None, permute=False, loss_on_labels=False,
                 rank_meter=None):
        self.calls.append(('eval', generator, sampler, epoch, batch_size))
        return self._Meter(self.val_losses[epoch])


def test_evaluate_validates_its_meter():
    tr = _StubTrainer([])
    tr.params = torch.zeros(1)
    with pytest.raises(ValueError, match='meter'):
        FgnnTrainer.evaluate(tr, None, EpochSampler(4), 2, meter={})
    with pytest.raises(RuntimeError, match='GPU'):          # a fresh meter for CPU parameters: there is no CPU path
        FgnnTrainer.evaluate(tr, None, EpochSampler(4), 2)
    with pytest.raises(ValueError, match='batch_size'):
        EpochSampler(4).live_count(0, 0)


@pytest.mark.parametrize('M,B,w,drop_last', [(10, 4, 1, False), (10, 4, 1, True), (10, 4, 2, False), (10, 4, 2, True), (10, 3, 3, False),
                                             (8, 4, 2, False), (1, 4, 3, False), (7, 1, 1, False)])
def test_sampler_live_counts(M, B, w, drop_last):
    """over the ranks and steps of an epoch the live positions are exactly the positions below num_examples, each once"""
    samplers = [EpochSampler(M, shuffle=False, rank=r, world_size=w, drop_last=drop_last) for r in range(w)]
    steps = samplers[0].steps_per_epoch(B)
    assert steps == (M // (B * w) if drop_last else -(-M // (B * w)))
    seen = []
    for step in range(steps):
        for s in samplers:
            first, count = s.window(step, B)
            live = s.live_count(step, B)
            assert 0 <= live <= count == B
            assert live == sum(1 for p in range(first, first + count) if p < M)
            seen += list(range(first, first + live))
    want = steps * B * w if drop_last else M
    assert sorted(seen) == list(range(want))
    if drop_last:
        assert all(s.live_count(k, B) == B for s in samplers for k in range(steps))
    with pytest.raises(ValueError, match='step'):
        samplers[0].live_count(steps, B)


def test_short_last_step_examples():
    s = EpochSampler(10, shuffle=False)
    assert [s.live_count(k, 4) for k in range(3)] == [4, 4, 2]
    two = [EpochSampler(10, shuffle=False, rank=r, world_size=2) for r in range(2)]
    assert [[t.live_count(k, 4) for k in range(2)] for t in two] == [[4, 2], [4, 0]]


VAL = [1.0, 0.9, 0.95, 0.95, 0.95, 0.95, 0.95, 0.8, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9,
       0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9]


def test_fit_drives_the_learning_rate_like_torch():
    """train_epoch, evaluate, scheduler.step(val_loss) per epoch; the default scheduler is the reference's ReduceLROnPlateau
    (factor 0.5, patience 3, min_lr 1e-5: models/trainers.py:92-104)"""
    tr = _StubTrainer(VAL)
    hist = tr.fit('tg', 'ts', 'vg', 'vs', len(VAL), 8)
    p = torch.nn.Parameter(torch.zeros(1))
    topt = torch.optim.Adam([p], lr=1e-3)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(topt, factor=0.5, patience=3, min_lr=1e-5)
    want = []
    for v in VAL:
        sched.step(v)
        want.append(topt.param_groups[0]['lr'])
    assert [h['lr'] for h in hist] == pytest.approx(want, rel=1e-12)
    assert want[0] == 1e-3 and want[-1] == 1e-5 and len(set(want)) > 3          # the script exercises decay and the floor
    assert [h['val_loss'] for h in hist] == VAL and [h['epoch'] for h in hist] == list(range(len(VAL)))
    assert hist[2]['train_losses'] == 'losses2' and hist[0]['val_acc'] == 0.5 and hist[0]['val_acc_max'] == 0.25
    # the order of events: train on the train pair, then evaluate on the validation pair, with the rate the scheduler left
    assert tr.calls[0] == ('train', 'tg', 'ts', 0, 8, 1e-3) and tr.calls[1] == ('eval', 'vg', 'vs', 0, 8)
    assert [c[0] for c in tr.calls] == ['train', 'eval'] * len(VAL)
    assert [c[5] for c in tr.calls[2::2]] == pytest.approx(want[:-1], rel=1e-12)
    # a scheduler of the caller's is used as it is
    class Sched:
        seen = []

        def step(self, v):
            self.seen.append(v)
    tr2 = _StubTrainer(VAL[:3])
    s = Sched()
    tr2.fit('tg', 'ts', 'vg', 'vs', 3, 8, scheduler=s)
    assert s.seen == VAL[:3] and tr2.opt.lr == 1e-3
