"""CPU: the host side of the noise curve (no launch): the two entry points in the header and in _lib, the threshold table of
PairGenerator.levels against tests/pairgen_ref.py, argument validation, and the example -> (pair, level) arithmetic of
FgnnTrainer.noise_curve with its live counts."""
import os
import re

import pytest
import torch

import pairgen_ref as P
from graph_neural_net_amd import _lib, dp
from graph_neural_net_amd.evaluation import BinnedEvalMeter, evaluate_scores
from graph_neural_net_amd.pairgen import NoiseLevels, PairGenerator, same_device
from graph_neural_net_amd.sampler import EpochSampler
from graph_neural_net_amd.trainer import FgnnTrainer
from util import ROOT


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'fgnn_hip.h')).read()
    assert int(re.search(r'#define FGNN_MAX_LEVELS (\d+)', hdr).group(1)) == _lib.FGNN_MAX_LEVELS == 64
    lib = _lib.load()
    for name in ('fgnn_pairgen_levels', 'fgnn_eval_fold_bins'):
        m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, hdr)
        assert m, '%s is not declared in include/fgnn_hip.h' % name
        args = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
        assert name in _lib.EXPORTS and hasattr(lib, name) and len(_lib._SIGNATURES[name]) == len(args.split(',')), name


@pytest.mark.parametrize('p', [0.2, 0.5])
def test_threshold_table(p):
    noises = (0.0, 0.1, 1.0)
    g = PairGenerator(50, 'ErdosRenyi', 'ErdosRenyi', edge_density=p, noise=0.3, device='cpu')
    lv = g.levels(noises)
    assert isinstance(lv, NoiseLevels) and len(lv) == 3 and lv.noises == noises
    assert lv.table.dtype == torch.int64 and tuple(lv.table.shape) == (3, 2)
    assert lv.table.tolist() == [[P.threshold(v), P.threshold(p * v / (1 - p))] for v in noises]
    assert lv.table[2, 0].item() == 1 << 32 and lv.table[0].tolist() == [0, 0]
    # a level's row is what a generator of that single noise value compares with
    for k, v in enumerate(noises):
        one = PairGenerator(50, 'ErdosRenyi', 'ErdosRenyi', edge_density=p, noise=v, device='cpu')
        assert tuple(lv.table[k].tolist()) == one._thr[1:3]


def test_levels_are_validated():
    g = PairGenerator(20, 'ErdosRenyi', device='cpu')
    for bad in ([-0.1], [0.2, 1.5], [float('nan')]):
        with pytest.raises(ValueError, match='noise'):
            g.levels(bad)
    with pytest.raises(ValueError, match='levels'):
        g.levels([])
    with pytest.raises(ValueError, match='levels'):
        g.levels([0.01 * k for k in range(65)])
    assert len(g.levels([0.01 * k for k in range(64)])) == 64
    lv = g.levels([0.0, 0.5])
    for method in (g.bits, g.dense, g.spectral):
        with pytest.raises(ValueError, match='go together'):
            method(0, 2, level=[0, 1])
        with pytest.raises(ValueError, match='go together'):
            method(0, 2, levels=lv)
    with pytest.raises(ValueError, match='level must be'):
        g.bits(0, 2, levels=lv, level=[0, 1, 0])
    with pytest.raises(ValueError, match='level must be'):
        g.bits(0, 2, levels=lv, level=torch.zeros(2))
    other = PairGenerator(20, 'ErdosRenyi', edge_density=0.4, device='cpu')
    with pytest.raises(ValueError, match='this generator'):
        other.bits(0, 2, levels=lv, level=[0, 1])
    with pytest.raises(RuntimeError, match='no CPU path'):          # everything valid: only the device is missing
        g.bits(0, 2, levels=lv, level=[0, 1])


def test_binned_meter_and_bins_go_together():
    s = torch.zeros(2, 4, 4)
    with pytest.raises(ValueError, match='go together'):
        evaluate_scores(s, bins=torch.zeros(2, dtype=torch.int32))
    binned = BinnedEvalMeter.__new__(BinnedEvalMeter)       # (never initialised: the check comes before anything looks at it)
    with pytest.raises(ValueError, match='go together'):
        evaluate_scores(s, meter=binned)
    for K in (0, 65):
        with pytest.raises(ValueError, match='records'):
            BinnedEvalMeter('cpu', K)
    with pytest.raises(ValueError, match='values'):
        BinnedEvalMeter('cpu', 2, values=(0.1,))
    with pytest.raises(RuntimeError, match='GPU'):
        BinnedEvalMeter('cpu', 2)


def test_noise_curve_arithmetic_on_two_ranks():
    """K * M = 15 examples, B = 4, two ranks: every example once, level-major, full batches, the filling wraps to example 0"""
    K, M, B, w = 3, 5, 4, 2
    samplers = [EpochSampler(K * M, shuffle=False, rank=r, world_size=w, drop_last=False, device='cpu') for r in range(w)]
    assert samplers[0].steps_per_epoch(B) == 2
    seen, lives = [], []
    for step in range(2):
        for r, smp in enumerate(samplers):
            pair, level, live = FgnnTrainer.noise_curve_batch(smp, step, B, M)
            assert pair.dtype == level.dtype == torch.int64 and tuple(pair.shape) == tuple(level.shape) == (B,)
            first = step * B * w + r * B
            e = [(first + i) % (K * M) for i in range(B)]
            assert pair.tolist() == [x % M for x in e] and level.tolist() == [x // M for x in e]
            assert int(level.min()) >= 0 and int(level.max()) < K
            lives.append(live)
            seen += [(int(level[i]), int(pair[i])) for i in range(live)]
    assert lives == [4, 4, 4, 3]
    assert seen == [(k, m) for k in range(K) for m in range(M)]
    # rank 1's last position is past the end: it repeats example 0 (pair 0 at level 0) and is masked by live
    pair, level, live = FgnnTrainer.noise_curve_batch(samplers[1], 1, B, M)
    assert (pair[3].item(), level[3].item(), live) == (0, 0, 3)


def test_levels_device_is_compared_by_what_it_names(monkeypatch):
    """a generator built with device='cuda' keeps no index while its table reports 'cuda:<current>': the same device"""
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 1)
    D = torch.device
    assert D('cuda') != D('cuda:1')          # (why the comparison is not torch's)
    assert same_device('cuda', 'cuda:1') and same_device(D('cuda:1'), D('cuda')) and same_device('cuda', 'cuda')
    assert same_device('cuda:0', 'cuda:0') and same_device('cpu', 'cpu')
    assert not same_device('cuda', 'cuda:0') and not same_device('cuda:0', 'cuda:1') and not same_device('cpu', 'cuda')

    class _Table:          # a table where `.to('cuda')` would have put it
        device = D('cuda:1')

    g = PairGenerator(20, 'ErdosRenyi', device='cuda')
    lv = PairGenerator(20, 'ErdosRenyi', device='cpu').levels([0.0, 0.5])
    with pytest.raises(ValueError, match='this generator'):
        g._level(lv, [0, 1], 2)
    lv.table = _Table()
    monkeypatch.setattr(torch.Tensor, 'to', lambda self, *a, **k: self)          # (no device here: keep the level list where it is)
    assert g._level(lv, [0, 1], 2).tolist() == [0, 1]
    assert PairGenerator(20, 'ErdosRenyi', device='cuda:1')._level(lv, [1, 1], 2).tolist() == [1, 1]
    with pytest.raises(ValueError, match='this generator'):
        PairGenerator(20, 'ErdosRenyi', device='cuda:0')._level(lv, [0, 1], 2)


def test_a_generator_without_levels_checks_the_device_first():
    """the order of the checks without the new arguments is the one it was: no CPU path before anything about the selection"""
    g = PairGenerator(20, 'ErdosRenyi', device='cpu')
    for method in (g.bits, g.dense, g.spectral):
        with pytest.raises(RuntimeError, match='no CPU path'):
            method()
        with pytest.raises(RuntimeError, match='no CPU path'):
            method(-1, 2)


class _CurveTrainer(FgnnTrainer):
    """noise_curve without a device: the steps are recorded"""

    def __init__(self):
        self.steps = []

    def eval_step_bits(self, bits1, bits2, nvalid=None, labels=None, meter=None, live=None, hungarian=True, loss_on_labels=False,
                       bins=None, rank_meter=None):
        self.steps.append((bits1.tolist(), bins.tolist(), live, (loss_on_labels, rank_meter)))


class _CurveGenerator:
    device = torch.device('cpu')

    def levels(self, noises):
        return PairGenerator(20, 'ErdosRenyi', device='cpu').levels(noises)

    def bits(self, index=None, levels=None, level=None, permute=False):
        assert len(levels) == 3 and isinstance(permute, bool)          # (any other keyword is a TypeError)
        return (index, level, None) + ((index,) if permute else ())


def _curve_meter():
    meter = BinnedEvalMeter.__new__(BinnedEvalMeter)
    meter.K, meter.reduced = 3, 0

    def allreduce_():
        meter.reduced += 1
    meter.allreduce_ = allreduce_
    return meter


def test_noise_curve_loop_and_its_all_reduce(monkeypatch):
    """which steps a rank runs, what they are handed, and that the records are summed exactly when torch.distributed's ranks split the work"""
    K, M, B = 3, 5, 4
    args = (_CurveGenerator(), (0.0, 0.2, 0.5), M, B)
    tr, meter = _CurveTrainer(), _curve_meter()
    assert tr.noise_curve(*args, meter=meter) is meter and meter.reduced == 0
    assert [s[2] for s in tr.steps] == [4, 4, 4, 3]
    seen = [(l, p) for pair, lev, live, kw in tr.steps for p, l in list(zip(pair, lev))[:live]]
    assert seen == [(k, m) for k in range(K) for m in range(M)] and all(s[3] == (False, None) for s in tr.steps)
    # parts of a split walked in one process: nothing is reduced
    tr, meter = _CurveTrainer(), _curve_meter()
    tr.noise_curve(*args, meter=meter, rank=1, world_size=2, permute=True, loss_on_labels=True)
    assert [s[2] for s in tr.steps] == [4, 3] and meter.reduced == 0 and all(s[3] == (True, None) for s in tr.steps)
    # two ranks of torch.distributed: this rank's share, one all-reduce; with world_size=1 a whole curve of its own, none
    monkeypatch.setattr(dp, 'world_size', lambda: 2)
    monkeypatch.setattr(torch.distributed, 'get_rank', lambda: 1)
    tr, meter = _CurveTrainer(), _curve_meter()
    tr.noise_curve(*args, meter=meter)
    assert [s[2] for s in tr.steps] == [4, 3] and tr.steps[0][0] == [4, 0, 1, 2] and meter.reduced == 1
    tr, meter = _CurveTrainer(), _curve_meter()
    tr.noise_curve(*args, meter=meter, world_size=1)
    assert [s[2] for s in tr.steps] == [4, 4, 4, 3] and meter.reduced == 0
    with pytest.raises(ValueError, match='meter'):
        tr.noise_curve(*args, meter={})
