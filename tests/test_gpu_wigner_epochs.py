"""GPU: the weighted steps and epochs -- evaluate_scores(adj=), FgnnTrainer.eval_step(qap_meter=...) and features='weighted' on
train_epoch / evaluate / noise_curve / fit -- against the hand-written loops over WignerGenerator.weighted, train_step, eval_step
and decode_scores_weighted.  Everything compared is a device tensor of a fixed launch sequence: torch.equal.

A 1-block 2/32/32 fp32 trainer, N = 12, a dataset of 10 examples in batches of 4: the short last step exercises `live`."""
import math

import pytest
import torch

from graph_neural_net_amd import _lib
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.evaluation import (BinnedEvalMeter, BinnedWeightedQapMeter, EvalMeter, QapMeter, SeedMeter, WeightedQapMeter,
                                             decode_scores_weighted, evaluate_scores)
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.sampler import EpochSampler
from graph_neural_net_amd.trainer import FgnnTrainer
from graph_neural_net_amd.wigner import WignerGenerator

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LAY = ParamLayout(2, 1, 32, 32, 3)
N, M, TB = 12, 10, 4
REC = _lib.QapwRecord
STEPS = REC.steps.offset


def _gen(noise=0.3, seed=11, **kw):
    return WignerGenerator(N, noise=noise, seed=seed, device=DEV, **kw)


def _trainer(**kw):
    return FgnnTrainer(LAY, LAY.init_flat(7, DEV), lr=2e-3, **kw)


def _sampler(shuffle=False):
    return EpochSampler(M, seed=3, shuffle=shuffle, device=DEV)


def _but_steps(buf):
    out = buf.clone().view(-1, STEPS + 8)          # (steps is the record's last word)
    out[:, STEPS:STEPS + 8] = 0
    return out


def test_train_epoch_equals_the_hand_written_loop():
    gen, smp = _gen(), _sampler(shuffle=True)
    a, b = _trainer(), _trainer()
    losses = a.train_epoch(gen, smp, 1, TB, permute=True, exact_last=True, features='weighted')
    steps = smp.steps_per_epoch(TB)
    assert steps == 3 and losses.shape == (3,) and bool(torch.isfinite(losses).all())
    for step in range(steps):
        x1, x2, nv, lab = gen.weighted(index=smp.batch_index(1, step, TB), permute=True)
        loss, _ = b.train_step(x1, x2, nv, labels=lab, live=smp.live_count(step, TB))
        assert torch.equal(loss, losses[step]), step
    assert torch.equal(a.params, b.params) and torch.equal(a.opt.exp_avg, b.opt.exp_avg)
    assert not torch.equal(a.params, LAY.init_flat(7, DEV))


def _hand_evaluate(tr, gen, smp, B, **decode):
    meter, qm = EvalMeter(DEV), WeightedQapMeter(DEV)
    for step in range(smp.steps_per_epoch(B)):
        live = smp.live_count(step, B)
        x1, x2, nv, lab = gen.weighted(index=smp.batch_index(0, step, B), permute=True)
        out = tr.eval_step(x1, x2, nv, labels=lab, meter=meter, live=live)
        scores = tr._eval_forward(B, N, nv, x=torch.cat([x1, x2]).contiguous())
        decode_scores_weighted(scores, x1, x2, nvalid=nv, labels=lab, meter=qm, live=live, assign=out['assign'], **decode)
    return meter, qm


def test_evaluate_equals_the_hand_written_loop_and_does_not_depend_on_the_batching():
    tr, gen, smp = _trainer(), _gen(), _sampler()
    before = tr.params.clone()
    qm = WeightedQapMeter(DEV)
    meter = tr.evaluate(gen, smp, TB, permute=True, features='weighted', qap_meter=qm, refine=1, two_opt=True)
    hm, hq = _hand_evaluate(tr, gen, smp, TB, refine=1, two_opt=True)
    assert torch.equal(meter.buf, hm.buf) and torch.equal(qm.buf, hq.buf) and qm.refined
    res = qm.result()
    assert res['pairs'] == M and res['nodes'] == M * N and res['unmatched'] == 0 and math.isfinite(res['qap_ratio'])
    q3 = WeightedQapMeter(DEV)
    m3 = tr.evaluate(gen, smp, 3, permute=True, features='weighted', qap_meter=q3, refine=1, two_opt=True)
    assert torch.equal(_but_steps(q3.buf), _but_steps(qm.buf)) and q3.record()['steps'] == 4 and qm.record()['steps'] == 3
    assert m3.record()['correct_lsap'] == meter.record()['correct_lsap'] and m3.record()['nodes'] == meter.record()['nodes']
    assert torch.equal(tr.params, before)


def test_the_labels_matching_reaches_the_planted_objective():
    gen = _gen()
    x1, x2, nv, lab = gen.weighted(0, TB, permute=True)
    s = torch.zeros(TB, N, N, device=DEV)
    out = decode_scores_weighted(s, x1, x2, labels=lab, assign=lab)
    assert torch.equal(out['qap'], out['planted']) and bool((out['qap'] > 0).all())
    assert out['meter'].result()['recovered'] == 1.0 and out['correct'].tolist() == [N] * TB


def test_evaluate_with_faq_and_revealed_seeds():
    tr, gen, smp = _trainer(), _gen(), _sampler()
    qm, sm = WeightedQapMeter(DEV), SeedMeter(DEV)
    tr.evaluate(gen, smp, TB, permute=True, features='weighted', qap_meter=qm, faq={'P0': 'barycenter'}, seeds=2, seed_meter=sm)
    res, sres = qm.result(), sm.result()
    assert res['pairs'] == M and math.isfinite(res['qap_ratio']) and math.isfinite(res['refined_qap_ratio'])
    assert sres['seeds'] == 2 * M and sres['seed_precision'] == 1.0 and math.isfinite(sres['free_acc'])
    with pytest.raises(ValueError, match='permute=True'):
        tr.evaluate(gen, smp, TB, features='weighted', qap_meter=WeightedQapMeter(DEV), faq={'P0': 'barycenter'}, seeds=2)


def test_noise_curve_equals_evaluate_per_level():
    tr, noises = _trainer(), (0.0, 0.5)
    gen = _gen(noise=0.9)                            # (its own noise must not matter)
    qm = BinnedWeightedQapMeter(DEV, 2, values=noises)
    meter = tr.noise_curve(gen, noises, M, TB, permute=True, features='weighted', qap_meter=qm, two_opt=True)
    assert isinstance(meter, BinnedEvalMeter) and len(meter.result()) == 2
    for k, s in enumerate(noises):
        q1 = WeightedQapMeter(DEV)
        m1 = tr.evaluate(_gen(noise=s), _sampler(), TB, permute=True, features='weighted', qap_meter=q1, two_opt=True)
        assert torch.equal(_but_steps(qm[k].buf), _but_steps(q1.buf)), k
        assert meter[k].record()['correct_lsap'] == m1.record()['correct_lsap'] and meter[k].record()['nodes'] == M * N
    # noise 0: the two sides are one graph relabelled, so the labels' matching has ratio 1
    x1, x2, _, lab = _gen(noise=0.0).weighted(0, TB, permute=True)
    out = decode_scores_weighted(torch.zeros(TB, N, N, device=DEV), x1, x2, labels=lab, assign=lab)
    assert out['ratio'].tolist() == [1.0] * TB
    with pytest.raises(ValueError, match='BinnedWeightedQapMeter'):
        from graph_neural_net_amd.evaluation import BinnedQapMeter
        tr.noise_curve(gen, noises, M, TB, features='weighted', qap_meter=BinnedQapMeter(DEV, 2))


def test_fit_reports_the_documented_keys():
    tr = _trainer()
    hist = tr.fit(_gen(seed=1), _sampler(shuffle=True), _gen(seed=2), _sampler(), 2, TB, permute=True, exact_last=True,
                  features='weighted', decode_refine=0)
    assert [h['epoch'] for h in hist] == [0, 1]
    for h in hist:
        assert set(h) == {'epoch', 'train_losses', 'val_loss', 'val_acc', 'val_acc_max', 'lr', 'val_qap_ratio', 'val_recovered'}
        assert h['train_losses'].shape == (3,) and math.isfinite(h['val_loss']) and math.isfinite(h['val_qap_ratio'])
        assert 0.0 <= h['val_acc'] <= 1.0 and 0.0 <= h['val_recovered'] <= 1.0


def test_one_bf16_step_on_the_same_tensors():
    tr = _trainer(precision='bf16')
    x1, x2, nv = _gen().weighted(0, TB)
    loss, scores = tr.train_step(x1, x2, nv)
    assert bool(torch.isfinite(loss)) and scores.shape[0] == TB
    losses = tr.train_epoch(_gen(), _sampler(), 0, TB, features='weighted')
    assert bool(torch.isfinite(losses).all())


def test_a_ragged_weighted_epoch():
    tr, gen = _trainer(), _gen(vertex_proba=0.7)
    losses = tr.train_epoch(gen, _sampler(), 0, TB, permute=True, exact_last=True, features='weighted')
    qm = WeightedQapMeter(DEV)
    meter = tr.evaluate(gen, _sampler(), TB, permute=True, features='weighted', qap_meter=qm)
    nodes = int(gen.weighted(0, M)[2].sum())
    assert bool(torch.isfinite(losses).all()) and meter.record()['nodes'] == nodes and qm.record()['nodes'] == nodes


def test_refusals():
    tr, gen, smp = _trainer(), _gen(), _sampler()
    bits = PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, device=DEV)
    for call in (lambda g: tr.train_epoch(g, smp, 0, TB, features='weighted'), lambda g: tr.evaluate(g, smp, TB, features='weighted'),
                 lambda g: tr.noise_curve(g, (0.0, 0.5), M, TB, features='weighted'),
                 lambda g: tr.fit(g, smp, g, smp, 1, TB, features='weighted')):
        with pytest.raises(ValueError, match='weighted'):
            call(bits)
    with pytest.raises(ValueError, match='tensor_representation'):
        _trainer(input_form='tensor_representation').train_epoch(gen, smp, 0, TB, features='weighted')
    lay32 = ParamLayout(32, 1, 32, 32, 3)            # fp32: the input has exactly original_features_num channels
    with pytest.raises(ValueError, match='original_features_num'):
        FgnnTrainer(lay32, lay32.init_flat(7, DEV)).evaluate(gen, smp, TB, features='weighted')
    with pytest.raises(ValueError, match="'weighted'"):
        tr.evaluate(gen, smp, TB, features='dense')
    with pytest.raises(ValueError, match='WeightedQapMeter'):
        tr.evaluate(gen, smp, TB, features='weighted', qap_meter=QapMeter(DEV))
    with pytest.raises(RuntimeError, match='weighted'):
        tr.evaluate(gen, smp, TB)                     # the bits loop on a WignerGenerator: .bits names .weighted
    x1, x2, _ = gen.weighted(0, TB)
    b1, b2, _ = bits.bits(0, TB)
    s = torch.zeros(TB, N, N, device=DEV)
    with pytest.raises(ValueError, match='not both'):
        evaluate_scores(s, qap_meter=WeightedQapMeter(DEV), bits=(b1, b2), adj=(x1, x2))
    with pytest.raises(ValueError):
        evaluate_scores(s, qap_meter=QapMeter(DEV), adj=(x1, x2))
    with pytest.raises(ValueError):
        evaluate_scores(s, qap_meter=WeightedQapMeter(DEV), bits=(b1, b2))
    with pytest.raises(ValueError, match='qap_meter'):
        evaluate_scores(s, adj=(x1, x2))
    with pytest.raises(ValueError):
        tr.eval_step(x1, x2, qap_meter=QapMeter(DEV))


def test_eval_step_without_the_new_keywords_is_unchanged():
    tr = _trainer()
    x1, x2, _ = _gen().weighted(0, TB)
    out = tr.eval_step(x1, x2)
    assert set(out) == {'ce', 'n', 'correct_max', 'correct_lsap', 'assign', 'meter'}
    qm = WeightedQapMeter(DEV)
    dec = tr.eval_step(x1, x2, qap_meter=qm, two_opt=True)
    assert set(dec) == set(out) | {'decode'} and torch.equal(dec['assign'], out['assign']) and torch.equal(dec['ce'], out['ce'])
    by_hand = decode_scores_weighted(tr._eval_forward(TB, N, None, x=torch.cat([x1, x2]).contiguous()), x1, x2, two_opt=True)
    assert torch.equal(qm.buf, by_hand['meter'].buf) and torch.equal(dec['decode']['perm'], by_hand['perm'])
