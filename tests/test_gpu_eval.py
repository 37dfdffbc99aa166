"""GPU: validation on the device -- fgnn_eval_pairs / fgnn_eval_fold (csrc/eval.hip), evaluation.evaluate_scores / EvalMeter /
all_losses_acc and FgnnTrainer.eval_step_bits / evaluate -- against the fp64 references of tests/eval_ref.py.

Scores carry NaN in their padding and every output buffer is NaN- or sentinel-filled before each call, so a kernel that reads
padding, writes outside the valid corner or leaves an output unwritten fails here.

Measured on the MI355X, worst over every case of test_eval_pairs_and_fold as a fraction of the CE bound 1e-5 (|lse| + |s|): a cost
entry 0.029, a pair CE sum 0.005."""
import numpy as np
import pytest
import torch

import eval_ref as R
from graph_neural_net_amd import _lib
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.evaluation import EvalMeter, all_losses_acc, evaluate_scores
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.sampler import EpochSampler
from graph_neural_net_amd.siamese import Siamese_Node_Exp
from graph_neural_net_amd.trainer import FgnnTrainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
SENTINEL = -77


def _launch(sd, nvd, labd, B, N, live=None, meter=None, hungarian=True):
    """fgnn_eval_pairs -> fgnn_lsap_accuracy (-> fgnn_count_matches) -> fgnn_eval_fold on filled buffers -> dict of device tensors"""
    f32 = dict(dtype=torch.float32, device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    o = {'cost': torch.full((B, N, N), NAN, **f32), 'row_ce': torch.full((B, N), NAN, **f32),
         'row_hit': torch.full((B, N), SENTINEL, **i32), 'pair_ce': torch.full((B,), NAN, dtype=torch.float64, device=DEV),
         'pair_max': torch.full((B,), SENTINEL, **i32), 'correct': torch.full((B,), SENTINEL, **i32),
         'assign': torch.full((B, N), SENTINEL, **i32), 'meter': meter if meter is not None else EvalMeter(DEV)}
    st = _lib.stream_ptr()
    _lib.call('fgnn_eval_pairs', _lib.ptr(sd), _lib.ptr(nvd), _lib.ptr(labd), B, N, _lib.ptr(o['cost']), N * N, N,
              _lib.ptr(o['row_ce']), _lib.ptr(o['row_hit']), st)
    if hungarian:
        _lib.call('fgnn_lsap_accuracy', _lib.ptr(o['cost']), N * N, N, _lib.ptr(nvd), B, N, _lib.ptr(o['correct']), _lib.ptr(o['assign']), st)
        if labd is not None:
            _lib.call('fgnn_count_matches', _lib.ptr(o['assign']), _lib.ptr(labd), _lib.ptr(nvd), B, N, _lib.ptr(o['correct']), st)
    _lib.call('fgnn_eval_fold', _lib.ptr(o['row_ce']), _lib.ptr(o['row_hit']), _lib.ptr(o['correct']) if hungarian else None,
              _lib.ptr(nvd), B, N, B if live is None else live, _lib.ptr(o['pair_ce']), _lib.ptr(o['pair_max']), _lib.ptr(o['meter'].buf), st)
    return o


def _accuracy_max(sd, nvd, labd, B, N):
    correct = torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV)
    if labd is None:
        _lib.call('fgnn_accuracy_max', _lib.ptr(sd), _lib.ptr(nvd), B, N, _lib.ptr(correct), _lib.stream_ptr())
    else:
        _lib.call('fgnn_accuracy_max_labels', _lib.ptr(sd), _lib.ptr(labd), _lib.ptr(nvd), B, N, _lib.ptr(correct), _lib.stream_ptr())
    return correct.cpu().tolist()


def _check_against_reference(c, o, B, N, ragged, with_labels):
    """every output of one launch sequence against the shared reference `c`; returns the worst error / bound ratios"""
    nv, pairs = c['nv'], c['pairs']
    corner = R.corner(nv, N)
    rows = torch.arange(N)[None, :] < nv.long()[:, None]
    cost, row_ce, row_hit = o['cost'].cpu(), o['row_ce'].cpu(), o['row_hit'].cpu()
    # nothing outside the corner was written
    assert bool(torch.isnan(cost[~corner]).all()) and bool(torch.isnan(row_ce[~rows]).all())
    assert bool((row_hit[~rows] == SENTINEL).all()) and bool(((row_hit[rows] == 0) | (row_hit[rows] == 1)).all())
    hits_ref = [p['hits_labels' if with_labels else 'hits'] for p in pairs]
    assert [int(row_hit[b, :p['n']].sum()) for b, p in enumerate(pairs)] == hits_ref
    assert o['pair_max'].cpu().tolist() == hits_ref
    pair_ce = o['pair_ce'].cpu().numpy()
    worst_cost = worst_ce = 0.0
    for b, p in enumerate(pairs):
        n = p['n']
        if n == 0:
            assert pair_ce[b] == 0.0
            continue
        s = c['scores'][b, :n, :n].double().numpy()
        bound = R.CE_BOUND * (np.abs(p['lse'])[:, None] + np.abs(s))
        err = np.abs(cost[b, :n, :n].double().numpy() - p['cost'])
        worst_cost = max(worst_cost, float((err / bound).max()))
        worst_ce = max(worst_ce, abs(pair_ce[b] - p['ce']) / (R.CE_BOUND * p['scale']))
        # the fold is the fp64 sum of the fp32 rows
        assert abs(pair_ce[b] - float(row_ce[b, :n].double().sum())) <= 1e-12 * p['scale']
    print('N %d B %d ragged %d labels %d: cost error / bound %.3f, pair CE error / bound %.3f' % (N, B, ragged, with_labels, worst_cost, worst_ce))
    assert worst_cost <= 1.0 and worst_ce <= 1.0, (worst_cost, worst_ce)
    # the solver on the new cost: SciPy's assignment on the stable pairs
    assign, correct = o['assign'].cpu().numpy(), o['correct'].cpu().tolist()
    for b, p in enumerate(pairs):
        if p['stable']:
            assert np.array_equal(assign[b, :p['n']], p['assign']), b
            assert correct[b] == p['lsap_labels' if with_labels else 'lsap'], b
        assert bool((assign[b, p['n']:] == -1).all())
    # the record: the pairs in pair order, one at a time
    rec = o['meter'].record()
    want = R.fold_record(pair_ce, nv.tolist(), correct, hits_ref, B)
    assert rec == want, (rec, want)
    return worst_cost, worst_ce


@pytest.mark.parametrize('B', R.BATCHES)
@pytest.mark.parametrize('N', R.SIZES)
def test_eval_pairs_and_fold(N, B):
    for ragged in (False, True):
        c = R.case(N, B, ragged)
        sd = c['scores'].to(DEV)
        nvd = c['nv'].to(DEV) if ragged else None
        for with_labels in (False, True):
            labd = c['labels'].to(DEV) if with_labels else None
            o = _launch(sd, nvd, labd, B, N)
            _check_against_reference(c, o, B, N, ragged, with_labels)
            assert o['pair_max'].cpu().tolist() == _accuracy_max(sd, nvd, labd, B, N)
            o2 = _launch(sd, nvd, labd, B, N)          # the same call twice: the same bits
            for k in ('cost', 'row_ce', 'row_hit', 'pair_ce', 'pair_max', 'correct', 'assign'):
                a, b = o[k], o2[k]
                assert torch.equal(torch.nan_to_num(a.double(), nan=-1e300), torch.nan_to_num(b.double(), nan=-1e300)), k
            assert torch.equal(o['meter'].buf, o2['meter'].buf)
    if N == R.SIZES[-1] and B == R.BATCHES[-1]:
        bad, tot = R.unstable_fraction()
        assert bad <= R.UNSTABLE_CAP * tot, (bad, tot)


@pytest.mark.parametrize('N', [5, 16, 17, 64, 65, 130])
def test_adversarial_rows_hold_the_argmax_rule(N):
    """duplicated maxima, NaN (first NaN wins), +inf, a row of -inf (column 0): np.argmax's order, and IEEE propagation into lse"""
    g = torch.Generator().manual_seed(N)
    B = 3
    nv = torch.tensor([N, N - 1, max(N - 3, 1)], dtype=torch.int32)
    s = torch.randint(-3, 4, (B, N, N), generator=g).float()          # small integers: every row has duplicated maxima
    for b in range(B):
        n = int(nv[b])
        s[b, 0, :] = float('-inf')
        s[b, 1 % n, n - 1] = NAN
        if n > 2:
            s[b, 2, n - 1] = NAN
            s[b, 2, n // 2] = NAN
            s[b, 2, 0] = float('inf')
        if n > 3:
            s[b, 3, n - 1] = float('inf')
            s[b, 3, n // 3] = float('inf')
        if n > 4:
            s[b, 4, :] = 2.0
    s = s.masked_fill(~R.corner(nv, N), NAN)
    lab = R.random_labels(nv, N, g)
    sd, nvd = s.to(DEV), nv.to(DEV)
    for labd, labh in ((None, None), (lab.to(DEV), lab)):
        o = _launch(sd, nvd, labd, B, N, hungarian=False)
        row_hit, cost, row_ce = o['row_hit'].cpu(), o['cost'].cpu(), o['row_ce'].cpu()
        for b in range(B):
            n = int(nv[b])
            blk = s[b, :n, :n].numpy()
            want = np.arange(n) if labh is None else labh[b, :n].numpy()
            assert np.array_equal(row_hit[b, :n].numpy(), (np.argmax(blk, 1) == want).astype(np.int32)), b
            ref = R.cost_corner(blk)
            got = cost[b, :n, :n].double().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref)), b
            fin = np.isfinite(ref)
            lse = R.lse_rows(blk)
            bound = R.CE_BOUND * (np.abs(lse)[:, None] + np.abs(blk.astype(np.float64)))
            assert bool((np.abs(got - ref)[fin] <= bound[fin]).all()), b
            assert np.array_equal(np.isnan(row_ce[b, :n].numpy()), np.isnan(lse - np.diagonal(blk)))
        assert o['pair_max'].cpu().tolist() == _accuracy_max(sd, nvd, labd, B, N)
        assert o['meter'].record()['correct_lsap'] == 0


def test_pair_alone_equals_pair_in_batch():
    N, B = 50, 32
    c = R.case(N, B, True)
    sd, nvd, labd = c['scores'].to(DEV), c['nv'].to(DEV), c['labels'].to(DEV)
    full = _launch(sd, nvd, labd, B, N)
    for b in (0, 3, 17, 31):
        one = _launch(sd[b:b + 1].contiguous(), nvd[b:b + 1].contiguous(), labd[b:b + 1].contiguous(), 1, N)
        for k in ('pair_ce', 'pair_max', 'correct'):
            assert torch.equal(one[k], full[k][b:b + 1]), (b, k)
        n = int(c['nv'][b])
        assert torch.equal(one['cost'][0, :n, :n], full['cost'][b, :n, :n]) and torch.equal(one['assign'][0], full['assign'][b])


FOLDED = ('ce_sum', 'nodes', 'correct_lsap', 'correct_max', 'pairs')


def test_live_masks_the_surplus_pairs():
    N, B = 17, 32
    c = R.case(N, B, True)
    sd, nvd = c['scores'].to(DEV), c['nv'].to(DEV)
    for live in (0, 1, 5, 31, 32):
        o = _launch(sd, nvd, None, B, N, live=live)
        rec = o['meter'].record()
        if live == 0:
            assert rec == R.fold_record([], [], [], [], 0) and not bool(o['meter'].buf.any())
            assert bool(torch.isnan(o['pair_ce']).all()) and bool((o['pair_max'] == SENTINEL).all())
            continue
        first = _launch(sd[:live].contiguous(), nvd[:live].contiguous(), None, live, N)
        assert rec == first['meter'].record() and rec['pairs'] == live and rec['steps'] == 1
        assert torch.equal(o['pair_ce'][:live], first['pair_ce']) and bool(torch.isnan(o['pair_ce'][live:]).all())
    # live = 0 on a record that holds something: nothing changes, the step count included
    before = o['meter'].buf.clone()
    _launch(sd, nvd, None, B, N, live=0, meter=o['meter'])
    assert torch.equal(o['meter'].buf, before)
    with pytest.raises(RuntimeError, match='fgnn_eval_fold'):
        _launch(sd, nvd, None, B, N, live=B + 1)


def test_meter_does_not_depend_on_how_the_examples_are_cut():
    """10 examples as 10 x 1, 2 x 5, 1 x 10 and 3 x 4 with a short last step filled with other pairs and masked by live"""
    N = 50
    c = R.case(N, 32, True)
    s, nv, lab = c['scores'][3:13], c['nv'][3:13], c['labels'][3:13]
    filler = (c['scores'][20:22], c['nv'][20:22], c['labels'][20:22])
    recs = []
    for B in (1, 5, 10, 4):
        meter = EvalMeter(DEV)
        for lo in range(0, 10, B):
            live = min(B, 10 - lo)
            parts = [(s[lo:lo + live], nv[lo:lo + live], lab[lo:lo + live])] + ([tuple(t[:B - live] for t in filler)] if live < B else [])
            sb, nb, lb = (torch.cat([p[k] for p in parts]).contiguous().to(DEV) for k in range(3))
            out = evaluate_scores(sb, nvalid=nb, labels=lb, meter=meter, live=live)
            assert out['meter'] is meter and out['assign'].shape == (B, N) and out['ce'].dtype == torch.float64
        recs.append(meter.record())
        assert recs[-1]['pairs'] == 10 and recs[-1]['steps'] == -(-10 // B)
    for r in recs[1:]:
        assert all(r[k] == recs[0][k] for k in FOLDED), (r, recs[0])
    ps = c['pairs'][3:13]
    assert recs[0]['nodes'] == sum(p['n'] for p in ps) and recs[0]['correct_max'] == sum(p['hits_labels'] for p in ps)
    if all(p['stable'] for p in ps):
        assert recs[0]['correct_lsap'] == sum(p['lsap_labels'] for p in ps)
    res = meter.result()
    assert res['loss'] == recs[-1]['ce_sum'] / recs[-1]['nodes'] and res['pairs'] == 10
    assert meter.loss.item() == res['loss'] and meter.acc.item() == res['acc'] and meter.acc_max.item() == res['acc_max']
    assert meter.allreduce_().record() == recs[-1]            # one rank: the sum over the ranks is the record
    assert not bool(meter.reset().buf.any())


def test_evaluate_scores_refuses_what_it_cannot_run():
    with pytest.raises(RuntimeError, match='at most'):
        evaluate_scores(torch.empty(1, _lib.FGNN_LSAP_MAX_N + 1, _lib.FGNN_LSAP_MAX_N + 1, device=DEV))
    s = torch.zeros(2, 4, 4, device=DEV)
    with pytest.raises(ValueError, match='live'):
        evaluate_scores(s, live=3)
    with pytest.raises(ValueError, match='nvalid'):
        evaluate_scores(s, nvalid=torch.zeros(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match='meter'):
        evaluate_scores(s, meter={})
    out = evaluate_scores(s, hungarian=False)
    assert out['assign'] is None and out['meter'].record()['correct_lsap'] == 0 and out['n'].tolist() == [4, 4]


# ---------------------------------------------------------------------------------------------------------- trainer
LAY = ParamLayout(2, 4, 32, 32, 3)
TB = 2


def _gen(N, seed=11):
    return PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.05, seed=seed, device=DEV)


def _state(tr):
    return [t.clone() for t in (tr.params, tr.grads, tr.opt.exp_avg, tr.opt.exp_avg_sq, tr.opt._dev_state()[1][0:1])]


def _host_check(scores, out, labels=None):
    """per-pair counts of an evaluation against the host reference on the scores it evaluated"""
    s = scores.cpu()
    for b in range(s.shape[0]):
        blk = s[b].numpy()
        lab = None if labels is None else labels[b].cpu().numpy()
        assert int(out['correct_max'][b]) == R.argmax_hits(blk, lab), b
        ok, assign = R.stable(blk)
        if ok:
            assert np.array_equal(out['assign'][b].cpu().numpy(), assign), b
            assert int(out['correct_lsap'][b]) == int(np.sum(assign == (np.arange(len(assign)) if lab is None else lab))), b
    return s


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('N', [16, 50])
def test_eval_step_leaves_the_training_state_alone(N, precision):
    gen = _gen(N)
    batches = [gen.bits(TB * k, TB)[:2] for k in range(3)]
    # (the 16-bit engine takes bit-packed input through the structured block 1 only; fp32 runs the generic kernels)
    kw = dict(lr=2e-3, precision=precision, block1='structured' if precision == 'bf16' else None)
    for capture in (False, True):
        a = FgnnTrainer(LAY, LAY.init_flat(5, DEV), capture=capture, **kw)
        b = FgnnTrainer(LAY, LAY.init_flat(5, DEV), capture=capture, **kw)
        a.train_step_bits(*batches[0])
        b.train_step_bits(*batches[0])
        before = _state(a)
        meter = EvalMeter(DEV)
        out = a.eval_step_bits(*batches[1], meter=meter)
        after = _state(a)
        assert all(torch.equal(x, y) for x, y in zip(before, after)) and a.opt.t == 1
        assert meter.record()['pairs'] == TB and meter.record()['nodes'] == TB * N
        _host_check(a._engine(2 * TB, N, False).scores, out)
        # the evaluated loss is the loss the training step reports for the same batch and parameters
        m2 = EvalMeter(DEV)
        out2 = a.eval_step_bits(*batches[2], meter=m2)
        s2 = _host_check(a._engine(2 * TB, N, False).scores.clone(), out2)
        loss_eval = m2.result()['loss']
        loss_train, _ = a.train_step_bits(*batches[2])
        b.train_step_bits(*batches[2])
        scale = sum(R.ce_scale(s2[k].numpy()) for k in range(TB))
        err = abs(loss_eval - loss_train.item()) * TB * N
        print('N %d %s capture %d: eval loss %.8f, train loss %.8f, error / bound %.3f' % (N, precision, capture, loss_eval,
                                                                                          loss_train.item(), err / (R.CE_BOUND * scale)))
        assert err <= R.CE_BOUND * scale
        # train, eval, eval, train == train, train
        assert torch.equal(a.params, b.params) and torch.equal(a.opt.exp_avg, b.opt.exp_avg) and a.opt.t == b.opt.t == 2


def test_eval_step_dense_and_labels():
    N = 16
    gen = _gen(N)
    tr = FgnnTrainer(LAY, LAY.init_flat(5, DEV))
    b1, b2, nv, labels = gen.bits(0, TB, permute=True)
    out = tr.eval_step_bits(b1, b2, labels=labels)
    s = _host_check(tr._engine(2 * TB, N, False).scores.clone(), out, labels)
    x1, x2, _ = gen.dense(0, TB, permute=True)
    out_d = tr.eval_step(x1['input'], x2['input'], labels=labels)
    _host_check(tr._engine(2 * TB, N, False).scores, out_d, labels)
    ce = out['ce'].cpu().numpy()
    for k in range(TB):         # the two input forms run the same function: equal to the CE bound
        assert abs(ce[k] - R.pair_ce(s[k].numpy())) <= R.CE_BOUND * R.ce_scale(s[k].numpy())
        assert abs(out_d['ce'][k].item() - ce[k]) <= 2 * R.CE_BOUND * R.ce_scale(s[k].numpy())


@pytest.mark.parametrize('permute', [False, True])
def test_evaluate_counts_every_example_once(permute):
    N, M, B = 16, 10, 4
    gen = _gen(N, seed=3)
    tr = FgnnTrainer(LAY, LAY.init_flat(7, DEV))
    before = _state(tr)
    rec = tr.evaluate(gen, EpochSampler(M, shuffle=False), B, permute=permute).record()
    assert rec['pairs'] == M and rec['steps'] == 3 and rec['nodes'] == M * N
    one = tr.evaluate(gen, EpochSampler(M, shuffle=False), 1, permute=permute).record()
    assert one['pairs'] == M and one['steps'] == M
    print('evaluate B = 4: %r\nevaluate B = 1: %r' % (rec, one))
    assert all(rec[k] == one[k] for k in FOLDED), (rec, one)          # ce_sum included, bit for bit
    # a shuffled order covers the same examples: the same counts, the CE sum in another order (ce_i <= |lse_i| + |s_ii|, so the CE
    # bound on a sum is at least CE_BOUND * ce_sum)
    shuf = tr.evaluate(gen, EpochSampler(M, shuffle=True, seed=5), B, epoch=2, permute=permute).record()
    assert all(shuf[k] == rec[k] for k in FOLDED[1:]) and abs(shuf['ce_sum'] - rec['ce_sum']) <= 2 * R.CE_BOUND * rec['ce_sum']
    # a meter of the caller's accumulates; nothing of the training state moved
    meter = EvalMeter(DEV)
    assert tr.evaluate(gen, EpochSampler(M, shuffle=False), B, meter=meter, permute=permute) is meter
    tr.evaluate(gen, EpochSampler(M, shuffle=False), B, meter=meter, hungarian=False, permute=permute)
    r2 = meter.record()
    assert r2['pairs'] == 2 * M and r2['correct_max'] == 2 * rec['correct_max'] and r2['correct_lsap'] == rec['correct_lsap']
    assert all(torch.equal(x, y) for x, y in zip(before, _state(tr)))


def test_fit_runs_epochs_and_steps_the_scheduler():
    N, B = 16, 4
    tr = FgnnTrainer(LAY, LAY.init_flat(7, DEV), lr=1e-3)
    hist = tr.fit(_gen(N, seed=1), EpochSampler(8, seed=1), _gen(N, seed=2), EpochSampler(6, shuffle=False), epochs=2, batch_size=B)
    assert [h['epoch'] for h in hist] == [0, 1] and all(h['train_losses'].shape == (2,) for h in hist)
    assert all(np.isfinite(h['val_loss']) and 0.0 <= h['val_acc'] <= 1.0 for h in hist) and hist[-1]['lr'] == tr.opt.lr == 1e-3
    assert tr.opt.t == 4


@pytest.mark.parametrize('eval_score', ['linear_assignment', 'max'])
def test_all_losses_acc_through_the_module(eval_score):
    N, B = 16, 3
    torch.manual_seed(3)
    ne = dict(type='node_embedding', block_init='block_emb', block_inside='block', num_blocks=2,
              in_features=32, out_features=32, depth_of_mlp=3)
    model = Siamese_Node_Exp(2, ne).to(DEV)
    gen = _gen(N, seed=9)
    batches = [gen.dense(B * k, B)[:2] for k in range(2)]
    losses, accs = all_losses_acc(batches, model, eval_score=eval_score)
    assert losses.shape == (2,) and accs.shape == (2 * B,) and losses.dtype == np.float64
    for k, (d1, d2) in enumerate(batches):
        with torch.no_grad():
            s = model(d1, d2).cpu()
        blocks = [s[b].numpy() for b in range(B)]
        ref = R.loss_of(blocks)
        assert abs(losses[k] - ref) * B * N <= R.CE_BOUND * sum(R.ce_scale(x) for x in blocks), (losses[k], ref)
        for b, blk in enumerate(blocks):
            if eval_score == 'max':
                assert accs[k * B + b] == R.argmax_hits(blk) / N
            else:
                ok, assign = R.stable(blk)
                if ok:
                    assert accs[k * B + b] == int(np.sum(assign == np.arange(N))) / N
    only_losses, none = all_losses_acc(batches, model, eval_score=None)
    assert np.array_equal(only_losses, losses) and none.shape == (0,)
    assert all(p.grad is None for p in model.parameters())
