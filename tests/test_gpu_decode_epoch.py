"""GPU: decode epochs -- evaluation.decode_scores / QapMeter / BinnedQapMeter / evaluate_scores(qap_meter=) and the trainer's
qap_meter= / refine= / decode_refine= -- against the host route of qap.py (the project's restatement of the reference loop of
toolbox/metrics.py:168-223), the reference's recorded results (tests/golden/qap_decode.npz) and the fold of tests/qap_fold_ref.py.

Everything compared is an integer or a chain of correctly rounded fp64 operations in a fixed order, so records are compared as
bytes.  `steps` counts fold calls, the one field that depends on how an epoch was cut: where two cuttings are compared that word
is masked and asserted separately.

The model is the smallest the fused engine runs: 2 blocks of 32 features (ParamLayout refuses other widths), N = 12."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import qap_fold_ref as QR
import qap_ref
from graph_neural_net_amd import _lib, qap
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.evaluation import (BinnedEvalMeter, BinnedQapMeter, EvalMeter, QapMeter, decode_scores, evaluate_scores,
                                             qap_result)
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.pairstore import PairStore
from graph_neural_net_amd.sampler import EpochSampler
from graph_neural_net_amd.trainer import FgnnTrainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LAY = ParamLayout(2, 2, 32, 32, 3)
N, M, TB = 12, 10, 4
REC = QR.REC
STEPS = _lib.QapRecord.steps.offset


def _gen(seed=11, noise=0.05, **kw):
    return PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=noise, seed=seed, device=DEV, **kw)


def _trained():
    tr = FgnnTrainer(LAY, LAY.init_flat(7, DEV), lr=2e-3)
    tr.train_step_bits(*_gen().bits(0, 4)[:2])
    return tr


def _state(tr):
    return [t.clone() for t in (tr.params, tr.grads, tr.opt.exp_avg, tr.opt.exp_avg_sq)]


def _but_steps(buf):
    out = buf.clone().view(-1, REC)
    out[:, STEPS:STEPS + 8] = 0
    return out


def _bytes(recs):
    return torch.from_numpy(QR.to_bytes(recs)).to(DEV)


# ---------------------------------------------------------------------------------------------------------- decode_scores
@pytest.mark.parametrize('permute', [False, True])
@pytest.mark.parametrize('T', [0, 3])
def test_decode_scores_equals_the_host_route(permute, T):
    """scores with a signal on the true match and continuous noise (no ties): the device chain and the host loop find the same
    matchings, so every sum is the host's, pair by pair"""
    B, live = 6, 5
    b1, b2, nv, *lab = _gen(seed=5, noise=0.15, vertex_proba=0.8).bits(0, B, permute=permute)
    lab = lab[0] if lab else None
    assert nv is not None and (lab is None) != permute
    g = torch.Generator().manual_seed(17 + T)
    s = 1.5 * torch.randn(B, N, N, generator=g)
    target = lab.cpu().long() if permute else torch.arange(N).expand(B, N)
    s.scatter_add_(2, target.clamp(0, N - 1)[:, :, None], torch.full((B, N, 1), 2.0))
    meter = QapMeter(DEV)
    out = decode_scores(s.to(DEV), b1, b2, nvalid=nv, labels=lab, meter=meter, live=live, refine=T)
    assert out['meter'] is meter and meter.refined == (T > 0)
    # the host route, pair by pair
    acc, q, planted = qap._all_acc_qap_host(s, b1, b2, nv, lab)
    sizes = nv.cpu().tolist()
    assign = np.full((B, N), -1, dtype=np.int32)
    for b, n in enumerate(sizes):
        assign[b, :n] = linear_sum_assignment(-torch.log_softmax(s[b, :n, :n], -1).numpy())[1]
    perm = refined = None
    if T:
        gr = qap._greedy_host(b1, b2, torch.from_numpy(assign), T, nv, lab)
        perm, refined = gr['perm'].numpy(), (2 * gr['s_best']).to(torch.int64).numpy()
    labn = None if lab is None else lab.cpu().numpy()
    want, wc, wr, wq = QR.fold(assign, perm, labn, q.numpy(), planted.numpy(), refined, sizes, live)
    assert wc[:live].tolist() == acc[:live].tolist()                    # (the restatement counts what the host loop counts)
    print('permute %d T %d: %r' % (permute, T, want[0]))
    assert torch.equal(out['assign'].cpu(), torch.from_numpy(assign))
    assert torch.equal(meter.buf, _bytes(want)), (meter.record(), want)
    assert out['qap'].cpu().tolist() == q.tolist() and out['planted'].cpu().tolist() == planted.tolist()
    assert out['correct'].cpu().tolist() == wc.tolist() and np.array_equal(out['ratio'].cpu().numpy(), wq)
    if T:
        assert torch.equal(out['perm'].cpu(), gr['perm']) and out['refined'].cpu().tolist() == refined.tolist()
        assert out['refined_correct'].cpu().tolist() == wr.tolist()
        assert want[0]['refined_sum'] >= want[0]['qap_sum']            # greedy_qap never keeps a worse matching
    else:
        assert out['perm'] is None and out['refined'] is None and out['refined_correct'] is None
    # the figures, on the host and on the device
    res, rec = meter.result(), meter.record()
    assert res == qap_result(rec) and res['pairs'] == live and res['unmatched'] == 0
    assert res['acc'] == meter.acc.item() and res['qap_ratio'] == meter.qap_ratio.item() and res['mean_ratio'] == meter.mean_ratio.item()
    assert ('refined_acc' in res) == (T > 0)
    if T:
        assert res['refined_acc'] == meter.refined_acc.item() and res['refined_qap_ratio'] == meter.refined_qap_ratio.item()
    # an assignment handed in: the same record without the solver
    again = QapMeter(DEV)
    decode_scores(s.to(DEV), b1, b2, nvalid=nv, labels=lab, meter=again, live=live, refine=T, assign=out['assign'])
    assert torch.equal(again.buf, meter.buf)
    assert not bool(meter.reset().buf.any()) and not meter.refined


@pytest.mark.parametrize('group', ['er50', 'ragged120'])
def test_meter_equals_the_sums_of_the_reference_fixture(group):
    g = qap_ref.fixture_groups()[group]
    s = torch.from_numpy(g['scores']).to(DEV)
    b1, b2 = (torch.from_numpy(g[k].view(np.int32)).to(DEV) for k in ('bits1', 'bits2'))
    nv = torch.from_numpy(g['nvalid']).to(DEV)
    out = decode_scores(s, b1, b2, nvalid=nv, refine=10)
    rec = out['meter'].record()
    assert torch.equal(out['assign'].cpu(), torch.from_numpy(g['assign0']))
    assert rec['qap_sum'] == int(g['qap'].sum()) and rec['planted_sum'] == int(g['planted'].sum()) and rec['correct'] == int(g['acc'].sum())
    assert rec['nodes'] == int(g['nvalid'].sum()) and rec['pairs'] == len(g['qap']) and rec['unmatched'] == 0
    assert rec['recovered'] == int((g['qap'] >= g['planted']).sum())
    # symmetric pairs: 2 s_best of the reference is the qap of the refined matching
    assert rec['refined_sum'] == int((2 * g['T10/s_best']).sum()) and rec['improved'] == int((2 * g['T10/s_best'] > g['qap']).sum())
    ratio = 0.0
    for q, p in zip(g['qap'].tolist(), g['planted'].tolist()):
        ratio += q / p
    assert rec['ratio_sum'] == ratio and rec['ratio_pairs'] == len(g['qap'])


def test_evaluate_scores_with_a_qap_meter_changes_nothing_else():
    B, K = 5, 3
    b1, b2, nv, lab = _gen(seed=6, vertex_proba=0.8).bits(0, B, permute=True)
    s = torch.randn(B, N, N, generator=torch.Generator().manual_seed(2)).to(DEV)
    for kw in ({}, {'labels': lab}, {'labels': lab, 'loss_on_labels': True, 'live': 3}):
        plain, with_decode, qm = EvalMeter(DEV), EvalMeter(DEV), QapMeter(DEV)
        a = evaluate_scores(s, nvalid=nv, meter=plain, **kw)
        b = evaluate_scores(s, nvalid=nv, meter=with_decode, qap_meter=qm, bits=(b1, b2), refine=2, **kw)
        assert torch.equal(plain.buf, with_decode.buf) and set(b) == set(a) | {'decode'} and b['decode']['meter'] is qm
        for key in ('ce', 'n', 'correct_max', 'correct_lsap', 'assign'):
            assert torch.equal(a[key], b[key]), key
        live = kw.get('live', B)
        assert torch.equal(b['decode']['correct'][:live], b['correct_lsap'][:live]) and b['decode']['assign'] is b['assign']
        assert qm.record()['correct'] == with_decode.record()['correct_lsap']
        alone = decode_scores(s, b1, b2, nvalid=nv, labels=kw.get('labels'), live=kw.get('live'), refine=2, assign=b['assign'])
        assert torch.equal(alone['meter'].buf, qm.buf)
    # bins: every record has the bytes of the plain chain on its pairs alone
    bins = torch.tensor([2, 0, 2, 5, 0], device=DEV)
    bm = BinnedQapMeter(DEV, K, values=(0.0, 0.1, 0.2))
    out = evaluate_scores(s, nvalid=nv, labels=lab, meter=BinnedEvalMeter(DEV, K), bins=bins, qap_meter=bm, bits=(b1, b2))
    for k in range(K):
        sel = [b for b in range(B) if int(bins[b]) == k]
        if not sel:
            assert not bool(bm[k].buf.any())
            continue
        one = decode_scores(s[sel], b1[sel], b2[sel], nvalid=nv[sel], labels=lab[sel], assign=out['assign'][sel])
        assert torch.equal(one['meter'].buf, bm[k].buf), k
    assert [r['noise'] for r in bm.result()] == [0.0, 0.1, 0.2] and [r['pairs'] for r in bm.record()] == [2, 0, 2]
    with pytest.raises(ValueError, match='qap meter'):
        evaluate_scores(s, qap_meter=EvalMeter(DEV), bits=(b1, b2))
    with pytest.raises(ValueError, match='go together'):
        evaluate_scores(s, qap_meter=bm, bits=(b1, b2))
    with pytest.raises(ValueError, match='records'):
        evaluate_scores(s, meter=BinnedEvalMeter(DEV, 2), bins=bins, qap_meter=bm, bits=(b1, b2))
    with pytest.raises(ValueError, match='bit words'):
        evaluate_scores(s, qap_meter=QapMeter(DEV), bits=(b1, b2[:, :, :0]))
    with pytest.raises(ValueError, match='bits='):
        evaluate_scores(s, qap_meter=QapMeter(DEV))


# ---------------------------------------------------------------------------------------------------------- the trainer
@pytest.mark.parametrize('permute,refine', [(False, 0), (True, 2)])
def test_evaluate_with_a_qap_meter_counts_every_example_once(permute, refine):
    """10 examples in batches of 4: the short last step has 2 live pairs"""
    tr, gen = _trained(), _gen(seed=3)
    before = _state(tr)
    meter, qm = EvalMeter(DEV), QapMeter(DEV)
    sampler = EpochSampler(M, shuffle=False)
    assert tr.evaluate(gen, sampler, TB, permute=permute, meter=meter, qap_meter=qm, refine=refine) is meter
    rec, ev = qm.record(), meter.record()
    print('evaluate permute %d refine %d: %r' % (permute, refine, rec))
    assert rec['pairs'] == M and rec['steps'] == 3 and rec['nodes'] == M * N and rec['refined'] == (refine > 0)
    assert rec['correct'] == ev['correct_lsap'] and rec['unmatched'] == 0 and rec['ratio_pairs'] == M
    # one example per step: the same record apart from its step count
    one = QapMeter(DEV)
    tr.evaluate(gen, sampler, 1, permute=permute, qap_meter=one, refine=refine)
    assert torch.equal(_but_steps(one.buf), _but_steps(qm.buf)) and one.record()['steps'] == M
    # the EvalMeter has the bytes it has without a qap_meter
    assert torch.equal(tr.evaluate(gen, sampler, TB, permute=permute).buf, meter.buf)
    # the same over a store of the generator's parents
    whole = gen.bits(0, M)
    store = PairStore.from_bits(whole[0], sizes=whole[2], noise_model=gen.noise_model, noise=gen.noise, seed=gen.seed,
                                edge_density=gen.edge_density)
    sm, sq = EvalMeter(DEV), QapMeter(DEV)
    tr.evaluate(store, sampler, TB, permute=permute, meter=sm, qap_meter=sq, refine=refine)
    assert torch.equal(sq.buf, qm.buf) and torch.equal(sm.buf, meter.buf)
    assert all(torch.equal(x, y) for x, y in zip(before, _state(tr))) and tr.opt.t == 1
    with pytest.raises(ValueError, match='qap_meter'):
        tr.evaluate(gen, sampler, TB, qap_meter=BinnedQapMeter(DEV, 2))
    with pytest.raises(ValueError, match='hungarian=True'):
        tr.evaluate(gen, sampler, TB, hungarian=False, qap_meter=QapMeter(DEV))
    with pytest.raises(ValueError, match='refine'):
        tr.evaluate(gen, sampler, TB, refine=2)


def test_noise_curve_with_a_binned_qap_meter_equals_separate_epochs():
    noises, per_level = (0.0, 0.2, 0.5), 6
    tr, gen = _trained(), _gen()
    qm = BinnedQapMeter(DEV, len(noises), values=noises)
    meter = tr.noise_curve(gen, noises, per_level, TB, qap_meter=qm, refine=1)
    assert torch.equal(meter.buf, tr.noise_curve(gen, noises, per_level, TB).buf)
    recs = qm.record()
    for j, v in enumerate(noises):
        one = QapMeter(DEV)
        tr.evaluate(_gen(noise=v), EpochSampler(per_level, shuffle=False), TB, qap_meter=one, refine=1)
        want = one.record()
        print('level %d: curve %r\n         epoch %r' % (j, recs[j], want))
        assert recs[j] == dict(want, noise=v, steps=recs[j]['steps']) and recs[j]['pairs'] == per_level
        assert torch.equal(_but_steps(qm[j].buf), _but_steps(one.buf))
    res = qm.result()
    assert [r['noise'] for r in res] == list(noises) and all('refined_acc' in r for r in res)
    with pytest.raises(ValueError, match='qap_meter'):
        tr.noise_curve(gen, noises, per_level, TB, qap_meter=QapMeter(DEV))
    with pytest.raises(ValueError, match='qap_meter'):
        tr.noise_curve(gen, noises, per_level, TB, qap_meter=BinnedQapMeter(DEV, 2))


def test_fit_reports_the_decode_figures_when_asked():
    old_keys = {'epoch', 'train_losses', 'val_loss', 'val_acc', 'val_acc_max', 'lr'}
    hists = []
    for kw in ({}, {'decode_refine': 0}, {'decode_refine': 2, 'rank_ks': (1, 5)}):
        tr = FgnnTrainer(LAY, LAY.init_flat(7, DEV), lr=1e-3)
        hists.append(tr.fit(_gen(seed=1), EpochSampler(8, seed=1), _gen(seed=2), EpochSampler(6, shuffle=False), epochs=1,
                            batch_size=TB, **kw))
    plain, decoded, both = hists
    new = {'val_qap_ratio', 'val_recovered'}
    assert set(plain[0]) == old_keys and set(decoded[0]) == old_keys | new
    assert set(both[0]) == old_keys | new | {'val_refined_acc', 'val_hits', 'val_mrr'}
    for h in (decoded[0], both[0]):
        assert all(h[k] == plain[0][k] for k in ('epoch', 'val_loss', 'val_acc', 'val_acc_max', 'lr'))
        assert torch.equal(h['train_losses'], plain[0]['train_losses'])
        assert h['val_qap_ratio'] > 0.0 and 0.0 <= h['val_recovered'] <= 1.0
    assert decoded[0]['val_qap_ratio'] == both[0]['val_qap_ratio'] and 0.0 <= both[0]['val_refined_acc'] <= 1.0


def test_the_default_step_issues_the_launches_it_issued(monkeypatch):
    tr = _trained()
    b1, b2 = _gen().bits(0, TB)[:2]
    names = []
    real = _lib.call

    def recording(name, *args, **kw):
        names.append(name)
        return real(name, *args, **kw)
    monkeypatch.setattr(_lib, 'call', recording)
    out = tr.eval_step_bits(b1, b2)
    default = list(names)
    assert default and default[-3:] == ['fgnn_eval_pairs', 'fgnn_lsap_accuracy', 'fgnn_eval_fold']
    assert not any(n.startswith(('fgnn_qap_', 'fgnn_greedy_')) for n in default) and 'decode' not in out
    del names[:]
    out = tr.eval_step_bits(b1, b2, qap_meter=QapMeter(DEV))
    assert names[:len(default)] == default and names[len(default):] == ['fgnn_qap_objective', 'fgnn_qap_fold']
    assert names.count('fgnn_lsap_accuracy') == 1 and out['decode']['perm'] is None
    del names[:]
    tr.eval_step_bits(b1, b2, qap_meter=QapMeter(DEV), refine=1)
    assert names.count('fgnn_greedy_qap') == 1 and names[-1] == 'fgnn_qap_fold' and names[:len(default)] == default
