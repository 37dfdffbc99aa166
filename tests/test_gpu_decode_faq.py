"""GPU: the faq= stage of the decode chain -- evaluation.decode_scores / evaluate_scores, the trainer's eval steps, evaluate,
noise_curve and fit, Siamese_Node_Exp.match -- against the same chain written out by hand from its public parts: metrics.lsap_device,
qap.sinkhorn, qap.faq, qap.objective_bits, qap.greedy_bits / qap.two_opt_bits and the fold entry point.  Everything compared is an
integer, a matrix one deterministic launch wrote, or a record of integers and fixed-order fp64 sums: tensors are compared with
torch.equal, meters as bytes.

Pairs: B = 4 planted (permute=True) Erdos-Renyi pairs with ragged vertex counts at N = 16 and N = 33; scores = 4 onehot(labels) +
standard normal noise from the device's Philox generator, so the start is informative."""
import pytest
import torch

from graph_neural_net_amd import _lib, qap
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.evaluation import BinnedEvalMeter, BinnedQapMeter, EvalMeter, QapMeter, decode_scores, evaluate_scores
from graph_neural_net_amd.metrics import lsap_device
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.sampler import EpochSampler
from graph_neural_net_amd.siamese import Siamese_Node_Exp
from graph_neural_net_amd.trainer import FgnnTrainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LAY = ParamLayout(2, 2, 32, 32, 3)
B = 4
FAQ_KEYS = ('faq_perm', 'faq_qap', 'faq_nit', 'faq_status', 'sinkhorn_err')


def _gen(N, seed=5, **kw):
    return PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.1, seed=seed, device=DEV, **kw)


def _pairs(N):
    b1, b2, nv, lab = _gen(N, vertex_proba=0.8).bits(0, B, permute=True)
    g = torch.Generator(device=DEV).manual_seed(100 + N)
    s = torch.randn(B, N, N, generator=g, device=DEV)
    s.scatter_add_(2, lab.long().clamp(0, N - 1)[:, :, None], torch.full((B, N, 1), 4.0, device=DEV))
    return s, b1, b2, nv.to(torch.int32), lab


def _fold(meter, assign, perm, refined, labels, q, planted, nv, live, bins=None):
    """fgnn_qap_fold(_bins) by hand -> (correct, refined_correct)"""
    n, N = assign.shape
    correct, rc = torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    ratio = torch.zeros(n, dtype=torch.float64, device=DEV)
    pairs = (_lib.ptr(assign), _lib.ptr(perm), _lib.ptr(labels), _lib.ptr(q), _lib.ptr(planted), _lib.ptr(refined), _lib.ptr(nv), n, N, live)
    outs = (_lib.ptr(correct), _lib.ptr(rc), _lib.ptr(ratio), _lib.ptr(meter.buf), _lib.stream_ptr())
    if bins is None:
        _lib.call('fgnn_qap_fold', *pairs, *outs)
    else:
        _lib.call('fgnn_qap_fold_bins', *pairs, _lib.ptr(bins), meter.K, *outs)
    return correct, rc


def _by_hand(s, b1, b2, nv, lab, faq_kw, refine, two_opt, assign=None):
    """The chain from its public parts -> (assign, q, planted, faq result, last perm, last refined)"""
    if assign is None:
        assign = lsap_device(s, nv, want_assign=True)[1]
    obj = qap.objective_bits(b1, b2, assign, nv, raw=True)
    planted = qap.objective_bits(b1, b2, lab, nv, raw=True)[0]
    sk = None
    if faq_kw.get('P0', 'scores') == 'scores':
        sk = qap.sinkhorn(s, nv, tau=faq_kw.get('tau', 1.0), iters=faq_kw.get('iters', 20))
    f = qap.faq(b1, b2, nvalid=nv, labels=lab, P0='barycenter' if sk is None else sk['P'], maxiter=faq_kw.get('maxiter', 30),
                tol=faq_kw.get('tol', 0.03))
    fq = qap.objective_bits(b1, b2, f['perm'], nv, raw=True)[0]
    failed = f['status'] == 2
    perm, refined = torch.where(failed[:, None], assign, f['perm']), torch.where(failed, obj[0], fq)
    if refine:
        g = qap.greedy_bits(b1, b2, perm, refine, nv, lab, raw=True)
        perm, refined = g['perm'], g['s_best2']
    if two_opt:
        t = qap.two_opt_bits(b1, b2, perm, nv, raw=True)
        perm, refined = t['perm'], t['qap']
    return assign, obj[0], planted, dict(f, raw_qap=fq, err=None if sk is None else sk['err']), perm, refined


@pytest.mark.parametrize('N', [16, 33])
@pytest.mark.parametrize('refine,two_opt', [(0, False), (2, False), (0, True)])
def test_the_stage_equals_the_chain_written_out(N, refine, two_opt):
    s, b1, b2, nv, lab = _pairs(N)
    live = 3
    meter = QapMeter(DEV)
    out = decode_scores(s, b1, b2, nvalid=nv, labels=lab, meter=meter, live=live, refine=refine, two_opt=two_opt, faq=True)
    assign, q, planted, f, perm, refined = _by_hand(s, b1, b2, nv, lab, {}, refine, two_opt)
    hand = QapMeter(DEV)
    correct, rc = _fold(hand, assign, perm, refined, lab, q, planted, nv, live)
    hand._mark_refined()
    assert torch.equal(out['assign'], assign) and torch.equal(out['qap'], q) and torch.equal(out['planted'], planted)
    assert torch.equal(out['faq_perm'], f['perm']) and torch.equal(out['faq_qap'], f['raw_qap'])
    assert torch.equal(out['faq_nit'].long(), f['nit']) and torch.equal(out['faq_status'].long(), f['status'])
    assert torch.equal(out['sinkhorn_err'], f['err'])
    assert torch.equal(out['perm'], perm) and torch.equal(out['refined'], refined)
    assert torch.equal(out['correct'], correct) and torch.equal(out['refined_correct'], rc)
    assert torch.equal(meter.buf, hand.buf) and meter.refined
    # the invariants of the stage's own matching
    status, fp, nvs = out['faq_status'].cpu().tolist(), out['faq_perm'].cpu(), nv.cpu().tolist()
    print('N %d: nvalid %r faq_status %r faq_nit %r faq_qap %r qap %r' % (N, nvs, status, out['faq_nit'].cpu().tolist(),
                                                                       out['faq_qap'].cpu().tolist(), q.cpu().tolist()))
    assert any(n > 1 for n in nvs[:live])
    for b, n in enumerate(nvs):
        if n > 0:
            assert status[b] != 2 and sorted(fp[b, :n].tolist()) == list(range(n)) and (fp[b, n:] == -1).all()
    assert torch.equal(out['faq_qap'].long(), qap.objective_bits(b1, b2, out['faq_perm'], nv)['qap'])
    # the final matching handed in as an assignment: its objective and its matches are the refined figures (qap's unit)
    if not refine:
        final = decode_scores(s, b1, b2, nvalid=nv, labels=lab, live=live, assign=out['perm'])
        assert torch.equal(final['qap'], out['refined']) and torch.equal(final['correct'], out['refined_correct'])
        rec, frec = meter.record(), final['meter'].record()
        assert rec['refined_sum'] == frec['qap_sum'] and rec['refined_correct'] == frec['correct']


@pytest.mark.parametrize('N', [16, 33])
def test_the_barycenter_start_and_options(N):
    s, b1, b2, nv, lab = _pairs(N)
    for kw in ({'P0': 'barycenter'}, {'P0': 'barycenter', 'maxiter': 4, 'tol': 1e-3}, {'tau': 0.5, 'iters': 7, 'maxiter': 9}):
        meter, hand = QapMeter(DEV), QapMeter(DEV)
        out = decode_scores(s, b1, b2, nvalid=nv, labels=lab, meter=meter, faq=kw)
        assign, q, planted, f, perm, refined = _by_hand(s, b1, b2, nv, lab, kw, 0, False)
        _fold(hand, assign, perm, refined, lab, q, planted, nv, B)
        assert torch.equal(out['faq_perm'], f['perm']) and torch.equal(out['faq_qap'], f['raw_qap'])
        assert torch.equal(out['faq_nit'].long(), f['nit']) and torch.equal(out['perm'], perm) and torch.equal(out['refined'], refined)
        assert (out['sinkhorn_err'] is None) == (kw.get('P0') == 'barycenter') and torch.equal(meter.buf, hand.buf)
    # the classical baseline: with the barycenter and an assignment handed in, the scores do not enter the stage's matching
    base = decode_scores(s, b1, b2, nvalid=nv, labels=lab, faq={'P0': 'barycenter'})
    other = decode_scores(torch.zeros_like(s), b1, b2, nvalid=nv, labels=lab, faq={'P0': 'barycenter'}, assign=base['assign'])
    assert torch.equal(other['faq_perm'], base['faq_perm']) and torch.equal(other['meter'].buf, base['meter'].buf)
    alone = qap.faq(b1, b2, nvalid=nv, labels=lab)
    assert torch.equal(base['faq_perm'], alone['perm']) and torch.equal(base['faq_qap'].long(), alone['qap'])


def test_fallbacks():
    N = 16
    s, b1, b2, nv, lab = _pairs(N)
    assert int(nv[1]) > 1
    # a corner that is all NaN: Sinkhorn hands the barycenter on, so FAQ still runs for the pair
    bad = s.clone()
    bad[1] = float('nan')
    assign = lsap_device(s, nv, want_assign=True)[1]
    out = decode_scores(bad, b1, b2, nvalid=nv, labels=lab, faq=True, assign=assign)
    sk = qap.sinkhorn(bad, nv)
    n1 = int(nv[1])
    assert sk['status'].cpu().tolist() == [0, 1, 0, 0] and bool((sk['P'][1, :n1, :n1] == 1.0 / n1).all()) and float(out['sinkhorn_err'][1]) == 0.0
    bary = qap.faq(b1, b2, nvalid=nv, labels=lab)
    assert int(out['faq_status'][1]) != 2 and int(out['faq_nit'][1]) >= 1 and torch.equal(out['faq_perm'][1], bary['perm'][1])
    clean = decode_scores(s, b1, b2, nvalid=nv, labels=lab, faq=True, assign=assign)
    for b in (0, 2, 3):
        assert torch.equal(out['faq_perm'][b], clean['faq_perm'][b]) and torch.equal(out['faq_qap'][b], clean['faq_qap'][b])
    # FAQ status 2 without a float in sight: a pair of no vertices; the stage keeps `assign` (no permutation here) and its
    # objective, and the fold counts the pair as it does without the stage
    nv0 = nv.clone()
    nv0[2] = 0
    junk = assign.clone()
    junk[2] = 5
    with_stage, without = QapMeter(DEV), QapMeter(DEV)
    out = decode_scores(s, b1, b2, nvalid=nv0, labels=lab, meter=with_stage, faq={'P0': 'barycenter'}, assign=junk)
    ref = decode_scores(s, b1, b2, nvalid=nv0, labels=lab, meter=without, assign=junk)
    assert out['faq_status'].cpu().tolist()[2] == 2 and int(out['faq_nit'][2]) == 0 and int(out['faq_status'][0]) != 2
    assert bool((out['faq_perm'][2] == -1).all())
    assert torch.equal(out['perm'][2], junk[2]) and torch.equal(out['refined'][2], ref['qap'][2])
    assert torch.equal(out['assign'], ref['assign']) and torch.equal(out['qap'], ref['qap']) and torch.equal(out['correct'], ref['correct'])
    a, b = with_stage.record(), without.record()
    same = ('ratio_sum', 'ratio_pairs', 'qap_sum', 'planted_sum', 'correct', 'recovered', 'exact', 'unmatched', 'nodes', 'pairs', 'steps')
    assert all(a[k] == b[k] for k in same) and a['refined'] and not b['refined']
    # ... and with the search after it
    chain = decode_scores(s, b1, b2, nvalid=nv0, labels=lab, faq={'P0': 'barycenter'}, assign=junk, two_opt=True)
    assert torch.equal(chain['faq_perm'], out['faq_perm']) and chain['status'].cpu().tolist()[2] == 0       # (no vertices: nothing to search)


def test_bins_defaults_and_evaluate_scores():
    N, K = 16, 2
    s, b1, b2, nv, lab = _pairs(N)
    bins = torch.tensor([1, 0, 1, 0], device=DEV)
    bm = BinnedQapMeter(DEV, K)
    out = decode_scores(s, b1, b2, nvalid=nv, labels=lab, meter=bm, bins=bins, faq=True, two_opt=True)
    for k in range(K):
        sel = [b for b in range(B) if int(bins[b]) == k]
        one = decode_scores(s[sel], b1[sel], b2[sel], nvalid=nv[sel], labels=lab[sel], faq=True, two_opt=True)
        assert torch.equal(one['meter'].buf, bm[k].buf), k
        assert torch.equal(one['faq_perm'], out['faq_perm'][sel]) and torch.equal(one['perm'], out['perm'][sel])
    assert bm.refined
    # without the keyword: today's tensors under today's keys, plus the new keys as None
    for kw in ({}, {'refine': 2}, {'two_opt': True}):
        m0, m1 = QapMeter(DEV), QapMeter(DEV)
        a = decode_scores(s, b1, b2, nvalid=nv, labels=lab, meter=m0, **kw)
        b = decode_scores(s, b1, b2, nvalid=nv, labels=lab, meter=m1, faq=None, **kw)
        assert set(a) == set(b) and torch.equal(m0.buf, m1.buf) and m0.refined == m1.refined
        for key in a:
            if key == 'meter' or a[key] is None:
                assert key == 'meter' or b[key] is None
            else:
                assert torch.equal(a[key], b[key]), key
        assert all(a[key] is None for key in FAQ_KEYS)
    ea, eb, qa, qb = EvalMeter(DEV), EvalMeter(DEV), QapMeter(DEV), QapMeter(DEV)
    a = evaluate_scores(s, nvalid=nv, labels=lab, meter=ea, qap_meter=qa, bits=(b1, b2))
    b = evaluate_scores(s, nvalid=nv, labels=lab, meter=eb, qap_meter=qb, bits=(b1, b2), faq=None)
    assert torch.equal(ea.buf, eb.buf) and torch.equal(qa.buf, qb.buf) and all(b['decode'][key] is None for key in FAQ_KEYS)
    assert all(torch.equal(a[key], b[key]) for key in ('ce', 'n', 'correct_max', 'correct_lsap', 'assign'))
    # with it: the EvalMeter keeps its bytes and the decode is decode_scores' on the solver's assignment
    ec, qc = EvalMeter(DEV), QapMeter(DEV)
    c = evaluate_scores(s, nvalid=nv, labels=lab, meter=ec, qap_meter=qc, bits=(b1, b2), faq=True, refine=1)
    alone = decode_scores(s, b1, b2, nvalid=nv, labels=lab, faq=True, refine=1)
    assert torch.equal(ec.buf, ea.buf) and torch.equal(qc.buf, alone['meter'].buf) and torch.equal(c['decode']['perm'], alone['perm'])
    with pytest.raises(ValueError, match='faq= belongs to a qap_meter'):
        evaluate_scores(s, nvalid=nv, faq=True)
    with pytest.raises(ValueError, match='unknown key'):
        evaluate_scores(s, nvalid=nv, qap_meter=QapMeter(DEV), bits=(b1, b2), faq={'P': 'scores'})
    em = BinnedEvalMeter(DEV, K)
    bq = BinnedQapMeter(DEV, K)
    evaluate_scores(s, nvalid=nv, labels=lab, meter=em, bins=bins, qap_meter=bq, bits=(b1, b2), faq=True, two_opt=True)
    assert torch.equal(bq.buf, bm.buf)


def _trainer(N):
    tr = FgnnTrainer(LAY, LAY.init_flat(7, DEV), lr=2e-3)
    tr.train_step_bits(*_gen(N).bits(0, B)[:2])
    return tr


def test_through_the_trainer_eager_and_captured(monkeypatch):
    N = 16
    tr = _trainer(N)
    b1, b2, nv, lab = _gen(N, seed=9).bits(0, B, permute=True)
    meter, qm = EvalMeter(DEV), QapMeter(DEV)
    out = tr.eval_step_bits(b1, b2, labels=lab, meter=meter, qap_meter=qm, faq=True)
    scores = tr._eval_forward(B, N, None, bits=torch.cat([b1, b2]).contiguous()).clone()
    em, dm = EvalMeter(DEV), QapMeter(DEV)
    ev = evaluate_scores(scores, labels=lab, meter=em)
    dec = decode_scores(scores, b1, b2, labels=lab, meter=dm, faq=True)
    assert torch.equal(meter.buf, em.buf) and torch.equal(qm.buf, dm.buf) and torch.equal(out['assign'], ev['assign'])
    for key in ('perm', 'refined', 'refined_correct') + FAQ_KEYS:
        assert torch.equal(out['decode'][key], dec[key]), key
    # the spectral twin takes the keyword as well
    sq = QapMeter(DEV)
    sp = tr.eval_step_spectral(b1, b2, n_powers=2, labels=lab, qap_meter=sq, faq={'P0': 'barycenter'})
    assert torch.equal(sp['decode']['faq_perm'], qap.faq(b1, b2, labels=lab)['perm']) and sq.refined
    # the launches: the default step is the one it was; the stage adds its own between the objective and the fold
    names = []
    real = _lib.call

    def recording(name, *args, **kw):
        names.append(name)
        return real(name, *args, **kw)
    monkeypatch.setattr(_lib, 'call', recording)
    runs = []
    for kw in ({}, {'faq': None}, {'faq': True}, {'faq': {'P0': 'barycenter', 'maxiter': 2}}):
        del names[:]
        tr.eval_step_bits(b1, b2, qap_meter=QapMeter(DEV), **kw)
        runs.append(list(names))
    monkeypatch.setattr(_lib, 'call', real)
    assert runs[0] == runs[1] and not any(n in ('fgnn_sinkhorn', 'fgnn_qapw_faq') for n in runs[0])
    assert runs[2] == runs[0][:-1] + ['fgnn_sinkhorn', 'fgnn_expand_adjacency', 'fgnn_expand_adjacency', 'fgnn_qapw_faq',
                                      'fgnn_qap_objective', 'fgnn_qap_fold']
    assert runs[3] == runs[0][:-1] + ['fgnn_expand_adjacency', 'fgnn_expand_adjacency', 'fgnn_qapw_faq', 'fgnn_qap_objective', 'fgnn_qap_fold']
    with pytest.raises(ValueError, match='faq'):
        tr.eval_step_bits(b1, b2, faq=True)
    # captured: no host read and no allocation the replay could miss -- the replayed chain writes the eager chain's bytes
    gm, gq = EvalMeter(DEV), QapMeter(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tr.eval_step_bits(b1, b2, labels=lab, meter=gm, qap_meter=gq, faq=True, two_opt=True)      # warm-up: every engine buffer exists
    torch.cuda.current_stream().wait_stream(side)
    eager_e, eager_q = gm.buf.clone(), gq.buf.clone()
    gm.reset(), gq.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = tr.eval_step_bits(b1, b2, labels=lab, meter=gm, qap_meter=gq, faq=True, two_opt=True)
    gm.reset(), gq.reset()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gm.buf, eager_e) and torch.equal(gq.buf, eager_q)
    ref = decode_scores(scores, b1, b2, labels=lab, faq=True, two_opt=True)
    assert torch.equal(cap['decode']['perm'], ref['perm']) and torch.equal(cap['decode']['faq_perm'], ref['faq_perm'])


def test_evaluate_noise_curve_and_fit_take_the_keyword():
    N, TB = 16, 2
    tr, gen = _trainer(N), _gen(N, seed=3)
    sampler = EpochSampler(4, shuffle=False)
    qm, hand = QapMeter(DEV), QapMeter(DEV)
    tr.evaluate(gen, sampler, TB, permute=True, qap_meter=qm, faq=True)
    for step in range(2):
        b1, b2, nv, lab = gen.bits(index=sampler.batch_index(0, step, TB), permute=True)
        tr.eval_step_bits(b1, b2, nvalid=nv, labels=lab, qap_meter=hand, faq=True)
    assert torch.equal(qm.buf, hand.buf) and qm.refined and qm.record()['pairs'] == 4
    with pytest.raises(ValueError, match='faq'):
        tr.evaluate(gen, sampler, TB, faq=True)
    noises = (0.0, 0.3)
    bq = BinnedQapMeter(DEV, 2, values=noises)
    tr.noise_curve(gen, noises, 2, TB, permute=True, qap_meter=bq, faq={'P0': 'barycenter'})
    assert bq.refined and all('refined_qap_ratio' in r and r['pairs'] == 2 for r in bq.result())
    # fit: one epoch of two steps
    a, b = (FgnnTrainer(LAY, LAY.init_flat(7, DEV), lr=1e-3) for _ in range(2))
    val = EpochSampler(4, shuffle=False)
    hist = a.fit(gen, EpochSampler(4, seed=1), gen, val, epochs=1, batch_size=TB, decode_refine=0, decode_faq=True)
    plain = b.fit(gen, EpochSampler(4, seed=1), gen, val, epochs=1, batch_size=TB, decode_refine=0)
    assert set(hist[0]) == set(plain[0]) | {'val_refined_acc', 'val_refined_qap_ratio'}
    assert all(hist[0][k] == plain[0][k] for k in ('val_loss', 'val_acc', 'val_qap_ratio', 'val_recovered'))
    again = QapMeter(DEV)
    a.evaluate(gen, val, TB, qap_meter=again, faq=True)
    res = again.result()
    assert hist[0]['val_refined_acc'] == res['refined_acc'] and hist[0]['val_refined_qap_ratio'] == res['refined_qap_ratio']
    with pytest.raises(ValueError, match='decode_faq'):
        a.fit(gen, EpochSampler(4, seed=1), gen, val, epochs=1, batch_size=TB, decode_faq=True)


def test_match_runs_the_stage_on_zero_one_batches():
    from graph_neural_net_amd import synthetic
    torch.manual_seed(3)
    ne = dict(type='node_embedding', block_init='block_emb', block_inside='block', num_blocks=2, in_features=32, out_features=32,
              depth_of_mlp=3)
    model = Siamese_Node_Exp(2, ne).to(DEV)
    x1, x2 = (x.to(DEV) for x in synthetic.make_batch(11, 4, 20, 'ErdosRenyi', 0.2, 0.1))
    base = model.match(x1, x2)
    out = model.match(x1, x2, faq=True, two_opt=True)
    sk = qap.sinkhorn(base['scores'])
    f = qap.faq(x1, x2, P0=sk['P'])
    t = qap.two_opt(x1, x2, f['perm'])
    assert all(torch.equal(out[k], base[k]) for k in base)
    assert torch.equal(out['faq_perm'], f['perm']) and torch.equal(out['qap_faq'], f['qap']) and torch.equal(out['acc_faq'], f['acc'])
    assert torch.equal(out['sinkhorn_err'], sk['err']) and torch.equal(out['perm'], t['perm']) and torch.equal(out['qap_2opt'], t['qap'])
    with pytest.raises(NotImplementedError, match='faq'):
        model.match(x1, x2, weighted=True, faq=True)
