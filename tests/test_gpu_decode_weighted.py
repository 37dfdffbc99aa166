"""GPU: the decode chain on real-weighted pairs -- evaluation.decode_scores_weighted, Siamese_Node_Exp.match_weighted and the
WeightedQapMeter -- against (1) the same chain written out by hand from the stand-alone functions (metrics.lsap_device,
qap.objective_weighted, qap.sinkhorn, qap.faq(weighted=True), qap.greedy_weighted, qap.two_opt_weighted and the fold entry point),
torch.equal on every key, and (2) the bit-word path: on 0/1 generator pairs handed over as float every fp32 product and sum is
exact, so every matching and every integer of the meter must be what decode_scores gives on the bit words of the same pairs, and
the fp64 sums must equal its int64 sums exactly.

Pairs: B = 5 spectral pairs (PairGenerator.spectral, L = D^-1/2 W D^-1/2 in channel 0) at N = 20 and 50 through a model of 2 blocks;
for the cross-check B = 5 planted 0/1 pairs with ragged vertex counts and informative random scores."""
import numpy as np
import pytest
import torch

from graph_neural_net_amd import _lib, qap
from graph_neural_net_amd.evaluation import (BinnedWeightedQapMeter, QapMeter, SeedMeter, WeightedQapMeter, decode_scores,
                                             decode_scores_weighted)
from graph_neural_net_amd.metrics import count_matches, lsap_device
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.siamese import Siamese_Node_Exp

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B = 5
INT_FIELDS = ('ratio_pairs', 'correct', 'refined_correct', 'recovered', 'exact', 'improved', 'unmatched', 'nodes', 'pairs', 'steps')


def _gen(N, seed=5, **kw):
    return PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.1, seed=seed, device=DEV, **kw)


_CACHE = {}


def _spectral(N):
    """-> (model, x1, x2, scores): one forward per N, shared by the tests and left unchanged"""
    if N not in _CACHE:
        torch.manual_seed(5)
        ne = dict(type='node_embedding', block_init='block_emb', block_inside='block', num_blocks=2, in_features=32, out_features=32,
                  depth_of_mlp=3)
        model = Siamese_Node_Exp(4, ne).to(DEV)
        x1, x2 = (d['input'] for d in _gen(N, seed=3).spectral(0, B))
        with torch.no_grad():
            s = model(x1, x2).detach().float().contiguous()
        _CACHE[N] = (model, x1, x2, s)
    return _CACHE[N]


def _identity_seeds(N, every=4):
    sd = torch.full((B, N), -1, dtype=torch.int32, device=DEV)
    sd[:, ::every] = torch.arange(0, N, every, dtype=torch.int32, device=DEV)
    return sd


def _fold(meter, assign, perm, refined, labels, q, planted, nv, live, bins=None):
    n, N = assign.shape
    correct, rc = torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    ratio = torch.zeros(n, dtype=torch.float64, device=DEV)
    pairs = (_lib.ptr(assign), _lib.ptr(perm), _lib.ptr(labels), _lib.ptr(q), _lib.ptr(planted), _lib.ptr(refined), _lib.ptr(nv), n, N, live)
    outs = (_lib.ptr(correct), _lib.ptr(rc), _lib.ptr(ratio), _lib.ptr(meter.buf), _lib.stream_ptr())
    if bins is None:
        _lib.call('fgnn_qapw_fold', *pairs, *outs)
    else:
        _lib.call('fgnn_qapw_fold_bins', *pairs, _lib.ptr(bins), meter.K, *outs)
    return correct, rc, ratio


def _by_hand(s, x1, x2, nv, lab, faq, refine, two_opt, seeds=None):
    """The chain from the stand-alone functions -> dict"""
    assign = lsap_device(s, nv, want_assign=True)[1]
    obj = qap.objective_weighted(x1, x2, assign, nv)
    h = {'assign': assign, 'qap': obj['qap'],
         'planted': obj['planted'] if lab is None else qap.objective_weighted(x1, x2, lab, nv)['qap'], 'perm': None, 'refined': None}
    if faq is not None:
        kw = {} if faq is True else faq
        if isinstance(seeds, str):
            seeds = qap.confident_seeds(s, nv)['seeds']
        P0 = 'barycenter'
        if kw.get('P0', 'scores') == 'scores':
            if seeds is None:
                sk = qap.sinkhorn(s, nv)
                P0 = sk['P']
            else:       # Sinkhorn on the free block; qap.faq gathers a full-size P0's free block itself, so embed it back
                ix = qap.seed_index_device(seeds, nv)
                u = torch.where(ix['valid'] != 0, ix['nfree'], torch.zeros_like(ix['nfree']))
                sk = qap.sinkhorn(qap.seed_gather_device(s, ix['free_a'], ix['free_b'], u), u)
                P0 = None
            h['sinkhorn_err'] = sk['err']
        R = kw.get('restarts', 1)
        if P0 is None:  # the seeded start in free coordinates has no public spelling in qap.faq: the raw chain, as the stage runs it
            f = qap.faq_weighted(x1, x2, nv, sk['P'], None, 30, 0.03, seeds=seeds, p0_free=True)
            f = {'perm': f['perm'], 'nit': f['nit'].long(), 'status': f['status'].long(), 'seeded': f['seeded']}
        else:
            f = qap.faq(x1, x2, nvalid=nv, labels=lab, P0=P0, weighted=True, seeds=seeds, restarts=R, seed=kw.get('seed', 0),
                        polish=kw.get('polish', False) and seeds is None)
        fq = qap.objective_weighted(x1, x2, f['perm'], nv)['qap']
        failed = f['status'] == 2
        h.update(faq_perm=f['perm'], faq_qap=fq, faq_nit=f['nit'], faq_status=f['status'], faq_restart=f.get('restart'),
                 perm=torch.where(failed[:, None], assign, f['perm']), refined=torch.where(failed, obj['qap'], fq), seeds=seeds)
        h['stage_perm'] = h['perm']
    if refine:
        g = qap.greedy_weighted(x1, x2, assign if h['perm'] is None else h['perm'], refine, nv, lab)
        h.update(perm=g['perm'], refined=g['s_best'] * 2, greedy=g)
    if two_opt:
        t = qap.two_opt_weighted_seeded(x1, x2, assign if h['perm'] is None else h['perm'], seeds, nvalid=nv, labels=lab)
        h.update(perm=t['perm'], refined=qap.objective_weighted(x1, x2, t['perm'], nv)['qap'], swaps=t['swaps'], nit=t['nit'],
                 status=t['status'], two_opt=t)
    return h


STAGES = [dict(), dict(refine=2), dict(two_opt=True), dict(faq=True), dict(faq={'P0': 'barycenter'}, two_opt=True),
          dict(faq=True, refine=2, two_opt=True), dict(faq={'restarts': 3, 'seed': 7}), dict(faq={'restarts': 3, 'polish': True}),
          dict(faq={'restarts': 1, 'polish': True}, two_opt=True)]


@pytest.mark.parametrize('N', [20, 50])
@pytest.mark.parametrize('stages', STAGES, ids=['plain', 'refine', 'two_opt', 'faq', 'barycenter+two_opt', 'all', 'restarts', 'restarts+polish',
                                                'polish+two_opt'])
def test_the_chain_equals_the_stand_alone_functions(N, stages):
    model, x1, x2, s = _spectral(N)
    faq, refine, two_opt = stages.get('faq'), stages.get('refine', 0), stages.get('two_opt', False)
    live = 4
    meter = WeightedQapMeter(DEV)
    out = decode_scores_weighted(s, x1, x2, meter=meter, live=live, refine=refine, two_opt=two_opt, faq=faq)
    h = _by_hand(s, x1, x2, None, None, faq, refine, two_opt)
    for k in ('assign', 'qap', 'planted'):
        assert torch.equal(out[k], h[k]), k
    assert out['qap'].dtype == out['planted'].dtype == torch.float32
    if faq is not None:
        assert torch.equal(out['faq_perm'], h['faq_perm']) and torch.equal(out['faq_qap'], h['faq_qap']) and out['faq_qap'].dtype == torch.float32
        assert torch.equal(out['faq_nit'].long(), h['faq_nit']) and torch.equal(out['faq_status'].long(), h['faq_status'])
        if 'sinkhorn_err' in h:
            assert torch.equal(out['sinkhorn_err'], h['sinkhorn_err'])
        else:
            assert out['sinkhorn_err'] is None
        if h['faq_restart'] is not None:
            assert torch.equal(out['faq_restart'].long(), h['faq_restart'])
    else:
        assert out['faq_perm'] is None and out['faq_qap'] is None
    if h['perm'] is None:
        assert out['perm'] is None and out['refined'] is None and out['refined_correct'] is None and not meter.refined
    else:
        assert torch.equal(out['perm'], h['perm']) and torch.equal(out['refined'], h['refined']) and out['refined'].dtype == torch.float32
        assert meter.refined
    if two_opt:
        assert torch.equal(out['swaps'].long(), h['swaps']) and torch.equal(out['status'].long(), h['status']) and torch.equal(out['nit'], h['nit'])
        assert torch.equal(out['refined'], torch.where(h['status'] == 2, out['refined'], h['two_opt']['qap']))
    hand = WeightedQapMeter(DEV)
    correct, rc, ratio = _fold(hand, h['assign'], h['perm'], h['refined'], None, h['qap'], h['planted'], None, live)
    assert torch.equal(out['correct'], correct) and torch.equal(out['ratio'], ratio) and torch.equal(meter.buf, hand.buf)
    if h['perm'] is not None:
        assert torch.equal(out['refined_correct'], rc)
    assert meter.record()['pairs'] == live
    # the same through the model
    m = model.match_weighted(x1, x2, refine=refine, two_opt=two_opt, faq=faq)
    assert torch.equal(m['assign'], h['assign']) and torch.equal(m['qap'], h['qap']) and torch.equal(m['planted'], h['planted'])
    assert torch.equal(m['acc'], count_matches(h['assign'], torch.arange(N, dtype=torch.int32, device=DEV).expand(B, N).contiguous(), None).long())
    if faq is not None:
        assert torch.equal(m['faq_perm'], h['faq_perm']) and torch.equal(m['qap_faq'], h['faq_qap'])
        if not (refine or two_opt):
            assert torch.equal(m['perm'], h['stage_perm'])
    if refine:
        assert all(torch.equal(m[k], h['greedy'][k]) for k in ('s_best', 'na', 'nb', 'acc_best', 'T_best'))
    if two_opt:
        t = h['two_opt']
        assert torch.equal(m['perm'], t['perm']) and torch.equal(m['qap_2opt'], h['refined']) and torch.equal(m['acc_2opt'], t['acc'])
        assert all(torch.equal(m[k], t[k]) for k in ('swaps', 'nit', 'status'))
    elif refine:
        assert torch.equal(m['perm'], h['greedy']['perm'])


@pytest.mark.parametrize('N', [20, 50])
def test_match_weighted_with_refine_equals_match_weighted_true(N):
    model, x1, x2, s = _spectral(N)
    for T in (0, 3):
        a, b = model.match(x1, x2, refine=T, weighted=True), model.match_weighted(x1, x2, refine=T)
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype, k
    with pytest.raises(NotImplementedError, match='two_opt'):
        model.match(x1, x2, weighted=True, two_opt=True)
    with pytest.raises(NotImplementedError, match='faq'):
        model.match(x1, x2, weighted=True, faq=True)
    with pytest.raises(ValueError, match='match_weighted: seeds= needs the faq= stage'):
        model.match_weighted(x1, x2, seeds=_identity_seeds(N))
    with pytest.raises(ValueError, match='match_weighted: seeds= and refine > 0'):
        model.match_weighted(x1, x2, seeds=_identity_seeds(N), faq=True, refine=1)


@pytest.mark.parametrize('N', [20, 50])
@pytest.mark.parametrize('spec', ['tensor', 'scores'])
@pytest.mark.parametrize('polish', [False, True], ids=['plain', 'polish'])
def test_the_seeded_decode_holds_its_seeds_and_counts_them(N, spec, polish):
    model, x1, x2, s = _spectral(N)
    seeds = _identity_seeds(N) if spec == 'tensor' else 'scores'
    faq = {'restarts': 3, 'polish': True, 'seed': 1} if polish else True
    meter, sm = WeightedQapMeter(DEV), SeedMeter(DEV)
    out = decode_scores_weighted(s, x1, x2, meter=meter, two_opt=True, faq=faq, seeds=seeds, seed_meter=sm)
    sd = out['seeds']
    if spec == 'tensor':
        assert torch.equal(sd, seeds)
    else:
        picked = qap.confident_seeds(s)
        assert torch.equal(sd, picked['seeds']) and torch.equal(out['nseeds'].long(), picked['nseeds'].long())
    fixed = sd >= 0
    assert torch.equal(out['perm'][fixed], sd[fixed]) and torch.equal(out['faq_perm'][fixed], sd[fixed])     # the seeds hold to the end
    assert bool((out['status'] != 2).all()) and bool((out['faq_status'] != 2).all())
    perm = out['perm'].cpu().numpy()
    assert all(sorted(p.tolist()) == list(range(N)) for p in perm)
    assert torch.equal(out['refined'], qap.objective_weighted(x1, x2, out['perm'], None)['qap'])
    if not polish:      # the chain by hand, seeded exchange search included
        h = _by_hand(s, x1, x2, None, None, True, 0, True, seeds=seeds)
        assert torch.equal(out['faq_perm'], h['faq_perm']) and torch.equal(out['perm'], h['perm']) and torch.equal(out['refined'], h['refined'])
        assert torch.equal(out['seeded'].long(), fixed.sum(1)) and torch.equal(out['nseeds'].long(), fixed.sum(1))
        m = model.match_weighted(x1, x2, two_opt=True, faq=True, seeds=seeds)
        assert torch.equal(m['perm'], h['perm']) and torch.equal(m['seeds'], sd) and torch.equal(m['faq_perm'], h['faq_perm'])
    else:               # seeds, restarts R = 3 and polish: the starts, ONE chain on B R problems, the seeded search on all, the choice
        R = faq['restarts']
        ix = qap.seed_index_device(sd, None)
        u = torch.where(ix['valid'] != 0, ix['nfree'], torch.zeros_like(ix['nfree']))
        sk = qap.sinkhorn(qap.seed_gather_device(s, ix['free_a'], ix['free_b'], u), u)
        starts = qap.random_starts_device(sk['P'], u, None, faq['seed'], B, N, R, torch.device(DEV))
        x1r, x2r, sdr = x1[:, 0].repeat_interleave(R, 0), x2[:, 0].repeat_interleave(R, 0), sd.repeat_interleave(R, 0)
        run = qap.faq_weighted(x1r, x2r, None, starts, None, 30, 0.03, seeds=sdr, p0_free=True)
        t = qap.two_opt_weighted_seeded(x1r, x2r, run['perm'], sdr)
        best = qap.best_of_device(t['qap'], run['status'], run['nit'], t['perm'], R, t['status'].to(torch.int32))
        assert torch.equal(out['sinkhorn_err'], sk['err']) and torch.equal(out['faq_restart'], best['restart'])
        assert torch.equal(out['faq_perm'], best['perm']) and torch.equal(out['faq_qap'], best['qap'])
        assert torch.equal(out['faq_nit'], best['nit']) and torch.equal(out['faq_status'], best['status'])
        last = qap.two_opt_weighted_seeded(x1, x2, best['perm'], sd)
        assert torch.equal(out['perm'], last['perm']) and torch.equal(out['refined'], last['qap'])
        assert torch.equal(out['swaps'].long(), last['swaps']) and torch.equal(out['nit'], last['nit'])
        m = model.match_weighted(x1, x2, two_opt=True, faq=faq, seeds=seeds)
        assert torch.equal(m['perm'], last['perm']) and torch.equal(m['faq_perm'], best['perm']) and torch.equal(m['qap_2opt'], last['qap'])
    # the SeedMeter's integers against a host count (identity targets)
    sdn, stage, final = sd.cpu().numpy(), torch.where((out['faq_status'] == 2)[:, None], out['assign'], out['faq_perm']).cpu().numpy(), perm
    rows = np.arange(N)[None, :]
    want = {'seeds': int((sdn >= 0).sum()), 'seed_correct': int(((sdn >= 0) & (sdn == rows)).sum()), 'free_nodes': int((sdn < 0).sum()),
            'free_correct': int(((sdn < 0) & (stage == rows)).sum()), 'free_refined_correct': int(((sdn < 0) & (final == rows)).sum()),
            'nodes': B * N, 'pairs': B}
    rec = sm.record()
    print('N %d %s: seed record %r' % (N, spec, rec))
    assert {k: rec[k] for k in want} == want and out['seed_meter'] is sm
    assert meter.record()['pairs'] == B and meter.refined


def _zero_one(N):
    b1, b2, nv, lab = _gen(N, vertex_proba=0.8).bits(0, B, permute=True)
    g = torch.Generator(device=DEV).manual_seed(100 + N)
    s = torch.randn(B, N, N, generator=g, device=DEV)
    s.scatter_add_(2, lab.long().clamp(0, N - 1)[:, :, None], torch.full((B, N, 1), 4.0, device=DEV))
    nv = nv.to(torch.int32)
    x = torch.zeros(2, B, 2, N, N, dtype=torch.float32, device=DEV)
    for side, bits in enumerate((b1, b2)):
        _lib.call('fgnn_expand_adjacency', _lib.ptr(bits), _lib.ptr(nv), B, N, _lib.ptr(x[side]), _lib.stream_ptr())
    return s, b1, b2, x[0], x[1], nv, lab


@pytest.mark.parametrize('N', [20, 50])
@pytest.mark.parametrize('stages', [dict(), dict(refine=2), dict(two_opt=True), dict(faq=True, two_opt=True), dict(faq=True, refine=2),
                                    dict(faq=True, two_opt=True, seeds=True), dict(faq={'restarts': 3, 'polish': True}, seeds=True)],
                         ids=['plain', 'refine', 'two_opt', 'faq+two_opt', 'faq+refine', 'seeded', 'seeded+restarts+polish'])
def test_zero_one_pairs_as_float_give_the_bit_paths_matchings_and_integers(N, stages):
    s, b1, b2, x1, x2, nv, lab = _zero_one(N)
    kw = dict(stages)
    if kw.pop('seeds', False):
        sd = torch.where(torch.arange(N, device=DEV)[None, :] % 3 == 0, lab, torch.full_like(lab, -1)).to(torch.int32)
        kw['seeds'] = torch.where(torch.arange(N, device=DEV)[None, :] < nv[:, None], sd, torch.full_like(sd, -1))
    live = 4
    bins = torch.tensor([0, 1, 1, 0, 1], dtype=torch.int32, device=DEV)
    ref = decode_scores(s, b1, b2, nvalid=nv, labels=lab, meter=QapMeter(DEV), live=live, **kw)
    out = decode_scores_weighted(s, x1, x2, nvalid=nv, labels=lab, meter=WeightedQapMeter(DEV), live=live, **kw)
    for k in ('assign', 'faq_perm', 'perm', 'correct', 'refined_correct', 'faq_nit', 'faq_status', 'swaps', 'status', 'faq_restart'):
        assert (out[k] is None) == (ref[k] is None), k
        if ref[k] is not None:
            assert torch.equal(out[k], ref[k]), k
    for k in ('qap', 'planted', 'refined', 'faq_qap'):
        assert (out[k] is None) == (ref[k] is None), k
        if ref[k] is not None:
            assert out[k].dtype == torch.float32 and torch.equal(out[k].to(torch.int64), ref[k].to(torch.int64)), k
    assert torch.equal(out['ratio'], ref['ratio'])
    a, b = out['meter'].record(), ref['meter'].record()
    print('N %d %s: %r' % (N, sorted(stages), a))
    for k in INT_FIELDS + ('refined',):
        assert a[k] == b[k], k
    for k in ('qap_sum', 'planted_sum', 'refined_sum'):
        assert isinstance(a[k], float) and a[k] == b[k], k
    assert a['ratio_sum'] == b['ratio_sum'] and out['meter'].result() == ref['meter'].result()
    # the binned meter: every record the plain fold of its pairs
    binned = BinnedWeightedQapMeter(DEV, 2)
    decode_scores_weighted(s, x1, x2, nvalid=nv, labels=lab, meter=binned, live=live, bins=bins, assign=out['assign'], **kw)
    for k in range(2):
        alone = WeightedQapMeter(DEV)
        keep = (bins == k).cpu()
        keep[live:] = False
        idx = torch.nonzero(keep)[:, 0].to(DEV)
        sub = {n: (out[n][idx].contiguous() if out[n] is not None else None) for n in ('assign', 'perm', 'refined', 'qap', 'planted')}
        _fold(alone, sub['assign'], sub['perm'], sub['refined'], lab[idx].contiguous(), sub['qap'], sub['planted'], nv[idx].contiguous(),
              len(idx))
        assert torch.equal(binned[k].buf, alone.buf), k


def test_refusals_and_argument_checks():
    model, x1, x2, s = _spectral(20)
    with pytest.raises(ValueError, match='decode_scores_weighted: seeds= needs the faq= stage'):
        decode_scores_weighted(s, x1, x2, seeds=_identity_seeds(20))
    with pytest.raises(ValueError, match='decode_scores_weighted: seeds= and refine > 0'):
        decode_scores_weighted(s, x1, x2, seeds='scores', faq=True, refine=1)
    with pytest.raises(ValueError, match='decode_scores_weighted: the meter must be of class WeightedQapMeter'):
        decode_scores_weighted(s, x1, x2, meter=QapMeter(DEV))
    with pytest.raises(ValueError, match='must be of class QapMeter'):
        b1, b2, _, _ = _gen(20).bits(0, B, permute=True)
        decode_scores(s, b1, b2, meter=WeightedQapMeter(DEV))
    with pytest.raises(ValueError, match='bins= and a BinnedWeightedQapMeter'):
        decode_scores_weighted(s, x1, x2, bins=torch.zeros(B, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match='decode_scores_weighted: the graphs are'):
        decode_scores_weighted(s, x1[:, :, :19, :19], x2[:, :, :19, :19])
    with pytest.raises(ValueError, match='faq has unknown key'):
        decode_scores_weighted(s, x1, x2, faq={'P1': 3})
    # channel 0 in place: nothing is copied, and a (B, N, N) copy of it decodes the same
    v1, v2, gs, ld = qap.weighted_views(x1, x2)
    assert v1.data_ptr() == x1.data_ptr() and gs == x1.shape[1] * 400
    a = decode_scores_weighted(s, x1, x2, two_opt=True, faq=True)
    b = decode_scores_weighted(s, x1[:, 0].contiguous(), x2[:, 0].contiguous(), two_opt=True, faq=True)
    assert torch.equal(a['perm'], b['perm']) and torch.equal(a['refined'], b['refined']) and torch.equal(a['meter'].buf, b['meter'].buf)
