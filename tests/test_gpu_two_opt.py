"""GPU: the pairwise-exchange search -- fgnn_qap_2opt through qap.two_opt_bits / qap.two_opt, and the two_opt= keyword of the decode
chain -- against tests/two_opt_ref.py (held to SciPy by tests/test_two_opt_host.py) and, at two sizes, against SciPy itself.
Everything is an integer: perm, qap, swaps, nit and status are compared exactly, meters as bytes.

The shapes: every row width NW (N <= 32, 64, 128, 256) on both sides of each word boundary, one pair and more pairs than a wave has
rows, corners of 0, 1 and N vertices inside one batch with arbitrary bits and arbitrary `assign` entries outside the corner.  At
N = 256 the start is the planted matching with three transpositions, so the reference stays short."""
import numpy as np
import pytest
import torch
from scipy.optimize import quadratic_assignment

import qap_ref
import two_opt_ref as R
from graph_neural_net_amd import _lib, qap
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.evaluation import BinnedQapMeter, QapMeter, decode_scores
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.sampler import EpochSampler
from graph_neural_net_amd.siamese import Siamese_Node_Exp
from graph_neural_net_amd.trainer import FgnnTrainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KEYS = ('qap', 'swaps', 'nit', 'status')


def _words(mats, N, junk_seed=None):
    """pairs' matrices -> (B, N, ceil(N/32)) int32 device words; junk_seed: arbitrary bits outside each corner"""
    out = []
    for b, m in enumerate(mats):
        n = len(m)
        full = np.zeros((N, N), dtype=np.int64) if junk_seed is None else np.random.default_rng(junk_seed + b).integers(0, 2, (N, N))
        full[:n, :n] = m
        out.append(qap_ref.pack_bits(full, N))
    return torch.from_numpy(np.stack(out).view(np.int32)).to(DEV)


def _assign(starts, N, junk=False):
    a = np.full((len(starts), N), -1, dtype=np.int32)
    for b, s in enumerate(starts):
        a[b, :len(s)] = s
        if junk:
            a[b, len(s):] = b + 3
    return torch.from_numpy(a).to(DEV)


def _batch(N, B, symmetric, ragged):
    """-> (As, Bs, starts): pair b has n_b vertices (0, 1 and N among them when ragged), a random start up to N = 65 on every other
    pair and at N = 129 on the first, else the planted matching with three transpositions"""
    rng = np.random.default_rng(7 * N + B)
    sizes = [N] * B
    if ragged:
        sizes = ([0, 1, N] + rng.integers(0, N + 1, B).tolist())[:B]
    As, Bs, starts = [], [], []
    for b, n in enumerate(sizes):
        A, Bm, q = R.make_pair(n, b, symmetric)
        random_start = (N <= 65 and b % 2 == 0) or (N == 129 and b == 0)
        starts.append(rng.permutation(n) if random_start or n < 2 else R.transposed(q, 3, b))
        As.append(A), Bs.append(Bm)
    return As, Bs, starts


def _check(out, As, Bs, starts, N, max_swaps=None):
    got_perm = out['perm'].cpu().tolist()
    got = {k: out[k].cpu().tolist() for k in KEYS}
    total = 0
    for b, (A, Bm, s) in enumerate(zip(As, Bs, starts)):
        ref = R.two_opt(A, Bm, s, max_swaps)
        assert got_perm[b] == ref['perm'].tolist() + [-1] * (N - len(s)), b
        assert [got[k][b] for k in KEYS] == [ref[k] for k in KEYS], (b, len(s))
        total += ref['swaps']
    return total


CASES = [(1, 5, True), (2, 70, True), (31, 5, True), (32, 1, False), (33, 70, True), (33, 5, False), (50, 5, True), (64, 1, True),
         (65, 5, True), (65, 1, False), (129, 5, True), (129, 1, False), (256, 1, True), (256, 1, False)]


@pytest.mark.parametrize('N,B,symmetric', CASES)
def test_kernel_equals_the_serial_algorithm(N, B, symmetric):
    As, Bs, starts = _batch(N, B, symmetric, ragged=B > 1)
    b1, b2 = _words(As, N, junk_seed=N if B > 1 else None), _words(Bs, N, junk_seed=N + 99 if B > 1 else None)
    nv = torch.tensor([len(s) for s in starts], dtype=torch.int32, device=DEV) if B > 1 else None
    assign = _assign(starts, N, junk=B > 1)
    out = qap.two_opt_bits(b1, b2, assign, nv, raw=True)
    assert out['nit'].dtype == torch.int64 and all(out[k].dtype == torch.int32 for k in ('perm', 'qap', 'swaps', 'status'))
    total = _check(out, As, Bs, starts, N)
    print('N %d B %d symmetric %d: %d exchanges, nit %s' % (N, B, symmetric, total, out['nit'].cpu().tolist()[:5]))
    assert N < 3 or total > 0
    # the objective it reports is the objective of the matching it reports; a second run has the same bytes
    assert torch.equal(out['qap'].to(torch.int64), qap.qap_objective(b1, b2, out['perm'], nvalid=nv)['qap'])
    again = qap.two_opt_bits(b1, b2, assign, nv, raw=True)
    assert all(torch.equal(again[k], out[k]) for k in out)
    if not symmetric:
        assert any(len(A) > 2 and (not np.array_equal(A, A.T)) and A.diagonal().any() for A in As)


@pytest.mark.parametrize('n', [12, 33])
@pytest.mark.parametrize('symmetric', [True, False])
def test_kernel_equals_scipy(n, symmetric):
    A, Bm, q = R.make_pair(n, 4, symmetric)
    start = np.random.default_rng(n).permutation(n) if n == 12 else R.transposed(q, 3, 1)
    res = quadratic_assignment(A, Bm, method='2opt', options={'maximize': True, 'partial_guess': np.stack([np.arange(n), start], 1)})
    out = qap.two_opt_bits(_words([A], n), _words([Bm], n), _assign([start], n), None)
    assert out['perm'][0].cpu().tolist() == res.col_ind.tolist()
    assert (int(out['qap'][0]), int(out['nit'][0]), int(out['status'][0])) == (int(res.fun), int(res.nit), 0)
    assert int(out['swaps'][0]) > 0


@pytest.mark.parametrize('max_swaps', [0, 1, 2])
def test_max_swaps_stops_the_search(max_swaps):
    N = 50
    As, Bs, starts = _batch(N, 5, True, ragged=True)
    b1, b2, assign = _words(As, N), _words(Bs, N), _assign(starts, N)
    nv = torch.tensor([len(s) for s in starts], dtype=torch.int32, device=DEV)
    out = qap.two_opt_bits(b1, b2, assign, nv, max_swaps=max_swaps, raw=True)
    _check(out, As, Bs, starts, N, max_swaps)
    status = out['status'].cpu().tolist()
    assert status[0] == 0 and status[2] == 1 and int(out['swaps'][2]) == max_swaps      # (the empty pair; a pair that had more to do)
    if max_swaps == 0:
        assert torch.equal(out['perm'][2], assign[2]) and out['nit'].cpu().tolist()[1:] == [0] * 4
    with pytest.raises(ValueError, match='max_swaps'):
        qap.two_opt_bits(b1, b2, assign, nv, max_swaps=-2)


def test_an_invalid_start_is_reported_and_its_neighbours_are_not_touched():
    N, n = 33, 33
    pairs = [R.make_pair(n, b, b % 2 == 0) for b in range(5)]
    As, Bs = [p[0] for p in pairs], [p[1] for p in pairs]
    starts = [R.transposed(p[2], 3, b) for b, p in enumerate(pairs)]
    for b, (at, value) in {0: (4, -1), 2: (32, n), 4: (7, None)}.items():
        starts[b][at] = starts[b][at + 1 if at + 1 < n else 0] if value is None else value
    b1, b2, assign = _words(As, N), _words(Bs, N), _assign(starts, N)
    out = qap.two_opt_bits(b1, b2, assign, None, raw=True)
    _check(out, As, Bs, starts, N)
    assert out['status'].cpu().tolist() == [2, 0, 2, 0, 2] and out['qap'].cpu().tolist()[::2] == [-1, -1, -1]
    assert torch.equal(out['perm'][::2], assign[::2]) and out['nit'].cpu().tolist()[::2] == [0, 0, 0]
    alone = qap.two_opt_bits(b1[1:2], b2[1:2], assign[1:2], None, raw=True)
    assert all(torch.equal(alone[k][0], out[k][1]) for k in out)
    full = qap.two_opt(b1, b2, assign)
    assert full['status'].tolist() == [2, 0, 2, 0, 2] and full['swaps'].dtype == torch.int64


def test_public_function_dense_input_labels_and_the_host_route():
    N, B = 33, 5
    As, Bs, starts = _batch(N, B, True, ragged=True)
    sizes = [len(s) for s in starts]
    b1, b2, assign = _words(As, N), _words(Bs, N), _assign(starts, N)
    nv = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    labels = torch.from_numpy(np.stack([np.concatenate([np.random.default_rng(b).permutation(n), np.full(N - n, -1)])
                                        for b, n in enumerate(sizes)])).to(DEV)
    got = qap.two_opt(b1, b2, assign, nvalid=nv, labels=labels)
    assert set(got) == {'perm', 'qap', 'qap0', 'acc', 'swaps', 'nit', 'status'} and all(t.device.type == 'cuda' for t in got.values())
    host = qap.two_opt(b1.cpu(), b2.cpu(), assign.cpu(), nvalid=nv.cpu(), labels=labels.cpu())
    for k in got:
        assert got[k].dtype == host[k].dtype and torch.equal(got[k].cpu(), host[k]), k
    assert torch.equal(got['qap0'], qap.qap_objective(b1, b2, assign, nvalid=nv)['qap'])
    assert bool((got['qap'] >= got['qap0'] + got['swaps']).all())
    plain = qap.two_opt(b1, b2, assign, nvalid=nv)
    want_acc = [int((plain['perm'][b, :n].cpu().numpy() == np.arange(n)).sum()) for b, n in enumerate(sizes)]
    assert plain['acc'].tolist() == want_acc and torch.equal(plain['perm'], got['perm'])
    dense = []
    for mats in (As, Bs):
        x = torch.zeros(B, 2, N, N)
        for b, m in enumerate(mats):
            x[b, 0, :len(m), :len(m)] = torch.from_numpy(m).float()
            x[b, 1, :len(m), :len(m)] = torch.diag(torch.from_numpy(m.sum(1)).float())
        dense.append(x.to(DEV))
    again = qap.two_opt(dense[0], dense[1], assign, nvalid=nv, labels=labels)
    assert all(torch.equal(again[k], got[k]) for k in got)
    dense[0][2, 0, 0, 1] = 0.5
    with pytest.raises(RuntimeError, match='NOT the tensor'):
        qap.two_opt(dense[0], dense[1], assign, nvalid=nv)
    with pytest.raises(NotImplementedError, match='weighted'):
        qap.two_opt(dense[0], dense[1], assign, weighted=True)


# ------------------------------------------------------------------------------------------------------------ the decode chain
LAY = ParamLayout(2, 2, 32, 32, 3)


def _gen(N, seed=11, noise=0.15, **kw):
    return PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=noise, seed=seed, device=DEV, **kw)


def _fold_by_hand(meter, assign, perm, refined, labels, q, planted, nv, live, bins=None):
    B, N = assign.shape
    nv, labels = (None if t is None else t.to(torch.int32).contiguous() for t in (nv, labels))
    correct, refined_correct = torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    ratio = torch.zeros(B, dtype=torch.float64, device=DEV)
    pairs = (_lib.ptr(assign), _lib.ptr(perm), _lib.ptr(labels), _lib.ptr(q), _lib.ptr(planted), _lib.ptr(refined), _lib.ptr(nv), B, N, live)
    outs = (_lib.ptr(correct), _lib.ptr(refined_correct), _lib.ptr(ratio), _lib.ptr(meter.buf), _lib.stream_ptr())
    if bins is None:
        _lib.call('fgnn_qap_fold', *pairs, *outs)
    else:
        _lib.call('fgnn_qap_fold_bins', *pairs, _lib.ptr(bins), meter.K, *outs)
    meter._mark_refined()
    return refined_correct


@pytest.mark.parametrize('refine', [0, 2])
def test_decode_scores_folds_the_last_stage_of_the_chain(refine):
    N, B, live, K = 12, 6, 5, 3
    b1, b2, nv, lab = _gen(N, seed=5, vertex_proba=0.8).bits(0, B, permute=True)
    s = torch.randn(B, N, N, generator=torch.Generator().manual_seed(3 + refine)).to(DEV)
    bins = torch.tensor([2, 0, 2, 1, 0, 1], device=DEV)
    # the stages one by one
    base = decode_scores(s, b1, b2, nvalid=nv, labels=lab, live=live, refine=refine)
    start = base['perm'] if refine else base['assign']
    t = qap.two_opt_bits(b1, b2, start, nv, raw=True)
    assert bool((t['status'] == 0).all()) and int(t['swaps'].sum()) > 0
    hand, hand_bins = QapMeter(DEV), BinnedQapMeter(DEV, K)
    rc = _fold_by_hand(hand, base['assign'], t['perm'], t['qap'], lab, base['qap'], base['planted'], nv, live)
    _fold_by_hand(hand_bins, base['assign'], t['perm'], t['qap'], lab, base['qap'], base['planted'], nv, live, bins.to(torch.int32))
    # the chain
    meter, meter_bins = QapMeter(DEV), BinnedQapMeter(DEV, K)
    out = decode_scores(s, b1, b2, nvalid=nv, labels=lab, meter=meter, live=live, refine=refine, two_opt=True)
    decode_scores(s, b1, b2, nvalid=nv, labels=lab, meter=meter_bins, live=live, bins=bins, refine=refine, two_opt=True)
    assert torch.equal(meter.buf, hand.buf) and torch.equal(meter_bins.buf, hand_bins.buf) and meter.refined and meter_bins.refined
    assert set(out) == set(base) and torch.equal(out['assign'], base['assign']) and torch.equal(out['qap'], base['qap'])
    assert torch.equal(out['perm'], t['perm']) and torch.equal(out['refined'], t['qap']) and torch.equal(out['refined_correct'], rc)
    assert torch.equal(out['swaps'], t['swaps']) and torch.equal(out['status'], t['status'])
    res = meter.result()
    print('refine %d: %r' % (refine, res))
    assert res['refined_qap_ratio'] >= res['qap_ratio'] and 'refined_acc' in res
    if refine:
        assert meter.record()['refined_sum'] >= base['meter'].record()['refined_sum']
    # two_opt=False is the call without the keyword
    off, none = QapMeter(DEV), QapMeter(DEV)
    a = decode_scores(s, b1, b2, nvalid=nv, labels=lab, meter=off, live=live, refine=refine, two_opt=False)
    b = decode_scores(s, b1, b2, nvalid=nv, labels=lab, meter=none, live=live, refine=refine)
    assert set(a) == set(b) and torch.equal(off.buf, none.buf) and off.refined == none.refined == (refine > 0)
    assert a['swaps'] is None and a['status'] is None and b['swaps'] is None
    with pytest.raises(ValueError, match='two_opt'):
        decode_scores(s, b1, b2, two_opt=1)


def test_the_default_steps_issue_the_launches_they_issued(monkeypatch):
    N = 12
    tr = FgnnTrainer(LAY, LAY.init_flat(7, DEV), lr=2e-3)
    b1, b2 = _gen(N).bits(0, 4)[:2]
    names = []
    real = _lib.call

    def recording(name, *args, **kw):
        names.append(name)
        return real(name, *args, **kw)
    monkeypatch.setattr(_lib, 'call', recording)
    runs = []
    for kw in ({}, {'two_opt': False}, {'two_opt': True}, {'refine': 1}, {'refine': 1, 'two_opt': False}, {'refine': 1, 'two_opt': True}):
        del names[:]
        tr.eval_step_bits(b1, b2, qap_meter=QapMeter(DEV), **kw)
        runs.append(list(names))
    assert runs[0] == runs[1] and runs[3] == runs[4] and 'fgnn_qap_2opt' not in runs[0] + runs[3]
    assert runs[2] == runs[0][:-1] + ['fgnn_qap_2opt', 'fgnn_qap_fold'] and runs[5] == runs[3][:-1] + ['fgnn_qap_2opt', 'fgnn_qap_fold']
    with pytest.raises(ValueError, match='two_opt'):
        tr.eval_step_bits(b1, b2, two_opt=True)


def test_evaluate_with_two_opt_equals_the_loop_written_out():
    """8 examples of 20 vertices in 2 steps of 4"""
    N, M, TB = 20, 8, 4
    gen = _gen(N, seed=3)
    tr = FgnnTrainer(LAY, LAY.init_flat(7, DEV), lr=2e-3)
    tr.train_step_bits(*gen.bits(0, 4)[:2])
    sampler = EpochSampler(M, shuffle=False)
    qm = QapMeter(DEV)
    tr.evaluate(gen, sampler, TB, qap_meter=qm, two_opt=True)
    hand, swaps = QapMeter(DEV), 0
    for step in range(2):
        b1, b2, nv = gen.bits(index=sampler.batch_index(0, step, TB))[:3]
        assign = tr.eval_step_bits(b1, b2, nvalid=nv)['assign']
        obj = qap.objective_bits(b1, b2, assign, nv, raw=True)
        t = qap.two_opt(b1, b2, assign, nvalid=nv)
        _fold_by_hand(hand, assign, t['perm'], t['qap'].to(torch.int32), None, obj[0], obj[1], nv, TB)
        swaps += int(t['swaps'].sum())
    assert torch.equal(qm.buf, hand.buf) and qm.refined and swaps > 0
    rec = qm.record()
    print('evaluate(two_opt=True): %r' % (rec,))
    assert rec['pairs'] == M and rec['steps'] == 2 and rec['refined_sum'] >= rec['qap_sum'] + swaps
    plain = QapMeter(DEV)
    tr.evaluate(gen, sampler, TB, qap_meter=plain, two_opt=False)
    again = QapMeter(DEV)
    tr.evaluate(gen, sampler, TB, qap_meter=again)
    assert torch.equal(plain.buf, again.buf) and not plain.refined
    with pytest.raises(ValueError, match='two_opt'):
        tr.evaluate(gen, sampler, TB, two_opt=True)
    # the noise curve and fit take the keyword
    noises = (0.0, 0.3)
    bq = BinnedQapMeter(DEV, 2, values=noises)
    tr.noise_curve(gen, noises, 4, TB, qap_meter=bq, two_opt=True)
    assert bq.refined and all(r['refined_qap_ratio'] >= r['qap_ratio'] for r in bq.result())
    hist = tr.fit(gen, EpochSampler(4, seed=1), gen, EpochSampler(4, shuffle=False), epochs=1, batch_size=TB, decode_refine=0,
                  decode_two_opt=True)
    assert hist[0]['val_refined_qap_ratio'] >= hist[0]['val_qap_ratio'] and 0.0 <= hist[0]['val_refined_acc'] <= 1.0
    with pytest.raises(ValueError, match='decode_two_opt'):
        tr.fit(gen, EpochSampler(4, seed=1), gen, EpochSampler(4, shuffle=False), epochs=1, batch_size=TB, decode_two_opt=True)


@pytest.mark.parametrize('refine', [0, 3])
def test_match_with_two_opt_equals_the_function_on_the_same_matching(refine):
    from graph_neural_net_amd import synthetic
    torch.manual_seed(3)
    ne = dict(type='node_embedding', block_init='block_emb', block_inside='block', num_blocks=2, in_features=32, out_features=32,
              depth_of_mlp=3)
    model = Siamese_Node_Exp(2, ne).to(DEV)
    x1, x2 = (x.to(DEV) for x in synthetic.make_batch(11, 4, 40, 'ErdosRenyi', 0.2, 0.1))
    base = model.match(x1, x2, refine=refine)
    out = model.match(x1, x2, refine=refine, two_opt=True)
    t = qap.two_opt(x1, x2, base['perm'] if refine else base['assign'])
    assert set(out) == set(base) | {'perm', 'qap_2opt', 'acc_2opt', 'swaps', 'nit', 'status'}
    assert all(torch.equal(out[k], base[k]) for k in base if k != 'perm')
    for mine, theirs in (('perm', 'perm'), ('qap_2opt', 'qap'), ('acc_2opt', 'acc'), ('swaps', 'swaps'), ('nit', 'nit'), ('status', 'status')):
        assert torch.equal(out[mine], t[theirs]), mine
    assert int(out['swaps'].sum()) > 0 and bool((out['qap_2opt'] >= out['qap']).all())
    with pytest.raises(NotImplementedError, match='two_opt'):
        model.match(x1, x2, weighted=True, two_opt=True)
