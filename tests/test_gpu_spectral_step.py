"""GPU: the spectral step -- spectral= of the two engines, FgnnTrainer.train_step_spectral / eval_step_spectral and
features='spectral' of train_epoch / evaluate / noise_curve / fit -- against the route that existed before: spectral_features (or
generator.spectral) handed to the dense step.  The engines promise the same bytes in block 1's input, and everything after it is
the same launch sequence, so every comparison is torch.equal.

Model: 4 spectral channels -> 32 -> 32, depth 3, 2 blocks, on the 32-channel layout (ParamLayout has no 4-channel one).  The bf16
engine takes the 4 channels as they are (its input conversion zero-fills the slab); the fp32 kernels read their input at the
layout's width, so the dense fp32 route hands over the features zero-padded to 32 channels (`_dense`)."""
import pytest
import torch

from graph_neural_net_amd.engine import FgnnEngine, ParamLayout
from graph_neural_net_amd.engine16 import FgnnEngineBF16
from graph_neural_net_amd.evaluation import (BinnedEvalMeter, BinnedQapMeter, BinnedRankMeter, EvalMeter, QapMeter, RankMeter,
                                             decode_scores)
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.pairstore import PairStore
from graph_neural_net_amd.sampler import EpochSampler
from graph_neural_net_amd.spectral import spectral_features
from graph_neural_net_amd.trainer import FgnnTrainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
P = 4
LAYS = {'fp32': ParamLayout(32, 2, 32, 32, 3), 'bf16': ParamLayout(32, 2, 32, 32, 3)}
CASES = [('fp32', False, 20, 2), ('fp32', True, 40, 3), ('bf16', False, 40, 3), ('bf16', True, 20, 2)]


def _gen(N, ragged=False, seed=11, noise=0.05):
    kw = {'vertex_proba': 0.8} if ragged else {}
    return PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=noise, seed=seed, device=DEV, **kw)


def _trainer(precision, **kw):
    lay = LAYS[precision]
    return FgnnTrainer(lay, lay.init_flat(7, DEV), lr=2e-3, precision=precision, **kw)


def _state(tr):
    return [tr.params, tr.opt.exp_avg, tr.opt.exp_avg_sq]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _dense(f, precision):
    """what the dense step of `precision` takes for the features f: (G, P, N, N) as they are, or zero-padded to the fp32 layout's 32"""
    if precision == 'bf16':
        return f
    x = torch.zeros(f.shape[0], 32, f.shape[2], f.shape[3], device=f.device)
    x[:, :f.shape[1]] = f
    return x


def _feat(b, nv, precision='bf16'):
    return _dense(spectral_features(b, nv, P), precision)


# ---------------------------------------------------------------------------------------------- engines
@pytest.mark.parametrize('precision,ragged,N,B', CASES)
def test_engine_step_from_words_equals_step_on_features(precision, ragged, N, B):
    lay = LAYS[precision]
    cls = FgnnEngine if precision == 'fp32' else FgnnEngineBF16
    b1, b2, nv, lab = _gen(N, ragged).bits(0, B, permute=True)
    assert (nv is not None) == ragged
    bits = torch.cat([b1, b2]).contiguous()
    nv2 = None if nv is None else torch.cat([nv, nv]).to(torch.int32)
    params = lay.init_flat(3, DEV)
    weights = torch.tensor([0.5, 2.0, 0.0][:B], device=DEV)
    total = float(B * N if nv is None else int(nv.sum()))
    for kw in ({'labels': lab, 'total_nodes': total}, {'weights': weights}, {'labels': lab, 'weights': weights}):
        res = []
        for src in ({'x': _feat(bits, nv2, precision)}, {'spectral': (bits, P)}):
            eng = cls(lay, 2 * B, N, DEV, ragged=ragged)
            grads = torch.zeros_like(params)
            scores, loss = eng.step(params, grads, nvalid=nv2, **src, **kw)
            res.append((scores.clone(), loss.clone(), grads, eng.E.clone()))
        for name, a, b in zip(('scores', 'loss', 'grads', 'E'), *res):
            assert torch.equal(a, b), (name, sorted(kw))
        assert bool(res[0][2].any()) and bool(torch.isfinite(res[0][1]).all())
    # the forward alone, and the words are read in place
    eng = cls(lay, 2 * B, N, DEV, ragged=ragged)
    s_x = eng.forward(params, _feat(bits, nv2, precision), nvalid=nv2)[0].clone()
    keep = bits.clone()
    assert torch.equal(eng.forward(params, nvalid=nv2, spectral=(bits, P))[0], s_x) and torch.equal(bits, keep)


def test_engine_refusals():
    N, B = 20, 2
    b1, b2, _ = _gen(N).bits(0, B)
    bits = torch.cat([b1, b2]).contiguous()
    for precision, cls in (('fp32', FgnnEngine), ('bf16', FgnnEngineBF16)):
        lay = LAYS[precision]
        params, eng = lay.init_flat(3, DEV), cls(lay, 2 * B, N, DEV)
        with pytest.raises(RuntimeError, match='not two of them'):
            eng.forward(params, _feat(bits, None, precision), spectral=(bits, P))
        with pytest.raises(RuntimeError, match='not two of them'):
            eng.forward(params, bits=bits, spectral=(bits, P))
        with pytest.raises(RuntimeError, match='32-bit words'):
            eng.forward(params, spectral=(bits[:, :, :0], P))
    lay2 = ParamLayout(2, 2, 32, 32, 3)
    with pytest.raises(RuntimeError, match='at least that many channels'):         # n_powers > layout.c0
        FgnnEngineBF16(lay2, 2 * B, N, DEV).forward(lay2.init_flat(3, DEV), spectral=(bits, P))
    with pytest.raises(RuntimeError, match='does not fit original_features_num = 2'):
        FgnnEngine(lay2, 2 * B, N, DEV).forward(lay2.init_flat(3, DEV), spectral=(bits, P))
    with pytest.raises(RuntimeError, match='does not fit original_features_num = 2'):
        FgnnEngine(lay2, 2 * B, N, DEV).forward(lay2.init_flat(3, DEV), spectral=(bits, 1))
    for cls in (FgnnEngine, FgnnEngineBF16):
        eng = cls(lay2, 2 * B, N, DEV, block1='structured')
        assert eng.struct1
        with pytest.raises(RuntimeError, match='structured'):
            eng.forward(lay2.init_flat(3, DEV), spectral=(bits, 2))
    # a 2-channel layout with 2 powers runs, on both engines
    for cls in (FgnnEngine, FgnnEngineBF16):
        a = cls(lay2, 2 * B, N, DEV).forward(lay2.init_flat(3, DEV), spectral=(bits, 2))[0].clone()
        b = cls(lay2, 2 * B, N, DEV).forward(lay2.init_flat(3, DEV), spectral_features(bits, None, 2))[0]
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- train steps
@pytest.mark.parametrize('precision,ragged,N,B', CASES)
def test_three_eager_steps_equal_three_dense_steps(precision, ragged, N, B):
    gen = _gen(N, ragged)
    a, b = _trainer(precision), _trainer(precision)
    for step in range(3):
        b1, b2, nv = gen.bits(step * B, B)
        la, _ = a.train_step_spectral(b1, b2, nv, n_powers=P)
        lb, _ = b.train_step(_feat(b1, nv, precision), _feat(b2, nv, precision), nvalid=nv)
        assert torch.equal(la, lb), step
    assert _same(_state(a), _state(b)) and a.opt.t == b.opt.t == 3
    # labels, weights and live go the way they go for bits
    b1, b2, nv, lab = gen.bits(20, B, permute=True)
    w = torch.tensor([1.5, 0.25, 1.0][:B])
    la, _ = a.train_step_spectral(b1, b2, nv, labels=lab, weights=w, live=B - 1)
    lb, _ = b.train_step(_feat(b1, nv, precision), _feat(b2, nv, precision), nvalid=nv, labels=lab, weights=w, live=B - 1)
    assert torch.equal(la, lb) and _same(_state(a), _state(b))


@pytest.mark.parametrize('precision,N,B', [('fp32', 20, 3), ('bf16', 40, 2)])
def test_captured_step_replays_on_fresh_words(precision, N, B):
    gen = _gen(N)
    cap, eager, dense = _trainer(precision, capture=True), _trainer(precision), _trainer(precision, capture=True)
    for step in range(3):                       # a different batch each time: the static words are refreshed before every replay
        b1, b2, nv = gen.bits(step * B, B)
        assert nv is None
        lc, sc = cap.train_step_spectral(b1, b2, n_powers=P)
        le, se = eager.train_step_spectral(b1, b2, n_powers=P)
        ld, _ = dense.train_step(_feat(b1, None, precision), _feat(b2, None, precision))
        assert torch.equal(lc, le) and torch.equal(lc, ld) and torch.equal(sc, se), step
    assert _same(_state(cap), _state(eager)) and _same(_state(cap), _state(dense))
    assert list(cap._graphs) == [(B, N, 'spectral', P)] and not eager._graphs
    b1, b2, _, lab = gen.bits(30, B, permute=True)
    lc, _ = cap.train_step_spectral(b1, b2, labels=lab, live=B - 1)
    le, _ = eager.train_step_spectral(b1, b2, labels=lab, live=B - 1)
    assert torch.equal(lc, le) and _same(_state(cap), _state(eager))
    assert set(cap._graphs) == {(B, N, 'spectral', P), (B, N, 'spectral', P, 'labels', 'weights')}


def test_bits_and_spectral_graphs_live_side_by_side():
    """one capturing trainer on a 2-channel layout alternates train_step_bits and train_step_spectral(n_powers=2) over two graph
    sizes: four captured graphs on two engines, each replayed after the others were recorded and replayed"""
    lay = ParamLayout(2, 2, 32, 32, 3)
    cap = FgnnTrainer(lay, lay.init_flat(5, DEV), lr=2e-3, capture=True)
    eager = FgnnTrainer(lay, lay.init_flat(5, DEV), lr=2e-3)
    B = 2
    gens = {N: _gen(N, seed=N) for N in (20, 40)}
    for rnd in range(3):
        for N in (20, 40):
            b1, b2, _ = gens[N].bits(rnd * B, B)
            for step in ('train_step_bits', 'train_step_spectral'):
                kw = {'n_powers': 2} if step == 'train_step_spectral' else {}
                lc, sc = getattr(cap, step)(b1, b2, **kw)
                le, se = getattr(eager, step)(b1, b2, **kw)
                assert torch.equal(lc, le) and torch.equal(sc, se), (rnd, N, step)
    assert _same(_state(cap), _state(eager)) and cap.opt.t == 12
    assert set(cap._graphs) == {(B, 20, 'bits'), (B, 20, 'spectral', 2), (B, 40, 'bits'), (B, 40, 'spectral', 2)}


# ---------------------------------------------------------------------------------------------- the loops
M, TB = 7, 3


def _hand_epoch(tr, gen, sampler, epoch, exact_last):
    losses = []
    for step in range(sampler.steps_per_epoch(TB)):
        f1, f2 = (_dense(f['input'], tr.precision) for f in gen.spectral(index=sampler.batch_index(epoch, step, TB), n_powers=P))
        losses.append(tr.train_step(f1, f2, live=sampler.live_count(step, TB) if exact_last else None)[0])
    return torch.stack(losses)


@pytest.mark.parametrize('precision,capture', [('fp32', False), ('bf16', True)])
@pytest.mark.parametrize('exact_last', [False, True])
def test_train_epoch_equals_the_hand_written_loop(precision, capture, exact_last):
    gen, sampler = _gen(20), EpochSampler(M, seed=2)
    a, b = _trainer(precision, capture=capture), _trainer(precision, capture=capture)
    for epoch in range(2):
        got = a.train_epoch(gen, sampler, epoch, TB, exact_last=exact_last, features='spectral', n_powers=P)
        want = _hand_epoch(b, gen, sampler, epoch, exact_last)
        assert got.shape == (3,) and torch.equal(got, want), epoch
    assert _same(_state(a), _state(b)) and a.opt.t == 6


def _trained(precision, N):
    tr = _trainer(precision)
    tr.train_step_spectral(*_gen(N).bits(0, 4)[:2], n_powers=P)
    return tr


@pytest.mark.parametrize('precision,ragged,N', [('fp32', True, 20), ('bf16', False, 40)])
def test_evaluate_equals_dense_steps_plus_decode(precision, ragged, N):
    tr, gen = _trained(precision, N), _gen(N, ragged, seed=3)
    sampler = EpochSampler(M, shuffle=False)
    whole = gen.bits(0, M)
    store = PairStore.from_bits(whole[0], sizes=whole[2], noise_model=gen.noise_model, noise=gen.noise, seed=gen.seed,
                                edge_density=gen.edge_density)
    before = [t.clone() for t in _state(tr)]
    for source in (gen, store):
        meter, rm, qm = EvalMeter(DEV), RankMeter(DEV), QapMeter(DEV)
        assert tr.evaluate(source, sampler, TB, meter=meter, rank_meter=rm, qap_meter=qm, refine=1, features='spectral', n_powers=P) is meter
        m2, r2, q2 = EvalMeter(DEV), RankMeter(DEV), QapMeter(DEV)
        for step in range(sampler.steps_per_epoch(TB)):
            live = sampler.live_count(step, TB)
            b1, b2, nv = source.bits(index=sampler.batch_index(0, step, TB))
            out = tr.eval_step(_feat(b1, nv, precision), _feat(b2, nv, precision), nvalid=nv, meter=m2, live=live, rank_meter=r2)
            scores = tr._engine(2 * TB, N, nv is not None).scores
            decode_scores(scores, b1, b2, nvalid=nv, meter=q2, live=live, refine=1, assign=out['assign'])
        assert torch.equal(meter.buf, m2.buf) and torch.equal(rm.buf, r2.buf) and torch.equal(qm.buf, q2.buf)
        rec = qm.record()
        assert rec['pairs'] == M and rec['steps'] == 3 and rec['refined'] and meter.record()['pairs'] == M
    assert _same(before, _state(tr)) and tr.opt.t == 1
    # permuted pairs: the decode stays on the bit words, the labels are the planted ones
    qp = QapMeter(DEV)
    tr.evaluate(gen, sampler, TB, permute=True, loss_on_labels=True, qap_meter=qp, features='spectral')
    assert qp.record()['pairs'] == M


def test_noise_curve_equals_separate_epochs():
    N, noises, per_level = 20, (0.0, 0.3), 5
    tr, gen = _trained('bf16', N), _gen(N)
    K = len(noises)
    meter, rm, qm = BinnedEvalMeter(DEV, K, values=noises), BinnedRankMeter(DEV, K), BinnedQapMeter(DEV, K, values=noises)
    assert tr.noise_curve(gen, noises, per_level, TB, meter=meter, rank_meter=rm, qap_meter=qm, refine=1, features='spectral') is meter
    recs, ranks, qaps = meter.record(), rm.record(), qm.record()
    for j, v in enumerate(noises):
        m1, r1, q1 = EvalMeter(DEV), RankMeter(DEV), QapMeter(DEV)
        tr.evaluate(_gen(N, noise=v), EpochSampler(per_level, shuffle=False), TB, meter=m1, rank_meter=r1, qap_meter=q1, refine=1,
                    features='spectral')
        for got, want in ((recs[j], m1.record()), (ranks[j], r1.record()), (qaps[j], q1.record())):
            want = dict(want, steps=got['steps'])
            assert {k: got[k] for k in want} == want, (j, got, want)
        assert recs[j]['pairs'] == per_level


def _hand_fit(tr, tg, ts, vg, vs, epochs):
    from graph_neural_net_amd.optim import ReduceLROnPlateau
    sched, hist = ReduceLROnPlateau(tr.opt), []
    for epoch in range(epochs):
        losses = _hand_epoch(tr, tg, ts, epoch, False)
        meter = EvalMeter(DEV)
        for step in range(vs.steps_per_epoch(TB)):
            f1, f2 = (_dense(f['input'], tr.precision) for f in vg.spectral(index=vs.batch_index(epoch, step, TB), n_powers=P))
            tr.eval_step(f1, f2, meter=meter, live=vs.live_count(step, TB))
        res = meter.result()
        sched.step(res['loss'])
        hist.append({'epoch': epoch, 'train_losses': losses, 'val_loss': res['loss'], 'val_acc': res['acc'],
                     'val_acc_max': res['acc_max'], 'lr': tr.opt.lr})
    return hist


def test_fit_equals_the_hand_written_loop():
    N = 20
    tg, ts, vg, vs = _gen(N, seed=1), EpochSampler(M, seed=1), _gen(N, seed=2), EpochSampler(5, shuffle=False)
    a, b = _trainer('bf16', capture=True), _trainer('bf16', capture=True)
    got = a.fit(tg, ts, vg, vs, epochs=2, batch_size=TB, features='spectral', n_powers=P)
    want = _hand_fit(b, tg, ts, vg, vs, 2)
    assert len(got) == 2 and set(got[0]) == {'epoch', 'train_losses', 'val_loss', 'val_acc', 'val_acc_max', 'lr'}
    for g, w in zip(got, want):
        assert torch.equal(g['train_losses'], w['train_losses'])
        assert {k: g[k] for k in g if k != 'train_losses'} == {k: w[k] for k in w if k != 'train_losses'}
    assert _same(_state(a), _state(b))
    extra = _trainer('fp32').fit(tg, ts, vg, vs, epochs=1, batch_size=TB, features='spectral', rank_ks=(1, 5), decode_refine=1)
    assert {'val_hits', 'val_mrr', 'val_qap_ratio', 'val_recovered', 'val_refined_acc'} <= set(extra[0])


def test_trainer_refusals():
    N = 20
    gen, sampler = _gen(N), EpochSampler(M, shuffle=False)
    b1, b2, _ = gen.bits(0, 2)
    lay2 = ParamLayout(2, 2, 32, 32, 3)
    for precision in ('fp32', 'bf16'):
        narrow = FgnnTrainer(lay2, lay2.init_flat(1, DEV), precision=precision)
        with pytest.raises(RuntimeError, match='do not fit this layout'):          # n_powers > layout.c0
            narrow.train_step_spectral(b1, b2, n_powers=P)
        with pytest.raises(RuntimeError, match='do not fit this layout'):
            narrow.evaluate(gen, sampler, TB, features='spectral')
        struct = FgnnTrainer(lay2, lay2.init_flat(1, DEV), precision=precision, block1='structured')
        for call in (lambda: struct.train_epoch(gen, sampler, 0, TB, features='spectral', n_powers=2),
                     lambda: struct.evaluate(gen, sampler, TB, features='spectral', n_powers=2),
                     lambda: struct.noise_curve(gen, (0.0, 0.1), 2, TB, features='spectral', n_powers=2),
                     lambda: struct.fit(gen, sampler, gen, sampler, 1, TB, features='spectral', n_powers=2),
                     lambda: struct.eval_step_spectral(b1, b2, n_powers=2)):
            with pytest.raises(RuntimeError, match='structured'):
                call()
    tr = _trainer('bf16')
    for call in (lambda: tr.train_epoch(gen, sampler, 0, TB, features='laplacian'), lambda: tr.evaluate(gen, sampler, TB, features='dense'),
                 lambda: tr.noise_curve(gen, (0.0,), 2, TB, features=4), lambda: tr.fit(gen, sampler, gen, sampler, 1, TB, features='x')):
        with pytest.raises(ValueError, match="None or 'spectral'"):
            call()
    with pytest.raises(RuntimeError, match='train_step_spectral'):
        tr.train_step_spectral(b1, b2[:, :, :0])
    assert tr.opt.t == 0
