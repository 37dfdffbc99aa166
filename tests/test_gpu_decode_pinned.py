"""GPU: the decode chain pinned launch for launch and byte for byte -- evaluation.decode_scores / decode_scores_weighted,
evaluate_scores(bits=) / (adj=), Siamese_Node_Exp.match / match(weighted=True) / match_weighted -- against a recording of the same
calls made before the 0/1 and the real-weighted chain were folded into one (tests/golden/decode_pinned.json).  Per run the fixture
holds the names handed to _lib.call, in order, and for every key of the returned dict (nested dicts and meters included) whether it
is None, its dtype, its shape and the SHA-256 of its bytes; its key sets also say which route returns 'nit' and 'greedy'.

The fixture is a recording: `record()` below, run on the commit before the fold, twice (the second time over freshly dirtied
allocator blocks); the two recordings agreed on every digest.  It is not regenerated from the code under test.

Pairs: B = 3 at N = 20 with nvalid = (20, 17, 20): planted (permute=True) Erdos-Renyi pairs of PairGenerator.bits, the middle one a
17-vertex pair in the corner of zero words; the same pairs as fp32 matrices; and correlated Gaussian pairs of WignerGenerator laid
out the same way.  Scores: 4 onehot(labels) + standard normal noise from the device's Philox generator for the functions, the
model's own for `match`."""
import hashlib
import json
import os

import pytest
import torch

from graph_neural_net_amd import _lib
from graph_neural_net_amd.evaluation import (BinnedEvalMeter, BinnedQapMeter, BinnedSeedMeter, BinnedWeightedQapMeter, EvalMeter, QapMeter,
                                             SeedMeter, WeightedQapMeter, decode_scores, decode_scores_weighted, evaluate_scores)
from graph_neural_net_amd.inputs import expand_adjacency
from graph_neural_net_amd.masked import MaskedTensor
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.siamese import Siamese_Node_Exp
from graph_neural_net_amd.wigner import WignerGenerator

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B, N, SMALL, K = 3, 20, 17, 2
NVALID = (N, SMALL, N)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'decode_pinned.json')
TENSOR, METER, BINS = 'a (B, N) seed tensor', 'a fresh seed meter', 'bins= and binned meters'       # placeholders of CONFIGS

CONFIGS = {
    'plain': {},
    'refine2': {'refine': 2},
    'two_opt': {'two_opt': True},
    'faq': {'faq': True},
    'barycenter+two_opt': {'faq': {'P0': 'barycenter'}, 'two_opt': True},
    'faq+refine1+two_opt': {'faq': True, 'refine': 1, 'two_opt': True, 'live': 2},
    'restarts3': {'faq': {'restarts': 3, 'seed': 5}},
    'restarts2+polish': {'faq': {'restarts': 2, 'polish': True}},
    'seeds': {'faq': True, 'two_opt': True, 'seeds': TENSOR},
    'score_seeds+seed_meter': {'faq': True, 'two_opt': True, 'seeds': 'scores', 'seed_meter': METER},
    'restarts2+seeds': {'faq': {'restarts': 2}, 'seeds': TENSOR},
    'bins': {'faq': True, 'two_opt': True, 'seeds': 'scores', 'seed_meter': METER, 'bins': BINS, 'live': 2},
}
# route -> (the data it runs on, the configurations it accepts)
EVERY = tuple(CONFIGS)
NO_BINS = tuple(c for c in CONFIGS if c != 'bins')
ROUTES = {
    'decode_scores': (('bits',), EVERY),
    'decode_scores_weighted': (('float', 'wigner'), EVERY),
    'evaluate_scores_bits': (('bits',), EVERY),
    'evaluate_scores_adj': (('float', 'wigner'), EVERY),
    'match': (('bits',), NO_BINS),
    'match_weighted_flag': (('float', 'wigner'), ('plain', 'refine2')),
    'match_weighted': (('float', 'wigner'), NO_BINS),
}


def _ragged(full, small):
    """pair 1 of `full` replaced by the one pair of `small`, a 17-vertex graph, in the corner of zeros"""
    out = torch.zeros_like(full)
    out[0], out[2] = full[0], full[2]
    out[1][..., :SMALL, :small.shape[-1]] = small[0]
    return out


def _labels(full, small):
    out = full.clone()
    out[1] = -1
    out[1, :SMALL] = small[0]
    return out


def _scores(lab, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    s = torch.randn(B, N, N, generator=g, device=DEV)
    s.scatter_add_(2, lab.long().clamp(0, N - 1)[:, :, None], torch.full((B, N, 1), 4.0, device=DEV))
    return s


def _seeds(lab):
    """every fourth row of the planted matching (past n_b the labels are -1: free)"""
    sd = torch.full((B, N), -1, dtype=torch.int32, device=DEV)
    sd[:, ::4] = lab[:, ::4]
    return sd


def _inputs():
    """-> {'bits' | 'float' | 'wigner': dict(g1, g2, labels, scores, seeds, m1, m2)}, the model"""
    nv = torch.tensor(NVALID, dtype=torch.int32, device=DEV)
    er = dict(edge_density=0.3, noise=0.1, seed=5, device=DEV)
    b1, b2, _, lab = PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', **er).bits(0, B, permute=True)
    c1, c2, _, clab = PairGenerator(SMALL, 'ErdosRenyi', 'ErdosRenyi', **er).bits(1, 1, permute=True)
    b1, b2, lab = _ragged(b1, c1), _ragged(b2, c2), _labels(lab, clab)
    f1, f2 = expand_adjacency(b1, N, nv), expand_adjacency(b2, N, nv)
    w1, w2, _, wlab = WignerGenerator(N, noise=0.2, seed=7, device=DEV).weighted(0, B, permute=True)
    v1, v2, _, vlab = WignerGenerator(SMALL, noise=0.2, seed=7, device=DEV).weighted(1, 1, permute=True)
    w1, w2, wlab = _ragged(w1, v1), _ragged(w2, v2), _labels(wlab, vlab)
    data = {}
    for name, g1, g2, x1, x2, labels, seed in (('bits', b1, b2, f1, f2, lab, 120), ('float', f1, f2, f1, f2, lab, 120),
                                               ('wigner', w1, w2, w1, w2, wlab, 121)):
        data[name] = dict(g1=g1, g2=g2, labels=labels, scores=_scores(labels, seed), seeds=_seeds(labels), nvalid=nv,
                          m1=MaskedTensor(x1, nv, (2, 3), 'N'), m2=MaskedTensor(x2, nv, (2, 3), 'M'))
    torch.manual_seed(3)
    ne = dict(type='node_embedding', block_init='block_emb', block_inside='block', num_blocks=2, in_features=32, out_features=32,
              depth_of_mlp=3, constant_n_vertices=False)
    return data, Siamese_Node_Exp(2, ne).to(DEV)


def _run(route, d, model, config):
    """One call of `route` on the data d -> the dict it returned (a seed meter that `match` does not return is added to it)"""
    kw = dict(CONFIGS[config])
    binned = kw.pop('bins', None) is not None
    live = kw.pop('live', None)
    if kw.get('seeds') is TENSOR:
        kw['seeds'] = d['seeds']
    if kw.get('seed_meter') is METER:
        kw['seed_meter'] = BinnedSeedMeter(DEV, K) if binned else SeedMeter(DEV)
    if route.startswith('match'):
        if route == 'match':
            out = model.match(d['m1'], d['m2'], labels=d['labels'], **kw)
        elif route == 'match_weighted_flag':
            out = model.match(d['m1'], d['m2'], weighted=True, labels=d['labels'], **kw)
        else:
            out = model.match_weighted(d['m1'], d['m2'], labels=d['labels'], **kw)
        if kw.get('seed_meter') is not None:
            out = dict(out, seed_meter=kw['seed_meter'])
        return out
    weighted = not route.endswith('bits') and route != 'decode_scores'
    plain, many = (WeightedQapMeter, BinnedWeightedQapMeter) if weighted else (QapMeter, BinnedQapMeter)
    meter = many(DEV, K) if binned else plain(DEV)
    shared = dict(nvalid=d['nvalid'], labels=d['labels'], live=live, bins=torch.tensor([1, 0, 1], device=DEV) if binned else None, **kw)
    if route == 'decode_scores':
        return decode_scores(d['scores'], d['g1'], d['g2'], meter=meter, **shared)
    if route == 'decode_scores_weighted':
        return decode_scores_weighted(d['scores'], d['g1'], d['g2'], meter=meter, **shared)
    graphs = {'adj' if weighted else 'bits': (d['g1'], d['g2'])}
    return evaluate_scores(d['scores'], meter=BinnedEvalMeter(DEV, K) if binned else EvalMeter(DEV), qap_meter=meter, **graphs, **shared)


def _describe(v):
    """None, [dtype, shape, SHA-256 of the bytes] of a tensor, the dict of a dict, the class, bytes and `refined` of a meter"""
    if v is None:
        return None
    if isinstance(v, MaskedTensor):
        return {'tensor': _describe(v.tensor), 'nvalid': _describe(v.nvalid)}
    if torch.is_tensor(v):
        t = v.detach()
        t = (t.rename(None) if t.has_names() else t).cpu().contiguous()
        return [str(t.dtype), list(t.shape), hashlib.sha256(t.numpy().tobytes()).hexdigest()]
    if isinstance(v, dict):
        return {str(k): _describe(x) for k, x in v.items()}
    if hasattr(v, 'buf'):
        return {'class': type(v).__name__, 'buf': _describe(v.buf), 'refined': getattr(v, 'refined', None)}
    return repr(v)


def record(before=None):
    """Every run of ROUTES x its data x its configurations -> {'route/data/config': {'calls': the names handed to _lib.call, 'out':
    _describe of the returned dict}}.  before: called ahead of every run (the recording of the fixture dirties the allocator there)"""
    data, model = _inputs()
    names, real = [], _lib.call

    def recording(name, *args, **kw):
        names.append(name)
        return real(name, *args, **kw)
    runs = {}
    _lib.call = recording
    try:
        for route, (sets, configs) in ROUTES.items():
            for which in sets:
                for config in configs:
                    if before is not None:
                        before()
                    del names[:]
                    out = _run(route, data[which], model, config)
                    runs['%s/%s/%s' % (route, which, config)] = {'calls': list(names), 'out': _describe(out)}
    finally:
        _lib.call = real
    return runs


def _differences(got, want, at):
    """the places where a described value differs from the fixture's (a tensor whose digest the fixture leaves out: dtype and shape)"""
    if isinstance(want, dict):
        if not isinstance(got, dict) or list(got) != list(want):
            return ['%s: keys %r, recorded %r' % (at, list(got) if isinstance(got, dict) else got, list(want))]
        return [line for k in want for line in _differences(got[k], want[k], '%s[%r]' % (at, k))]
    if isinstance(want, list) and isinstance(got, list):
        got = got[:len(want)]
    return [] if got == want else ['%s: %r, recorded %r' % (at, got, want)]


@pytest.fixture(scope='module')
def runs():
    return record()


@pytest.fixture(scope='module')
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_covers_every_run_and_the_key_sets(recorded):
    want = {'%s/%s/%s' % (r, w, c) for r, (sets, configs) in ROUTES.items() for w in sets for c in configs}
    assert set(recorded) == want
    for name, run in recorded.items():
        route = name.split('/')[0]
        decode = run['out'].get('decode', run['out'])
        if route in ('decode_scores', 'evaluate_scores_bits'):              # the 0/1 route did not gain the weighted route's keys
            assert 'nit' not in decode and 'greedy' not in decode, name
        elif route in ('decode_scores_weighted', 'evaluate_scores_adj'):
            assert 'nit' in decode and 'greedy' in decode, name


@pytest.mark.parametrize('route', list(ROUTES))
def test_the_chain_is_the_recorded_one(route, runs, recorded):
    bad = []
    for name in (n for n in recorded if n.split('/')[0] == route):
        got, want = runs[name], recorded[name]
        if got['calls'] != want['calls']:
            bad.append('%s: launches %r, recorded %r' % (name, got['calls'], want['calls']))
        bad += _differences(got['out'], want['out'], name)
    assert not bad, '\n'.join(bad)
