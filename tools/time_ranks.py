"""Price of the rank metrics (evaluation.rank_scores, csrc/rank.hip) on the cfg2 shape: 4 blocks, Regular N = 50 with ErdosRenyi
noise, 32 pairs handed over as bit-packed adjacency, structured block 1.

(a) fgnn_eval_ranks + fgnn_rank_fold on a batch of scores against the torch composition that gives the same integers: gather of the
    target score, the comparisons of the beats rule, sum(-1), reciprocal, the per-pair sums and the add into an epoch vector.
(b) `eval_step_bits(hungarian=False)` with and without `rank_meter=`, and -- with --parent-root, the root of a built checkout of
    the parent commit -- that checkout's `eval_step_bits(hungarian=False)` in the same process, taking turns with the other two.

Protocol (tools/time_pairgen_indexed.py): device events on one stream, warm-up, then WINDOWS rounds in which the variants take turns
with one window of `reps` calls each; reported per variant: the median window and the spread (fastest - slowest window) of the same
run.  `exceeds_spread` says whether the added cost is larger than the larger of the two spreads.
usage: python tools/time_ranks.py [--reps 100] [--precision fp32|bf16] [--parent-root DIR] [--out file.json]"""
import argparse
import ctypes
import importlib
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from graph_neural_net_amd import _lib
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.evaluation import EvalMeter, RankMeter, rank_scores
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.trainer import FgnnTrainer
from time_pairgen_indexed import DEV, WINDOWS, alternate, row

B, N = 32, 50
KS = (1, 5, 10)


def added(t, new, old):
    r = row(t)
    r['%s_minus_%s_us' % (new, old)] = round(t[new][0] - t[old][0], 2)
    r['spread_us'] = max(r[new]['spread_us'], r[old]['spread_us'])
    r['exceeds_spread'] = abs(t[new][0] - t[old][0]) > r['spread_us']
    return r


def parent_package(root):
    """the package of another checkout under a name of its own (it imports itself relatively and loads the library next to it)"""
    pkg = os.path.join(os.path.abspath(root), 'graph_neural_net_amd')
    spec = importlib.util.spec_from_file_location('fgnn_parent', os.path.join(pkg, '__init__.py'), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules['fgnn_parent'] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--precision', default='fp32', choices=('fp32', 'bf16'))
    ap.add_argument('--parent-root', default=None)
    ap.add_argument('--out', default=None)
    o = ap.parse_args()
    lay = ParamLayout(2, 4, 32, 32, 3)
    p0 = lay.init_flat(0, DEV)
    gen = PairGenerator(N, 'Regular', 'ErdosRenyi', seed=1, device=DEV)
    b1, b2 = gen.bits(0, B)[:2]
    tr = FgnnTrainer(lay, p0.clone(), lr=1e-3, capture=True, precision=o.precision, block1='structured')
    meter, rmeter = EvalMeter(DEV), RankMeter(DEV, ks=KS)
    steps = {'eval_step_bits_ranks': lambda: tr.eval_step_bits(b1, b2, meter=meter, hungarian=False, rank_meter=rmeter),
             'eval_step_bits': lambda: tr.eval_step_bits(b1, b2, meter=meter, hungarian=False)}
    if o.parent_root:
        parent_package(o.parent_root)
        ptrainer, pengine, peval = (importlib.import_module('fgnn_parent.' + m) for m in ('trainer', 'engine', 'evaluation'))
        assert not hasattr(peval, 'RankMeter'), 'the parent checkout already has the rank metrics'
        par = ptrainer.FgnnTrainer(pengine.ParamLayout(2, 4, 32, 32, 3), p0.clone(), lr=1e-3, capture=True, precision=o.precision,
                                   block1='structured')
        pmeter = peval.EvalMeter(DEV)
        steps['parent_eval_step_bits'] = lambda: par.eval_step_bits(b1, b2, meter=pmeter, hungarian=False)
    for _ in range(5):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()
    ta = alternate(steps, o.reps)
    assert rmeter.result()['pairs'] > 0 and meter.result()['pairs'] > 0

    scores = tr._engine(2 * B, N, False).scores.clone()
    nvalid = torch.full((B,), N, dtype=torch.int32, device=DEV)
    rank = torch.empty(B, N, dtype=torch.int32, device=DEV)
    hits = torch.empty(B, len(KS), dtype=torch.int32, device=DEV)
    rr = torch.empty(B, dtype=torch.float64, device=DEV)
    rank_sum = torch.empty(B, dtype=torch.int64, device=DEV)
    targets = torch.empty(B, dtype=torch.int32, device=DEV)
    ks_c = (ctypes.c_int * len(KS))(*KS)
    ks_t = torch.tensor(KS, device=DEV)
    tgt = torch.arange(N, device=DEV)[None, :, None].expand(B, N, 1).contiguous()
    first = torch.arange(N, device=DEV)[None, None, :] < tgt
    epoch = torch.zeros(3 + len(KS), dtype=torch.float64, device=DEV)

    def new():
        st = _lib.stream_ptr()
        _lib.call('fgnn_eval_ranks', _lib.ptr(scores), N * N, N, _lib.ptr(nvalid), None, B, N, _lib.ptr(rank), st)
        _lib.call('fgnn_rank_fold', _lib.ptr(rank), _lib.ptr(nvalid), B, N, B, ks_c, len(KS), None, 1, _lib.ptr(hits), _lib.ptr(rr),
                  _lib.ptr(rank_sum), _lib.ptr(targets), _lib.ptr(rmeter.buf), st)

    def torch_chain():
        st_ = scores.gather(2, tgt)
        vnan, tnan = torch.isnan(scores), torch.isnan(st_)
        beats = torch.where(tnan, vnan & first, vnan | (scores > st_) | ((scores == st_) & first))
        r = 1 + beats.sum(-1)
        h = (r[:, :, None] <= ks_t).sum(1)
        pr = r.to(torch.float64).reciprocal().sum(1)
        epoch.add_(torch.cat([pr.sum().reshape(1), r.sum().reshape(1).double(), h.sum(0).double(), r.new_tensor([B * N]).double()]))
        return r, h, pr

    new()
    r_t, h_t, _ = torch_chain()
    assert torch.equal(rank.long(), r_t) and torch.equal(hits.long(), h_t), 'the two sides do not give the same integers'
    out = rank_scores(scores, ks=KS)
    assert torch.equal(out['rank'], rank)
    tb = alternate({'eval_ranks_fold': new, 'torch_chain': torch_chain}, o.reps)
    res = {'tool': 'time_ranks', 'reps': o.reps, 'windows': WINDOWS, 'precision': o.precision, 'pairs': B, 'n_vertices': N, 'ks': KS,
           'step': added(ta, 'eval_step_bits_ranks', 'eval_step_bits'), 'kernels': added(tb, 'eval_ranks_fold', 'torch_chain')}
    if o.parent_root:
        res['step_vs_parent'] = {k: v for k, v in added(ta, 'eval_step_bits', 'parent_eval_step_bits').items()
                                 if k in ('eval_step_bits_minus_parent_eval_step_bits_us', 'spread_us', 'exceeds_spread')}
    for t in (ta, tb):
        print('  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
    line = json.dumps(res)
    print(line)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
