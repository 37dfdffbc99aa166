"""Price of the cross-entropy against labels in the captured cfg2 training step -- 4 blocks, Regular N = 50 with
ErdosRenyi noise, 32 pairs handed over as bit-packed adjacency, structured block 1, one replayed graph per step -- and of the two score
launches alone.

(a) `plain` = train_step_bits(b1, b2), `labelled` = train_step_bits(b1, b2p, labels=pi) on the relabelled pairs, two trainers from the
same parameters; with --parent-lib also `parent` = the label-less step captured from another build of the library (the parent
commit's): its kernels are recorded into that trainer's graph while the other build is the process's library, the replays need none.
(b) fgnn_score_ce_fwd_blocks / fgnn_score_ce_bwd against their _labels twins on the embeddings of that batch: 20 launches per
captured graph, one replay per call, reported per launch.

Protocol (tools/time_pairgen_indexed.py): device events on one stream, warm-up for every variant (capture included), then WINDOWS
rounds in which the variants take turns with one window of `reps` calls each; per variant the median window and the spread (fastest -
slowest window) of the same run.  A difference below the larger spread is not distinguishable.
usage: python tools/time_ce_labels.py [--reps 200] [--precision fp32|bf16] [--parent-lib lib.so [--parent-first]] [--out file.json]"""
import argparse
import contextlib
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from graph_neural_net_amd import _lib
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.trainer import FgnnTrainer
from time_pairgen_indexed import DEV, WINDOWS, alternate, row

B, N, LAUNCHES = 32, 50, 20


@contextlib.contextmanager
def library(path):
    """make another build the library of _lib.call for the duration (entry points it lacks stay unbound)"""
    lib = C.CDLL(os.path.abspath(path))
    for name, argtypes in _lib._SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argtypes, _lib._RESTYPES.get(name, C.c_int)
    mine = _lib.load()
    _lib._lib = lib
    try:
        yield lib
    finally:
        _lib._lib = mine


def captured(fn):
    """LAUNCHES calls of fn in one graph -> the replay"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(LAUNCHES):
            fn()
    return g.replay


def compare(t, a, b):
    r = row(t)
    r['%s_minus_%s_us' % (a, b)] = round(t[a][0] - t[b][0], 2)
    r['spread_us'] = max(r[a]['spread_us'], r[b]['spread_us'])
    r['distinguishable'] = abs(r['%s_minus_%s_us' % (a, b)]) > r['spread_us']
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--precision', default='fp32', choices=('fp32', 'bf16'))
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--parent-first', action='store_true', help='capture the parent trainer before the other two')
    ap.add_argument('--out', default=None)
    o = ap.parse_args()
    lay = ParamLayout(2, 4, 32, 32, 3)
    p0 = lay.init_flat(0, DEV)
    gen = PairGenerator(N, 'Regular', 'ErdosRenyi', seed=1, device=DEV)
    b1, b2 = gen.bits(0, B)[:2]
    _, b2p, _, lab = gen.bits(0, B, permute=True)
    make = lambda: FgnnTrainer(lay, p0.clone(), lr=1e-3, capture=True, precision=o.precision, block1='structured')
    trainers, steps = {}, {}

    def add(name, fn):
        trainers[name] = make()
        steps[name] = lambda tr=trainers[name]: fn(tr)
        for _ in range(5):                  # capture + a few replays
            steps[name]()
        torch.cuda.synchronize()

    def add_parent():
        with library(o.parent_lib):
            add('parent', lambda tr: tr.train_step_bits(b1, b2))

    if o.parent_lib and o.parent_first:     # (the order of capture is the order in which the trainers' buffers are allocated)
        add_parent()
    add('plain', lambda tr: tr.train_step_bits(b1, b2))
    add('labelled', lambda tr: tr.train_step_bits(b1, b2p, labels=lab))
    if o.parent_lib and not o.parent_first:
        add_parent()
    if o.parent_lib:
        assert torch.equal(trainers['parent'].params, trainers['plain'].params)       # the same step, bit for bit
    torch.cuda.synchronize()
    t = alternate(steps, o.reps)
    assert all(torch.isfinite(tr.params).all().item() for tr in trainers.values())
    step = compare(t, 'labelled', 'plain')
    if o.parent_lib:
        step['plain_minus_parent_us'] = round(t['plain'][0] - t['parent'][0], 2)
        step['parent_spread_us'] = max(step['plain']['spread_us'], step['parent']['spread_us'])
    print('  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)

    # (b) the two score launches alone, on the embeddings the label-less step left in its engine
    eng = trainers['plain']._engine(2 * B, N, False)
    e1, e2 = eng.E[:B].clone(), eng.E[B:].clone()
    f32 = dict(dtype=torch.float32, device=DEV)
    s, lse, pl = torch.empty(B, N, N, **f32), torch.empty(B, N, **f32), torch.empty(B * eng.score_blocks, **f32)
    d1, d2, gs = torch.empty(B, 32, N, **f32), torch.empty(B, 32, N, **f32), torch.full((1,), 1.0 / (B * N), **f32)
    P = _lib.ptr
    launches = {
        'fwd': lambda: _lib.call('fgnn_score_ce_fwd_blocks', P(e1), P(e2), None, B, 32, N, eng.score_blocks, P(s), P(lse), P(pl), _lib.stream_ptr()),
        'fwd_labels': lambda: _lib.call('fgnn_score_ce_fwd_blocks_labels', P(e1), P(e2), None, P(lab), B, 32, N, eng.score_blocks, P(s), P(lse),
                                        P(pl), _lib.stream_ptr()),
        'bwd': lambda: _lib.call('fgnn_score_ce_bwd', P(e1), P(e2), P(s), P(lse), None, P(gs), B, 32, N, P(d1), P(d2), _lib.stream_ptr()),
        'bwd_labels': lambda: _lib.call('fgnn_score_ce_bwd_labels', P(e1), P(e2), P(s), P(lse), None, P(lab), P(gs), B, 32, N, P(d1), P(d2),
                                        _lib.stream_ptr()),
    }
    tk = alternate({k: captured(fn) for k, fn in launches.items()}, max(1, o.reps // 4))
    tk = {k: tuple(v / LAUNCHES for v in t3) for k, t3 in tk.items()}
    kern = {'fwd': compare({k: tk[k] for k in ('fwd', 'fwd_labels')}, 'fwd_labels', 'fwd'),
            'bwd': compare({k: tk[k] for k in ('bwd', 'bwd_labels')}, 'bwd_labels', 'bwd')}
    print('  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + tk[k]) for k in tk), flush=True)
    res = {'tool': 'time_ce_labels', 'reps': o.reps, 'windows': WINDOWS, 'precision': o.precision, 'pairs': B, 'n_vertices': N,
           'parent_lib': bool(o.parent_lib), 'parent_first': bool(o.parent_first), 'cfg2_captured_step': step, 'score_launches': kern}
    line = json.dumps(res)
    print(line)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
