"""Price of the pairwise-exchange search (qap.two_opt_bits, csrc/qap_2opt.hip) at the end of the decode chain, on the cfg2 shape
(4 blocks, Regular N = 50 with ErdosRenyi noise 0.1, 32 pairs as bit-packed adjacency, structured block 1) and at N = 200 (generic
block 1).  The start is the Hungarian matching of the scores of a model with initial parameters.

(a) the fgnn_qap_2opt launch alone on that matching, beside one round of greedy_qap (the difference of T = 11 and T = 1, over 10);
(b) `eval_step_bits(qap_meter=...)` alone, with two_opt=True, with refine=10, with both;
(c) the host loop: scipy.optimize.quadratic_assignment(method='2opt') on the first --scipy-pairs pairs, seconds per pair.  At N = 200
    one SciPy search takes minutes, so there the figure is SciPy's own evaluation (`_calc_score`) timed on the pair, times the
    evaluation count nit the kernel reports for it (nit is SciPy's count; tests hold it to SciPy) -- marked "estimated";
(d) the distribution of the exchanges per pair, and the QAP ratio of the chains on the same pairs.

Protocol (tools/time_pairgen_indexed.py): device events on one stream, warm-up, then WINDOWS rounds in which the variants take turns
with one window of `reps` calls each; reported per variant: the median window and the spread of the same run.
usage: python tools/time_two_opt.py [--reps 20] [--sizes 50,200] [--scipy-pairs 4] [--out profiles/two_opt_time.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from graph_neural_net_amd import _lib, qap
from graph_neural_net_amd.engine import ParamLayout
from graph_neural_net_amd.evaluation import EvalMeter, QapMeter
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.trainer import FgnnTrainer
from time_pairgen_indexed import DEV, WINDOWS, alternate, row

B = 32
REFINE = 10


def unpack(words, n):
    w = words.cpu().numpy().view(np.uint32)
    return np.unpackbits(w.view(np.uint8), axis=-1, bitorder='little')[..., :n, :n].astype(np.int64)


def scipy_leg(b1, b2, assign, nit, pairs, N):
    from scipy.optimize import _qap, quadratic_assignment
    A, Bm, starts = unpack(b1[:pairs], N), unpack(b2[:pairs], N), assign[:pairs].cpu().numpy().astype(np.int64)
    if N <= 64:
        t0 = time.perf_counter()
        for b in range(pairs):
            res = quadratic_assignment(A[b], Bm[b], method='2opt',
                                       options={'maximize': True, 'partial_guess': np.stack([np.arange(N), starts[b]], 1)})
            assert int(res.nit) == int(nit[b]), 'the kernel does not count the evaluations SciPy makes'
        return {'seconds_per_pair': round((time.perf_counter() - t0) / pairs, 4), 'pairs': pairs, 'estimated': False}
    evals = 2000
    t0 = time.perf_counter()
    for _ in range(evals):
        _qap._calc_score(A[0], Bm[0], starts[0])
    per = (time.perf_counter() - t0) / evals
    return {'seconds_per_pair': round(per * float(nit[:pairs].double().mean()), 2), 'pairs': pairs, 'estimated': True,
            'seconds_per_evaluation': per}


def one_size(N, reps, scipy_pairs):
    lay = ParamLayout(2, 4, 32, 32, 3)
    gen = PairGenerator(N, 'Regular', 'ErdosRenyi', noise=0.1, seed=1, device=DEV)
    b1, b2 = gen.bits(0, B)[:2]
    tr = FgnnTrainer(lay, lay.init_flat(0, DEV), lr=1e-3, capture=True, block1='structured' if N == 50 else None)
    meter = EvalMeter(DEV)
    chains = {'decode': {}, 'decode_two_opt': {'two_opt': True}, 'decode_refine': {'refine': REFINE},
              'decode_refine_two_opt': {'refine': REFINE, 'two_opt': True}}
    meters = {k: QapMeter(DEV) for k in chains}
    steps = {k: (lambda k=k: tr.eval_step_bits(b1, b2, meter=meter, qap_meter=meters[k], **chains[k])) for k in chains}
    # (d) one pass of every chain over the same pairs, read before the timing adds to the meters
    outs = {k: fn() for k, fn in steps.items()}
    ratios = {}
    for k, m in meters.items():
        r = m.result()
        ratios[k] = {'qap_ratio': r['qap_ratio'], 'final_qap_ratio': r.get('refined_qap_ratio', r['qap_ratio']),
                     'acc': r['acc'], 'final_acc': r.get('refined_acc', r['acc'])}
    swaps = {k: outs[k]['decode']['swaps'].cpu().tolist() for k in ('decode_two_opt', 'decode_refine_two_opt')}
    assert all(int(outs[k]['decode']['status'].max()) == 0 for k in swaps)
    dist = {k: {'min': min(v), 'median': statistics.median(v), 'mean': round(sum(v) / len(v), 2), 'max': max(v)} for k, v in swaps.items()}
    tb = alternate(steps, reps)
    # (a) the launch alone, from the Hungarian matching
    assign = outs['decode']['decode']['assign'].clone()
    perm = torch.empty(B, N, dtype=torch.int32, device=DEV)
    o32 = torch.empty(3, B, dtype=torch.int32, device=DEV)
    nit = torch.empty(B, dtype=torch.int64, device=DEV)

    def launch():
        _lib.call('fgnn_qap_2opt', _lib.ptr(b1), _lib.ptr(b2), _lib.ptr(assign), None, B, N, -1, _lib.ptr(perm), _lib.ptr(o32[0]),
                  _lib.ptr(o32[1]), _lib.ptr(nit), _lib.ptr(o32[2]), _lib.stream_ptr())
    ta = alternate({'two_opt_launch': launch, 'greedy_T1': lambda: qap.greedy_bits(b1, b2, assign, 1, None, raw=True),
                    'greedy_T11': lambda: qap.greedy_bits(b1, b2, assign, 11, None, raw=True)}, reps)
    res = {'n_vertices': N, 'pairs': B, 'reps': reps, 'launch': row(ta), 'steps': row(tb),
           'greedy_round_us': round((ta['greedy_T11'][0] - ta['greedy_T1'][0]) / 10, 2),
           'two_opt_minus_decode_us': round(tb['decode_two_opt'][0] - tb['decode'][0], 2),
           'refine_minus_decode_us': round(tb['decode_refine'][0] - tb['decode'][0], 2),
           'refine_two_opt_minus_refine_us': round(tb['decode_refine_two_opt'][0] - tb['decode_refine'][0], 2),
           'swaps': dist, 'nit_mean': float(nit.double().mean()), 'chains': ratios,
           'scipy': scipy_leg(b1, b2, assign, nit, scipy_pairs, N)}
    for t in (ta, tb):
        print('N %d  ' % N + '  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sizes', default='50,200')
    ap.add_argument('--scipy-pairs', type=int, default=4)
    ap.add_argument('--out', default=None)
    o = ap.parse_args()
    res = {'tool': 'time_two_opt', 'windows': WINDOWS, 'refine': REFINE, 'sizes': []}
    for n in map(int, o.sizes.split(',')):          # (the file is rewritten after every size: a long run leaves what it finished)
        res['sizes'].append(one_size(n, o.reps if n <= 64 else max(2, o.reps // 4), o.scipy_pairs))
        line = json.dumps(res)
        if o.out:
            os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
            with open(o.out, 'w') as f:
                f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
