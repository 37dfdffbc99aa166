"""Price and quality of random restarts for FAQ (qap.faq(restarts=R), csrc/qap_restarts.hip) on the shapes of the README's QAP table:
Regular N = 50 and N = 200 with ErdosRenyi noise 0.1, 32 relabelled pairs as bit-packed adjacency (seed 1, permute=True).

(a) the start launch alone (fgnn_faq_restart_starts, barycenter base) at R = 2, 4, 8;
(b) qap.faq(restarts=R) at R = 1, 2, 4, 8 against R sequential single-start calls of the same library -- faq(P0=starts[:, k]), the
    starts made beforehand, so the sequential side is not charged for them: the claim under test is that R starts in one chain cost
    far less than R chains, because one chain leaves most of the device idle;
(c) restarts=1 against the parent commit's library (--parent-lib, the same Python driving both): the single path did not move;
(d) the QAP ratio (objective of the found matching over the planted one, mean over the pairs) and the accuracy at each R, without
    and with polish=True, and how often a restart k >= 1 won.

Protocol (tools/time_pairgen_indexed.py): device events on one stream, warm-up, then WINDOWS = 7 rounds in which the variants take
turns with one window of `reps` calls each; reported per variant: the median window and the spread of the same run.
usage: python tools/time_restarts.py [--reps 3] [--sizes 50,200] [--parent-lib lib.so] [--out profiles/restarts_time.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from graph_neural_net_amd import _lib, qap
from graph_neural_net_amd.pairgen import PairGenerator
from time_pairgen_indexed import DEV, WINDOWS, alternate, row

B = 32
RS = (1, 2, 4, 8)
SEED = 1


def load_parent(path):
    """an older build of the library, bound like _lib.load() binds the current one (entry points it lacks stay unbound)"""
    lib = C.CDLL(os.path.abspath(path))
    for name, argtypes in _lib._SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argtypes, _lib._RESTYPES.get(name, C.c_int)
    return lib


def through(lib, fn):
    """fn with every _lib.call going to `lib`"""
    def run():
        own, _lib._lib = _lib._lib, lib
        try:
            return fn()
        finally:
            _lib._lib = own
    return run


def ratio(q, planted):
    return float((q.double() / planted.double()).mean())


def one_size(N, reps, parent):
    gen = PairGenerator(N, 'Regular', 'ErdosRenyi', noise=0.1, seed=1, device=DEV)
    b1, b2, _, lab = gen.bits(0, B, permute=True)
    planted = qap.objective_bits(b1, b2, lab, None)['qap']
    quality = {}
    for R in RS:
        for polish in (False, True):
            out = qap.faq(b1, b2, labels=lab, restarts=R, seed=SEED, polish=polish)
            quality['R%d%s' % (R, '_polish' if polish else '')] = {
                'qap_ratio': ratio(out['qap'], planted), 'acc': float(out['acc'].double().mean()) / N,
                'later_restart_won': int((out['restart'] > 0).sum()) if 'restart' in out else 0}
    starts = {R: qap.random_starts(B, N, R, seed=SEED, device=DEV) for R in RS}

    def sequential(R):
        def run():
            for k in range(R):
                qap.faq(b1, b2, P0=starts[R][:, k])
        return run

    variants = {}
    for R in RS[1:]:
        variants['starts_R%d' % R] = lambda R=R: qap.random_starts_device(None, None, None, SEED, B, N, R, DEV)
    for R in RS:
        variants['faq_R%d' % R] = lambda R=R: qap.faq(b1, b2, restarts=R, seed=SEED)
        if R > 1:
            variants['sequential_R%d' % R] = sequential(R)
            variants['faq_R%d_polish' % R] = lambda R=R: qap.faq(b1, b2, restarts=R, seed=SEED, polish=True)
    if parent is not None:
        variants['faq_R1_parent_lib'] = through(parent, lambda: qap.faq(b1, b2))
    t = alternate(variants, reps)
    res = {'n_vertices': N, 'pairs': B, 'reps': reps, 'times': row(t), 'quality': quality,
           'restarted_over_sequential': {'R%d' % R: round(t['faq_R%d' % R][0] / t['sequential_R%d' % R][0], 3) for R in RS[1:]},
           'restarted_over_single': {'R%d' % R: round(t['faq_R%d' % R][0] / t['faq_R1'][0], 3) for R in RS[1:]}}
    if parent is not None:
        res['single_minus_parent_us'] = round(t['faq_R1'][0] - t['faq_R1_parent_lib'][0], 2)
    print('N %d  ' % N + '  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
    print('N %d  quality %s' % (N, json.dumps(quality)), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--sizes', default='50,200')
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=None)
    o = ap.parse_args()
    _lib.load()
    parent = load_parent(o.parent_lib) if o.parent_lib else None
    res = {'tool': 'time_restarts', 'windows': WINDOWS, 'parent_lib': bool(parent), 'sizes': []}
    for n in map(int, o.sizes.split(',')):          # (the file is rewritten after every size: a long run leaves what it finished)
        res['sizes'].append(one_size(n, o.reps if n <= 64 else max(1, o.reps // 2), parent))
        line = json.dumps(res)
        if o.out:
            os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
            with open(o.out, 'w') as f:
                f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
