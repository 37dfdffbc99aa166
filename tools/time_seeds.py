"""Price of seeds (qap.faq(seeds=), csrc/qap_seeds.hip) on the shapes of the README's QAP table: Regular N = 50 and N = 200 with
ErdosRenyi noise 0.1, 32 relabelled pairs as bit-packed adjacency (seed 1), 8 seeds per pair revealed from the planted labels.

(a) the seeded chain against the unseeded one (qap.faq with and without seeds=; the seeded one works on u = N - 8 vertices and pays
    the set-up launches), with the default tol and with a tol no pair meets;
(b) the three set-up launches alone: fgnn_seed_index, fgnn_seed_gather (one of A22 / B22), fgnn_seed_const;
(c) the four solver entry points -- qap.faq and qap.two_opt, each without and with seeds= -- of THIS library and, with
    --parent-lib, of the parent commit's build: each build is then timed in a fresh process of its own (the parent's loaded
    through FGNN_LIB) that runs nothing but these windows, so that both meet the same allocator and runtime state.  Per variant
    `vs_parent` holds this library's median minus the parent's beside the larger of the two spreads: a median further above the
    parent's than that margin is a regression;
(d) quality: free vertices recovered with and without the seeds.

Protocol (tools/time_pairgen_indexed.py): device events on one stream, warm-up, then WINDOWS = 7 rounds in which the variants take
turns with one window of `reps` calls each; reported per variant: the median window and the spread of the same run.
usage: python tools/time_seeds.py [--reps 5] [--sizes 50,200] [--parent-lib path/to/libfgnn_hip.so] [--out profiles/seeds_time.json]"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from graph_neural_net_amd import _lib

B, SEEDS = 32, 8
NEVER = 1e-30             # a tol no pair meets


def pairs_of(N):
    from graph_neural_net_amd.pairgen import PairGenerator
    from time_pairgen_indexed import DEV
    gen = PairGenerator(N, 'Regular', 'ErdosRenyi', noise=0.1, seed=1, device=DEV)
    return gen.bits(0, B, permute=True)


def solvers(N, reps):
    """leg (c): qap.faq and qap.two_opt without and with seeds=, the seeded two_opt from the seeded faq's matching"""
    from graph_neural_net_amd import planted, qap
    from time_pairgen_indexed import alternate, row
    b1, b2, _, labels = pairs_of(N)
    seeds = planted.reveal_seeds(labels, None, SEEDS, seed=1)
    start, start_seeded = qap.faq(b1, b2)['perm'], qap.faq(b1, b2, seeds=seeds)['perm']
    return row(alternate({'faq': lambda: qap.faq(b1, b2), 'two_opt': lambda: qap.two_opt(b1, b2, start),
                          'faq_seeded': lambda: qap.faq(b1, b2, seeds=seeds),
                          'two_opt_seeded': lambda: qap.two_opt(b1, b2, start_seeded, seeds=seeds)}, reps))


def one_size(N, reps):
    from graph_neural_net_amd import planted, qap
    from time_pairgen_indexed import DEV, alternate, row
    b1, b2, _, labels = pairs_of(N)
    seeds = planted.reveal_seeds(labels, None, SEEDS, seed=1)
    free = seeds < 0
    plain, seeded = qap.faq(b1, b2, labels=labels), qap.faq(b1, b2, labels=labels, seeds=seeds)
    assert int(seeded['status'].max()) < 2 and bool((seeded['perm'][~free] == seeds[~free]).all())
    quality = {'free_recovered_unseeded': float(((plain['perm'] == labels) & free).sum()) / float(free.sum()),
               'free_recovered_seeded': float(((seeded['perm'] == labels) & free).sum()) / float(free.sum()),
               'nit_unseeded': float(plain['nit'].double().mean()), 'nit_seeded': float(seeded['nit'].double().mean())}
    x = torch.empty(2, B, 2, N, N, dtype=torch.float32, device=DEV)
    for side, bits in enumerate((b1, b2)):
        _lib.call('fgnn_expand_adjacency', _lib.ptr(bits), None, B, N, _lib.ptr(x[side]), _lib.stream_ptr())
    ix = qap.seed_index_device(seeds, None)
    C = torch.empty(B, N, N, dtype=torch.float32, device=DEV)

    def const():
        _lib.call('fgnn_seed_const', _lib.ptr(x[0]), _lib.ptr(x[1]), 2 * N * N, N, _lib.ptr(ix['free_a']), _lib.ptr(ix['free_b']),
                  _lib.ptr(ix['seed_a']), _lib.ptr(ix['seed_b']), _lib.ptr(ix['nfree']), _lib.ptr(ix['nseed']), B, N, _lib.ptr(C),
                  _lib.stream_ptr())

    t = alternate({'faq': lambda: qap.faq(b1, b2), 'faq_seeded': lambda: qap.faq(b1, b2, seeds=seeds),
                   'faq_30_rounds': lambda: qap.faq(b1, b2, tol=NEVER), 'faq_seeded_30_rounds': lambda: qap.faq(b1, b2, tol=NEVER, seeds=seeds),
                   'seed_index': lambda: qap.seed_index_device(seeds, None),
                   'seed_gather': lambda: qap.seed_gather_device(x[0][:, 0], ix['free_a'], ix['free_a'], ix['nfree']),
                   'seed_const': const}, reps)
    print('N %d  ' % N + '  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
    print('N %d  quality %s' % (N, json.dumps(quality)), flush=True)
    return {'n_vertices': N, 'pairs': B, 'seeds': SEEDS, 'reps': reps, 'times': row(t), 'quality': quality}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sizes', default='50,200')
    ap.add_argument('--parent-lib', default=None, help="the parent commit's libfgnn_hip.so, for leg (c)")
    ap.add_argument('--solvers-only', action='store_true', help='leg (c) of the library FGNN_LIB names; prints one JSON line')
    ap.add_argument('--out', default=None)
    o = ap.parse_args()
    sizes = list(map(int, o.sizes.split(',')))
    reps = {n: o.reps if n <= 64 else max(2, o.reps // 2) for n in sizes}
    if o.solvers_only:
        _lib.load(allow_missing=True)
        print(json.dumps({str(n): solvers(n, reps[n]) for n in sizes}))
        return
    from time_pairgen_indexed import WINDOWS
    res = {'tool': 'time_seeds', 'windows': WINDOWS, 'sizes': []}
    for n in sizes:
        res['sizes'].append(one_size(n, reps[n]))
        res['sizes'][-1]['solvers_this_library'] = solvers(n, reps[n])
    if o.parent_lib:                 # fresh processes: a library is loaded once per process, and both builds meet the same conditions
        def fresh(lib):
            cmd = [sys.executable, os.path.abspath(__file__), '--solvers-only', '--reps', str(o.reps), '--sizes', o.sizes]
            env = dict(os.environ, FGNN_LIB=os.path.abspath(lib)) if lib else {k: v for k, v in os.environ.items() if k != 'FGNN_LIB'}
            out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True)
            return json.loads(out.stdout.strip().splitlines()[-1])

        this, parent = fresh(None), fresh(o.parent_lib)
        for s in res['sizes']:
            ours, theirs = this[str(s['n_vertices'])], parent[str(s['n_vertices'])]
            s['solvers_this_library'], s['solvers_parent_library'] = ours, theirs
            s['vs_parent'] = {k: {'delta_us': round(ours[k]['us'] - theirs[k]['us'], 2),
                                  'margin_us': max(ours[k]['spread_us'], theirs[k]['spread_us'])} for k in ours}
            for v in s['vs_parent'].values():
                v['within'] = v['delta_us'] <= v['margin_us']
    line = json.dumps(res)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
