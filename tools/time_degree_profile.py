"""Price and quality of degree-profile matching (qap.degree_profile, csrc/degree_profile.hip): 32 relabelled pairs, N = 50 and 200,
weighted Wigner pairs (``WignerGenerator(N, noise=0.2, seed=1).weighted(0, 32, permute=True)``, the pairs of tools/time_grampa.py) and
0/1 pairs (``PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=0.02, seed=1).bits(0, 32, permute=True)``).

(a) the whole chain through ``qap.degree_profile``, objective and count included, and the five launches of the entry point alone
    (``qap.degree_profile_device``); beside them the launch floor: the same five launches with every corner cut to 1 vertex (status
    2: no kernel does any work);
(b) the distance launch alone.  No entry point issues it by itself, so its time comes from a kernel trace taken in a run of its
    own: ``rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/time_degree_profile.py --trace weighted:200`` runs nothing but
    20 chains of that one case, and ``--merge-stats weighted:200=DIR/kt_results.db --out FILE`` writes the per-kernel averages of the
    dp_* kernels, the solver, the objective and the count into the JSON under `kernel_trace`;
(c) a torch composition of the same matrix on the device: weighted, sort and the equal-length L1 (``torch.cdist(p=1) / (n - 1)``);
    0/1, per pair the pooled sort of the two padded profile slabs and sum |F - G| dx with ``torch.searchsorted`` -- timed from the
    inputs (weighted) resp. from the device's own profiles (0/1), and compared with the chain's X;
(d) ``qap.grampa`` at its defaults on the same pairs;
(e) recovered pairs (every row right) and rows of the 32 pairs at s = 0 / 0.2 / 0.4 / 0.6 (Wigner noise; for the 0/1 pairs the
    generator's edge noise), degree profile next to GRAMPA.

No existing source file is compiled differently by the change that added this tool, so there is no parent-library leg.
Protocol (tools/time_pairgen_indexed.py): device events on one stream, warm-up, then WINDOWS = 7 rounds in which the variants take
turns with one window of `reps` calls each; reported per variant: the median window and the spread of the same run.
usage: python tools/time_degree_profile.py [--reps 3] [--sizes 50,200] [--out profiles/degree_profile_time.json]"""
import argparse
import json
import os
import sqlite3
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from graph_neural_net_amd import qap

B = 32
NOISES = (0.0, 0.2, 0.4, 0.6)
KINDS = ('weighted', 'bits')


def pairs(kind, N, noise, dev):
    from graph_neural_net_amd.pairgen import PairGenerator
    from graph_neural_net_amd.wigner import WignerGenerator
    if kind == 'weighted':
        return WignerGenerator(N, noise=noise, seed=1, device=dev).weighted(0, B, permute=True)
    return PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.3, noise=noise, seed=1, device=dev).bits(0, B, permute=True)


def torch_weighted(a, b):
    """(B, n, n) fp32 matrices -> -Z: the off-diagonal entries of every row sorted, the mean |a_(k) - b_(k)| of every two rows"""
    n = a.shape[-1]
    eye = torch.eye(n, dtype=torch.bool, device=a.device)
    pa = a.masked_fill(eye, float('inf')).sort(-1).values[..., :n - 1]
    pb = b.masked_fill(eye, float('inf')).sort(-1).values[..., :n - 1]
    return -torch.cdist(pa, pb, p=1) / (n - 1)


def torch_w1_padded(P1, c1, P2, c2):
    """+inf-padded sorted profile slabs (B, n, n) and their counts (B, n) -> -Z, pair by pair: int |F - G| dx over the pooled values"""
    out = []
    for a, ma, b, mb in zip(P1, c1, P2, c2):
        n, w = a.shape
        a, b = a.clone(), b.clone()
        a[ma == 0, 0], b[mb == 0, 0] = 0.0, 0.0                             # an empty profile is the point mass at 0
        ma, mb = ma.clamp(min=1).float(), mb.clamp(min=1).float()
        ae, be = a[:, None, :].expand(n, n, w).contiguous(), b[None, :, :].expand(n, n, w).contiguous()
        x = torch.cat([ae, be], -1).sort(-1).values
        F = torch.searchsorted(ae, x[..., :-1].contiguous(), right=True).float().clamp(max=ma[:, None, None]) / ma[:, None, None]
        G = torch.searchsorted(be, x[..., :-1].contiguous(), right=True).float().clamp(max=mb[None, :, None]) / mb[None, :, None]
        dx = torch.where(torch.isfinite(x[..., 1:]), x[..., 1:] - x[..., :-1], torch.zeros_like(x[..., 1:]))
        out.append(-((F - G).abs() * dx).sum(-1))
    return torch.stack(out)


def recovery(kind, N, dev):
    out = {}
    for s in NOISES:
        x1, x2, nv, lab = pairs(kind, N, s, dev)
        kw = dict(nvalid=nv, labels=lab, weighted=kind == 'weighted')
        d, g = qap.degree_profile(x1, x2, **kw), qap.grampa(x1, x2, **kw)
        out['s%g' % s] = {'degree_profile_recovered_pairs': int((d['acc'] == N).sum()),
                          'degree_profile_acc': float(d['acc'].double().mean()) / N,
                          'grampa_recovered_pairs': int((g['acc'] == N).sum()), 'grampa_acc': float(g['acc'].double().mean()) / N,
                          'degree_profile_status_0': int((d['status'] == 0).sum())}
    return out


def one_case(kind, N, reps):
    from time_pairgen_indexed import DEV, alternate, row
    weighted = kind == 'weighted'
    x1, x2, nv, lab = pairs(kind, N, 0.2 if weighted else 0.02, DEV)
    kw = dict(nvalid=nv, labels=lab, weighted=weighted)
    one = torch.ones(B, dtype=torch.int32, device=DEV)
    nv32 = None if nv is None else nv.to(torch.int32)
    src = {'weighted': qap.weighted_views(x1, x2)} if weighted else {'bits': (x1, x2)}
    full = qap.degree_profile(x1, x2, return_profiles=True, **kw)
    if weighted:
        a, b = x1[:, 0].contiguous(), x2[:, 0].contiguous()
        compose = lambda: torch_weighted(a, b)
    else:
        compose = lambda: torch_w1_padded(full['profiles'][0], full['counts'][:, 0], full['profiles'][1], full['counts'][:, 1])
    ref = compose()
    diff = float(((full['X'] - ref).abs().amax((1, 2)) / ref.abs().amax((1, 2))).max())
    t = alternate({'chain': lambda: qap.degree_profile(x1, x2, **kw),
                   'entry_point_5_launches': lambda: qap.degree_profile_device(B, N, DEV, nv32, **src),
                   'floor_5_launches': lambda: qap.degree_profile_device(B, N, DEV, one, **src),
                   'torch_composition': compose,
                   'grampa_chain': lambda: qap.grampa(x1, x2, **kw)}, reps)
    res = {'input': kind, 'n_vertices': N, 'pairs': B, 'reps': reps, 'times': row(t),
           'torch_composition_max_rel_diff_to_chain': diff, 'mean_profile_length': float(full['counts'].double().mean()),
           'recovery': recovery(kind, N, DEV)}
    print('%s N %d  ' % (kind, N) + '  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
    print('%s N %d  %s' % (kind, N, json.dumps({k: res[k] for k in ('torch_composition_max_rel_diff_to_chain', 'recovery')})), flush=True)
    return res


def trace(case):
    """nothing but 20 chains of one case, for a kernel trace"""
    from time_pairgen_indexed import DEV
    kind, N = case.split(':')
    x1, x2, nv, lab = pairs(kind, int(N), 0.2 if kind == 'weighted' else 0.02, DEV)
    for _ in range(20):
        qap.degree_profile(x1, x2, nvalid=nv, labels=lab, weighted=kind == 'weighted')
    torch.cuda.synchronize()


def kernel_stats(path):
    """the rows of the `top_kernels` view of a rocprofv3 database (kt_results.db) for the chain's kernels -> {kernel: {'calls',
    'avg_us'}}"""
    out = {}
    con = sqlite3.connect(path)
    for name, calls, _, average, _ in con.execute('select name, total_calls, total_duration, average, percentage from top_kernels'):
        short = next((k for k in ('dp_scan_kernel', 'dp_profiles_kernel', 'dp_distance_kernel', 'dp_finish_kernel', 'lsap_kernel',
                                  'qap_objective_kernel', 'qapw_objective_kernel', 'count_matches_kernel') if k in name), None)
        if short:
            out[short] = {'calls': int(calls), 'avg_us': round(float(average), 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--sizes', default='50,200')
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace', default=None, metavar='KIND:N')
    ap.add_argument('--merge-stats', action='append', default=[], metavar='KIND:N=DB')
    o = ap.parse_args()
    if o.trace:
        return trace(o.trace)
    if o.merge_stats:
        with open(o.out) as f:
            res = json.load(f)
        res['kernel_trace'] = {case: kernel_stats(path) for case, path in (m.split('=', 1) for m in o.merge_stats)}
    else:
        from time_pairgen_indexed import WINDOWS
        res = {'tool': 'time_degree_profile', 'windows': WINDOWS, 'cases': []}
        for n in map(int, o.sizes.split(',')):
            for kind in KINDS:
                res['cases'].append(one_case(kind, n, o.reps))
    line = json.dumps(res)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
