"""Price and quality of the GRAMPA chain (qap.grampa, csrc/grampa.hip) on relabelled Wigner pairs: 32 pairs, N = 50 and 200,
``WignerGenerator(N, noise=0.2, seed=1).weighted(0, 32, permute=True)`` (the pairs of tools/time_wigner.py's recovery record).

(a) the whole chain through ``qap.grampa(weighted=True)`` at the defaults (128 rounds issued, tol 1e-4: pairs freeze as they
    converge), objective and count included;
(b) the price of a round = (chain of 128 rounds - chain of 8 rounds) / 120 at a tol no pair meets (``qap.grampa_weighted``).  No
    entry point issues one of a round's three kernels alone, so the launches are not timed one by one; what is measured beside the
    round is its launch floor: the same difference on the same batch with every corner cut to 1 vertex (three launches that do
    next to no work), a third of it per launch.  Round minus floor is what the two product kernels and the step kernel compute;
(c) the reference point: ``torch.linalg.eigh`` on the device plus the torch composition of the eigen formula in fp32, if this torch
    build has a working eigh on the device -- else numpy float64 on the host (two eigh per pair and the same composition), timed
    with the host clock over all pairs; `eigen_reference.where` says which one ran;
(d) the recovery rate -- pairs whose planted matching is recovered on every row -- of GRAMPA next to ``qap.faq(weighted=True)`` from
    the barycenter on the same pairs, at s = 0 / 0.2 / 0.4 / 0.6, and the rounds GRAMPA took.

No existing source file is compiled differently by the change that added this tool, so there is no parent-library leg.
Protocol (tools/time_pairgen_indexed.py): device events on one stream, warm-up, then WINDOWS = 7 rounds in which the variants take
turns with one window of `reps` calls each; reported per variant: the median window and the spread of the same run.
usage: python tools/time_grampa.py [--reps 3] [--sizes 50,200] [--out profiles/grampa_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from graph_neural_net_amd import qap
from graph_neural_net_amd.wigner import WignerGenerator
from time_pairgen_indexed import DEV, WINDOWS, alternate, row

B = 32
NOISES = (0.0, 0.2, 0.4, 0.6)
NEVER = 1e-30             # a tol no pair meets
ETA = 0.2


def recovery(N):
    out = {}
    for s in NOISES:
        x1, x2, _, lab = WignerGenerator(N, noise=s, seed=1, device=DEV).weighted(0, B, permute=True)
        g = qap.grampa(x1, x2, labels=lab, weighted=True)
        f = qap.faq(x1, x2, labels=lab, weighted=True)
        out['s%g' % s] = {'grampa_recovered_pairs': int((g['acc'] == N).sum()), 'grampa_acc': float(g['acc'].double().mean()) / N,
                          'faq_recovered_pairs': int((f['acc'] == N).sum()), 'faq_acc': float(f['acc'].double().mean()) / N,
                          'grampa_nit': {'min': int(g['nit'].min()), 'max': int(g['nit'].max())},
                          'grampa_stopped_on_tol': int((g['status'] == 0).sum())}
    return out


def torch_eigen(a, b):
    lam, U = torch.linalg.eigh(a)
    mu, V = torch.linalg.eigh(b)
    K = 1.0 / ((lam[:, :, None] - mu[:, None, :]) ** 2 + ETA * ETA)
    H = torch.ones_like(a)
    return U @ (K * (U.transpose(1, 2) @ H @ V)) @ V.transpose(1, 2)


def numpy_eigen(a, b):
    out = []
    for A, Bm in zip(a, b):
        lam, U = np.linalg.eigh(A)
        mu, V = np.linalg.eigh(Bm)
        K = 1.0 / ((lam[:, None] - mu[None, :]) ** 2 + ETA * ETA)
        out.append(U @ (K * (U.T @ np.ones_like(A) @ V)) @ V.T)
    return np.stack(out)


def eigen_reference(x1, x2, X, reps):
    a, b = x1[:, 0].contiguous(), x2[:, 0].contiguous()
    try:
        ref = torch_eigen(a, b)
        torch.cuda.synchronize()
        t = alternate({'torch_eigh_composition': lambda: torch_eigen(a, b)}, reps)
        where = 'torch.linalg.eigh on the device, fp32'
        us = row(t)['torch_eigh_composition']
    except Exception as e:                      # a torch build without a device eigh: say so, and time the host
        an, bn = a.double().cpu().numpy(), b.double().cpu().numpy()
        t0 = time.perf_counter()
        ref = torch.from_numpy(numpy_eigen(an, bn)).to(DEV)
        us = {'us': round((time.perf_counter() - t0) * 1e6, 2), 'clock': 'host, one pass over the %d pairs' % B}
        where = 'numpy float64 on the host (torch.linalg.eigh on the device failed: %s)' % type(e).__name__
    err = float(((X.double() - ref.double()).abs().amax((1, 2)) / ref.double().abs().amax((1, 2))).max())
    return {'where': where, 'time': us, 'max_rel_diff_to_chain': err}


def one_size(N, reps):
    x1, x2, _, lab = WignerGenerator(N, noise=0.2, seed=1, device=DEV).weighted(0, B, permute=True)
    one = torch.ones(B, dtype=torch.int32, device=DEV)
    out = qap.grampa(x1, x2, labels=lab, weighted=True)
    t = alternate({'chain': lambda: qap.grampa(x1, x2, labels=lab, weighted=True),
                   'chain_128_rounds': lambda: qap.grampa_weighted(x1, x2, None, tol=NEVER, maxiter=128),
                   'chain_8_rounds': lambda: qap.grampa_weighted(x1, x2, None, tol=NEVER, maxiter=8),
                   'floor_128_rounds': lambda: qap.grampa_weighted(x1, x2, one, tol=NEVER, maxiter=128),
                   'floor_8_rounds': lambda: qap.grampa_weighted(x1, x2, one, tol=NEVER, maxiter=8),
                   'faq_chain': lambda: qap.faq(x1, x2, labels=lab, weighted=True)}, reps)
    round_us = (t['chain_128_rounds'][0] - t['chain_8_rounds'][0]) / 120
    floor_us = (t['floor_128_rounds'][0] - t['floor_8_rounds'][0]) / 120
    res = {'n_vertices': N, 'pairs': B, 'reps': reps, 'times': row(t), 'round_us': round(round_us, 2),
           'round_launch_floor_us': round(floor_us, 2), 'launch_floor_us_each_of_3': round(floor_us / 3, 2),
           'round_flop': 8 * B * N ** 3, 'round_tflops': round(8 * B * N ** 3 / round_us * 1e-6, 3),
           'nit': {'min': int(out['nit'].min()), 'max': int(out['nit'].max())}, 'stopped_on_tol': int((out['status'] == 0).sum()),
           'eigen_reference': eigen_reference(x1, x2, out['X'], reps), 'recovery': recovery(N)}
    print('N %d  ' % N + '  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + t[k]) for k in t), flush=True)
    print('N %d  %s' % (N, json.dumps({k: res[k] for k in ('round_us', 'round_launch_floor_us', 'eigen_reference', 'recovery')})), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--sizes', default='50,200')
    ap.add_argument('--out', default=None)
    o = ap.parse_args()
    res = {'tool': 'time_grampa', 'windows': WINDOWS, 'eta': ETA, 'sizes': []}
    for n in map(int, o.sizes.split(',')):          # (the file is rewritten after every size: a long run leaves what it finished)
        res['sizes'].append(one_size(n, o.reps))
        line = json.dumps(res)
        if o.out:
            os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
            with open(o.out, 'w') as f:
                f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
