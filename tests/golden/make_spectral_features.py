#!/usr/bin/env python3
"""Generate tests/golden/spectral_features.npz FROM THE REFERENCE ITSELF: the fixture of the spectral input features
(graph_neural_net_amd/spectral.py, csrc/spectral.hip).  Runs only where the reference is readable (make_golden.py's REF, imported
behind the same shims); its files never travel.  The reference's own `make_laplacian` and `make_spectral_feature`
(loaders/data_generator.py:221-232) are imported and evaluated; nothing here restates them.

The fixture is a set of groups `<g>/...`, each a batch of seeded graphs in the device's wire form:

    bits      (B, N, ceil(N/32)) uint32   bit j of word row i = W[i][j], zero outside the graph's n x n corner
    nvalid    (B,) int32                  vertex counts (== N except in the ragged group)
    ref32     (B, 4, N, N) float32        make_spectral_feature(make_laplacian(W)) as the reference computes it (fp32, n = 4); only in
                                          the groups with N <= 64
    ref_err   (B, 8) float64              per graph and power p = 1 .. 8 the yard-stick: max |fp32 chain - fp64 chain| with both chains
                                          the reference's functions (n = 8; the fp64 run under torch.set_default_dtype(float64))

Groups: ER graphs at N in {7, 33, 50, 64, 65, 120, 200, 256}, Regular graphs at N = 50, a ragged ER group (N = 120, n in [30, 120])
and `directed`: one NON-symmetric W (a directed thinning of an ER graph).  Every graph is drawn again until its minimum (row) degree
is >= 1 -- the reference is NaN otherwise -- and the script asserts it.  The large groups' fp64 truth is not stored: the tests
recompute it with tests/spectral_ref.py.

Usage:  python tests/golden/make_spectral_features.py     (from the repo root)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True
from make_golden import OUT, import_reference  # noqa: E402

import spectral_ref as R  # noqa: E402
from graph_neural_net_amd import synthetic  # noqa: E402

# name -> (family, N, graphs, edge density, (n_lo, n_hi) or None)
GROUPS = {'er7': ('ErdosRenyi', 7, 3, 0.5, None), 'er33': ('ErdosRenyi', 33, 2, 0.3, None), 'er50': ('ErdosRenyi', 50, 2, 0.2, None),
          'reg50': ('Regular', 50, 2, 0.2, None), 'er64': ('ErdosRenyi', 64, 2, 0.2, None), 'er65': ('ErdosRenyi', 65, 1, 0.2, None),
          'er120': ('ErdosRenyi', 120, 1, 0.2, None), 'er200': ('ErdosRenyi', 200, 1, 0.1, None),
          'er256': ('ErdosRenyi', 256, 1, 0.2, None), 'ragged120': ('ErdosRenyi', 120, 4, 0.2, (30, 120)),
          'directed': ('ErdosRenyi', 33, 1, 0.3, None)}


def draw(rng, name, family, n, p):
    while True:
        W = synthetic.make_pair(rng, n, family, edge_density=p, noise=0.1)[0][0].astype(np.float32)
        if name == 'directed':
            W = W * (1 - np.triu(rng.random((n, n)) < 0.4, 1)).astype(np.float32)          # drop some i < j arcs, keep their reversals
            if np.array_equal(W, W.T):
                continue
        if W.sum(1).min() >= 1:
            return W


def main():
    import_reference()
    from loaders.data_generator import make_laplacian, make_spectral_feature
    out = {}
    for gi, (name, (family, N, B, p, ragged)) in enumerate(GROUPS.items()):
        rng = np.random.default_rng(2000 + gi)
        bits, nvalid, ref32, ref_err = [], [], [], []
        for b in range(B):
            n = int(rng.integers(ragged[0], ragged[1] + 1)) if ragged else N
            W = draw(rng, name, family, n, p)
            assert W.sum(1).min() >= 1, 'isolated vertex: the reference is NaN'
            Wt = torch.from_numpy(W)
            f32 = make_spectral_feature(make_laplacian(Wt), R.FIXTURE_POWERS)
            torch.set_default_dtype(torch.float64)          # torch.ones / zeros / eye inside the reference's functions follow it
            try:
                f64 = make_spectral_feature(make_laplacian(Wt.double()), R.FIXTURE_POWERS)
            finally:
                torch.set_default_dtype(torch.float32)
            assert f32.dtype == torch.float32 and f64.dtype == torch.float64 and torch.isfinite(f32).all()
            four = make_spectral_feature(make_laplacian(Wt))                   # the reference's default n = 4
            assert torch.equal(four, f32[:4])
            bits.append(R.pack_bits(W, N))
            nvalid.append(n)
            ref_err.append((f32.double() - f64).abs().amax((1, 2)).numpy())
            if N <= 64:
                ref32.append(four.numpy())
        out[name + '/bits'] = np.stack(bits)
        out[name + '/nvalid'] = np.asarray(nvalid, dtype=np.int32)
        out[name + '/ref_err'] = np.stack(ref_err)
        if ref32:
            out[name + '/ref32'] = np.stack(ref32)
        print('%-10s ref_err per power (max over the group): %s' % (name, ' '.join('%.1e' % e for e in np.stack(ref_err).max(0))))
    path = os.path.join(OUT, 'spectral_features.npz')
    np.savez_compressed(path, **out)
    print('%s: %d bytes' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
