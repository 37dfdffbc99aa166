#!/usr/bin/env python3
"""Record the distribution of the reference's QAP pairs -> tests/golden/pairgen_stats.npz.

Runs only in the build container (needs the reference checkout and networkx).  Imports the reference's
``GENERATOR_FUNCTIONS`` / ``NOISE_FUNCTIONS`` (loaders/data_generator.py) behind the ``numpy.lib.arraysetops`` shim of
make_golden.py, draws K pairs per config of tests/pairgen_stats.py the way ``QAP_Generator.compute_example`` does (Regular / ER,
Regular / EdgeSwap, ER / ER, BA / ER at N = 50 with K = 2000; Regular / ER at N = 200 with K = 500; ER / ER with vertex_proba 0.8
at N = 50), and stores recorded numbers only: per config and statistic (edge count, degree variance, triangles, edges shared by
both sides, max degree, n) the entry '<config>/<statistic>' = [mean, std, K].  The on-device pair generator's distribution gate
(tests/test_pairgen_host.py, tests/test_gpu_pairgen.py) reads it.

Usage:  python tests/golden/make_pairgen_stats.py     (from the repo root)
"""
import os
import random
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

from make_golden import import_reference  # noqa: E402
from pairgen_stats import CONFIGS, statistics, summarize  # noqa: E402

K = {50: 2000, 200: 500}


def main():
    import_reference()
    from loaders.data_generator import GENERATOR_FUNCTIONS, NOISE_FUNCTIONS
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    out = {}
    for name, cfg in CONFIGS.items():
        t0 = time.time()
        N = cfg['n_vertices']
        sampler = torch.distributions.Binomial(N, cfg['vertex_proba'])
        a1 = np.zeros((K[N], N, N))
        a2 = np.zeros((K[N], N, N))
        n = np.zeros(K[N])
        for k in range(K[N]):
            nk = int(sampler.sample().item())
            g, W = GENERATOR_FUNCTIONS[cfg['generative_model']](cfg['edge_density'], nk)
            Wn = NOISE_FUNCTIONS[cfg['noise_model']](g, W, cfg['noise'], cfg['edge_density'])
            a1[k, :nk, :nk] = np.asarray(W)
            a2[k, :nk, :nk] = np.asarray(Wn)
            n[k] = nk
        st = statistics(torch.from_numpy(a1), torch.from_numpy(a2), torch.from_numpy(n))
        out.update(summarize(name, {s: v.numpy() for s, v in st.items()}))
        print('%-22s K=%d  %.1fs  %s' % (name, K[N], time.time() - t0,
                                         '  '.join('%s %.3f' % (s, out['%s/%s' % (name, s)][0]) for s in st)), flush=True)
    np.savez(os.path.join(HERE, 'pairgen_stats.npz'), **out)


if __name__ == '__main__':
    main()
