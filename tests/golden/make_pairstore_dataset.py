#!/usr/bin/env python3
"""Record a small dataset of the reference's loader -> tests/golden/pairstore_dataset.pt.

Runs only in the build container (needs the reference checkout and networkx).  Imports the reference's ``QAP_Generator``
(loaders/data_generator.py:175-219) behind the shims of make_golden.py, lets ``create_dataset`` draw 6 ErdosRenyi / ErdosRenyi
pairs at n_vertices 12 with vertex_proba 0.8 (ragged sizes) and saves the list of (B, B_noise) tensor representations the way
``Base_Generator.load_dataset`` does (torch.save of the list): data only, read with ``torch.load(weights_only=True)`` by
``PairStore.from_reference_dataset`` (tests/test_pairstore_host.py, tests/test_gpu_pairstore.py).

Usage:  python tests/golden/make_pairstore_dataset.py     (from the repo root)
"""
import os
import random
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

from make_golden import import_reference  # noqa: E402

ARGS = dict(generative_model='ErdosRenyi', noise_model='ErdosRenyi', edge_density=0.3, noise=0.1, n_vertices=12, vertex_proba=0.8,
            num_examples_train=6)


def main():
    import_reference()
    from loaders.data_generator import QAP_Generator
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        data = QAP_Generator('train', ARGS, tmp).create_dataset()
    sizes = [b.shape[-1] for b, _ in data]
    assert len(set(sizes)) > 1 and all(b.shape == bn.shape == (2, n, n) for (b, bn), n in zip(data, sizes))
    torch.save(data, os.path.join(HERE, 'pairstore_dataset.pt'))
    print('sizes', sizes, 'edges', [int(b[0].sum()) // 2 for b, _ in data])


if __name__ == '__main__':
    main()
