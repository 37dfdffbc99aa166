#!/usr/bin/env python3
"""Generate tests/golden/planted_labels.npz FROM THE REFERENCE ITSELF: its two label-taking metrics (toolbox/metrics.py:92-141,
accuracy_linear_assignment and accuracy_max) imported and called with list-valued `labels`.  Runs only where the reference is
readable (make_golden.py's REF, imported behind the same shims); its files never travel.

The fixture is six score batches `<g>/...`:

    scores        (B, N, N) float32   values exact in bf16 (the file compresses), 0 outside each graph's n x n corner
    nvalid        (B,) int32          vertex counts (== N except in the ragged groups)
    labels        (B, N) int32        a seeded permutation of [0, n_b) per graph, -1 in the padding
    lsap_correct, max_correct   (B,) int64     the counts the reference returns with aggregate_score=True, graph by graph
    lsap_acc, max_acc           (B,) float64   the entries of its aggregate_score=False lists

Each graph goes through the reference on its own (a batch of one n x n matrix, labels=[row]): that is also how a ragged batch has
to be fed to it.  Groups: random scores at N = 5 and N = 64, small-integer scores (many ties in every row) at N = 8, constant
scores at N = 7 (the assignment is then the identity, so lsap_correct is the number of fixed points of the label), a ragged random
group (N = 12, n in {12, 5, 1, 9}) and a ragged constant group (N = 65, n in {65, 33}).  A Hungarian matching that hangs on the last
bits of a log_softmax would not survive another torch build or the device's log_softmax: scores are drawn again until the matching
survives eight perturbations of its cost matrix, each row shifted by a relative 1e-6 (what a different log-sum-exp does) --
constant and small-integer groups included; the script fails if a group never settles.

Usage:  python tests/golden/make_planted.py     (from the repo root)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
from make_golden import OUT, import_reference  # noqa: E402

# name -> (kind, N, sizes)
GROUPS = {'rand5': ('random', 5, [5, 5, 5, 5]), 'rand64': ('random', 64, [64, 64]), 'ties8': ('ties', 8, [8, 8, 8, 8]),
          'const7': ('const', 7, [7, 7, 7]), 'ragged12': ('random', 12, [12, 5, 1, 9]), 'ragged_const65': ('const', 65, [65, 33])}


def bf16_exact(x):
    return torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()


def draw(kind, rng, n):
    if kind == 'random':
        return bf16_exact((2.0 * rng.standard_normal((n, n))).astype(np.float32))
    if kind == 'ties':
        return rng.integers(0, 4, (n, n)).astype(np.float32)
    return np.full((n, n), 1.5, dtype=np.float32)


def settled(s, rng):
    from scipy.optimize import linear_sum_assignment
    cost = -torch.log_softmax(torch.from_numpy(s), -1).numpy().astype(np.float64)
    col = linear_sum_assignment(cost)[1]
    for _ in range(8):
        shifted = cost + 1e-6 * np.abs(cost).max() * rng.standard_normal((cost.shape[0], 1))
        if not np.array_equal(linear_sum_assignment(shifted.astype(np.float32))[1], col):
            return False
    return True


def main():
    import_reference()
    from toolbox.metrics import accuracy_linear_assignment, accuracy_max
    out = {}
    for gi, (name, (kind, N, sizes)) in enumerate(GROUPS.items()):
        rng = np.random.default_rng(7000 + gi)
        B = len(sizes)
        scores = np.zeros((B, N, N), dtype=np.float32)
        labels = np.full((B, N), -1, dtype=np.int32)
        rec = {k: [] for k in ('lsap_correct', 'max_correct', 'lsap_acc', 'max_acc')}
        for b, n in enumerate(sizes):
            for _ in range(500):
                s = draw(kind, rng, n)
                if settled(s, rng):
                    break
            else:
                raise SystemExit('%s: graph %d never settled' % (name, b))
            lab = rng.permutation(n)
            scores[b, :n, :n] = s
            labels[b, :n] = lab
            t = torch.from_numpy(s)[None]
            for key, fn in (('lsap', accuracy_linear_assignment), ('max', accuracy_max)):
                acc, total = fn(t, [lab], aggregate_score=True)
                assert total == n
                rec[key + '_correct'].append(int(acc))
                rec[key + '_acc'].append(float(fn(t, [lab], aggregate_score=False)[0]))
        out[name + '/scores'], out[name + '/labels'] = scores, labels
        out[name + '/nvalid'] = np.asarray(sizes, dtype=np.int32)
        for k, v in rec.items():
            out['%s/%s' % (name, k)] = np.asarray(v, dtype=np.int64 if k.endswith('correct') else np.float64)
        print(name, rec['lsap_correct'], rec['max_correct'])
    path = os.path.join(OUT, 'planted_labels.npz')
    np.savez_compressed(path, **out)
    print('%s: %d bytes' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
