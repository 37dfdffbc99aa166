"""fp64 references of the device evaluation (csrc/eval.hip, graph_neural_net_amd/evaluation.py) in numpy / torch on the CPU, shared
by tests/test_eval_host.py and tests/test_gpu_eval.py: the row log-sum-exp, the cost corner -log_softmax, the per-pair cross-entropy
sum against the identity, np.argmax counts, SciPy's assignment on the fp64 cost and the arithmetic of the epoch record.

Assignments are compared on STABLE pairs only: a pair whose optimal assignment is the same on the fp64 cost and on a float32
log_softmax cost computed by torch on the CPU.  Where the two differ the optimum hangs on the rounding of the cost and no fp32
evaluation is right or wrong about it.  At most 1 pair in 20 of the committed cases may be unstable (UNSTABLE_CAP; asserted by both
test files; the seeds below were checked on the CPU against the reference alone)."""
import functools
import math

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

SIZES = (1, 2, 15, 16, 17, 50, 63, 64, 65, 130)
BATCHES = (1, 3, 32)
CHANNELS = 32
UNSTABLE_CAP = 1.0 / 20.0
# the bound tests/test_gpu_score_loss.py applies to fgnn_ce_fwd's pair loss: |error| <= CE_BOUND * sum(|lse_i| + |s_ii|) -- 84 fp32 eps on
# the magnitude the fp32 values are rounded against; a cost entry is held to the same multiple of |lse_i| + |s_ij|
CE_BOUND = 1e-5


def case_seed(N, B, ragged):
    return 1009 * N + 31 * B + (7 if ragged else 0)


def nv_pattern(B, N, g):
    """Ragged vertex counts: N first, then 0 and 1 (when B allows), the rest random in [1, N]."""
    nv = torch.randint(1, N + 1, (B,), generator=g, dtype=torch.int32)
    for k, v in enumerate((N, 0, 1)[:B]):
        nv[k] = v
    return nv


def corner(nv, N):
    """(B, N, N) bool: the valid block of each pair."""
    r = torch.arange(N)
    m = r[None, :] < nv.long()[:, None]
    return m[:, :, None] & m[:, None, :]


def make_scores(B, N, nv, g):
    """(B, N, N) fp32 scores e1^T e2 of random-normal (B, 32, N) embeddings scaled as in tests/test_gpu_score_loss.py::_embeddings
    (scores of standard deviation about 2; their optimum is essentially never tied); NaN outside the valid corner."""
    s = math.sqrt(2.0) / CHANNELS ** 0.25
    e1 = torch.randn(B, CHANNELS, N, generator=g) * s
    e2 = torch.randn(B, CHANNELS, N, generator=g) * s
    sc = torch.matmul(e1.transpose(1, 2), e2)
    return sc.masked_fill(~corner(nv, N), float('nan'))


def random_labels(nv, N, g):
    """(B, N) int32: a random permutation of [0, n_b) in the first n_b entries of row b, -1 in the padding."""
    lab = torch.full((nv.numel(), N), -1, dtype=torch.int32)
    for b, n in enumerate(nv.tolist()):
        lab[b, :n] = torch.randperm(n, generator=g).to(torch.int32)
    return lab


def lse_rows(blk):
    """fp64 m + log(sum exp(s - m)) per row of an (n, n) block, by the formula the kernel states (non-finite rows propagate)."""
    blk = np.asarray(blk, dtype=np.float64)
    if blk.shape[0] == 0:
        return np.zeros(0)
    with np.errstate(all='ignore'):
        m = blk.max(axis=1)
        return m + np.log(np.exp(blk - m[:, None]).sum(axis=1))


def cost_corner(blk):
    blk = np.asarray(blk, dtype=np.float64)
    with np.errstate(all='ignore'):
        return lse_rows(blk)[:, None] - blk


def pair_ce(blk):
    """fp64 sum over the rows of lse_i - s_ii: the reference loss of one pair before its division by the node count."""
    blk = np.asarray(blk, dtype=np.float64)
    return float((lse_rows(blk) - np.diagonal(blk)).sum()) if blk.shape[0] else 0.0


def ce_scale(blk):
    """sum_i |lse_i| + |s_ii|: the magnitude an fp32 CE sum is rounded against."""
    blk = np.asarray(blk, dtype=np.float64)
    return float((np.abs(lse_rows(blk)) + np.abs(np.diagonal(blk))).sum()) if blk.shape[0] else 0.0


def argmax_hits(blk, label=None):
    blk = np.asarray(blk)
    n = blk.shape[0]
    if n == 0:
        return 0
    want = np.arange(n) if label is None else np.asarray(label)[:n]
    return int(np.sum(np.argmax(blk, 1) == want))


def scipy_assign(cost):
    if cost.shape[0] == 0:
        return np.zeros(0, dtype=np.int64)
    return linear_sum_assignment(cost)[1]


def stable(blk):
    """(stable?, SciPy's assignment on the fp64 cost) of one pair's (n, n) fp32 scores."""
    blk = torch.as_tensor(blk, dtype=torch.float32)
    a64 = scipy_assign(cost_corner(blk.numpy()))
    a32 = scipy_assign((-torch.log_softmax(blk, -1)).numpy()) if blk.shape[0] else a64
    return bool(np.array_equal(a64, a32)), a64


def fold_record(pair_ces, nodes, lsap, maxhits, live, start=None):
    """The arithmetic of fgnn_eval_fold on per-pair values: the first `live` pairs added to the record in pair order."""
    rec = dict(start) if start else {'ce_sum': 0.0, 'nodes': 0, 'correct_lsap': 0, 'correct_max': 0, 'pairs': 0, 'steps': 0}
    for b in range(live):
        rec['ce_sum'] = rec['ce_sum'] + float(pair_ces[b])
        rec['nodes'] += int(nodes[b])
        rec['correct_lsap'] += int(lsap[b])
        rec['correct_max'] += int(maxhits[b])
        rec['pairs'] += 1
    rec['steps'] += 1 if live > 0 else 0
    return rec


def loss_of(blocks):
    """ce_sum / nodes over a list of (n, n) score blocks: triplet_loss('mean') in fp64."""
    nodes = sum(b.shape[0] for b in blocks)
    return sum(pair_ce(b) for b in blocks) / nodes


@functools.lru_cache(maxsize=None)
def case(N, B, ragged):
    """One committed case, with everything the tests compare against (computed once, shared, never modified): scores, nv, labels
    and per pair the fp64 cost corner, CE sum, scale, arg-max hits (identity / labels), SciPy's assignment and its stability."""
    g = torch.Generator().manual_seed(case_seed(N, B, ragged))
    nv = nv_pattern(B, N, g) if ragged else torch.full((B,), N, dtype=torch.int32)
    s = make_scores(B, N, nv, g)
    labels = random_labels(nv, N, g)
    pairs = []
    for b, n in enumerate(nv.tolist()):
        blk = s[b, :n, :n].numpy()
        ok, assign = stable(blk)
        lab = labels[b, :n].numpy()
        pairs.append({'n': n, 'cost': cost_corner(blk), 'lse': lse_rows(blk), 'ce': pair_ce(blk), 'scale': ce_scale(blk),
                      'hits': argmax_hits(blk), 'hits_labels': argmax_hits(blk, lab), 'assign': assign, 'stable': ok,
                      'lsap': int(np.sum(assign == np.arange(n))), 'lsap_labels': int(np.sum(assign == lab))})
    return {'scores': s, 'nv': nv, 'labels': labels, 'pairs': pairs}


def unstable_fraction():
    """Over every committed case: (unstable pairs, pairs)."""
    bad = tot = 0
    for N in SIZES:
        for B in BATCHES:
            for ragged in (False, True):
                ps = case(N, B, ragged)['pairs']
                bad += sum(not p['stable'] for p in ps)
                tot += len(ps)
    return bad, tot
