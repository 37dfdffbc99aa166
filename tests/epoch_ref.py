"""Numpy restatement of the epoch permutation (``fgnn_epoch_index`` in ``graph_neural_net_amd/csrc/pairgen.hip``).

Test infrastructure only; the package never imports it.  Written from the construction, not from the kernel's output:

* ``pi`` is a permutation of [0, M) selected by (seed, epoch): a balanced Feistel network on 2 h bits,
  h = max(1, ceil(ceil(log2 M) / 2)), ``ROUNDS`` rounds (L, R) -> (R, L ^ F_r(R)), applied again and again (cycle-walking)
  until the value is below M.  A Feistel pass is a bijection of [0, 4^h) whatever F is, so the walk from a value below M comes
  back below M, and the walked map is a bijection of [0, M);
* F_r(R) = the low h bits of word 0 of Philox4x64-10 (``pairgen_ref.philox4x64``) at counter (epoch, r, R, STREAM) under key
  (seed, 0).  Every stream of the pair generator has 0 in the fourth counter word, so none of its blocks is used here;
* position p >= M is position p mod M of the same epoch.
"""
import numpy as np

from pairgen_ref import philox4x64

ROUNDS = 8
STREAM = 6
MAX_M = 1 << 40


def half_bits(M):
    """h: the Feistel network works on 2 h >= ceil(log2 M) bits, h >= 1."""
    bits = (int(M) - 1).bit_length()            # ceil(log2 M)
    return max(1, (bits + 1) // 2)


def feistel(x, h, seed, epoch):
    """One pass over the uint64 array x of values below 4^h (epoch: one uint64 per element of x)."""
    mask = np.uint64((1 << h) - 1)
    L, R = x >> np.uint64(h), x & mask
    for r in range(ROUNDS):
        ctr = [epoch, np.full_like(R, np.uint64(r)), R, np.full_like(R, np.uint64(STREAM))]
        f = philox4x64(ctr, (seed, 0))[0] & mask
        L, R = R, L ^ f
    return (L << np.uint64(h)) | R


def permute(seed, epoch, M, pos):
    """pi_{seed, epoch}(pos mod M) as int64; `pos` is a sequence of positions, `epoch` one epoch or one per position (many epochs
    in one call, for the statistical tests)."""
    M = int(M)
    if not 1 <= M <= MAX_M:
        raise ValueError('M must be in [1, 2^40], got %d' % M)
    h = half_bits(M)
    x = np.array([int(p) % M for p in pos], dtype=np.uint64)
    ep = np.array([int(e) for e in epoch] if np.ndim(epoch) else [int(epoch)] * len(x), dtype=np.uint64)
    if len(ep) != len(x):
        raise ValueError('%d epochs for %d positions' % (len(ep), len(x)))
    out = np.zeros(len(x), dtype=np.uint64)
    todo = np.arange(len(x))
    while len(todo):
        x = feistel(x, h, seed, ep)
        done = x < np.uint64(M)
        out[todo[done]] = x[done]
        todo, x, ep = todo[~done], x[~done], ep[~done]
    return out.astype(np.int64)


def epoch_index(seed, epoch, M, first_pos, count):
    """What fgnn_epoch_index writes: pi_{seed, epoch}((first_pos + i) mod M) for i < count."""
    return permute(seed, epoch, M, [int(first_pos) + i for i in range(int(count))])
