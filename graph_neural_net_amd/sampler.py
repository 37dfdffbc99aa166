"""The order of an epoch over a fixed dataset of on-device pairs (the reference's ``siamese_loader(..., shuffle=True)`` over
``num_examples_train`` pairs, reshuffled every epoch; ``shuffle=False`` for validation and test).

``EpochSampler`` names the dataset indices of one step of one rank; ``PairGenerator.bits(index=...)`` generates those pairs.  The
epoch order is a permutation of [0, M) that depends on (seed, epoch) only and is evaluated per position by ``fgnn_epoch_index``
(``csrc/pairgen.hip``: a Feistel network on Philox4x64-10, cycle-walked; no sort, no M-sized buffer), so position p of epoch e is
the same on every rank and for every batch size, and nothing is exchanged or stored between steps.

Global step s of batch size B on w ranks covers positions ``[s * B * w, (s + 1) * B * w)`` of the epoch order; rank r takes
``r * B ... r * B + B - 1`` of them.  Positions >= M wrap with the epoch's own permutation (position p is position p mod M), which
is how a short last step is filled when ``drop_last=False`` (as ``torch.utils.data.DistributedSampler`` pads).

Nothing here synchronises with the device.  The shuffled order has no CPU path (``_lib``).
"""
import torch

from . import _lib

MAX_EXAMPLES = 1 << 40        # include/fgnn_hip.h: FGNN_EPOCH_MAX_LOG2_M


def epoch_index(seed, epoch, num_examples, first_pos, count, device=None, out=None):
    """Positions first_pos .. first_pos + count - 1 of the order of epoch `epoch` of dataset `seed` over num_examples examples:
    a (count,) int64 device tensor (written into `out` when given).  Enqueued on the current stream."""
    seed, epoch, M, first_pos, count = int(seed), int(epoch), int(num_examples), int(first_pos), int(count)
    if not 0 <= seed < 1 << 64 or not 0 <= epoch < 1 << 64:
        raise ValueError('seed and epoch must be in [0, 2^64), got %d, %d' % (seed, epoch))
    if not 1 <= M <= MAX_EXAMPLES:
        raise ValueError('num_examples must be in [1, 2^40], got %d' % M)
    if first_pos < 0 or not 0 <= count < 1 << 31:
        raise ValueError('first_pos must be >= 0 and count in [0, 2^31), got %d, %d' % (first_pos, count))
    if out is None:
        device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        if device.type != 'cuda':
            raise RuntimeError('epoch_index: device %s; the epoch permutation runs on the GPU only (there is no CPU path)' % (device,))
        out = torch.empty(count, dtype=torch.int64, device=device)
    elif out.dtype != torch.int64 or out.shape != (count,) or not out.is_contiguous():
        raise ValueError('out must be a contiguous (%d,) int64 tensor, got %s %s' % (count, tuple(out.shape), out.dtype))
    if count:
        with torch.cuda.device(out.device):
            _lib.call('fgnn_epoch_index', seed, epoch, M, first_pos, count, _lib.ptr(out), _lib.stream_ptr())
    return out


class EpochSampler:
    """Which examples of a fixed dataset a rank sees at a step of an epoch."""

    def __init__(self, num_examples, seed=0, shuffle=True, rank=0, world_size=1, drop_last=False, device=None):
        M, w, r = int(num_examples), int(world_size), int(rank)
        if not 1 <= M <= MAX_EXAMPLES:
            raise ValueError('num_examples must be in [1, 2^40], got %d' % M)
        if w < 1 or not 0 <= r < w:
            raise ValueError('rank must be in [0, world_size), got rank %d of %d' % (r, w))
        if not 0 <= int(seed) < 1 << 64:
            raise ValueError('seed must be in [0, 2^64), got %r' % (seed,))
        self.num_examples, self.seed, self.shuffle = M, int(seed), bool(shuffle)
        self.rank, self.world_size, self.drop_last = r, w, bool(drop_last)
        self.device = torch.device(device) if device is not None else None      # None: the current GPU at the time of the call

    @classmethod
    def from_config(cls, cfg, split='train', **kw):
        """The reference's ``data.train`` / ``data.test`` dict: ``num_examples_<split>`` (split 'train', 'val' or 'test')."""
        if split not in ('train', 'val', 'test'):
            raise ValueError("split must be 'train', 'val' or 'test', got %r" % (split,))
        return cls(cfg['num_examples_%s' % split], **kw)

    def steps_per_epoch(self, batch_size):
        per_step = self._batch(batch_size) * self.world_size
        return self.num_examples // per_step if self.drop_last else -(-self.num_examples // per_step)

    def window(self, step, batch_size):
        """(first position, count) of this rank's slice of global step `step` in the epoch order (host arithmetic only)."""
        B, step = self._batch(batch_size), int(step)
        if not 0 <= step < self.steps_per_epoch(B):
            raise ValueError('step %d outside the %d steps of an epoch' % (step, self.steps_per_epoch(B)))
        return step * B * self.world_size + self.rank * B, B

    def batch_index(self, epoch, step, batch_size):
        """The (batch_size,) int64 device tensor of this rank's dataset indices at `step` of `epoch`."""
        first, count = self.window(step, batch_size)
        if self.shuffle:
            return epoch_index(self.seed, epoch, self.num_examples, first, count, device=self.device)
        device = self.device if self.device is not None else torch.device('cuda', torch.cuda.current_device())
        return torch.arange(first, first + count, dtype=torch.int64, device=device) % self.num_examples

    def live_count(self, step, batch_size):
        """How many of this rank's batch_size positions at `step` are examples of their own (positions below num_examples): the
        others wrap around and repeat examples the epoch has already shown, which an evaluation must not count twice.  batch_size
        everywhere but in the last global step of a drop_last=False epoch (host arithmetic only)."""
        first, count = self.window(step, batch_size)
        return max(0, min(count, self.num_examples - first))

    @staticmethod
    def _batch(batch_size):
        B = int(batch_size)
        if B < 1:
            raise ValueError('batch_size must be >= 1, got %d' % B)
        return B
