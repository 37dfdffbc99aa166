"""The two matching accuracies of the reference on the device: accuracy_max (toolbox/metrics.py:119-141: argmax over each
score row compared with the identity matching) and accuracy_linear_assignment (toolbox/metrics.py:92-116: the minimum-cost
matching of -log_softmax(scores), SciPy's assignment reproduced by csrc/lsap.hip).  Neither copies the scores to the host;
the only synchronisation is the final count handed back as Python numbers, as the reference's return type demands.
Scores that live on the host (saved scores, evaluation scripts), and graphs beyond the device solver's FGNN_LSAP_MAX_N, take
the reference's own route: a host loop over the graphs with scipy.optimize.linear_sum_assignment (toolbox/metrics.py:104-112).

Both take the reference's ``labels`` (toolbox/metrics.py:92,118) -- a keyword here, the second positional argument there: a (B, N)
integer tensor with labels[b, i] = the column row i should match (``planted.py``; entries past n_b are ignored), or a list of
per-graph arrays as in the reference.  None is the identity matching."""
import numpy as np
import torch

from . import _lib
from .masked import MaskedTensor


def labels_tensor(labels, B, N, device):
    """labels= of the metrics and decoders -> (B, N) int32 tensor on `device`, -1 in the padding.  Accepts a (B, N) integer tensor
    or array, or the reference's list of B per-graph integer arrays (graph b's of length n_b <= N)."""
    if labels is None:
        return None
    if isinstance(labels, (list, tuple)):
        if len(labels) != B:
            raise ValueError('labels: %d per-graph arrays for a batch of %d' % (len(labels), B))
        rows = np.full((B, N), -1, dtype=np.int64)
        for b, lab in enumerate(labels):
            lab = np.asarray(lab.cpu() if torch.is_tensor(lab) else lab)
            if lab.ndim != 1 or lab.shape[0] > N or lab.dtype.kind not in 'iu':
                raise ValueError('labels[%d] must be a 1-D integer array of at most %d entries, got %s %s' % (b, N, lab.shape, lab.dtype))
            rows[b, :lab.shape[0]] = lab
        labels = torch.from_numpy(rows)
    elif isinstance(labels, np.ndarray):
        labels = torch.from_numpy(labels)
    if not torch.is_tensor(labels) or labels.is_floating_point() or labels.dtype == torch.bool or labels.is_complex():
        raise ValueError('labels must be an integer tensor or a list of integer arrays, got %s'
                         % (labels.dtype if torch.is_tensor(labels) else type(labels).__name__))
    if tuple(labels.shape) != (B, N):
        raise ValueError('labels must have shape (%d, %d), got %s' % (B, N, tuple(labels.shape)))
    return labels.to(device=device, dtype=torch.int32).contiguous()


def count_matches(assign, labels, nvalid=None):
    """fgnn_count_matches: #{i < n_b : assign[b, i] == labels[b, i]} per pair -> (B,) int32 device tensor; assign, labels (B, N) int32."""
    B, N = assign.shape
    correct = torch.empty(B, dtype=torch.int32, device=assign.device)
    _lib.call('fgnn_count_matches', _lib.ptr(assign), _lib.ptr(labels), _lib.ptr(nvalid), B, N, _lib.ptr(correct), _lib.stream_ptr())
    return correct


def accuracy_max(weights, aggregate_score=True, labels=None):
    """weights: (bs, n, n) device tensor or MaskedTensor.  Returns (n_correct, n_vertices), or the list
    of per-graph accuracies with aggregate_score=False.  labels: see the module docstring."""
    if isinstance(weights, MaskedTensor):
        s, nvalid = weights.tensor, weights.nvalid
        sizes = nvalid.to(torch.int64)
    else:
        s, nvalid = weights, None
        sizes = torch.full((s.shape[0],), s.shape[1], dtype=torch.int64, device=s.device)
    labels = labels_tensor(labels, s.shape[0], s.shape[1], s.device)
    if not s.is_cuda:           # host scores: the reference's arg-max comparison (toolbox/metrics.py:127-137), per graph
        want = [torch.arange(n) if labels is None else labels[b, :n] for b, n in enumerate(sizes.tolist())]
        n_ok = [int((s[b, :n, :n].argmax(-1) == want[b]).sum()) if n else 0 for b, n in enumerate(sizes.tolist())]
        if aggregate_score:
            return sum(n_ok), int(sizes.sum().item())
        return [c / n if n else float('nan') for c, n in zip(n_ok, sizes.tolist())]     # an empty graph: 0 / 0, as on the device
    s = s.contiguous()
    B, N, _ = s.shape
    correct = torch.empty(B, dtype=torch.int32, device=s.device)
    if labels is None:
        _lib.call('fgnn_accuracy_max', _lib.ptr(s), _lib.ptr(nvalid) if nvalid is not None else None, B, N,
                  _lib.ptr(correct), _lib.stream_ptr())
    else:
        _lib.call('fgnn_accuracy_max_labels', _lib.ptr(s), _lib.ptr(labels), _lib.ptr(nvalid), B, N, _lib.ptr(correct), _lib.stream_ptr())
    if aggregate_score:
        return int(correct.sum().item()), int(sizes.sum().item())
    return (correct.to(torch.float64) / sizes.to(torch.float64)).tolist()


def _ranks_host(blk, want):
    """The rank of column want[i] in row i of an (n, n) block of host scores: 1 + the columns that beat it in the order of the arg-max
    above (a larger score; NaN above every number; on equal scores, or two NaN, the smaller index) -- 0 where want[i] is no column."""
    n = blk.shape[0]
    want = want.to(torch.int64)
    valid = (want >= 0) & (want < n)
    t = want.clamp(0, max(n - 1, 0))[:, None]
    st = blk.gather(1, t)
    first = torch.arange(n)[None, :] < t
    vnan, tnan = torch.isnan(blk), torch.isnan(st)
    beats = torch.where(tnan, vnan & first, vnan | (blk > st) | ((blk == st) & first))
    return torch.where(valid, 1 + beats.sum(1), torch.zeros_like(want)).to(torch.int32)


def match_ranks(scores, labels=None):
    """scores: (bs, n, n) tensor or MaskedTensor -> (bs, n) int32 ranks on the scores' device: rank[b, i] = 1 + the number of columns
    j < n_b that beat the column row i should match (labels[b, i]; None: i) -- rank 1 is what accuracy_max counts; 0 for a row whose
    label is no column of the graph and for the padding rows.  Host scores take a host route, device scores fgnn_eval_ranks."""
    if isinstance(scores, MaskedTensor):
        s, nvalid = scores.tensor, scores.nvalid
    else:
        s, nvalid = scores, None
    s = s.detach()
    B, N, _ = s.shape
    labels = labels_tensor(labels, B, N, s.device)
    if not s.is_cuda:
        rank = torch.zeros(B, N, dtype=torch.int32)
        sizes = [N] * B if nvalid is None else [min(max(int(n), 0), N) for n in nvalid.tolist()]
        for b, n in enumerate(sizes):
            if n:
                rank[b, :n] = _ranks_host(s[b, :n, :n].float(), torch.arange(n) if labels is None else labels[b, :n])
        return rank
    s = s.to(torch.float32).contiguous()
    nv32 = nvalid.to(device=s.device, dtype=torch.int32).contiguous() if nvalid is not None else None
    rank = torch.zeros(B, N, dtype=torch.int32, device=s.device)
    with torch.cuda.device(s.device):
        _lib.call('fgnn_eval_ranks', _lib.ptr(s), N * N, N, _lib.ptr(nv32), _lib.ptr(labels), B, N, _lib.ptr(rank), _lib.stream_ptr())
    return rank


def hits_at_k(scores, k, labels=None, aggregate_score=True):
    """Hits@k with the return convention of accuracy_max: (rows whose match ranks among the first k, n_vertices), or the list of
    per-graph fractions with aggregate_score=False.  k = 1 is accuracy_max."""
    k = int(k)
    if k < 1:
        raise ValueError('hits_at_k: k must be at least 1, got %d' % k)
    rank = match_ranks(scores, labels)
    B, N = rank.shape
    if isinstance(scores, MaskedTensor):
        sizes = scores.nvalid.to(device=rank.device, dtype=torch.int64).clamp(0, N)
    else:
        sizes = torch.full((B,), N, dtype=torch.int64, device=rank.device)
    hits = ((rank >= 1) & (rank <= k)).sum(1)
    if aggregate_score:
        return int(hits.sum().item()), int(sizes.sum().item())
    return [h / n if n else float('nan') for h, n in zip(hits.tolist(), sizes.tolist())]


def accuracy_linear_assignment(rawscores, aggregate_score=True, labels=None):
    """rawscores: (bs, n, n) device tensor or MaskedTensor.  Minimum-cost matching on -log_softmax(scores) per graph (the
    assignment scipy.optimize.linear_sum_assignment returns, computed on the device by fgnn_lsap_accuracy: no copy of the
    scores to the host, no host loop), counted against the identity matching, or against `labels` (see the module docstring;
    one more launch, fgnn_count_matches): (n_correct, n_vertices) or the list of per-graph accuracies."""
    if isinstance(rawscores, MaskedTensor):
        s, nvalid = rawscores.tensor, rawscores.nvalid
        sizes = nvalid.to(torch.int64)
    else:
        s, nvalid = rawscores, None
        sizes = torch.full((s.shape[0],), s.shape[1], dtype=torch.int64, device=s.device)
    s = s.detach()
    labels = labels_tensor(labels, s.shape[0], s.shape[1], s.device)
    if not s.is_cuda or s.shape[-1] > _lib.FGNN_LSAP_MAX_N:
        return _accuracy_lsap_host(s, sizes, aggregate_score, labels)
    correct, assign = lsap_device(s, nvalid, want_assign=labels is not None)
    if labels is not None:
        correct = count_matches(assign, labels, nvalid)
    if aggregate_score:
        return int(correct.sum().item()), int(sizes.sum().item())
    return (correct.to(torch.float64) / sizes.to(torch.float64).to(correct.device)).tolist()


def lsap_device(s, nvalid=None, want_assign=False):
    """The device route of accuracy_linear_assignment, shared with qap.all_acc_qap: s (B, N, N) raw scores on the GPU, nvalid the
    vertex counts or None -> (correct (B,) int32, assign (B, N) int32 or None): -log_softmax over the valid columns, then SciPy's
    assignment by fgnn_lsap_accuracy.  Nothing is copied to the host."""
    if nvalid is not None:          # padding columns must not take part in the row softmax
        col = torch.arange(s.shape[-1], device=s.device)[None, None, :] < nvalid.to(s.device)[:, None, None]
        s = s.masked_fill(~col, float('-inf'))
    cost = (-torch.log_softmax(s.float(), -1)).contiguous()
    B, N, _ = cost.shape
    correct = torch.empty(B, dtype=torch.int32, device=s.device)
    assign = torch.empty(B, N, dtype=torch.int32, device=s.device) if want_assign else None
    nv32 = nvalid.to(device=s.device, dtype=torch.int32).contiguous() if nvalid is not None else None
    _lib.call('fgnn_lsap_accuracy', _lib.ptr(cost), N * N, N, _lib.ptr(nv32), B, N, _lib.ptr(correct), _lib.ptr(assign), _lib.stream_ptr())
    return correct, assign


def _accuracy_lsap_host(s, sizes, aggregate_score, labels=None):
    """The reference's host loop (toolbox/metrics.py:100-112): -log_softmax of each graph's valid n x n scores -> SciPy's
    assignment -> matches with the identity, or with the graph's label row.  Used for scores that are not on the GPU and for
    n > FGNN_LSAP_MAX_N."""
    from scipy.optimize import linear_sum_assignment
    n_ok = []
    lab = labels.cpu().numpy() if labels is not None else None
    for b, n in enumerate(sizes.tolist()):
        n = int(n)
        cost = -torch.log_softmax(s[b, :n, :n].float(), -1).cpu().numpy()
        row, col = linear_sum_assignment(cost)
        n_ok.append(int((col == (row if lab is None else lab[b, :n])).sum()))
    if aggregate_score:
        return sum(n_ok), int(sizes.sum().item())
    return [c / int(n) for c, n in zip(n_ok, sizes.tolist())]
