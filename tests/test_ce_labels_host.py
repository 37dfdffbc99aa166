"""CPU: the cross-entropy against labels without a launch -- tests/ce_labels_ref.py pinned against torch's
CrossEntropyLoss(reduction='sum', ignore_index=-1) (the call of the reference's triplet_loss, toolbox/losses.py:20-34, with
target = labels instead of arange), the new entry points' prototypes against the ctypes tables, and the host wiring of the
trainer (labels through the size buckets, fit(permute=True))."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ce_labels_ref as R
from graph_neural_net_amd import _lib
from graph_neural_net_amd.trainer import FgnnTrainer
from util import ROOT

NEW_ENTRY_POINTS = ('fgnn_score_ce_fwd_blocks_labels', 'fgnn_score_ce_bwd_labels', 'fgnn_ce_fwd_labels', 'fgnn_ce_bwd_labels',
                    'fgnn_eval_pairs_labels')


@pytest.mark.parametrize('N', [1, 2, 17, 50])
def test_reference_is_torch_cross_entropy_with_ignore_index(N):
    """loss and dS of the reference against fp64 autograd through torch's cross-entropy, per pair on its n x n corner; ragged
    counts (N, 0, 1, random) and rows without a target.  torch refuses a target >= n: such labels are handed to it as
    ignore_index, which is what the no-target rule says they are."""
    B, gscale = 6, 0.37
    rng = np.random.default_rng(N)
    nv = rng.integers(1, N + 1, B)
    nv[:3] = (N, 0, 1)
    S = rng.standard_normal((B, N, N)) * 3
    crit = torch.nn.CrossEntropyLoss(reduction='sum', ignore_index=-1)
    for name, lab in R.label_cases(B, N, nv, rng).items():
        lse, loss, dS = R.batch_ce(S, lab, nv, gscale)
        ok = R.has_target(lab, nv)
        for b in range(B):
            n = int(nv[b])
            if n == 0:
                assert loss[b] == 0 and not dS[b].any() and not lse[b].any()
                continue
            s = torch.from_numpy(S[b, :n, :n].copy()).requires_grad_(True)
            t = torch.from_numpy(np.where(ok[b, :n], lab[b, :n], -1).astype(np.int64))
            ref = crit(s, t)
            (gscale * ref).backward()
            assert abs(loss[b] - ref.item()) <= 1e-12 * max(abs(ref.item()), 1.0), (name, b)
            assert np.abs(dS[b, :n, :n] - s.grad.numpy()).max() <= 1e-12, (name, b)
            assert np.abs(lse[b, :n] - torch.logsumexp(s.detach(), -1).numpy()).max() <= 1e-12
            assert not dS[b, n:].any() and not dS[b, :, n:].any() and not lse[b, n:].any()
            assert not dS[b, :n][~ok[b, :n]].any()                     # a row without a target: exactly no gradient
        if name == 'holes' and N >= 17:
            assert (~ok & (np.arange(N)[None, :] < nv[:, None])).sum() > 0       # the case is present
        if name == 'identity':          # ... and the identity is the reference's own loss (target arange(n))
            for b in range(B):
                n = int(nv[b])
                if n:
                    s = torch.from_numpy(S[b, :n, :n])
                    assert abs(loss[b] - torch.nn.functional.cross_entropy(s, torch.arange(n), reduction='sum').item()) <= 1e-12 * max(loss[b], 1)


def test_embedding_grads_are_the_bmm_backward():
    rng = np.random.default_rng(5)
    B, Cc, N = 3, 4, 7
    nv = np.array([7, 3, 0])
    e1, e2 = rng.standard_normal((B, Cc, N)), rng.standard_normal((B, Cc, N))
    m = np.arange(N)[None, None, :] < nv[:, None, None]
    a = torch.from_numpy(np.where(m, e1, 0)).requires_grad_(True)
    b = torch.from_numpy(np.where(m, e2, 0)).requires_grad_(True)
    S = torch.matmul(a.transpose(1, 2), b)
    lab = R.label_cases(B, N, nv, rng)['holes']
    _, _, dS = R.batch_ce(S.detach().numpy(), lab, nv, 1.0)
    (S * torch.from_numpy(dS)).sum().backward()
    d1, d2 = R.embedding_grads(np.where(m, e1, np.nan), np.where(m, e2, np.nan), dS, nv)
    assert np.abs(d1 - a.grad.numpy()).max() <= 1e-12 and np.abs(d2 - b.grad.numpy()).max() <= 1e-12


_CTYPE = {'const float *': C.c_void_p, 'float *': C.c_void_p, 'const int *': C.c_void_p, 'int *': C.c_void_p, 'void *': C.c_void_p,
          'int': C.c_int, 'long long': C.c_longlong}


def test_new_entry_points_declared_and_bound():
    """include/fgnn_hip.h and _lib._SIGNATURES agree on the new entry points, argument by argument, and the library exports them"""
    hdr = open(os.path.join(ROOT, 'include', 'fgnn_hip.h')).read()
    lib = _lib.load()
    for name in NEW_ENTRY_POINTS:
        m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, hdr)
        assert m, '%s is not declared in include/fgnn_hip.h' % name
        args = [a.strip() for a in re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')]
        types = [re.sub(r'\s*\w+$', '', a).strip() for a in args]
        assert name in _lib._SIGNATURES, name
        assert [_CTYPE[t] for t in types] == _lib._SIGNATURES[name], (name, types)
        assert hasattr(lib, name), name
    # the labelled entry points take the label-less argument lists with `labels` after `nvalid`
    for plain, lab in (('fgnn_score_ce_fwd_blocks', 'fgnn_score_ce_fwd_blocks_labels'), ('fgnn_score_ce_bwd', 'fgnn_score_ce_bwd_labels'),
                       ('fgnn_ce_fwd', 'fgnn_ce_fwd_labels'), ('fgnn_ce_bwd', 'fgnn_ce_bwd_labels')):
        assert len(_lib._SIGNATURES[lab]) == len(_lib._SIGNATURES[plain]) + 1
    assert _lib._SIGNATURES['fgnn_eval_pairs_labels'] == _lib._SIGNATURES['fgnn_eval_pairs']


class _Host(FgnnTrainer):
    def __init__(self):
        self.params = torch.zeros(1)


def test_labels_follow_their_pairs_through_the_size_buckets():
    tr = _Host()
    sizes = [5, 20, 7, 33, 18]
    xs = [torch.zeros(2, n, n) for n in sizes]
    labels = [np.arange(n)[::-1].copy() + 0 * k for k, n in enumerate(sizes)]
    labels[2] = labels[2][:4]                                        # a partially known alignment: the rest has no target
    batch = tr.prepare_ragged(xs, xs, granule=16, labels=labels)
    seen = []
    for b in batch['buckets']:
        lab = b['labels']
        assert lab.dtype == torch.int32 and tuple(lab.shape) == (b['pairs'], b['npad'])
        for k, i in enumerate(b['idx']):
            want = np.full(b['npad'], -1)
            want[:len(labels[i])] = labels[i]
            assert lab[k].tolist() == want.tolist()
            seen.append(i)
        assert bool((lab[len(b['idx']):] == -1).all())               # the filling pairs of a bucket
    assert sorted(seen) == list(range(len(sizes)))
    assert all('labels' not in b for b in tr.prepare_ragged(xs, xs, granule=16)['buckets'])
    with pytest.raises(ValueError, match='label arrays'):
        tr.prepare_ragged(xs, xs, labels=labels[:2])
    with pytest.raises(ValueError, match='labels'):
        tr.prepare_ragged(xs, xs, labels=[np.zeros(n) for n in sizes])      # floating-point labels


def test_fit_permute_trains_and_validates_on_the_labels():
    calls = []

    class Meter:
        def result(self):
            return {'loss': 1.0, 'acc': 0.5, 'acc_max': 0.25, 'nodes': 1, 'pairs': 1}

    class Stub(FgnnTrainer):
        def __init__(self):
            self.opt = type('O', (), {'lr': 1e-3})()

        def train_epoch(self, generator, sampler, epoch, batch_size, permute=False, exact_last=False):
            calls.append(('train', permute))
            return None

        def evaluate(self, generator, sampler, batch_size, epoch=0, hungarian=True, meter=None, permute=False, loss_on_labels=False,
                     rank_meter=None):
            calls.append(('eval', permute, loss_on_labels))
            return Meter()

    seen = []
    sched = type('S', (), {'step': lambda self, v: seen.append(v)})()
    hist = Stub().fit('tg', 'ts', 'vg', 'vs', 2, 8, scheduler=sched, permute=True)
    assert calls == [('train', True), ('eval', True, True)] * 2 and seen == [1.0, 1.0] and hist[1]['val_acc'] == 0.5
    calls.clear()
    Stub().fit('tg', 'ts', 'vg', 'vs', 1, 8, scheduler=sched)
    assert calls == [('train', False), ('eval', False, False)]
