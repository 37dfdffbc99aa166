"""CPU: the per-pair loss weights of the fused step -- tests/pair_weights_ref.py against torch autograd and
against the oracle's triplet_loss('mean_of_mean'); the C prototypes in the ctypes tables; the host restatement of the weights
(FgnnTrainer.ragged_weights) against the reference."""
import ctypes as C
import inspect

import numpy as np
import torch

import ce_labels_ref as R
import pair_weights_ref as P
from graph_neural_net_amd import _lib
from oracle import fgnn_oracle as O


def _ragged_case(seed, B=6, N=11):
    rng = np.random.default_rng(seed)
    nv = rng.integers(1, N + 1, B)
    nv[0], nv[1] = N, 0
    S = rng.normal(0, 2, (B, N, N))
    lab = R.label_cases(B, N, nv, rng)['holes']
    return rng, nv, S, lab


def test_reference_against_torch_autograd_with_a_nan_filler():
    rng, nv, S, lab = _ragged_case(3)
    B, N = lab.shape
    w = rng.uniform(0.2, 3.0, B)
    w[2] = 0.0
    w[4] = 0.0
    S[2] = np.nan                                        # a switched-off pair full of NaN ...
    S[4, :, 0] = np.inf                                  # ... and one with inf
    D = 7.5
    ok = R.has_target(lab, nv)
    tce = torch.nn.CrossEntropyLoss(reduction='sum', ignore_index=-1)
    for labels in (lab, None):
        # torch sees the switched-off pairs with finite scores and weight 0 (its 0 * NaN would poison the sum: the select is the point)
        St = torch.from_numpy(np.where((w != 0)[:, None, None], S, 0.0)).requires_grad_(True)
        tot = 0
        for b in range(B):
            n = int(nv[b])
            if n == 0:
                continue
            t = np.arange(n) if labels is None else np.where(ok[b, :n], lab[b, :n], -1)
            tot = tot + w[b] * tce(St[b, :n, :n], torch.from_numpy(t.astype(np.int64)))
        (tot / D).backward()
        loss, pair, dS = P.weighted_ce(S, labels, nv, w, gscale=1.0 / D)
        assert np.isfinite(loss) and np.isfinite(dS).all()
        assert abs(loss / D - tot.item() / D) <= 1e-12 * abs(tot.item() / D)
        assert np.abs(dS - St.grad.numpy()).max() <= 1e-13
        assert (dS[2] == 0).all() and (dS[4] == 0).all() and pair[2] == 0 and pair[4] == 0
        assert (dS[1] == 0).all()                        # the empty pair


def test_mean_of_mean_weights_against_the_oracle():
    rng = np.random.default_rng(5)
    # equal-size graphs: the oracle's function on the (B, n, n) tensor
    B, n = 5, 9
    S = rng.normal(0, 2, (B, n, n))
    w, D = P.reduction_weights('mean_of_mean', [n] * B)
    assert D == B and np.allclose(w, 1.0 / n, rtol=0, atol=0)
    loss, _, _ = P.weighted_ce(S, None, [n] * B, w)
    ref = O.triplet_loss_mean_of_mean(torch.from_numpy(S)).item()
    assert abs(loss / D - ref) <= 1e-13 * abs(ref)
    wm, Dm = P.reduction_weights('mean', [n] * B)
    assert Dm == B * n and abs(P.weighted_ce(S, None, [n] * B, wm)[0] / Dm - O.triplet_loss_mean(torch.from_numpy(S)).item()) <= 1e-13 * abs(ref)
    # ragged: a per-graph loop (an empty graph does not count)
    nv = np.array([9, 0, 4, 1, 7])
    w, D = P.reduction_weights('mean_of_mean', nv)
    assert D == 4 and w[1] == 0
    loss, _, _ = P.weighted_ce(S, None, nv, w)
    per = [torch.nn.functional.cross_entropy(torch.from_numpy(S[b, :m, :m]), torch.arange(m), reduction='sum').item() / m
           for b, m in enumerate(nv) if m > 0]
    assert abs(loss / D - sum(per) / len(per)) <= 1e-13 * abs(sum(per) / len(per))
    ragged = [torch.from_numpy(S[b, :m, :m]) for b, m in enumerate(nv) if m > 0]
    assert abs(loss / D - O.triplet_loss_mean_of_mean(ragged).item()) <= 1e-13 * abs(loss / D)
    # on ragged data the two reductions are different losses
    wm, Dm = P.reduction_weights('mean', nv)
    assert abs(P.weighted_ce(S, None, nv, wm)[0] / Dm - loss / D) > 1e-3
    # a short last step: the live pairs alone
    w2, D2 = P.reduction_weights('mean_of_mean', nv, live=3)
    assert D2 == 2 and (w2[3:] == 0).all() and (w2[:3] == w[:3]).all()
    wm2, Dm2 = P.reduction_weights('mean', nv, live=3, user=[2, 2, 2, 2, 2])
    assert Dm2 == 2 * 13 and (wm2 == [2, 2, 2, 0, 0]).all()
    w0, D0 = P.reduction_weights('mean', nv, live=0)
    assert D0 == 0 and (w0 == 0).all()


def test_prototypes_are_in_the_ctypes_tables():
    want = {'fgnn_score_ce_bwd_w': 14, 'fgnn_pair_weights': 9, 'fgnn_pair_loss_w': 6}
    for name, nargs in want.items():
        assert name in _lib.EXPORTS and len(_lib._SIGNATURES[name]) == nargs, name
        assert _lib._SIGNATURES[name][-1] is C.c_void_p                      # the stream
    # fgnn_score_ce_bwd_w is fgnn_score_ce_bwd_labels plus one pointer (the weights) in front of gscale
    assert _lib._SIGNATURES['fgnn_score_ce_bwd_w'] == (_lib._SIGNATURES['fgnn_score_ce_bwd_labels'][:6] + [C.c_void_p]
                                                       + _lib._SIGNATURES['fgnn_score_ce_bwd_labels'][6:])
    header = open(__import__('os').path.join(__import__('util').ROOT, 'include', 'fgnn_hip.h')).read()
    for name in want:
        assert 'int %s(' % name in header, name


def test_the_public_surface_takes_the_new_arguments():
    from graph_neural_net_amd.engine_base import EngineBase
    from graph_neural_net_amd.trainer import FgnnTrainer
    for fn in (EngineBase.forward, EngineBase.step):
        assert inspect.signature(fn).parameters['weights'].default is None
    assert inspect.signature(FgnnTrainer.__init__).parameters['loss_reduction'].default == 'mean'
    for fn in (FgnnTrainer.train_step, FgnnTrainer.train_step_bits, FgnnTrainer.train_step_ragged):
        p = inspect.signature(fn).parameters
        assert p['weights'].default is None and p['live'].default is None
    for fn in (FgnnTrainer.train_epoch, FgnnTrainer.fit):
        assert inspect.signature(fn).parameters['exact_last'].default is False


def test_host_weights_of_the_ragged_step_are_the_reference():
    from graph_neural_net_amd.trainer import FgnnTrainer
    sizes = [9, 20, 0, 14, 17]
    user = [1.0, 0.5, 2.0, 3.0, 0.25]
    for mode in ('mean', 'mean_of_mean'):
        tr = FgnnTrainer.__new__(FgnnTrainer)
        tr.loss_reduction = mode
        for live in (None, 0, 1, 4, 5):
            for u in (None, user):
                w, D = tr.ragged_weights(sizes, u, live)
                wr, Dr = P.reduction_weights(mode, sizes, live, u)
                assert D == Dr, (mode, live, u)
                assert np.abs(np.asarray(w) - wr).max() <= 2.0 ** -23 * max(1e-30, np.abs(wr).max()), (mode, live, u)
                assert all((a == 0) == (b == 0) for a, b in zip(w, wr))
