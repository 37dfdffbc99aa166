"""CPU: the host route of qap.sinkhorn against tests/sinkhorn_ref.py, the argument refusals of qap.sinkhorn, and the faq= argument
checks of the decode chain, which all come before any device work."""
import numpy as np
import pytest
import torch

import sinkhorn_ref as R
from graph_neural_net_amd import _lib, qap
from graph_neural_net_amd.evaluation import FAQ_DEFAULTS, decode_scores, evaluate_scores
from graph_neural_net_amd.masked import MaskedTensor


@pytest.mark.parametrize('N', R.SIZES)
def test_host_route_equals_the_restatement(N):
    s, nv = R.batch(N)
    out = qap.sinkhorn(torch.from_numpy(s), torch.from_numpy(nv), tau=1.0, iters=20)
    P, err, status = R.sinkhorn(s, nv, 1.0, 20)
    assert set(out) == {'P', 'err', 'status'} and out['status'].dtype == torch.int64
    assert np.abs(out['P'].numpy() - P).max() <= 1e-12 and np.abs(out['err'].numpy() - err).max() <= 1e-12
    assert out['status'].tolist() == status.tolist() == [0, 0, int(nv[2] == 0)]
    for b, n in enumerate(nv):
        assert not out['P'][b, n:].any() and not out['P'][b, :, n:].any()
        if n:
            assert np.abs(out['P'][b, :n, :n].sum(0).numpy() - 1.0).max() <= 1e-12


def test_host_route_small_tau_masked_tensor_and_degenerate_pairs():
    rng = np.random.default_rng(3)
    s = rng.uniform(-1, 1, (6, 9, 9)).astype(np.float32)
    s[0, 2, 3] = np.nan
    s[1, 4, 4] = np.inf
    s[2, 5, :] = -np.inf
    s[3, :, 0] = -np.inf
    s[4, 1, 2] = s[4, 7, 7] = -np.inf                      # isolated: legal
    s[5, 8, 8] = np.nan                                    # outside the corner of 8
    nv = torch.tensor([9, 9, 9, 9, 9, 8])
    out = qap.sinkhorn(MaskedTensor(torch.from_numpy(s), nv, (1, 2)), tau=0.05, iters=50)
    P, err, status = R.sinkhorn(s, nv.tolist(), 0.05, 50)
    assert out['status'].tolist() == status.tolist() == [1, 1, 1, 1, 0, 0]
    assert np.abs(out['P'].numpy() - P).max() <= 1e-12 and np.abs(out['err'].numpy() - err).max() <= 1e-12
    assert bool((out['P'][:4] == 1.0 / 9).all()) and not out['err'][:4].any()
    assert out['P'][4, 1, 2] == 0 and out['P'][4, 7, 7] == 0 and bool(torch.isfinite(out['P']).all())
    # more than FGNN_QAP_MAX_N vertices: the host route, whatever the device
    big = rng.uniform(-2, 2, (1, _lib.FGNN_QAP_MAX_N + 1, _lib.FGNN_QAP_MAX_N + 1)).astype(np.float32)
    got = qap.sinkhorn(torch.from_numpy(big), iters=3)
    assert np.abs(got['P'].numpy() - R.sinkhorn(big, None, 1.0, 3)[0]).max() <= 1e-12


def test_sinkhorn_refuses_bad_arguments():
    s = torch.zeros(2, 4, 4)
    for kw in ({'tau': 0.0}, {'tau': -1.0}, {'tau': float('nan')}, {'tau': float('inf')}, {'iters': 0}, {'iters': -3}, {'iters': 2.5},
               {'iters': True}):
        with pytest.raises(ValueError, match='tau|iters'):
            qap.sinkhorn(s, **kw)
    with pytest.raises(ValueError, match='scores'):
        qap.sinkhorn(torch.zeros(2, 4, 5))
    with pytest.raises(ValueError, match='scores'):
        qap.sinkhorn(torch.zeros(2, 4, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match='nvalid'):
        qap.sinkhorn(s, nvalid=torch.tensor([1, 2, 3]))


def test_the_signature_is_declared():
    C = _lib.C
    assert _lib._SIGNATURES['fgnn_sinkhorn'] == [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert 'fgnn_sinkhorn' in _lib.EXPORTS and _lib.FGNN_SINKHORN_LDS_MAX_N == 192
    header = open(__file__.rsplit('/tests/', 1)[0] + '/include/fgnn_hip.h').read()
    assert '#define FGNN_SINKHORN_LDS_MAX_N 192' in header and 'int fgnn_sinkhorn(const float *S, long long pair_stride, int ld,' in header


BAD_FAQ = [({'P0': 'scores', 'rounds': 3}, 'unknown key'), ({'P0': 'randomized'}, 'P0'), ({'tau': 0.0}, 'tau'), ({'tau': -2}, 'tau'),
           ({'iters': 0}, 'iters'), ({'iters': 1.5}, 'iters'), ({'maxiter': 0}, 'maxiter'), ({'maxiter': 2.0}, 'maxiter'),
           ({'tol': 0.0}, 'tol'), ('scores', 'faq must be'), (False, 'faq must be')]


@pytest.mark.parametrize('faq,match', BAD_FAQ)
def test_the_decode_checks_faq_before_any_device_work(faq, match):
    """CPU tensors: a call that got past the faq check would raise the RuntimeError of the device refusal instead"""
    s, words = torch.zeros(2, 4, 4), torch.zeros(2, 4, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match=match):
        decode_scores(s, words, words, faq=faq)
    with pytest.raises(ValueError, match=match):
        evaluate_scores(s, qap_meter=object(), bits=(words, words), faq=faq)


def test_faq_belongs_to_a_qap_meter_and_defaults():
    s = torch.zeros(2, 4, 4)
    for faq in (True, {'P0': 'barycenter'}):
        with pytest.raises(ValueError, match='faq= belongs to a qap_meter'):
            evaluate_scores(s, faq=faq)
    assert FAQ_DEFAULTS == {'P0': 'scores', 'maxiter': 30, 'tol': 0.03, 'tau': 1.0, 'iters': 20}
    # a well-formed faq gets as far as the device refusal
    words = torch.zeros(2, 4, 1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='GPU'):
        decode_scores(s, words, words, faq={'P0': 'barycenter', 'maxiter': 5})


def test_match_refuses_faq_on_weighted_batches():
    from graph_neural_net_amd.siamese import Siamese_Node_Exp
    ne = dict(type='node_embedding', block_init='block_emb', block_inside='block', num_blocks=2, in_features=32, out_features=32,
              depth_of_mlp=3)
    model = Siamese_Node_Exp(2, ne)
    x = torch.zeros(1, 2, 4, 4)
    with pytest.raises(NotImplementedError, match='faq'):
        model.match(x, x, weighted=True, faq=True)
    with pytest.raises(ValueError, match='unknown key'):
        model.match(x, x, faq={'start': 'scores'})
