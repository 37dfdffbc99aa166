"""GPU: fgnn_spectral_slab16 (csrc/spectral_slab.hip) -- the spectral features straight into the bf16 input slab.

The specification is an identity: the slab equals, byte for byte, fgnn_to_bf16_pad applied to what fgnn_spectral_features writes for
the same words.  Every case pre-fills the slab with 0xFF bytes (a NaN pattern no path writes) and compares the WHOLE buffer, so a
byte the launch leaves out shows as well as a wrong one.  Shapes: the NW template edges (32 / 33, 64 / 65, 128 / 129, 256), the
32-row panel edges, odd N, a lone last column (33, 65, 129), N = 1."""
import numpy as np
import pytest
import torch

import spectral_slab_ref as SR
from graph_neural_net_amd import _lib
from graph_neural_net_amd.spectral import spectral_features

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = [1, 7, 31, 32, 33, 50, 64, 65, 128, 129, 200, 256]


def _pack(w, garbage=None):
    """(G, N, N) bool -> (G, N, ceil(N/32)) int32 words; garbage: (G, N, 32 * words) bool OR-ed in at the columns >= N"""
    G, N, _ = w.shape
    words = (N + 31) // 32
    full = np.zeros((G, N, 32 * words), dtype=bool)
    if garbage is not None:
        full[:, :, N:] = garbage[:, :, N:]
    full[:, :, :N] = w
    by = np.packbits(full.reshape(G, N, words, 32), axis=-1, bitorder='little')
    return torch.from_numpy(np.ascontiguousarray(by).view('<u4').reshape(G, N, words).view(np.int32))


def _graphs(N, seed):
    """G = 5 graphs: density 0.2, density 0.5, an asymmetric W, one with isolated vertices, the empty graph"""
    r = np.random.RandomState(seed)
    def sym(p):
        u = np.triu(r.rand(N, N) < p, 1)
        return u | u.T
    iso = sym(0.4)
    dead = r.rand(N) < 0.3
    iso[dead, :] = False
    iso[:, dead] = False
    return np.stack([sym(0.2), sym(0.5), r.rand(N, N) < 0.3, iso, np.zeros((N, N), dtype=bool)])


def _ragged(N, variant):
    """vertex counts with 0, 1, N, a count <= N - 32 (whole panels in the padding, where N allows) and counts outside [0, N]"""
    if variant == 0:
        return [N, 1, 0, max(N - 32 - N % 5, 0), N + 9]
    return [-3, (N + 1) // 2, N, max(N - 33, 1), N - 1 if N > 1 else 1]


def _both(bits, nv, G, N, P, CP, ldr, ldp):
    st = _lib.stream_ptr()
    got = torch.full((G * CP * ldp,), -1, dtype=torch.int16, device=DEV)          # 0xFF bytes
    _lib.call('fgnn_spectral_slab16', _lib.ptr(bits), _lib.ptr(nv), G, N, P, CP, ldr, _lib.ptr(got), ldp, st)
    want = torch.full((G * CP * ldp,), -1, dtype=torch.int16, device=DEV)
    f = spectral_features(bits, nv, P)
    _lib.call('fgnn_to_bf16_pad', _lib.ptr(f), _lib.ptr(nv), G, P, CP, N, ldr, _lib.ptr(want), ldp, st)
    return got, want, f


@pytest.mark.parametrize('N', SIZES)
def test_slab_equals_features_then_conversion(N):
    w = _graphs(N, 7 * N + 1)
    G = w.shape[0]
    clean = _pack(w).to(DEV)
    r = np.random.RandomState(N)
    dirty = _pack(w, garbage=r.rand(G, N, 32 * ((N + 31) // 32)) < 0.5).to(DEV)      # set bits past column N: ignored
    ldr, ldp = SR.pitches(N)
    for variant in (None, 0, 1):
        nv = None if variant is None else torch.tensor(_ragged(N, variant), dtype=torch.int32, device=DEV)
        for CP, P in ((2, 1), (2, 2), (32, 1), (32, 4), (32, 8)):
            got, want, f = _both(dirty, nv, G, N, P, CP, ldr, ldp)
            assert torch.equal(got, want), (N, variant, CP, P, (got != want).nonzero()[:4].flatten().tolist())
            if variant != 1:
                continue
            # ragged: the words hold the full N x N graphs, so everything outside the n_g x n_g corner is a set bit to ignore; and the
            # numpy restatement of the layout gives the same bytes from the fp32 features
            ref = SR.slab(f.cpu().numpy(), nv.cpu().tolist(), CP, ldr, ldp)
            assert np.array_equal(got.cpu().numpy().view(np.uint16).reshape(G, CP, ldp), ref), (N, CP, P)
        got_clean = _both(clean, nv, G, N, 4, 32, ldr, ldp)[0]
        assert torch.equal(got_clean, _both(dirty, nv, G, N, 4, 32, ldr, ldp)[0]), (N, variant)


@pytest.mark.parametrize('N,extra_ldr,extra_ldp', [(33, 8, 0), (50, 0, 64), (32, 8, 64), (129, 8, 64)])
def test_slab_with_slack_in_the_pitches(N, extra_ldr, extra_ldp):
    """pitch columns beyond N rounded up to 8 (N = 32 with ldr = 40: past the last staged word) and a channel tail of its own"""
    w = _graphs(N, 3 * N)[:3]
    G = w.shape[0]
    bits = _pack(w).to(DEV)
    ldr, ldp = SR.pitches(N, extra_ldr, extra_ldp)
    for nv in (None, torch.tensor([N - 1, N, max(N - 40, 0)], dtype=torch.int32, device=DEV)):
        for CP, P in ((2, 2), (32, 4)):
            got, want, _ = _both(bits, nv, G, N, P, CP, ldr, ldp)
            assert torch.equal(got, want), (N, CP, P)


def test_values_are_the_rounded_fp32_features():
    """one direct look, independent of fgnn_to_bf16_pad: channel p of the slab = torch's bf16 rounding of the fp32 features"""
    N, G, P = 50, 5, 4
    bits = _pack(_graphs(N, 5)).to(DEV)
    ldr, ldp = SR.pitches(N)
    got, _, f = _both(bits, None, G, N, P, 32, ldr, ldp)
    slab = got.view(G, 32, ldp)
    vals = slab[:, :P, :N * ldr].reshape(G, P, N, ldr)
    assert torch.equal(vals[..., :N], f.to(torch.bfloat16).view(torch.int16)) and not bool(vals[..., N:].any())
    assert not bool(slab[:, P:].any()) and not bool(slab[:, :, N * ldr:].any())
    assert bool(vals[:3].any())


def test_refusals():
    N, G = 20, 3
    bits = _pack(_graphs(N, 1)[:G]).to(DEV)
    ldr, ldp = SR.pitches(N)
    y = torch.zeros(G * 32 * (ldp + 64), dtype=torch.int16, device=DEV)
    ok = dict(N=N, P=4, CP=32, ldr=ldr, ldp=ldp)
    for kw, msg in ((dict(P=3, CP=2), 'powers'), (dict(P=0), 'powers'), (dict(P=9), 'powers'), (dict(CP=4), '2 or 32 channels'),
                    (dict(CP=16), '2 or 32 channels'), (dict(ldr=N + 2), 'ldr'), (dict(ldr=16), 'ldr'), (dict(ldp=ldp + 8), 'ldp'),
                    (dict(ldp=ldp - 64), 'ldp'), (dict(N=257, ldr=264, ldp=257 * 264 + 56), 'vertices')):
        a = dict(ok, **kw)
        with pytest.raises(RuntimeError, match='fgnn_spectral_slab16.*' + msg):
            _lib.call('fgnn_spectral_slab16', _lib.ptr(bits), None, G, a['N'], a['P'], a['CP'], a['ldr'], _lib.ptr(y), a['ldp'],
                      _lib.stream_ptr())
    with pytest.raises(RuntimeError, match='fgnn_spectral_slab16'):
        _lib.call('fgnn_spectral_slab16', None, None, G, N, 4, 32, ldr, _lib.ptr(y), ldp, _lib.stream_ptr())
