"""The argument checks of fgnn_mlp_fwd and fgnn_mlp_fwd_x3: every refusal returns 1 with its exact fgnn_last_error() text, before any
launch (no GPU needed).  Pointers are small non-null integers that are never dereferenced; every case has exactly one fault, so
the text does not depend on the order of the checks; no case passes all of them."""
import pytest

from graph_neural_net_amd import _lib

PTR = 16
FP32, X3 = 'fgnn_mlp_fwd', 'fgnn_mlp_fwd_x3'
X3_BUILT = ('fgnn_mlp_fwd_x3: built for depth 3 and 2, 32, 32+2, 32+32 input channels (got depth %d, %d + %d, nmlp %d); '
            'use fgnn_mlp_fwd')
FP32_CHANNELS = 'fgnn_mlp_fwd: unsupported input channels (%d + %d) for nmlp=%d; built for 2, 16, 32 and, with nmlp=1, 32+2, 32+32'
TOO_BIG = '%s: a tensor exceeds 2 GiB (32-bit buffer addressing); split the batch'


def good_args(nmlp=1, ca=32, cb=0):
    """G = 2 graphs of N = 5 (25 pixels in rows of 32), depth 3: arguments that only lack real memory."""
    a = _lib.MlpFwdArgs()
    a.G, a.N, a.depth, a.nmlp = 2, 5, 3, nmlp
    a.a.ptr, a.a.gstride, a.a.ldp, a.a.C = PTR, ca * 32, 32, ca
    if cb:
        a.b.ptr, a.b.gstride, a.b.ldp, a.b.C = PTR, cb * 32, 32, cb
    for m in range(nmlp):
        for l in range(3):
            a.W[m][l] = a.bias[m][l] = PTR
        a.z[m] = a.part[m] = PTR
    a.ldz = 32
    a.cnt = a.packed = PTR
    return a


def with_xbits(a):
    a.xbits = a.xdeg = PTR
    return a


def change(a, **kw):
    for k, v in kw.items():
        obj = a
        *path, leaf = k.split('__')
        for p in path:
            obj = getattr(obj, p)
        setattr(obj, leaf, v)
    return a


def no_weight(a):
    a.W[0][1] = None
    return a


def no_output(a, m, field):
    getattr(a, field)[m] = None
    return a


# (entry, arguments, the text after "<entry>: " or the whole text)
SHARED = [      # refusals the two entries word alike, apart from their name
    ('bad G=0 N=5', lambda: change(good_args(), G=0)),
    ('bad G=2 N=-1', lambda: change(good_args(), N=-1)),
    ('nmlp must be 1 or 2 (got 3)', lambda: change(good_args(), nmlp=3)),
    ('xbits without xdeg (fgnn_adjacency_degree)', lambda: change(good_args(), xbits=PTR)),
    ('channel stride < N*N', lambda: change(good_args(), ldz=24)),
    ('channel stride < N*N', lambda: change(good_args(), a__ldp=24)),
    ('missing output 0', lambda: no_output(good_args(), 0, 'z')),
    ('missing output 1', lambda: no_output(good_args(nmlp=2), 1, 'part')),
    ('missing cnt', lambda: change(good_args(), cnt=None)),
    (TOO_BIG[4:], lambda: change(good_args(), a__gstride=1 << 30)),
    (TOO_BIG[4:], lambda: change(good_args(cb=2), b__gstride=1 << 30)),
    (TOO_BIG[4:], lambda: change(good_args(), ldz=1 << 24)),
]
CASES = [(fn, mk, '%s: %s' % (fn, text)) for fn in (FP32, X3) for text, mk in SHARED] + [
    (FP32, lambda: change(good_args(), depth=0), 'fgnn_mlp_fwd: depth 0 not in 1..3'),
    (FP32, lambda: change(good_args(), depth=4), 'fgnn_mlp_fwd: depth 4 not in 1..3'),
    (X3, lambda: change(good_args(), depth=2), X3_BUILT % (2, 32, 0, 1)),
    (FP32, lambda: change(good_args(), a__ptr=None), 'fgnn_mlp_fwd: slab a missing'),
    (FP32, lambda: change(good_args(), a__C=0), 'fgnn_mlp_fwd: slab a missing'),
    (X3, lambda: change(good_args(), a__ptr=None), 'fgnn_mlp_fwd_x3: slab pointer missing'),
    (FP32, lambda: change(good_args(cb=2), b__ptr=None), 'fgnn_mlp_fwd: slab b has channels but no pointer'),
    (X3, lambda: change(good_args(cb=2), b__ptr=None), 'fgnn_mlp_fwd_x3: slab pointer missing'),
    (FP32, lambda: no_weight(good_args()), 'fgnn_mlp_fwd: missing weights mlp 0 layer 1'),
    (FP32, lambda: change(good_args(), ranges=PTR), 'fgnn_mlp_fwd: ranges (fgnn_ragged_tile_ranges) only make sense with nvalid'),
    (X3, lambda: change(good_args(), ranges=PTR, nvalid=PTR),
     'fgnn_mlp_fwd_x3: no padding-tile skipping (ranges); use fgnn_mlp_fwd for ragged batches'),
    (X3, lambda: change(good_args(), packed=None), 'fgnn_mlp_fwd_x3: needs the operand image of fgnn_pack_x3_operands'),
    # channel pairs no kernel is built for (16 + 0 IS an fp32 form, with one MLP or two: only the x3 entry refuses it)
    (FP32, lambda: good_args(ca=7), FP32_CHANNELS % (7, 0, 1)),
    (FP32, lambda: good_args(nmlp=2, ca=7), FP32_CHANNELS % (7, 0, 2)),
    (FP32, lambda: good_args(nmlp=2, cb=2), FP32_CHANNELS % (32, 2, 2)),
    (X3, lambda: good_args(ca=7), X3_BUILT % (3, 7, 0, 1)),
    (X3, lambda: good_args(nmlp=2, ca=16), X3_BUILT % (3, 16, 0, 2)),
    (X3, lambda: good_args(nmlp=2, cb=2), X3_BUILT % (3, 32, 2, 2)),
    # the bit-packed input
    (FP32, lambda: with_xbits(change(good_args(ca=2), depth=2, a__ptr=None)),
     'fgnn_mlp_fwd: xbits needs depth 3 and a 2-channel slab (2 or 32+2 input channels), got depth 2, 2 + 0'),
    (FP32, lambda: with_xbits(good_args()),
     'fgnn_mlp_fwd: xbits needs depth 3 and a 2-channel slab (2 or 32+2 input channels), got depth 3, 32 + 0'),
    (X3, lambda: with_xbits(change(good_args(ca=2), depth=2, a__ptr=None)), X3_BUILT % (2, 2, 0, 1)),
    (X3, lambda: with_xbits(good_args()), 'fgnn_mlp_fwd_x3: xbits needs a 2-channel slab'),
]


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def test_null_args(lib):
    for fn in (FP32, X3):
        assert getattr(lib, fn)(None, None) == 1
        assert lib.fgnn_last_error().decode() == '%s: null args' % fn


@pytest.mark.parametrize('case', range(len(CASES)))
def test_refusal(lib, case):
    fn, make, text = CASES[case]
    assert getattr(lib, fn)(make(), None) == 1
    assert lib.fgnn_last_error().decode() == text


def test_too_many_tiles(lib):
    """A batch of 2^30 tiles or more is refused.  '<entry>: too many tiles' itself cannot be the text: the checks before it want
    N * N <= ldz and G * 32 * ldz < 2^29 floats, which leaves G * ceil(N * N / 32) below 2^19 + 2^24, so what refuses such a batch is
    the 2 GiB limit."""
    for fn in (FP32, X3):
        a = change(good_args(), G=1 << 20, N=200, ldz=200 * 200)
        a.a.ldp, a.a.gstride = 200 * 200, 32 * 200 * 200
        assert a.G * lib.fgnn_tiles_per_graph(a.N) >= 1 << 30
        assert getattr(lib, fn)(a, None) == 1
        assert lib.fgnn_last_error().decode() == TOO_BIG % fn
