"""The argument checks of fgnn_mlp_bwd16 and fgnn_mlp_bwd16_pair: every refusal returns 1 with its exact fgnn_last_error() text, before
any launch (no GPU needed).  Pointers are small non-null integers that are never dereferenced; every case has exactly one fault, so
the text does not depend on the order of the checks; no case passes all of them.  One refusal of the pair entry has no case: its
workgroup count is compared with fgnn_mlp_bwd's, two constants of one build."""
import pytest

from graph_neural_net_amd import _lib

PTR = 16
ONE, PAIR = 'fgnn_mlp_bwd16', 'fgnn_mlp_bwd16_pair'
N, LDR, LDP = 5, 8, 64          # 5 x 5 pixels in rows of 8, channel stride = one 64-element tile
MISSING = '%s: missing dy/z/wpart/coef'
TOO_BIG = '%s: a tensor exceeds 2 GiB (32-bit buffer addressing); split the batch'
S12_ONE = ('fgnn_mlp_bwd16: s12part needs dxa and either a single normalised 32-channel slab or a raw first slab of a two-slab MLP')
CHANNELS = 'fgnn_mlp_bwd16: unsupported input channels (%d + %d); built for 2, 32, 32+2, 32+32'
PAIR_SHAPE = 'fgnn_mlp_bwd16_pair: the two MLPs must share G, N and ldr (G=%d N=%d ldr=%d)'
PAIR_SLABS = 'fgnn_mlp_bwd16_pair: ONE input slab of 2 or 32 channels (got %d + %d); use fgnn_mlp_bwd16'
PAIR_SAME = 'fgnn_mlp_bwd16_pair: the two MLPs must read the same input slab'
PAIR_S12 = 'fgnn_mlp_bwd16_pair: s12part needs dxa and a normalised 32-channel slab'
PAIR_FIRST = 'fgnn_mlp_bwd16_pair: the input gradient and its tile sums belong to the SECOND argument block'


def good_args(ca=32, cb=0):
    """G = 2 graphs of N = 5, depth 3, no input gradient: arguments that only lack real memory."""
    a = _lib.MlpBwd16Args()
    a.G, a.N, a.ldr, a.depth = 2, N, LDR, 3
    a.a.ptr, a.a.gstride, a.a.ldp, a.a.C = PTR, ca * LDP, LDP, ca
    if cb:
        a.b.ptr, a.b.gstride, a.b.ldp, a.b.C = PTR, cb * LDP, LDP, cb
    a.dy = a.z = a.coef = a.wpart = a.packed = PTR
    a.dgstride = a.zgstride = 32 * LDP
    a.ldd = a.ldz = LDP
    return a


def with_dx(a, nrm=True):
    """... with the gradient of slab a, which is normalised (what s12part wants of a single slab) unless `nrm` is off"""
    a.dxa, a.dxa_gstride, a.dxa_ld = PTR, 32 * LDP, LDP
    if nrm:
        a.a.nrm = PTR
    return a


def change(a, **kw):
    for k, v in kw.items():
        obj = a
        *path, leaf = k.split('__')
        for p in path:
            obj = getattr(obj, p)
        setattr(obj, leaf, v)
    return a


def good_pair(ca=32, dx=False):
    a1, a2 = good_args(ca), good_args(ca)
    if dx:
        a1.a.nrm = PTR
        with_dx(a2)
    return a1, a2


def pair(which=None, ca=32, dx=False, **kw):
    """the pair's arguments with one block (0, 1) or both (None) changed"""
    blocks = good_pair(ca, dx)
    for i in ((0, 1) if which is None else (which,)):
        change(blocks[i], **kw)
    return blocks


def second(blocks, **kw):
    change(blocks[1], **kw)
    return blocks


# (arguments, text) per entry
ONE_CASES = [
    (lambda: change(good_args(), G=0), 'fgnn_mlp_bwd16: bad G=0 N=5 ldr=8'),
    (lambda: change(good_args(), N=-1), 'fgnn_mlp_bwd16: bad G=2 N=-1 ldr=8'),
    (lambda: change(good_args(), ldr=0), 'fgnn_mlp_bwd16: bad G=2 N=5 ldr=0'),             # ldr < N
    (lambda: change(good_args(), ldr=12), 'fgnn_mlp_bwd16: bad G=2 N=5 ldr=12'),           # no multiple of 8
    (lambda: change(good_args(), depth=2), 'fgnn_mlp_bwd16: built for depth_of_mlp = 3 (got 2)'),
    (lambda: change(good_args(), depth=4), 'fgnn_mlp_bwd16: built for depth_of_mlp = 3 (got 4)'),
    (lambda: change(good_args(), a__ptr=None), 'fgnn_mlp_bwd16: slab a / operand image missing'),
    (lambda: change(good_args(), a__C=0), 'fgnn_mlp_bwd16: slab a / operand image missing'),
    (lambda: change(good_args(), packed=None), 'fgnn_mlp_bwd16: slab a / operand image missing'),
    (lambda: change(good_args(cb=2), b__ptr=None), 'fgnn_mlp_bwd16: slab b has channels but no pointer'),
    (lambda: change(good_args(cb=32), b__ptr=None), 'fgnn_mlp_bwd16: slab b has channels but no pointer'),
] + [(lambda f=f: change(good_args(), **{f: None}), MISSING % ONE) for f in ('dy', 'z', 'wpart', 'coef')] + [
    (lambda f=f: change(good_args(cb=32), **{f: 1 << 29}), TOO_BIG % ONE)
    for f in ('a__gstride', 'dgstride', 'zgstride', 'dxa_gstride', 'b__gstride', 'dxb_gstride')
] + [
    # s12part: dxa, 32 channels in slab a, and a normalised single slab or a raw first slab of two
    (lambda: change(good_args(), a__nrm=PTR, s12part=PTR), S12_ONE),                        # no dxa
    (lambda: change(with_dx(good_args(), nrm=False), s12part=PTR), S12_ONE),               # single slab, not normalised
    (lambda: change(with_dx(good_args(cb=2)), s12part=PTR), S12_ONE),                      # two slabs, the first normalised
    (lambda: change(with_dx(good_args(cb=32)), s12part=PTR), S12_ONE),
    # channel pairs no kernel is built for
    (lambda: good_args(ca=16), CHANNELS % (16, 0)),
    (lambda: good_args(ca=7), CHANNELS % (7, 0)),
    (lambda: good_args(ca=2, cb=2), CHANNELS % (2, 2)),
    (lambda: good_args(ca=2, cb=32), CHANNELS % (2, 32)),
    (lambda: good_args(ca=32, cb=16), CHANNELS % (32, 16)),
    (lambda: change(good_args(ca=32), b__C=-1, b__ptr=PTR), CHANNELS % (32, -1)),
]
PAIR_CASES = [
    (lambda: pair(G=0), PAIR_SHAPE % (0, 5, 8)),
    (lambda: pair(N=-1), PAIR_SHAPE % (2, -1, 8)),
    (lambda: pair(ldr=0), PAIR_SHAPE % (2, 5, 0)),
    (lambda: pair(ldr=12), PAIR_SHAPE % (2, 5, 12)),
    (lambda: pair(1, G=3), PAIR_SHAPE % (2, 5, 8)),               # the text names the first block's figures
    (lambda: pair(1, N=4), PAIR_SHAPE % (2, 5, 8)),
    (lambda: pair(1, ldr=16), PAIR_SHAPE % (2, 5, 8)),
    (lambda: pair(0, depth=2), 'fgnn_mlp_bwd16_pair: built for depth_of_mlp = 3'),
    (lambda: pair(1, depth=4), 'fgnn_mlp_bwd16_pair: built for depth_of_mlp = 3'),
    (lambda: pair(a__C=16), PAIR_SLABS % (16, 0)),
    (lambda: pair(a__C=0), PAIR_SLABS % (0, 0)),
    (lambda: pair(0, b__C=2, b__ptr=PTR), PAIR_SLABS % (32, 2)),
    (lambda: pair(1, b__C=32, b__ptr=PTR), PAIR_SLABS % (32, 0)),
    (lambda: pair(a__ptr=None), PAIR_SAME),
    (lambda: pair(1, a__ptr=2 * PTR), PAIR_SAME),
    (lambda: pair(1, ca=2, a__C=32), PAIR_SAME),
    (lambda: pair(1, a__gstride=64 * LDP), PAIR_SAME),
    (lambda: pair(1, a__ldp=2 * LDP), PAIR_SAME),
    (lambda: pair(1, a__nrm=PTR), PAIR_SAME),
    (lambda: pair(0, a__beta=PTR), PAIR_SAME),
    (lambda: pair(1, nvalid=PTR), PAIR_SAME),
    (lambda: pair(0, ranges=PTR), 'fgnn_mlp_bwd16_pair: constant-size batches only; use fgnn_mlp_bwd16'),
    (lambda: pair(1, ranges=PTR), 'fgnn_mlp_bwd16_pair: constant-size batches only; use fgnn_mlp_bwd16'),
    (lambda: pair(nvalid=PTR), 'fgnn_mlp_bwd16_pair: constant-size batches only; use fgnn_mlp_bwd16'),
    (lambda: pair(0, packed=None), 'fgnn_mlp_bwd16_pair: needs both operand images (fgnn_pack16_operands, kind 1)'),
    (lambda: pair(1, packed=None), 'fgnn_mlp_bwd16_pair: needs both operand images (fgnn_pack16_operands, kind 1)'),
    (lambda: pair(0, dx=True, dxa=PTR), PAIR_FIRST),
    (lambda: pair(0, dx=True, s12part=PTR), PAIR_FIRST),
    (lambda: pair(1, ca=2, dxa=PTR), 'fgnn_mlp_bwd16_pair: the input gradient exists for the 32-channel slab only'),
    (lambda: second(pair(a__nrm=PTR), s12part=PTR), PAIR_S12),                             # no dxa
    (lambda: (good_args(), change(with_dx(good_args(), nrm=False), s12part=PTR)), PAIR_S12),       # not normalised
] + [(lambda i=i, f=f: pair(i, **{f: None}), MISSING % PAIR) for i in (0, 1) for f in ('dy', 'z', 'wpart', 'coef')] + [
    (lambda i=i, f=f: pair(i, **{f: 1 << 29}), TOO_BIG % PAIR) for i in (0, 1) for f in ('dgstride', 'zgstride', 'dxa_gstride')
] + [
    (lambda: pair(a__gstride=1 << 29), TOO_BIG % PAIR),            # (one block alone would no longer read the same slab)
]
CASES = [(ONE, mk, text) for mk, text in ONE_CASES] + [(PAIR, mk, text) for mk, text in PAIR_CASES]


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def refused(lib, fn, args):
    args = args if isinstance(args, tuple) else (args,)
    assert getattr(lib, fn)(*args, None) == 1
    return lib.fgnn_last_error().decode()


def test_null_args(lib):
    assert refused(lib, ONE, (None,)) == 'fgnn_mlp_bwd16: null args'
    a = good_args()
    for args in ((None, None), (a, None), (None, a)):
        assert refused(lib, PAIR, args) == 'fgnn_mlp_bwd16_pair: null args'


@pytest.mark.parametrize('case', range(len(CASES)))
def test_refusal(lib, case):
    fn, make, text = CASES[case]
    assert refused(lib, fn, make()) == text


def test_slab_b_strides_do_not_count_without_slab_b(lib):
    """The pair entry checks no slab-b stride (its MLPs have one slab): with a huge one the next check refuses, not the 2 GiB one."""
    for f in ('b__gstride', 'dxb_gstride'):
        assert refused(lib, PAIR, pair(0, **{f: 1 << 29, 'dy': None})) == MISSING % PAIR


def test_too_many_tiles(lib):
    """A batch of 2^30 tiles or more is refused with '<entry>: too many tiles': these entries bound no stride by N * ldr, so small
    strides carry such a batch past the 2 GiB check."""
    def huge(a):
        return change(a, G=1 << 20, N=256, ldr=256, a__gstride=0, dgstride=0, zgstride=0)
    assert (1 << 20) * lib.fgnn_tiles_per_graph16(256, 256) >= 1 << 30
    assert refused(lib, ONE, huge(good_args())) == 'fgnn_mlp_bwd16: too many tiles'
    assert refused(lib, PAIR, tuple(huge(a) for a in good_pair())) == 'fgnn_mlp_bwd16_pair: too many tiles'
