"""CPU: the host side of the 1 .. 32-channel bf16 input path -- the new entry point is declared, bound and exported alike, and the
padded layout a 16-bit module runs on is the fp32 one."""
import os
import re

import torch

from graph_neural_net_amd import _lib
from graph_neural_net_amd.siamese import Siamese_Node_Exp
from util import ROOT

NE = dict(type='node_embedding', block_init='block_emb', block_inside='block', num_blocks=2, in_features=32, out_features=32,
          depth_of_mlp=3)
CTYPES = {'const float *': 'c_void_p', 'const int *': 'c_void_p', 'void *': 'c_void_p', 'int': 'c_int', 'long long': 'c_longlong'}


def test_header_binding_and_library_agree_on_the_conversion_entry_point():
    hdr = open(os.path.join(ROOT, 'include', 'fgnn_hip.h')).read()
    m = re.search(r'int fgnn_to_bf16_pad\(([^)]*)\)', hdr)
    assert m, 'include/fgnn_hip.h does not declare fgnn_to_bf16_pad'
    params = [re.sub(r'\s+', ' ', p.strip()) for p in m.group(1).split(',')]
    names = [re.search(r'(\w+)$', p).group(1) for p in params]
    assert names == ['x', 'nvalid', 'G', 'c', 'CP', 'N', 'ldr', 'y', 'ldp', 'stream']
    types = [re.sub(r'\s*\w+$', '', p).replace(' *', '*').replace('*', ' *') for p in params]
    want = [getattr(_lib.C, CTYPES[t]) for t in types]
    got = list(_lib._SIGNATURES['fgnn_to_bf16_pad'])
    assert got == want, (got, want)
    assert 'fgnn_to_bf16_pad' in _lib.EXPORTS
    assert hasattr(_lib.load(), 'fgnn_to_bf16_pad')
    assert _lib.load().fgnn_to_bf16_pad.restype is _lib.C.c_int


def test_the_padded_layout_of_a_16_bit_module_is_the_fp32_one():
    for c0, width in ((4, 32), (3, 16), (4, 24), (1, 32), (31, 8)):
        ne = dict(NE, in_features=width, out_features=width)
        torch.manual_seed(0)
        a, b = Siamese_Node_Exp(c0, ne), Siamese_Node_Exp(c0, ne).half()
        assert b.node_embedder.precision == 'bf16' and all(p.dtype == torch.float32 for p in b.parameters())      # nothing is cast
        la, lb = a.node_embedder._standard_layout(), b.node_embedder._standard_layout()
        pa, pb = a.node_embedder._pad, b.node_embedder._pad
        assert la.c0 == lb.c0 == (2 if c0 <= 2 else 32) and la.total == lb.total and la.entries == lb.entries
        assert torch.equal(pa['idx'], pb['idx']) and {k: pa[k] for k in ('c0', 'c0p', 'cout', 'total')} == {k: pb[k] for k in ('c0', 'c0p', 'cout', 'total')}
        assert pa['idx'].numel() == sum(p.numel() for p in a.parameters()) and pa['idx'].unique().numel() == pa['idx'].numel()
