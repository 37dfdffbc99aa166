"""Records tests/golden/bf16_c2_digest.json: sha256 digests of (scores, loss, flat gradient) of the 2-channel bf16 engine on the cases
of tests/test_gpu_bf16_inputs.py::c2_digests, or, with the argument `nopair`, tests/golden/bf16_c2_nopair_digest.json: its dense cases
with FgnnEngineBF16.PAIR_BWD off (c2_digests(pair_bwd=False)).  Needs a GPU.  To record the digests of another build of the library,
point FGNN_LIB at it (graph_neural_net_amd/_lib.py):

    FGNN_LIB=/path/to/libfgnn_hip.so python tests/golden/make_bf16_c2_digest.py [nopair] [output.json]

bf16_c2_digest.json was recorded with the library of the commit before the bf16 engine learnt 32-channel input slabs; the test asserts
that the 2-channel path still produces these bits.  bf16_c2_nopair_digest.json was recorded with the library of commit 0ebc75b ("Run
inputs of 1 to 32 channels, spectral pairs included, in bf16"), the commit before mlp_bwd16.hip and mlp_bwd16_pair.hip took their
common tile body from fgnn_bwd16.h as macros."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

if __name__ == '__main__':
    from graph_neural_net_amd import _lib
    _lib.load(allow_missing=True)        # an older build lacks the newer entry points: the 2-channel path calls none of them
    from test_gpu_bf16_inputs import c2_digests
    argv = sys.argv[1:]
    nopair = argv[:1] == ['nopair']
    out = argv[nopair] if len(argv) > nopair else os.path.join(HERE, 'bf16_c2_nopair_digest.json' if nopair else 'bf16_c2_digest.json')
    with open(out, 'w') as f:
        json.dump(c2_digests(pair_bwd=not nopair), f, indent=1, sort_keys=True)
        f.write('\n')
    print(open(out).read())
