"""Records tests/golden/bf16c32_n{33,50}_b2_2blk.npz: the reference's own model with original_features_num = 32 (2 blocks, perturbed
biases / GraphNorm affine) run in fp32, fp64 and -- the Network.half recipe, make_golden.ref_step_bf16 -- in bf16 on a random
(2, 32, N, N) pair batch.  tests/test_gpu_bf16_inputs.py gates the 32-channel bf16 engine against them at the margin the other
multi-block reference fixtures use (util.BF16_CLASS x the reference-bf16 distance to the fp64 truth): on these two shapes the engine
and the same-point oracle take enough different discrete decisions (ReLU masks, pooling arg-max) that their distance, although far
below the bf16 error itself, is 0.6 - 0.9 x the oracle's own distance to the un-rounded evaluation, beyond the 0.5 x same-point gate.

The inputs are not stored (1.3 MB): bf16c32_inputs() regenerates them from the seed and the fixture holds their sha256.

    python tests/golden/make_bf16_c32.py          (needs the reference checkout, like make_golden.py)"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE]

SHAPES = ((33, 2), (50, 2))


def bf16c32_inputs(N, B):
    """The batch of tests/test_gpu_bf16_inputs.py::test_c32_engine_* for (N, B), and its sha256."""
    gen = torch.Generator().manual_seed(N)
    x1, x2 = torch.randn(B, 32, N, N, generator=gen), torch.randn(B, 32, N, N, generator=gen)
    return x1, x2, hashlib.sha256(x1.numpy().tobytes() + x2.numpy().tobytes()).hexdigest()


if __name__ == '__main__':
    import make_golden as M
    M.import_reference()
    from models.trainers import Siamese_Node_Exp
    torch.set_num_threads(8)
    for N, B in SHAPES:
        torch.manual_seed(40 + N)
        model = Siamese_Node_Exp(32, dict(M.NODE_EMB, num_blocks=2))
        M.perturb_(model, 41 + N)
        x1, x2, digest = bf16c32_inputs(N, B)
        s, l, g = M.ref_step(model, x1, x2)
        s64, l64, g64 = M.ref_step(M.f64(model), x1.double(), x2.double())
        s16, l16, g16 = M.ref_step_bf16(model, x1, x2)
        d = {'n': np.array(N), 'b': np.array(B), 'x_sha256': np.frombuffer(bytes.fromhex(digest), dtype=np.uint8), 'scores': s.numpy(), 'scores64_as_f32': s64.float().numpy(),
             'scores_refbf16': s16.numpy(), 'loss': l.numpy(), 'loss64': l64.numpy(), 'loss_refbf16': l16.numpy()}
        for k, v in model.state_dict().items():
            d['sd/' + k[len('node_embedder.'):]] = v.numpy()
        for tag, gg in (('grad/', g), ('grad64/', g64), ('grad_refbf16/', g16)):
            for k, v in gg.items():
                d[tag + k] = v.float().numpy()
        out = os.path.join(HERE, 'bf16c32_n%d_b%d_2blk.npz' % (N, B))
        np.savez_compressed(out, **d)
        names = [k for k in g if not k.endswith('convs.2.bias')]
        flat = lambda gg: torch.cat([gg[k].reshape(-1).double() for k in names])
        l2 = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
        print('%s: %d bytes; reference bf16 vs fp64: scores %.3e, flat gradient %.3e, loss %.3e' %
              (os.path.basename(out), os.path.getsize(out), l2(s16, s64), l2(flat(g16), flat(g64)), abs(l16.item() - l64.item())))
