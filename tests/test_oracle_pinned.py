"""CPU: the oracle is torch.equal to the reference -- scores, loss, every gradient and every intermediate of the node embedder -- on
the reference's own results of a perturbed 2-block model (tests/golden/oracle_pin_er_n17_b3_2blk.npz, `make_golden.py pins`, which
checks the same equality against the imported reference before it writes the file)."""
import torch

from oracle import fgnn_oracle as O
from util import load_golden, sub


def test_oracle_bit_equal_to_reference():
    d = load_golden('oracle_pin_er_n17_b3_2blk.npz')
    sd = sub(d, 'sd/')
    threads = torch.get_num_threads()
    torch.set_num_threads(1)            # ATen's CPU gradients depend on the thread count: the fixture was made with one thread
    try:
        s, l, g = O.step_fwd_bwd(d['x1'], d['x2'], sd)
        keep = {}
        O.node_embedding(d['x1'], sd, keep)
    finally:
        torch.set_num_threads(threads)
    assert torch.equal(s, d['scores']), 'scores differ'
    assert torch.equal(l, d['loss']), 'loss differs'
    ref = sub(d, 'grad/')
    assert sorted(g) == sorted(ref)
    for k, v in ref.items():
        assert torch.equal(g[k], v), 'gradient %s differs' % k
    inter = sub(d, 'inter/')
    assert inter and sorted(keep) == sorted(inter)
    for k, v in inter.items():
        assert torch.equal(keep[k], v), 'intermediate %s differs' % k
