"""Rate of the on-device QAP pair generator (graph_neural_net_amd/pairgen.py) on the shapes the training step eats, plus the
reference's whole default dataset (default_config.yaml: 20 000 train + 1 000 val pairs, Regular N = 50, ER noise 0.1).
Device events around the launches, after one warm-up call per shape.  usage: python tools/gpu_pairgen_rate.py [reps]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graph_neural_net_amd.pairgen import PairGenerator

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
DEV = torch.device('cuda:0')
SHAPES = [
    ('cfg2 batch: Regular N=50, B=32, ER noise', dict(n_vertices=50), 32),
    ('Regular N=50, B=32, EdgeSwap noise', dict(n_vertices=50, noise_model='EdgeSwap'), 32),
    ('BarabasiAlbert N=50, B=32, ER noise', dict(n_vertices=50, generative_model='BarabasiAlbert'), 32),
    ('cfg4 shape: ErdosRenyi N=200, B=8', dict(n_vertices=200, generative_model='ErdosRenyi'), 8),
    ('cfg4 shape, Regular N=200, B=8', dict(n_vertices=200), 8),
    ('cfg5-like ragged: ErdosRenyi N=120, vertex_proba 0.625, B=8', dict(n_vertices=120, generative_model='ErdosRenyi', vertex_proba=0.625), 8),
]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    rows = []
    for name, kw, B in SHAPES:
        gen = PairGenerator(seed=1, device=DEV, **kw)
        ms = timed(lambda: gen.bits(0, B), REPS)
        rows.append(dict(shape=name, B=B, ms_per_batch=round(ms, 4), pairs_per_s=round(B / ms * 1e3)))
        print('%-62s %8.3f ms/batch  %10.0f pairs/s' % (name, ms, B / ms * 1e3), flush=True)
    gen = PairGenerator(50, 'Regular', 'ErdosRenyi', 0.2, 0.1, seed=1, device=DEV)
    ms = timed(lambda: (gen.bits(0, 20000), gen.bits(20000, 1000)), 3)
    rows.append(dict(shape='default dataset: 21 000 pairs, Regular N=50, ER noise', B=21000, ms_per_batch=round(ms, 3),
                     pairs_per_s=round(21000 / ms * 1e3)))
    print('%-62s %8.3f ms        %10.0f pairs/s' % ('default dataset (20 000 + 1 000 pairs)', ms, 21000 / ms * 1e3))
    print(json.dumps(rows))


if __name__ == '__main__':
    main()
