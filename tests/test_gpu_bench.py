"""GPU: a plain `bench.py` run reports the headline alone over exactly --steps timed steps, and `--dump-outputs` writes what the
last timed step computed -- the scores, loss and flat gradient of the benchmarked batch, checked here against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from graph_neural_net_amd import synthetic
from graph_neural_net_amd.engine import ParamLayout
from oracle import fgnn_oracle as O
from util import ROOT, is_zero_grad, rel

pytestmark = pytest.mark.gpu

E2E_FWD_TOL = 3e-5       # scores after 4 blocks (tests/test_gpu_parity.py)
BIG_FLAT = 4.0           # batch-level flat-gradient gate in units of the oracle's own fp32 error (tests/test_gpu_parity.py)


def test_plain_bench_times_the_headline_and_dumps_its_outputs(tmp_path):
    out_dir = os.path.join(str(tmp_path), 'outputs')
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--settle', '2',
                        '--dump-outputs', out_dir], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['unit'] == 'pairs/s' and d['higher_is_better'] is True and d['dtype'] == 'f32' and 'N=50 regular pairs' in d['metric']
    assert d['steps'] == 3 and d['timed_windows'] == 1 and len(d['window_ms_per_step']) == 1
    assert d['value'] > 0 and abs(d['value'] - 32 / (d['ms_per_step'] * 1e-3)) < 1e-6 * d['value']
    # the measurements of --full are not taken
    assert d['cpu_baseline'] is None and d['roofline'] is None and not d['kernels']
    assert not {'dense_input', 'mfma_x3', 'precision16', 'batch256', 'wide64', 'module_surface', 'extra_configs'} & set(d)

    got = {k: np.load(os.path.join(out_dir, k + '.npy')) for k in ('scores', 'loss', 'grads')}
    assert sorted(os.listdir(out_dir)) == ['grads.npy', 'loss.npy', 'scores.npy']
    assert all(a.dtype == np.float32 for a in got.values())
    lay = ParamLayout(2, 4, 32, 32, 3)
    assert got['scores'].shape == (32, 50, 50) and got['loss'].shape == (1,) and got['grads'].shape == (lay.total,)
    # the benchmarked batch and weights (bench.py run_config, cfg2) through the oracle, in fp32 and in fp64
    x1, x2 = synthetic.make_batch(2000, 32, 50, 'Regular', 0.2, 0.1)
    sd = lay.unflatten(lay.init_flat(0, 'cpu'))
    s32, l32, g32 = O.step_fwd_bwd(x1, x2, sd)
    s64, l64, g64 = O.step_fwd_bwd(x1.double(), x2.double(), {k: v.double() for k, v in sd.items()})
    assert rel(torch.from_numpy(got['scores']), s64) < E2E_FWD_TOL
    assert abs(float(got['loss'][0]) - l64.item()) < 1e-5 * abs(l64.item())
    ours = lay.unflatten(torch.from_numpy(got['grads']))
    keys = [k for k in g64 if not is_zero_grad(k)]
    flat = lambda g: torch.cat([g[k].reshape(-1).double() for k in keys])
    truth = flat(g64)
    err = ((flat(ours) - truth).norm() / truth.norm()).item()
    yard = ((flat(g32) - truth).norm() / truth.norm()).item()
    assert err < BIG_FLAT * yard + 1e-6, (err, yard)
