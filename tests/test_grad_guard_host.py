"""CPU: the guarded optimizer step's reference and host side (no launch).

The numpy restatement tests/grad_guard_ref.py -- what the GPU tests compare the kernels with -- is pinned here against
torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam on CPU tensors, so the reference itself needs no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import grad_guard_ref as R
from graph_neural_net_amd import _lib
from graph_neural_net_amd.optim import FlatAdam, GradGuard
from util import ROOT

ADAM_PARITY = 1e-6          # the project's Adam parity bar, max-norm relative error


# (grad_scale, max_grad_norm): the scaled norms of make_case() are about 2, 20, 200, 2000, 20000 times grad_scale
CASES = [(1.0, 100.0), (1.0 / 96.0, 1.0), (1.0, None)]


@pytest.mark.parametrize('scale,max_norm', CASES)
def test_restatement_matches_torch_clip_and_adam(scale, max_norm):
    p0, grads = R.make_case()
    ref = R.torch_clip_adam(p0, grads, scale, max_norm)
    mine = R.GuardedAdam(p0, lr=1e-3, max_grad_norm=max_norm)
    coefs, worst = [], 0.0
    for t, g in enumerate(grads):
        mine.step(g, scale)
        coefs.append(mine.coef)
        errs = (R.rel(mine.p, ref[t]['p']), R.rel(mine.m, ref[t]['m']), R.rel(mine.v, ref[t]['v']),
                abs(mine.norm - ref[t]['norm']) / ref[t]['norm'])
        worst = max(worst, *errs)
        print('scale %g max_norm %s step %d: coef %.6g, rel err p %.2e m %.2e v %.2e norm %.2e' % ((scale, max_norm, t, mine.coef) + errs))
        # The 1e-6 bar is the one the fused Adam is held to against torch (tests/test_gpu_kernels.py); it is reused here for clip + Adam
        # without a derivation of its own.  Measured on these cases (worst step): parameters 5.0e-8, exp_avg 3.2e-7, exp_avg_sq
        # 6.0e-7, norm 3.5e-7.  The norm's difference is torch's: it sums the squares in fp32, the restatement in fp64; a clipped
        # step carries it into exp_avg once and into exp_avg_sq twice, while the parameters see only the ratio of the two.
        assert max(errs) < ADAM_PARITY, (t, errs)
    if max_norm is None:
        assert coefs == [1.0] * 5
    else:       # both kinds of step are in the case: the first two pass unclipped, the last three are clipped
        assert coefs[0] == coefs[1] == 1.0 and all(c < 1.0 for c in coefs[2:]), coefs
    assert mine.steps == 5 and mine.skipped == 0 and worst < ADAM_PARITY


def test_restatement_skip_rule_and_torch_nonfinite_semantics():
    p0, grads = R.make_case(n=1000, steps=3, seed=1)
    bad = grads[1].copy()
    bad[17] = np.nan
    # skip mode: the bad step changes nothing and does not count; the run equals the run without it
    a = R.GuardedAdam(p0, max_grad_norm=100.0, skip_nonfinite=True)
    b = R.GuardedAdam(p0, max_grad_norm=100.0)
    a.step(grads[0])
    before = (a.p.copy(), a.m.copy(), a.v.copy(), a.steps)
    a.step(bad)
    assert a.nonfinite and a.skipped == 1 and a.steps == before[3] == 1
    assert all(np.array_equal(x, y) for x, y in zip((a.p, a.m, a.v), before[:3]))
    a.step(grads[2])
    b.step(grads[0])
    b.step(grads[2])
    assert np.array_equal(a.p, b.p) and a.steps == b.steps == 2 and not a.nonfinite
    # without skip mode the gradient propagates as in torch: the norm is NaN, so is the coefficient, so is every parameter
    c = R.GuardedAdam(p0, max_grad_norm=100.0)
    c.step(bad)
    ref = R.torch_clip_adam(p0, [bad], 1.0, 100.0)
    assert np.isnan(c.coef) and np.isnan(c.p).all() and np.isnan(ref[0]['p']).all()
    # an inf: norm inf, coefficient 0, 0 * inf = NaN in that element only (torch: the same)
    bad[17] = np.inf
    d = R.GuardedAdam(p0, max_grad_norm=100.0)
    d.step(bad)
    ref = R.torch_clip_adam(p0, [bad], 1.0, 100.0)
    assert d.coef == 0.0 and np.array_equal(np.isnan(d.p), np.isnan(ref[0]['p'])) and np.isnan(d.p).sum() == 1
    # squares that overflow fp32 but not fp64: finite norm, nothing flagged
    norm, coef, nonfinite = R.guard(np.full(257, 1e30, dtype=np.float32))
    assert not nonfinite and coef == 1.0 and abs(norm - 1e30 * np.sqrt(257.0)) < 1e-6 * norm


def test_guard_record_mirror_and_declarations():
    """the ctypes mirror gives the offsets the Python side writes to: it must be the struct of include/fgnn_hip.h"""
    hdr = open(os.path.join(ROOT, 'include', 'fgnn_hip.h')).read()
    body = re.search(r'typedef struct \{([^}]*)\} fgnn_guard_record;', hdr).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = [(m.group(1), m.group(2), m.group(3)) for m in re.finditer(r'(double|int)\s+(\w+)(?:\[(\w+)\])?;', body)]
    assert int(re.search(r'#define FGNN_GUARD_MAX_PARTS (\d+)', hdr).group(1)) == _lib.FGNN_GUARD_MAX_PARTS
    ctype = {'double': C.c_double, 'int': C.c_int}
    want = [(name, ctype[t] * _lib.FGNN_GUARD_MAX_PARTS if dim else ctype[t]) for t, name, dim in fields]
    assert [(n, t) for n, t in _lib.GuardRecord._fields_] == want
    assert C.sizeof(_lib.GuardRecord) == 40 + 8 * _lib.FGNN_GUARD_MAX_PARTS and _lib.GuardRecord.partial.offset == 40
    lib = _lib.load()
    for name in ('fgnn_grad_guard', 'fgnn_adam_step_guarded'):
        m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, hdr)
        assert m, '%s is not declared in include/fgnn_hip.h' % name
        assert hasattr(lib, name) and len(_lib._SIGNATURES[name]) == len(m.group(1).split(',')), name


def test_guard_options_are_validated_before_anything_is_allocated():
    for bad in (0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='max_grad_norm'):
            GradGuard('cpu', max_grad_norm=bad)
    with pytest.raises(RuntimeError, match='GPU'):
        FlatAdam(torch.zeros(4), max_grad_norm=1.0, skip_nonfinite=True)
