"""numpy restatement of the guarded optimizer step (csrc/grad_guard.hip, include/fgnn_hip.h): the guard -- norm of the scaled gradient,
clip coefficient, non-finite flag -- and the Adam update that honours it.

Arithmetic as in the kernels: every gi = g[i] * (float)grad_scale is an fp32 product, the squares are summed in fp64 (numpy's
pairwise order; the kernel's fixed order differs from it by far less than half an fp32 ulp of the norm), norm = sqrt(sum),
coef = min(1, max_norm / (norm + 1e-6)) with torch.clamp's NaN (a NaN stays), the update runs on fp32 values with hyper-parameters
formed in fp64 and rounded once, and its gradient scale is (float)(grad_scale * coef).  The skip rule: in skip mode a non-finite
gradient changes nothing but the count of skipped steps -- the step count does not advance.

`torch_clip_adam` is the independent reference: torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on CPU tensors."""
import numpy as np


def guard(g, scale=1.0, max_norm=None):
    """-> (norm, coef, nonfinite) of the gradient g (fp32 array) scaled by `scale`"""
    gi = np.asarray(g, dtype=np.float32) * np.float32(scale)
    assert gi.dtype == np.float32
    with np.errstate(over='ignore', invalid='ignore'):
        s = np.sum(gi.astype(np.float64) ** 2, dtype=np.float64)
        norm = np.sqrt(s)
        coef = 1.0
        if max_norm is not None and max_norm > 0:
            c = np.float64(max_norm) / (norm + 1e-6)
            coef = 1.0 if c > 1.0 else float(c)           # NaN > 1 is False: the NaN stays
    return float(norm), coef, not np.isfinite(s)


class GuardedAdam:
    """FlatAdam(max_grad_norm, skip_nonfinite).step_dev restated on host arrays"""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, skip_nonfinite=False):
        self.p = np.array(params, dtype=np.float32)
        self.m = np.zeros_like(self.p)
        self.v = np.zeros_like(self.p)
        self.lr, self.betas, self.eps = lr, betas, eps
        self.max_grad_norm, self.skip_nonfinite = max_grad_norm, skip_nonfinite
        self.steps = 0          # the device step count: skipped steps do not advance it
        self.skipped = 0
        self.norm, self.coef, self.nonfinite = 0.0, 1.0, False

    def step(self, g, scale=1.0):
        self.norm, self.coef, self.nonfinite = guard(g, scale, self.max_grad_norm)
        if self.nonfinite and self.skip_nonfinite:
            self.skipped += 1
            return
        self.steps += 1
        f = np.float32
        b1, b2 = self.betas
        bc1, bc2 = 1.0 - b1 ** self.steps, 1.0 - b2 ** self.steps
        step_size, w1, beta2, w2 = f(self.lr / bc1), f(1.0 - b1), f(b2), f(1.0 - b2)
        inv_sqrt_bc2, eps = f(1.0 / np.sqrt(bc2)), f(self.eps)
        with np.errstate(over='ignore', invalid='ignore'):
            gi = np.asarray(g, dtype=np.float32) * f(np.float64(scale) * np.float64(self.coef))
            self.m = self.m + (gi - self.m) * w1
            self.v = self.v * beta2 + gi * gi * w2
            self.p = self.p - step_size * (self.m / (np.sqrt(self.v) * inv_sqrt_bc2 + eps))
        assert self.p.dtype == self.m.dtype == self.v.dtype == np.float32


def make_case(n=40000, steps=5, seed=0):
    """(p0, [g_0 ..]) as fp32 arrays: gradients whose size grows 10 x per step (as tests/test_gpu_kernels.py's Adam test), so that
    a fixed max_grad_norm leaves the first steps alone and clips the later ones"""
    rng = np.random.default_rng(seed)
    p0 = rng.standard_normal(n).astype(np.float32)
    return p0, [(rng.standard_normal(n) * 10.0 ** (t - 2)).astype(np.float32) for t in range(steps)]


def torch_clip_adam(p0, grads, scale, max_norm, lr=1e-3):
    """clip_grad_norm_(error_if_nonfinite=False) + torch.optim.Adam on CPU -> per step {'p', 'm', 'v', 'norm'} (numpy)"""
    import torch
    p = torch.from_numpy(np.array(p0, dtype=np.float32)).requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, amsgrad=False)
    out = []
    for g in grads:
        p.grad = torch.from_numpy(np.asarray(g, dtype=np.float32) * np.float32(scale))
        if max_norm is not None:
            norm = torch.nn.utils.clip_grad_norm_([p], max_norm, error_if_nonfinite=False)
        else:
            norm = p.grad.norm()
        opt.step()
        st = opt.state[p]
        out.append({'p': p.detach().numpy().copy(), 'm': st['exp_avg'].numpy().copy(), 'v': st['exp_avg_sq'].numpy().copy(),
                    'norm': float(norm)})
    return out


def rel(a, b):
    """max-norm relative error, util.rel on arrays"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    s = np.abs(b).max()
    d = np.abs(a - b).max()
    return d / s if s > 0 else d
