"""Optimizer / scheduler next to the hot path: Adam over the flat
parameter buffer as ONE fused HIP kernel right after the gradient all-reduce, and the reference's
ReduceLROnPlateau policy (models/trainers.py:92-104: Adam lr 1e-3, factor 0.5, patience 3, min_lr 1e-5)."""
import ctypes

import torch

from . import _lib


class GradGuard:
    """The device record of the guarded optimizer step (fgnn_guard_record, include/fgnn_hip.h): the clip bound and the skip mode go
    in once, here; fgnn_grad_guard leaves the norm, the clip coefficient, the non-finite flag and the count of skipped updates in
    it.  `norm`, `coef` (fp64), `flags` and `skipped` (int32) are 0-dim views of the record: reading one is the only host
    synchronisation."""

    def __init__(self, device, max_grad_norm=None, skip_nonfinite=False):
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError('max_grad_norm must be positive or None (got %r)' % (max_grad_norm,))
        R = _lib.GuardRecord
        self.buf = torch.zeros(ctypes.sizeof(R), dtype=torch.uint8, device=device)
        f64 = lambda f: self.buf[f.offset:f.offset + 8].view(torch.float64).reshape(())
        i32 = lambda f: self.buf[f.offset:f.offset + 4].view(torch.int32).reshape(())
        self.norm, self.coef, self.flags, self.skipped = f64(R.norm), f64(R.coef), i32(R.flags), i32(R.skipped)
        f64(R.max_norm).fill_(0.0 if max_grad_norm is None else float(max_grad_norm))       # <= 0: no clipping
        f64(R.coef).fill_(1.0)
        i32(R.mode).fill_(_lib.FGNN_GUARD_SKIP_NONFINITE if skip_nonfinite else 0)

    def launch(self, grads_flat, hp):
        _lib.call('fgnn_grad_guard', _lib.ptr(grads_flat), grads_flat.numel(), _lib.ptr(hp), _lib.ptr(self.buf), _lib.stream_ptr())


def _check_flat(t, who):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError('%s: expected a contiguous fp32 buffer, got %s%s' % (who, t.dtype, '' if t.is_contiguous() else ' (strided)'))


def grad_norm(flat, scale=1.0):
    """L2 norm of `flat * scale` (a contiguous fp32 device buffer; each product rounded to fp32 as in the Adam kernels, the squares
    summed in fp64 in an order that depends on the length alone) as a 0-dim fp64 device tensor: the norm kernel of the guarded
    step on its own.  No host synchronisation."""
    _check_flat(flat, 'grad_norm')
    guard = GradGuard(flat.device)
    hp = torch.full((5,), float(scale), dtype=torch.float64, device=flat.device)      # only hp[4] is read
    guard.launch(flat, hp)
    return guard.norm.clone()


class FlatAdam:
    """torch.optim.Adam(amsgrad=False, weight_decay=0) semantics on one flat fp32 device buffer.

    max_grad_norm / skip_nonfinite guard the device-side step (step_dev) without leaving the device or the captured graph:
    * the global L2 norm of the scaled gradient g * grad_scale is left in `grad_norm` (the norm BEFORE clipping, what
      torch.nn.utils.clip_grad_norm_ returns),
    * max_grad_norm=c clips to it with clip_grad_norm_ semantics: the gradient is multiplied by `clip_coef` = min(1, c / (norm + 1e-6))
      -- Lightning's gradient_clip_val,
    * skip_nonfinite=True drops the whole update when the gradient holds an inf or a NaN: parameters, moments and the DEVICE step
      count keep their values (a skipped step does not count towards the bias correction) and `skipped_steps` advances -- what the
      AMP GradScaler behind the reference's pl.Trainer(precision=16) does.  With skip_nonfinite=False such a gradient propagates
      as in torch (error_if_nonfinite=False).
    With skip_nonfinite the step count in device memory (step_count()) is the truth; `t` counts the steps ISSUED.  With both
    options off step_dev is the single launch it always was.  The host path step() is not guarded."""

    def __init__(self, params_flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, skip_nonfinite=False):
        if not params_flat.is_cuda:
            raise RuntimeError('FlatAdam: parameters must live on the GPU (no CPU path)')
        self.params = params_flat
        self.lr, self.betas, self.eps = lr, betas, eps
        self.exp_avg = torch.zeros_like(params_flat)
        self.exp_avg_sq = torch.zeros_like(params_flat)
        self.t = 0
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._guard = None
        if self.max_grad_norm is not None or self.skip_nonfinite:
            self._guard = GradGuard(params_flat.device, self.max_grad_norm, self.skip_nonfinite)

    # -- what the guard left in device memory (no synchronisation until a value is read) ------------------
    def _guarded(self, what):
        if self._guard is None:
            raise RuntimeError('FlatAdam.%s: this optimizer is not guarded (pass max_grad_norm and / or skip_nonfinite)' % what)
        return self._guard

    @property
    def grad_norm(self):
        """0-dim fp64 device tensor: norm of the last step_dev's scaled gradient, before clipping"""
        return self._guarded('grad_norm').norm

    @property
    def clip_coef(self):
        """0-dim fp64 device tensor: the factor the last step_dev applied to its gradient (1 when nothing was clipped)"""
        return self._guarded('clip_coef').coef

    @property
    def skipped_steps(self):
        """0-dim int32 device tensor: updates skipped so far (skip_nonfinite)"""
        return self._guarded('skipped_steps').skipped

    def step_count(self):
        """The step count in device memory, the one the bias correction of step_dev uses (one host synchronisation)."""
        return int(self._dev_state()[1][0].item())

    def step(self, grads_flat, grad_scale=1.0):
        if self.skip_nonfinite and getattr(self, '_state', None) is not None:
            self.t = self.step_count()      # skipped device-side steps did not count
        self.t += 1
        _lib.call('fgnn_adam_step', _lib.ptr(self.params), _lib.ptr(grads_flat), _lib.ptr(self.exp_avg),
                  _lib.ptr(self.exp_avg_sq), self.params.numel(), float(self.lr), float(self.betas[0]),
                  float(self.betas[1]), float(self.eps), self.t, float(grad_scale), _lib.stream_ptr())
        # the replayable form keeps its own step count in device memory: keep the two counters equal, so that
        # eager and captured / device-side steps can be mixed freely
        if getattr(self, '_state', None) is not None:
            self._state[0:1].fill_(self.t)

    # -- graph-replayable form: step count and hyper-parameters live in device memory ---------------------
    def _dev_state(self):
        if getattr(self, '_hp', None) is None:
            self._hp = torch.zeros(5, dtype=torch.float64, device=self.params.device)
            self._state = torch.tensor([self.t, 0], dtype=torch.int32, device=self.params.device)
            self._hp_host = None
        return self._hp, self._state

    def sync_hyper_parameters(self, grad_scale=1.0):
        """Push lr / betas / eps (and, unless it is None, grad_scale) to the device copy if they changed (outside any
        graph capture).  grad_scale=None leaves hp[4] alone: the caller writes it on the device
        (set_grad_scale_reciprocal)."""
        hp, _ = self._dev_state()
        cur = (float(self.lr), float(self.betas[0]), float(self.betas[1]), float(self.eps),
               None if grad_scale is None else float(grad_scale))
        if cur != self._hp_host:
            n = 4 if grad_scale is None else 5
            hp[:n].copy_(torch.tensor(cur[:n], dtype=torch.float64))
            self._hp_host = cur

    def set_grad_scale_reciprocal(self, denom):
        """grad_scale <- 1 / denom for the device-side step, `denom` a 1-element device tensor (no host sync):
        the global loss normaliser that arrives with the all-reduced gradient buffer."""
        hp, _ = self._dev_state()
        torch.reciprocal(denom.to(torch.float64), out=hp[4:5])
        if self._hp_host is not None:
            self._hp_host = self._hp_host[:4] + (None,)

    def step_dev(self, grads_flat):
        """One update whose launch can be captured in a HIP graph and replayed (call sync_hyper_parameters first); a guarded
        optimizer issues the guard and the guarded update instead, two launches, as capturable."""
        hp, state = self._dev_state()
        self.t += 1
        if self._guard is None:
            _lib.call('fgnn_adam_step_dev', _lib.ptr(self.params), _lib.ptr(grads_flat), _lib.ptr(self.exp_avg),
                      _lib.ptr(self.exp_avg_sq), self.params.numel(), _lib.ptr(hp), _lib.ptr(state), _lib.stream_ptr())
            return
        # guarded: norm / clip coefficient / non-finite flag, then the update that honours them -- two launches, both capturable
        _check_flat(grads_flat, 'FlatAdam.step_dev')
        if grads_flat.numel() != self.params.numel():
            raise RuntimeError('FlatAdam.step_dev: %d gradients for %d parameters' % (grads_flat.numel(), self.params.numel()))
        self._guard.launch(grads_flat, hp)
        _lib.call('fgnn_adam_step_guarded', _lib.ptr(self.params), _lib.ptr(grads_flat), _lib.ptr(self.exp_avg),
                  _lib.ptr(self.exp_avg_sq), self.params.numel(), _lib.ptr(hp), _lib.ptr(state), _lib.ptr(self._guard.buf),
                  _lib.stream_ptr())


class ReduceLROnPlateau:
    """mode='min', relative threshold 1e-4 -- the torch defaults the reference relies on."""

    def __init__(self, optimizer, factor=0.5, patience=3, min_lr=1e-5, threshold=1e-4):
        self.opt, self.factor, self.patience, self.min_lr, self.threshold = optimizer, factor, patience, min_lr, threshold
        self.best = float('inf')
        self.bad = 0

    def step(self, metric):
        if metric < self.best * (1.0 - self.threshold):
            self.best = metric
            self.bad = 0
        else:
            self.bad += 1
        if self.bad > self.patience:
            self.opt.lr = max(self.opt.lr * self.factor, self.min_lr)
            self.bad = 0
        return self.opt.lr
