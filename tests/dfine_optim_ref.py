"""Float64 restatement of what the D-FINE trainers end their step with: torch.nn.utils.clip_grad_norm_(params, max_norm) (2-norm,
error_if_nonfinite=False) and one step of torch.optim.Adam / AdamW with their default flags (torch 2.10 _single_tensor_adam,
non-capturable), in numpy.  tests/test_dfine_optim_host.py holds it to torch's own CPU optimizers; the GPU tests use it as the
reference that both the HIP step and torch's fp32 step are measured against.

Per element of a tensor whose gradient is not None, with t the tensor's own step count after the increment:
    g' = g * c                                  (only with a clip coefficient c = min(1, max_norm / (norm + 1e-6)); NaN stays NaN)
    AdamW: p *= 1 - lr * wd        Adam: g' += wd * p          (only with wd != 0)
    m += (g' - m) * (1 - beta1)
    v = v * beta2 + (1 - beta2) * g'^2
    p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
A tensor whose gradient is None keeps p, m, v and t."""
import math

import numpy as np


def total_norm(grads) -> float:
    """the 2-norm of all gradients that are not None, in float64"""
    with np.errstate(all="ignore"):
        return math.sqrt(sum(float(np.sum(np.square(np.asarray(g, np.float64)))) for g in grads if g is not None))


def clip_coefficient(norm: float, max_norm: float) -> float:
    c = max_norm / (norm + 1e-6)
    return 1.0 if c > 1.0 else c      # NaN is not > 1: it stays, as torch.clamp(max=1) keeps it


def cosine_lr(base_lr: float, k: int, t_max: int, eta_min: float = 0.0) -> float:
    """CosineAnnealingLR's learning rate after k scheduler steps, closed form"""
    return eta_min + (base_lr - eta_min) * (1.0 + math.cos(math.pi * k / t_max)) / 2.0


class AdamRef:
    """params: fp32 or fp64 arrays, copied to float64; group_of[i]: the group of parameter i; groups: one dict per group with
    lr, weight_decay, betas, eps (mutable: a test that schedules the learning rate writes groups[j]["lr"] between steps)."""

    def __init__(self, params, group_of, groups, adamw: bool):
        self.p = [np.array(p, np.float64) for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.t = [0] * len(self.p)
        self.group_of = list(group_of)
        self.groups = [dict(g) for g in groups]
        self.adamw = adamw

    def step(self, grads, max_norm=None):
        """grads[i]: array or None.  Returns the total norm when max_norm is given (the gradients passed in are not modified)."""
        norm = c = None
        if max_norm is not None:
            norm = total_norm(grads)
            c = clip_coefficient(norm, max_norm)
        with np.errstate(all="ignore"):
            for i, g in enumerate(grads):
                if g is None:
                    continue
                h = self.groups[self.group_of[i]]
                lr, wd, (beta1, beta2), eps = h["lr"], h["weight_decay"], h["betas"], h["eps"]
                g = np.array(g, np.float64)
                if c is not None:
                    g = g * c
                self.t[i] += 1
                t = self.t[i]
                if wd != 0:
                    if self.adamw:
                        self.p[i] *= 1.0 - lr * wd
                    else:
                        g = g + wd * self.p[i]
                self.m[i] += (g - self.m[i]) * (1.0 - beta1)
                self.v[i] = self.v[i] * beta2 + (1.0 - beta2) * g * g
                step_size = lr / (1.0 - beta1 ** t)
                bc2_sqrt = math.sqrt(1.0 - beta2 ** t)
                self.p[i] -= step_size * self.m[i] / (np.sqrt(self.v[i]) / bc2_sqrt + eps)
        return norm
