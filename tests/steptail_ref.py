"""Float64 numpy restatement of the scheduled step tail (uz_steptail.hip), the reference of tests/test_steptail*.py:
clip_grad_norm_ + AdamW, the five schedule forms, the EMA with and without warm-up, the k-fold mean gradient.  Written from
the formulas of include/unetzoo_hip.h and of torch's documentation, not from the kernels."""
import math

import numpy as np

SHAPES = [(64, 3, 3, 3), (64,), (7, 5), (1,), (129, 33), (2, 3, 5, 7)]      # the parameter list of tests/test_optim_gpu.py
DIRECT_N = (3, 1027, 1050627)       # no whole float4; a scalar tail; more workgroups than partial rows


def lr_at(kind, t, L, *, W=0.0, warmup_start=0.0, T=0.0, min_lr=0.0, power=1.0, gamma=1.0, every=1.0):
    """the rate of the 0-based optimizer step t for the base rate L"""
    t, L = float(t), float(L)
    if t < W:
        return L * (warmup_start + (1.0 - warmup_start) * t / W)
    if kind == "constant":
        return L
    if kind == "step":
        return max(min_lr, L * gamma ** math.floor((t - W) / every))
    u = min(1.0, max(0.0, (t - W) / (T - W)))
    if kind == "cosine":
        return min_lr + (L - min_lr) * 0.5 * (1.0 + math.cos(math.pi * u))
    if kind == "poly":
        return min_lr + (L - min_lr) * (1.0 - u) ** power
    raise ValueError(kind)


def ema_decay_at(t, decay, warmup):
    """the decay of the 0-based optimizer step t"""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


class Tail:
    """the state of one run: float64 arrays p, m, v (and ema), the step counter t"""

    def __init__(self, p, *, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=1.0, ema=None, ema_warmup=True):
        self.p = np.asarray(p, np.float64).copy()
        self.m, self.v = np.zeros_like(self.p), np.zeros_like(self.p)
        self.betas, self.eps, self.wd, self.max_norm = betas, eps, weight_decay, max_norm
        self.ema = self.p.copy() if ema is not None else None
        self.ema_decay, self.ema_warmup = ema, ema_warmup
        self.t = 0
        self.norm = None

    def step(self, grads, lr):
        """one optimizer step at the rate lr on the MEAN of `grads` (a list of k gradients; k = 1: the gradient itself)"""
        g = np.mean([np.asarray(x, np.float64) for x in grads], axis=0)
        self.norm = math.sqrt(float((g * g).sum()))
        if self.max_norm > 0:
            g = g * min(1.0, self.max_norm / (self.norm + 1e-6))
        b1, b2 = self.betas
        t = self.t + 1
        self.p *= 1.0 - lr * self.wd
        self.m = b1 * self.m + (1.0 - b1) * g
        self.v = b2 * self.v + (1.0 - b2) * g * g
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        self.p -= (lr / bc1) * self.m / (np.sqrt(self.v) / math.sqrt(bc2) + self.eps)
        if self.ema is not None:
            d = ema_decay_at(self.t, self.ema_decay, self.ema_warmup)
            self.ema += (1.0 - d) * (self.p - self.ema)
        self.t = t


def flat_layout(shapes, align=64):
    """(offsets, n) of the flat buffers: every tensor starts on a multiple of `align` elements"""
    offs, off = [], 0
    for s in shapes:
        offs.append(off)
        off += (int(np.prod(s)) + align - 1) // align * align
    return offs, off
