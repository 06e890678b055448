"""Learning-rate schedules the step tail evaluates ON THE DEVICE: ``LrSchedule``.

``GraphedStep(model, schedule=LrSchedule.cosine(total_steps=10_000, warmup_steps=500))`` hands the numbers below to
``uz_tail_step`` (uz_steptail.hip), whose prepare launch evaluates the schedule from the device's own step counter: a
per-step schedule costs no host work, no synchronize and no new capture.  The schedule is closed-form in t, the 0-based
index of the optimizer step being taken, so resuming a run needs only t.  With L the base rate (``GraphedStep(lr=...)``,
``set_lr``), W = warmup_steps, T = total_steps and u = clamp((t - W) / (T - W), 0, 1):

    t < W (every form)   lr = L * (warmup_start + (1 - warmup_start) * t / W)
    constant             lr = L
    cosine               lr = min_lr + (L - min_lr) * 0.5 * (1 + cos(pi * u))
    poly                 lr = min_lr + (L - min_lr) * (1 - u) ** power          (nnU-Net: power = 0.9)
    step_decay           lr = max(min_lr, L * gamma ** floor((t - W) / every))

The scheduler POLICY stays the caller's: a schedule that depends on a metric (the reference's DiceScheduler,
utils/lr_scheduler.py:70-81) is ``LrSchedule.constant()`` plus ``step.set_lr(new_rate)``, a device-side fill.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict

from . import _lib as L

_KINDS = {"constant": L.SCHED_CONSTANT, "cosine": L.SCHED_COSINE, "poly": L.SCHED_POLY, "step": L.SCHED_STEP}
_FIELDS = ("warmup_steps", "warmup_start", "total_steps", "min_lr", "power", "gamma", "every")


def _number(name: str, v, lo=None, lo_open: bool = False) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or abs(v) > 3.4e38:
        raise ValueError(f"LrSchedule: {name} must be a finite (float32) number, got {v!r}")
    if lo is not None and (v <= lo if lo_open else v < lo):
        raise ValueError(f"LrSchedule: {name} must be {'>' if lo_open else '>='} {lo}, got {v!r}")
    # kept as the float32 value the descriptor carries: lr_at() and the device then evaluate the same numbers (the float32
    # neighbour of warmup_start = 0.1 moves a warm-up rate by an ulp -- enough to part two bf16 runs after a few steps)
    return ctypes.c_float(v).value


class LrSchedule:
    """One of the four forms above; build it with the class methods.  Immutable numbers, no state: the step counter lives in
    the tail's device state."""

    def __init__(self, kind: str, *, warmup_steps=0, warmup_start=0.0, total_steps=0, min_lr=0.0, power=1.0, gamma=1.0, every=1):
        if kind not in _KINDS:
            raise ValueError(f"LrSchedule: kind is one of {sorted(_KINDS)}, got {kind!r}")
        self.kind = kind
        self.warmup_steps = _number("warmup_steps", warmup_steps, 0)
        self.warmup_start = _number("warmup_start", warmup_start, 0)
        self.min_lr = _number("min_lr", min_lr, 0)
        self.total_steps = _number("total_steps", total_steps)
        self.power = _number("power", power)
        self.gamma = _number("gamma", gamma)
        self.every = _number("every", every)
        if kind in ("cosine", "poly") and not self.total_steps > self.warmup_steps:
            raise ValueError(f"LrSchedule: total_steps must exceed warmup_steps ({warmup_steps!r}), got {total_steps!r}")
        if kind == "poly" and not self.power > 0.0:
            raise ValueError(f"LrSchedule: power must be > 0, got {power!r}")
        if kind == "step":
            if not 0.0 < self.gamma <= 1.0:
                raise ValueError(f"LrSchedule: gamma must be in (0, 1], got {gamma!r}")
            if not self.every >= 1.0:
                raise ValueError(f"LrSchedule: every must be >= 1, got {every!r}")

    @classmethod
    def constant(cls, warmup_steps=0, warmup_start=0.0) -> "LrSchedule":
        return cls("constant", warmup_steps=warmup_steps, warmup_start=warmup_start)

    @classmethod
    def cosine(cls, total_steps, warmup_steps=0, min_lr=0.0, warmup_start=0.0) -> "LrSchedule":
        return cls("cosine", total_steps=total_steps, warmup_steps=warmup_steps, min_lr=min_lr, warmup_start=warmup_start)

    @classmethod
    def poly(cls, total_steps, power=0.9, warmup_steps=0, min_lr=0.0, warmup_start=0.0) -> "LrSchedule":
        return cls("poly", total_steps=total_steps, power=power, warmup_steps=warmup_steps, min_lr=min_lr,
                   warmup_start=warmup_start)

    @classmethod
    def step_decay(cls, every, gamma, warmup_steps=0, min_lr=0.0, warmup_start=0.0) -> "LrSchedule":
        return cls("step", every=every, gamma=gamma, warmup_steps=warmup_steps, min_lr=min_lr, warmup_start=warmup_start)

    def lr_at(self, t, base_lr: float) -> float:
        """the rate of optimizer step t (0-based) for the base rate `base_lr`, in Python floats: for logging and the tests; the
        device evaluates the same formulas in double on the same (float32-held) numbers from its own counter and rounds once
        to float -- pass the base rate as the device holds it (its float32 value) and float32(lr_at) is the device's rate"""
        t, L_, W = float(t), float(base_lr), self.warmup_steps
        if t < W:
            return L_ * (self.warmup_start + (1.0 - self.warmup_start) * t / W)
        if self.kind == "constant":
            return L_
        if self.kind == "step":
            return max(self.min_lr, L_ * self.gamma ** math.floor((t - W) / self.every))
        u = min(1.0, max(0.0, (t - W) / (self.total_steps - W)))
        if self.kind == "cosine":
            return self.min_lr + (L_ - self.min_lr) * 0.5 * (1.0 + math.cos(math.pi * u))
        return self.min_lr + (L_ - self.min_lr) * (1.0 - u) ** self.power

    def numbers(self) -> Dict[str, object]:
        """the descriptor's numbers (what ``GraphedStep.state_dict()["schedule"]`` holds)"""
        out: Dict[str, object] = {"kind": self.kind}
        out.update((f, getattr(self, f)) for f in _FIELDS)
        return out

    def fill(self, desc: "L.TailDesc") -> None:
        """write this schedule into a uz_tail_desc"""
        desc.sched = _KINDS[self.kind]
        for f in _FIELDS:
            setattr(desc, f, getattr(self, f))

    def __repr__(self) -> str:
        shown = {"constant": (), "cosine": ("total_steps", "min_lr"), "poly": ("total_steps", "power", "min_lr"),
                 "step": ("every", "gamma", "min_lr")}[self.kind]
        args = [f"{f}={getattr(self, f):g}" for f in shown + (("warmup_steps", "warmup_start") if self.warmup_steps else ())]
        return f"LrSchedule.{'step_decay' if self.kind == 'step' else self.kind}({', '.join(args)})"
