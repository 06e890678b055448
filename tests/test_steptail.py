"""CPU: the scheduled step tail's host side -- LrSchedule's validation and values against tests/steptail_ref.py, the reference
itself against torch's clip_grad_norm_ + AdamW, the exports, and uz_tail_step's refusals (they come before any launch)."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import steptail_ref as R
import unet_zoo_amd
from unet_zoo_amd import LrSchedule, _lib

W, T = 2, 6
FORMS = {
    "constant": (LrSchedule.constant(), dict()),
    "warmup": (LrSchedule.constant(warmup_steps=W, warmup_start=0.1), dict(W=W, warmup_start=0.1)),
    "cosine": (LrSchedule.cosine(T, warmup_steps=W, min_lr=1e-4, warmup_start=0.25), dict(W=W, T=T, min_lr=1e-4, warmup_start=0.25)),
    "poly": (LrSchedule.poly(T, power=0.9, warmup_steps=W, min_lr=1e-5), dict(W=W, T=T, min_lr=1e-5, power=0.9)),
    "step": (LrSchedule.step_decay(every=2, gamma=0.5, warmup_steps=W, min_lr=2e-3), dict(W=W, min_lr=2e-3, gamma=0.5, every=2)),
}


def _ref_kind(name):
    return "constant" if name == "warmup" else name


@pytest.mark.parametrize("make,arg", [
    (lambda: LrSchedule.constant(warmup_steps=-1), "warmup_steps"),
    (lambda: LrSchedule.constant(warmup_steps=float("nan")), "warmup_steps"),
    (lambda: LrSchedule.constant(warmup_steps=2, warmup_start=float("inf")), "warmup_start"),
    (lambda: LrSchedule.constant(warmup_start=-0.5), "warmup_start"),
    (lambda: LrSchedule.cosine(total_steps=5, warmup_steps=5), "total_steps"),
    (lambda: LrSchedule.cosine(total_steps="100"), "total_steps"),
    (lambda: LrSchedule.cosine(total_steps=10, min_lr=float("nan")), "min_lr"),
    (lambda: LrSchedule.poly(total_steps=0), "total_steps"),
    (lambda: LrSchedule.poly(total_steps=10, power=0.0), "power"),
    (lambda: LrSchedule.poly(total_steps=10, power=float("inf")), "power"),
    (lambda: LrSchedule.step_decay(every=0, gamma=0.5), "every"),
    (lambda: LrSchedule.step_decay(every=10, gamma=0.0), "gamma"),
    (lambda: LrSchedule.step_decay(every=10, gamma=1.5), "gamma"),
    (lambda: LrSchedule("exponential"), "kind"),
])
def test_schedule_validation_names_the_argument(make, arg):
    with pytest.raises(ValueError, match=arg):
        make()


@pytest.mark.parametrize("name", list(FORMS))
def test_lr_at_matches_the_reference(name):
    sched, kw = FORMS[name]
    base = 1e-2
    # the schedule keeps its numbers as the float32 values the descriptor carries: the reference on those very numbers ...
    n = sched.numbers()
    held = dict(W=n["warmup_steps"], warmup_start=n["warmup_start"], T=n["total_steps"], min_lr=n["min_lr"], power=n["power"],
                gamma=n["gamma"], every=n["every"])
    for k, v in kw.items():
        assert held[k] == np.float32(v), (k, held[k], v)
    for t in (0, W - 1, W, W + 1, T - 1, T, T + 5):
        got = sched.lr_at(t, base)
        want = R.lr_at(_ref_kind(name), t, base, **held)
        assert math.isclose(got, want, rel_tol=1e-14, abs_tol=0.0), (name, t, got, want)
        # ... and on the numbers as written, to float32's precision of them (the bound of the GPU test)
        want = R.lr_at(_ref_kind(name), t, base, **kw)
        assert math.isclose(got, want, rel_tol=1e-6, abs_tol=0.0), (name, t, got, want)


def test_schedule_landmarks():
    """the values no formula is needed for"""
    base = 1e-2
    assert FORMS["warmup"][0].lr_at(0, base) == pytest.approx(0.1 * base) and FORMS["warmup"][0].lr_at(W, base) == base
    assert FORMS["cosine"][0].lr_at(W, base) == base
    assert FORMS["cosine"][0].lr_at(T, base) == pytest.approx(1e-4) and FORMS["cosine"][0].lr_at(T + 5, base) == pytest.approx(1e-4)
    assert FORMS["cosine"][0].lr_at((W + T) / 2, base) == pytest.approx((base + 1e-4) / 2)
    assert FORMS["poly"][0].lr_at(T, base) == pytest.approx(1e-5)
    assert FORMS["step"][0].lr_at(W + 1, base) == base and FORMS["step"][0].lr_at(W + 2, base) == base / 2
    assert FORMS["step"][0].lr_at(W + 40, base) == pytest.approx(2e-3)        # the floor
    assert [R.ema_decay_at(t, 0.9, True) for t in (0, 8, 80, 81)] == [0.1, 0.5, 0.9, 0.9] and R.ema_decay_at(0, 0.9, False) == 0.9


@pytest.mark.parametrize("max_norm,scale", [(1.0, 5.0), (1.0, 1e-3), (0.0, 1.0)])
def test_reference_matches_torch(max_norm, scale):
    """six constant-rate steps of steptail_ref against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW (float32, CPU) at the
    tolerances of tests/test_optim_gpu.py"""
    g = torch.Generator().manual_seed(51)
    ref = [nn.Parameter(torch.randn(s, generator=g)) for s in R.SHAPES]
    flat = np.concatenate([p.detach().numpy().reshape(-1) for p in ref])
    tail = R.Tail(flat, weight_decay=1e-2, max_norm=max_norm)
    topt = torch.optim.AdamW(ref, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    for step in range(6):
        for r in ref:
            r.grad = torch.randn(r.shape, generator=g) * scale
        grad = np.concatenate([r.grad.numpy().reshape(-1) for r in ref])
        total = float(torch.sqrt(sum((r.grad.double() ** 2).sum() for r in ref)))
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(ref, max_norm)
        topt.step()
        tail.step([grad], 1e-2)
        assert abs(tail.norm - total) < 1e-12 * total
        got = torch.from_numpy(tail.p).float()
        want = torch.cat([r.detach().reshape(-1) for r in ref])
        assert torch.allclose(got, want, rtol=2e-5, atol=2e-6), step
    assert tail.t == 6


def test_reference_mean_gradient_and_ema():
    rng = np.random.default_rng(0)
    p0, gs = rng.standard_normal(50), [rng.standard_normal(50) for _ in range(3)]
    a, b = R.Tail(p0, ema=0.9, ema_warmup=False), R.Tail(p0, ema=0.9, ema_warmup=True)
    a.step(gs, 1e-2)
    b.step([(gs[0] + gs[1] + gs[2]) / 3.0], 1e-2)
    assert np.allclose(a.p, b.p, rtol=1e-14, atol=0) and not np.array_equal(a.p, p0)
    assert np.allclose(a.ema, p0 + 0.1 * (a.p - p0), rtol=1e-14)          # e += (1 - d) (p_new - e), d = 0.9
    assert np.allclose(b.ema, p0 + 0.9 * (b.p - p0), rtol=1e-14)          # warm-up: d_0 = 1 / 10


def test_exports():
    assert unet_zoo_amd.LrSchedule is LrSchedule and "LrSchedule" in unet_zoo_amd.__all__
    from unet_zoo_amd.optim import FlatClipAdamW, FlatTail
    assert issubclass(FlatTail, FlatClipAdamW) and FlatTail.ALIGN == FlatClipAdamW.ALIGN
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("uz_tail_workspace_bytes", "uz_tail_step", "uz_tail_accumulate", "uz_tail_swap"):
        assert name in _lib.EXPORTS and getattr(raw, name)
    assert ctypes.sizeof(_lib.TailDesc) == 72 and _lib.TAIL_STATE == 8
    assert _lib.load().uz_tail_workspace_bytes() == 8192
    d = _lib.TailDesc()
    FORMS["poly"][0].fill(d)
    assert (d.sched, d.warmup_steps, d.total_steps, d.power) == (_lib.SCHED_POLY, W, T, pytest.approx(0.9))
    assert FORMS["poly"][0].numbers()["kind"] == "poly" and "poly" in repr(FORMS["poly"][0])


def _desc(**kw):
    d = _lib.TailDesc()
    d.n, d.beta1, d.beta2, d.eps, d.weight_decay, d.max_norm = 1024, 0.9, 0.999, 1e-8, 1e-2, 1.0
    LrSchedule.constant().fill(d)
    d.ema_decay, d.ema_warmup, d.accumulate = 0.9, 1, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,ema,word", [
    (dict(n=0), False, b"n="),
    (dict(sched=4), False, b"sched"),
    (dict(accumulate=0), False, b"accumulate"),
    (dict(beta1=float("nan")), False, b"finite"),
    (dict(warmup_steps=-1.0), False, b"warmup_steps"),
    (dict(sched=_lib.SCHED_COSINE, total_steps=2.0, warmup_steps=2.0), False, b"total_steps"),
    (dict(sched=_lib.SCHED_POLY, total_steps=5.0, power=0.0), False, b"power"),
    (dict(sched=_lib.SCHED_STEP, every=0.0, gamma=0.5), False, b"every"),
    (dict(sched=_lib.SCHED_STEP, every=2.0, gamma=1.5), False, b"gamma"),
    (dict(ema_decay=1.0), True, b"ema_decay"),
])
def test_tail_step_refuses_a_bad_descriptor_before_any_launch(kw, ema, word):
    lib = _lib.load()
    d = _desc(**kw)
    fake = 0x10000        # never dereferenced: every case is refused on the host
    rc = lib.uz_tail_step(ctypes.byref(d), fake, fake, None, fake, fake, fake if ema else None, fake, fake, None)
    assert rc == -1 and word in lib.uz_last_error_string(), lib.uz_last_error_string()


def test_tail_entries_refuse_bad_pointers_before_any_launch():
    lib = _lib.load()
    d = _desc()
    assert lib.uz_tail_step(ctypes.byref(d), 0x10004, 0x10000, None, 0x10000, 0x10000, None, 0x10000, 0x10000, None) == -1
    assert b"aligned" in lib.uz_last_error_string()
    assert lib.uz_tail_step(ctypes.byref(d), 0x10000, None, None, 0x10000, 0x10000, None, 0x10000, 0x10000, None) == -1
    assert lib.uz_tail_accumulate(0x10000, 0x10000, 0, 1, None) == -1
    assert lib.uz_tail_accumulate(0x10004, 0x10000, 16, 1, None) == -1
    assert lib.uz_tail_swap(0x10000, 0x10000 + 16, 16, None) == -1 and b"overlap" in lib.uz_last_error_string()
    assert lib.uz_tail_swap(0x10000, None, 16, None) == -1


@pytest.mark.parametrize("kw,err,arg", [
    (dict(accumulate=0), ValueError, "accumulate"),
    (dict(accumulate=2.0), ValueError, "accumulate"),
    (dict(ema=1.5), ValueError, "ema"),
    (dict(ema=-0.1), ValueError, "ema"),
    (dict(schedule="cosine"), TypeError, "schedule"),
])
def test_step_refuses_bad_tail_arguments_without_a_gpu(kw, err, arg):
    from unet_zoo_amd.optim import check_tail_args
    args = dict(schedule=None, ema=None, accumulate=1)
    args.update(kw)
    with pytest.raises(err, match=arg):
        check_tail_args(**args)
