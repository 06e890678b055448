"""GPU: the scheduled step tail (uz_steptail.hip, optim.FlatTail) -- bit for bit against the existing tail (uz_clip_adamw) where
they must agree, against the float64 restatement tests/steptail_ref.py for what is new.

Shapes: the parameter list of tests/test_optim_gpu.py, and direct ABI calls at n = 3 (no whole float4), 1027 (a scalar tail)
and 1 050 627 (1026 workgroups' worth of float4s for 1024 partial rows: the grid-stride loops run)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import steptail_ref as R
from unet_zoo_amd import LrSchedule, _lib as L
from unet_zoo_amd.optim import FlatClipAdamW, FlatTail

pytestmark = pytest.mark.gpu

DEV = "cuda"
BASE = 1e-2
BASE32 = float(np.float32(BASE))          # the base rate as the device holds it
HYPER = dict(lr=BASE, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
W, T = 2, 6
FORMS = {
    "constant": (LrSchedule.constant(), dict()),
    "warmup": (LrSchedule.constant(warmup_steps=W, warmup_start=0.1), dict(W=W, warmup_start=0.1)),
    "cosine": (LrSchedule.cosine(T, warmup_steps=W, min_lr=1e-4, warmup_start=0.25), dict(W=W, T=T, min_lr=1e-4, warmup_start=0.25)),
    "poly": (LrSchedule.poly(T, power=0.9, warmup_steps=W, min_lr=1e-5), dict(W=W, T=T, min_lr=1e-5, power=0.9)),
    "step": (LrSchedule.step_decay(every=2, gamma=0.5, warmup_steps=W, min_lr=2e-3), dict(W=W, min_lr=2e-3, gamma=0.5, every=2)),
}


def _params(seed=51):
    g = torch.Generator().manual_seed(seed)
    return [nn.Parameter(torch.randn(s, generator=g).to(DEV)) for s in R.SHAPES], g


def _set_grads(opt, g, scale):
    for p in opt.params:
        p.grad.copy_((torch.randn(p.shape, generator=g) * scale).to(DEV))


def _np(t):
    return t.detach().double().cpu().numpy()


class _Direct:
    """uz_tail_step / uz_clip_adamw through the raw ABI on flat tensors of n floats"""

    def __init__(self, n, seed, max_norm):
        g = torch.Generator().manual_seed(seed)
        self.n, self.gen, self.max_norm = n, g, max_norm
        self.p = torch.randn(n, generator=g).to(DEV)
        self.g = torch.zeros(n, device=DEV)
        self.m, self.v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        self.state = torch.zeros(L.TAIL_STATE, device=DEV)
        self.state[L.TAIL_BASE_LR] = BASE
        self.step_count = torch.zeros(1, device=DEV)
        self.ws = torch.zeros(L.load().uz_clip_adamw_workspace_bytes() // 4, device=DEV)
        d = self.desc = L.TailDesc()
        d.n, d.beta1, d.beta2, d.eps, d.weight_decay, d.max_norm = n, 0.9, 0.999, 1e-8, 1e-2, max_norm
        LrSchedule.constant().fill(d)
        d.accumulate = 1

    def draw(self, scale):
        self.g.copy_((torch.randn(self.n, generator=self.gen) * scale).to(DEV))

    def tail(self):
        L.check(L.load().uz_tail_step(ctypes.byref(self.desc), self.p.data_ptr(), self.g.data_ptr(), None, self.m.data_ptr(),
                                      self.v.data_ptr(), None, self.state.data_ptr(), self.ws.data_ptr(), L.stream_ptr()), "uz_tail_step")
        return self.state[L.TAIL_NORM]

    def legacy(self):
        L.check(L.load().uz_clip_adamw(self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n, BASE, 0.9,
                                       0.999, 1e-8, 1e-2, self.max_norm, self.step_count.data_ptr(), self.ws.data_ptr(),
                                       L.stream_ptr()), "uz_clip_adamw")
        return self.ws[2048 + 3]


# ---- 1. bit for bit against the existing tail ------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm,scale", [(1.0, 5.0), (1.0, 1e-3), (0.0, 1.0)])
def test_constant_tail_is_the_existing_tail_bitwise(max_norm, scale):
    # the parameter list, through the two classes
    ours, g1 = _params()
    theirs, g2 = _params()
    a = FlatTail(ours, max_norm=max_norm, **HYPER)
    b = FlatClipAdamW(theirs, max_norm=max_norm, **HYPER)
    assert a.n == b.n and a.spans == b.spans and a.ALIGN == b.ALIGN
    for step in range(5):
        _set_grads(a, g1, scale)
        _set_grads(b, g2, scale)
        a.step()
        b.step()
        assert torch.equal(a.flat_g, b.flat_g)
        assert a.last_grad_norm().item() == b.last_grad_norm().item(), step
        for name in ("flat_p", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (step, name)
    assert a.step_count.item() == 5.0 and a.last_lr().item() == BASE32
    # the three direct sizes, through the ABI
    for n in R.DIRECT_N:
        x, y = _Direct(n, 7, max_norm), _Direct(n, 7, max_norm)
        for step in range(5):
            x.draw(scale)
            y.draw(scale)
            nx, ny = x.tail(), y.legacy()
            assert nx.item() == ny.item(), (n, step)
            assert torch.equal(x.p, y.p) and torch.equal(x.m, y.m) and torch.equal(x.v, y.v), (n, step)
        total = float(np.sqrt((_np(x.g) ** 2).sum()))
        assert abs(x.state[L.TAIL_NORM].item() - total) < 1e-5 * total          # and the norm is the norm
        assert x.state[L.TAIL_T].item() == 5.0


# ---- 2. schedules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FORMS))
def test_schedule_on_the_device_matches_the_reference(name):
    sched, kw = FORMS[name]
    ours, g = _params()
    opt = FlatTail(ours, max_norm=1.0, schedule=sched, **HYPER)
    ref = R.Tail(_np(opt.flat_p), weight_decay=1e-2, max_norm=1.0)
    for t in range(8):                      # warm-up (t < 2), decay (2 <= t < 6), the clamp beyond T
        _set_grads(opt, g, 1.0)
        want = R.lr_at("constant" if name == "warmup" else name, t, BASE32, **kw)
        ref.step([_np(opt.flat_g)], want)
        opt.step()
        got = opt.last_lr().item()
        print(f"{name} t={t}: lr {got!r} want {want!r} rel {abs(got - want) / max(want, 1e-300):.2e}")
        assert abs(got - want) <= 1e-6 * want, (name, t, got, want)
        assert got == float(np.float32(sched.lr_at(t, BASE32))), (name, t)      # lr_at on the held numbers IS the device's rate
        assert abs(opt.last_grad_norm().item() - ref.norm) < 1e-5 * ref.norm
        assert torch.allclose(opt.flat_p, torch.from_numpy(ref.p).float().to(DEV), rtol=2e-5, atol=2e-6), (name, t)
    assert opt.state[L.TAIL_T].item() == 8.0 and opt.state[L.TAIL_BASE_LR].item() == BASE32


def test_set_lr_moves_the_base_rate_of_the_schedule():
    ours, g = _params()
    opt = FlatTail(ours, schedule=FORMS["cosine"][0], **HYPER)
    opt.set_lr(0.5)
    for t in range(3):
        _set_grads(opt, g, 1.0)
        opt.step()
        want = R.lr_at("cosine", t, 0.5, **FORMS["cosine"][1])
        assert abs(opt.last_lr().item() - want) <= 1e-6 * want


# ---- 3. EMA ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warmup", [False, True])
def test_ema_follows_the_float64_recurrence_and_leaves_adamw_alone(warmup):
    """rtol 2e-6: six float32 updates of a few ulps (1.2e-7) each.  torch.allclose's own atol of 1e-8 stays: an element of e
    that passes through zero has no relative error to speak of (the printed largest ratio, around 1e-5, is theirs), and its
    absolute error is that of the increment (1 - d)(p - e) <= 1e-2: 1e-9"""
    ours, g1 = _params()
    twin, g2 = _params()
    a = FlatTail(ours, ema=0.9, ema_warmup=warmup, **HYPER)
    b = FlatTail(twin, **HYPER)
    assert torch.equal(a.ema, a.flat_p) and a.ema.data_ptr() != a.flat_p.data_ptr() and b.ema is None
    e = _np(a.ema)
    for t in range(6):
        _set_grads(a, g1, 1.0)
        _set_grads(b, g2, 1.0)
        a.step()
        b.step()
        d = R.ema_decay_at(t, 0.9, warmup)
        e += (1.0 - d) * (_np(a.flat_p) - e)             # the recurrence on snapshots of the device's own p
        assert abs(a.state[L.TAIL_EMA_DECAY].item() - d) <= 1e-7
        got = a.ema.double().cpu()
        err = ((got - torch.from_numpy(e)).abs() / torch.from_numpy(e).abs().clamp_min(1e-30)).max().item()
        print(f"ema warmup={warmup} t={t}: d {d:.4f}, largest relative error {err:.2e}")
        assert torch.allclose(got, torch.from_numpy(e), rtol=2e-6), (t, err)      # (allclose's own atol of 1e-8)
        for name in ("flat_p", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (t, name)
    assert b.state[L.TAIL_EMA_DECAY].item() == 0.0


# ---- 4. accumulation ------------------------------------------------------------------------------------------------------------
def test_accumulated_step_takes_the_mean_gradient():
    ours, g = _params()
    opt = FlatTail(ours, accumulate=3, **HYPER)
    ref = R.Tail(_np(opt.flat_p), weight_decay=1e-2, max_norm=1.0)
    opt.acc.fill_(float("nan"))                  # first=1 must not read what the accumulator held
    grads = []
    for i in range(3):
        _set_grads(opt, g, 2.0)
        grads.append(opt.flat_g.clone())
        if i < 2:
            opt.accumulate_grad(first=(i == 0))
    assert torch.equal(opt.acc, grads[0] + grads[1])
    opt.step()
    ref.step([_np(x) for x in grads], BASE32)
    assert abs(opt.last_grad_norm().item() - ref.norm) < 1e-5 * ref.norm
    assert torch.allclose(opt.flat_p, torch.from_numpy(ref.p).float().to(DEV), rtol=2e-5, atol=2e-6)
    assert opt.step_count.item() == 1.0


@pytest.mark.parametrize("n", R.DIRECT_N)
def test_accumulate_at_the_direct_sizes(n):
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
    acc = torch.full((n,), float("nan"), device=DEV)
    lib = L.load()
    L.check(lib.uz_tail_accumulate(acc.data_ptr(), a.data_ptr(), n, 1, L.stream_ptr()), "uz_tail_accumulate")
    assert torch.equal(acc, a)
    L.check(lib.uz_tail_accumulate(acc.data_ptr(), b.data_ptr(), n, 0, L.stream_ptr()), "uz_tail_accumulate")
    assert torch.equal(acc, a + b)
    # ... and the tail reads it: one step on (b + acc) / 2 against the reference
    x = _Direct(n, 3, 1.0)
    x.desc.accumulate = 2
    ref = R.Tail(_np(x.p), weight_decay=1e-2, max_norm=1.0)
    x.g.copy_(b)
    L.check(lib.uz_tail_step(ctypes.byref(x.desc), x.p.data_ptr(), x.g.data_ptr(), acc.data_ptr(), x.m.data_ptr(), x.v.data_ptr(),
                             None, x.state.data_ptr(), x.ws.data_ptr(), L.stream_ptr()), "uz_tail_step")
    ref.step([_np(b), _np(acc)], BASE32)
    assert abs(x.state[L.TAIL_NORM].item() - ref.norm) < 1e-5 * ref.norm
    assert torch.allclose(x.p, torch.from_numpy(ref.p).float().to(DEV), rtol=2e-5, atol=2e-6)


# ---- 5. swap --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.DIRECT_N)
def test_swap_exchanges_the_contents_exactly(n):
    g = torch.Generator().manual_seed(n)
    a0, b0 = torch.randn(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
    a, b = a0.clone(), b0.clone()
    pa, pb = a.data_ptr(), b.data_ptr()
    lib = L.load()
    L.check(lib.uz_tail_swap(pa, pb, n, L.stream_ptr()), "uz_tail_swap")
    assert torch.equal(a, b0) and torch.equal(b, a0)
    L.check(lib.uz_tail_swap(pa, pb, n, L.stream_ptr()), "uz_tail_swap")
    assert torch.equal(a, a0) and torch.equal(b, b0) and (a.data_ptr(), b.data_ptr()) == (pa, pb)
