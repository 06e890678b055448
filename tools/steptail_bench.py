#!/usr/bin/env python3
"""The scheduled step tail (uz_steptail.hip, optim.FlatTail) measured, in ONE process on one GPU: unet bf16, B = 16, 256 x 256.

(1) the training step, ms per call over `iters` calls, `windows` windows each, the forms ALTERNATING window by window:
      (a) default            GraphedStep(model): FlatClipAdamW, a constant rate in the launch arguments
      (b) schedule=cosine    the rate evaluated on the device every step
      (c) (b) + ema          the averaged weights updated in the apply launch
      (d) (a) + eager lerp_  what a user does without (c): ema.lerp_(flat_p, 1 - d) after every step
      (e) (a) + set_lr       a new rate every step on the default tail: a synchronize and a new capture per step
      (f) accumulate=2       per MICRO-step (two calls make one optimizer step)
(2) the tail's launches alone, per call of a hipGraph of 20 (no host launch rate in the number), beside the bytes each must
    move: the three launches read g once for the norm (4 B per parameter) and stream p, g, m, v (28 B); ema adds 8 B, an
    accumulator 4 B in each of the two passes.  The default tail's entry is timed twice: on its own buffers and on the
    buffers of the scheduled tail timed next (the same memory under both sets of kernels).

    python tools/steptail_bench.py [--iters 30] [--windows 5] [--out profiles/steptail_bench.txt]
"""
import argparse
import datetime
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import unet_zoo_amd  # noqa: E402
from unet_zoo_amd import GraphedStep, LrSchedule, _lib as L  # noqa: E402
from unet_zoo_amd.optim import FlatClipAdamW, FlatTail  # noqa: E402

B, C, HW, DECAY = 16, 3, 256, 0.999


def graph_us(fn, reps=20, windows=5, replays=10):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / (reps * replays))
    return statistics.median(out), min(out), max(out)


def model():
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model("unet", in_channels=C, num_classes=1)
    m.run_dtype = torch.bfloat16
    return m.cuda().train()


def step_rows(iters, windows, lines):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, C, HW, HW, generator=g).cuda()
    t = (torch.rand(B, 1, HW, HW, generator=g) > 0.5).float().cuda()
    kw = dict(lr=1e-4, weight_decay=1e-5)
    cosine = LrSchedule.cosine(total_steps=100_000, warmup_steps=500)
    s_a, s_b = GraphedStep(model(), **kw), GraphedStep(model(), schedule=cosine, **kw)
    s_c = GraphedStep(model(), schedule=cosine, ema=DECAY, **kw)
    s_d, s_e = GraphedStep(model(), **kw), GraphedStep(model(), **kw)
    s_f = GraphedStep(model(), accumulate=2, **kw)
    s_d(x, t)
    ema_d = s_d.opt.flat_p.clone()

    def run_d():
        s_d(x, t)
        ema_d.lerp_(s_d.opt.flat_p, 1.0 - DECAY)

    def run_e():
        s_e.set_lr(cosine.lr_at(s_e.steps_done, 1e-4))
        s_e(x, t)

    forms = {"(a) default": (s_a, lambda: s_a(x, t)),
             "(b) schedule=cosine": (s_b, lambda: s_b(x, t)),
             "(c) schedule=cosine, ema": (s_c, lambda: s_c(x, t)),
             "(d) default + eager ema.lerp_": (s_d, run_d),
             "(e) default + set_lr every step": (s_e, run_e),
             "(f) accumulate=2, per micro-step": (s_f, lambda: s_f(x, t))}
    for _, fn in forms.values():
        for _ in range(6):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(windows):
        for name, (_, fn) in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / iters)
    med = {}
    for name, (step, _) in forms.items():
        ms = times[name]
        med[name] = statistics.median(ms)
        lines.append(f"step {name:34s} {med[name]:.3f} ms [{min(ms):.3f} .. {max(ms):.3f}]  loss {step.loss.item():.6f}")
    a, b, c, d, e, f = (med[k] for k in forms)
    lo, hi = min(times["(a) default"]), max(times["(a) default"])
    lines.append(f"# (b) - (a) = {1e3 * (b - a):+.1f} us per step; (a)'s own windows span [{lo:.3f} .. {hi:.3f}]: (b) is "
                 f"{'inside' if lo <= b <= hi else ('BELOW' if b < lo else 'ABOVE')} that spread")
    lines.append(f"# EMA: fused (c) - (b) = {1e3 * (c - b):+.1f} us per step; eager (d) - (a) = {1e3 * (d - a):+.1f} us per step")
    lines.append(f"# set_lr every step on the default tail (e) costs {e - a:+.3f} ms per step; on the scheduled tail it is (b)")
    lines.append(f"# accumulate=2: two calls = {2 * f:.3f} ms per optimizer step against {a:.3f} ms for one call of (a)")
    lines.append(f"# {s_c.describe()}")
    return s_a.opt.n


def kernel_rows(n, lines):
    p0 = torch.randn(n, device="cuda") * 0.05

    def param():
        return [torch.nn.Parameter(p0.clone())]
    legacy = FlatClipAdamW(param(), lr=1e-4, weight_decay=1e-5)
    plain = FlatTail(param(), lr=1e-4, weight_decay=1e-5, schedule=LrSchedule.cosine(100_000))
    const = FlatTail(param(), lr=1e-4, weight_decay=1e-5)
    ema = FlatTail(param(), lr=1e-4, weight_decay=1e-5, ema=DECAY)
    acc = FlatTail(param(), lr=1e-4, weight_decay=1e-5, ema=DECAY, accumulate=2)
    grad = torch.randn(n, device="cuda") * 1e-3
    for o in (legacy, plain, const, ema, acc):
        o.flat_g.copy_(grad)
    acc.acc.copy_(grad)
    # the default tail's entry on the scheduled tail's OWN buffers: the same memory under both sets of kernels
    lib, cnt = L.load(), torch.zeros(1, device="cuda")
    ws = torch.empty(lib.uz_clip_adamw_workspace_bytes() // 4, dtype=torch.float32, device="cuda")

    def legacy_on_plain():
        L.check(lib.uz_clip_adamw(plain.flat_p.data_ptr(), plain.flat_g.data_ptr(), plain.exp_avg.data_ptr(),
                                  plain.exp_avg_sq.data_ptr(), plain.n, 1e-4, 0.9, 0.999, 1e-8, 1e-5, 1.0, cnt.data_ptr(),
                                  ws.data_ptr(), L.stream_ptr()), "uz_clip_adamw")

    rows = [("uz_clip_adamw (the default tail)", legacy.step, 32),
            ("uz_clip_adamw, next row's buffers", legacy_on_plain, 32),
            ("uz_tail_step, cosine", plain.step, 32),
            ("uz_tail_step, constant", const.step, 32),
            ("uz_tail_step, ema", ema.step, 40),
            ("uz_tail_step, ema + accumulator", acc.step, 48),
            ("uz_tail_accumulate (add)", lambda: acc.accumulate_grad(False), 12),
            ("uz_tail_swap", acc.swap_ema, 16),
            ("eager ema.lerp_(flat_p, 1 - d)", lambda: ema.ema.lerp_(ema.flat_p, 1.0 - DECAY), 12)]
    for name, fn, per in rows:
        us = graph_us(fn)
        nbytes = per * n
        lines.append(f"{name:34s} hipGraph of 20: {us[0]:8.2f} us [{us[1]:.2f} .. {us[2]:.2f}] per call | {per} B x {n} = "
                     f"{nbytes / 1e6:.1f} MB = {nbytes / us[0] / 1e6:.2f} TB/s")


class _Lines:
    """every line goes to the screen and to the output file as soon as it exists"""

    def __init__(self, out):
        self.f = None
        if out:
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            self.f = open(out, "w")

    def append(self, line):
        print(line, flush=True)
        if self.f:
            self.f.write(line + "\n")
            self.f.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/steptail_bench.py measures on the GPU; none is visible")
    p = torch.cuda.get_device_properties(0)
    lines = _Lines(a.out)
    lines.append(f"# tools/steptail_bench.py on {p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs), "
                 f"{datetime.date.today()}; median [min .. max]; one process")
    lines.append(f"# unet train step, B = {B}, {HW} x {HW}, bf16, GraphedStep, ms per call over {a.iters} calls, {a.windows} windows each, alternating")
    n = step_rows(a.iters, a.windows, lines)
    lines.append(f"# the tail's launches alone on flat buffers of n = {n} floats ({4 * n / 1e6:.0f} MB each)")
    kernel_rows(n, lines)


if __name__ == "__main__":
    main()
