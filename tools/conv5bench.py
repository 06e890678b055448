"""Time the k = 5 convolution family (forward, input gradient, weight gradient) at VNet's layer shapes, next to the 3x3
kernels of the same library and to the vendor library (torch's conv2d: MIOpen with its solver search, bf16 channels_last, as
tools/miopen_yardstick.py runs it) at the same channels / map / batch in the same run.

    python tools/conv5bench.py [--batch 16] [--dtype bf16] [--iters 20]

One line per (C, H): milliseconds and achieved TFLOP/s (2 * P * C^2 * taps); each figure is the median of 5 groups of
`--iters` calls between events, after 3 warm-up calls (the yardstick's timing)."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from unet_zoo_amd import _lib as L  # noqa: E402
from unet_zoo_amd import ops  # noqa: E402

SHAPES = [(32, 256), (32, 128), (64, 128), (64, 64), (128, 64), (128, 32), (256, 32), (256, 16)]


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / iters)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    torch.backends.cudnn.benchmark = True      # MIOpen: search for the fastest solver per shape
    print(f"# B={a.batch} {a.dtype}: ms (TFLOP/s)   k5 fwd | k5 dgrad | k5 wgrad || vendor k5 fwd | dgrad | wgrad || k3 fwd | k3 wgrad")
    for C, H in SHAPES:
        N = a.batch
        x = ops.new_act(N, H, H, C, dt, "cuda")
        x.buf.normal_()
        y = ops.new_act(N, H, H, C, dt, "cuda")
        w5 = torch.randn(C, C, 5, 5, device="cuda") / (5 * C ** 0.5)
        wf, wd = ops.pack_weights(w5, L.PACK_CONV_FWD, dt), ops.pack_weights(w5, L.PACK_CONV_DGRAD, dt)
        fl5 = 2.0 * x.P * C * C * 25
        t = [timed(lambda: ops.conv5x5(x, wf, None, y, want_stats=True), a.iters),
             timed(lambda: ops.conv5x5(x, wd, None, y), a.iters),
             timed(lambda: ops.wgrad5x5(y, x, (C, C, 5, 5)), a.iters)]
        line = f"C={C:3d} H={H:3d} | " + " | ".join(f"{ms:7.3f} ({fl5 / ms * 1e-9:6.1f})" for ms in t)
        xv = torch.randn(N, C, H, H, device="cuda", dtype=dt).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        wv = w5.to(dt).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        yv = F.conv2d(xv, wv, padding=2)
        gv = torch.randn_like(yv)
        tv = [timed(lambda: F.conv2d(xv, wv, padding=2), a.iters),
              timed(lambda: torch.autograd.grad(yv, xv, gv, retain_graph=True), a.iters),
              timed(lambda: torch.autograd.grad(yv, wv, gv, retain_graph=True), a.iters)]
        line += " || " + " | ".join(f"{ms:7.3f} ({fl5 / ms * 1e-9:6.1f})" for ms in tv)
        del xv, wv, yv, gv
        if C >= 64:
            w3 = ops.pack_weights(torch.randn(C, C, 3, 3, device="cuda") / (3 * C ** 0.5), L.PACK_CONV_FWD, dt)
            fl3 = 2.0 * x.P * C * C * 9
            t3 = [timed(lambda: ops.conv_igemm(x, w3, None, y, ntaps=9, want_stats=True), a.iters),
                  timed(lambda: ops.wgrad(y, x, (C, C, 3, 3), ntaps=9), a.iters)]
            line += " || " + " | ".join(f"{ms:7.3f} ({fl3 / ms * 1e-9:6.1f})" for ms in t3)
        print(line, flush=True)


if __name__ == "__main__":
    main()
