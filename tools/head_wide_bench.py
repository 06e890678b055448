#!/usr/bin/env python3
"""The wide 1x1 head (uz_head_wide.hip) measured, in ONE process on one GPU:

(a) kernels, bf16, P = 16 * 256 * 256 pixels, C = 64: forward and backward (with dx) of
      the narrow head (uz_outconv_*) at K = 8,
      the wide head (uz_head_wide_*) at K = 8, 9, 16, 19, 32,
      torch's F.conv2d 1x1 (bf16, channels_last) at K = 19, forward and backward (input, weight and bias gradients),
    the library's own as the per-call time of a hipGraph of 20 back-to-back calls (no host launch rate in the number), torch's
    as 20 eager calls between two events.  The forms are
    measured INTERLEAVED: `--rounds` rounds, every form once per round, in the order shown; median [min .. max] over the rounds.
    GB/s = the bytes the product needs (x once per direction, dx once, logits / logit gradients once) over that time.
(b) the whole GraphedStep of unet (bf16, B = 16, 3 x 256 x 256) with num_classes = 8, 9 and 19 and MulticlassLoss.ce_dice(),
    interleaved in the same way, ms per step.

    python tools/head_wide_bench.py [--rounds 5] [--out profiles/head_wide_bench.txt] [--kernels-only | --steps-only]
    python tools/head_wide_bench.py --steps-only --classes 8 --root <another checkout>     # the same step from another tree
"""
import argparse
import datetime
import os
import statistics
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--out", default=None)
ap.add_argument("--append", action="store_true")
ap.add_argument("--kernels-only", action="store_true")
ap.add_argument("--steps-only", action="store_true")
ap.add_argument("--classes", default="8,9,19")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the checkout whose unet_zoo_amd is measured (default: this one)")
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.root))

import unet_zoo_amd  # noqa: E402
from unet_zoo_amd import MulticlassLoss, ops  # noqa: E402

B, S, C = 16, 256, 64


def graph_of(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return g, reps


def time_graph(g, reps, replays=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay() if reps > 1 else g()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * replays)     # us per call


def eager_of(fn, calls=20):
    """torch's own convolution is timed as `calls` eager calls between two events (its library calls are not captured here):
    the number contains the host's launch rate where that is slower than the kernels"""
    def many():
        for _ in range(calls):
            fn()
    for _ in range(3):
        many()
    torch.cuda.synchronize()
    return many, 1


def kernel_rows(lines, rounds):
    gen = torch.Generator().manual_seed(0)
    P = B * S * S
    x = ops.Act(torch.randn(P, C, generator=gen).to(torch.bfloat16).cuda(), 0, C, B, S, S)
    forms = []        # (label, graph, reps, bytes)
    keep = []         # the operands the captured calls read and write live as long as the graphs: a replay uses their addresses,
    #                   and the next capture's empty_cache() hands freed blocks back to the driver

    def add(label, K, fwd, bwd):
        w = (torch.randn(K, C, generator=gen) / 8).cuda()
        b = torch.zeros(K).cuda()
        gl = torch.randn(B, K, S, S, generator=gen).cuda()
        dx = ops.new_act(B, S, S, C, torch.bfloat16, "cuda")
        keep.append((w, b, gl, dx))
        forms.append((f"{label} K={K:2d} forward ", *graph_of(lambda: fwd(x, w, b)), 2.0 * P * C + 4.0 * K * P))
        forms.append((f"{label} K={K:2d} backward", *graph_of(lambda: bwd(x, w, gl, dx)), 4.0 * P * C + 4.0 * K * P))

    add("narrow uz_outconv  ", 8, ops.outconv_fwd, ops.outconv_bwd)
    for K in (8, 9, 16, 19, 32):
        add("wide   uz_head_wide", K, ops.head_wide_fwd, ops.head_wide_bwd)
    K = 19
    conv = torch.nn.Conv2d(C, K, 1).cuda().to(torch.bfloat16).to(memory_format=torch.channels_last)
    xt = x.buf.view(B, S, S, C).permute(0, 3, 1, 2).detach().requires_grad_(True)      # NCHW view of NHWC memory: channels_last
    assert xt.is_contiguous(memory_format=torch.channels_last)
    gt = torch.randn(B, K, S, S, generator=gen).cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

    def stock_fwd():
        with torch.no_grad():
            return conv(xt)

    def stock_bwd():
        return torch.ops.aten.convolution_backward(gt, xt, conv.weight, [K], [1, 1], [0, 0], [1, 1], False, [0, 0], 1, [True, True, True])

    forms.append((f"stock  F.conv2d 1x1 (eager) K={K:2d} forward ", *eager_of(stock_fwd), 2.0 * P * C + 2.0 * K * P))
    forms.append((f"stock  F.conv2d 1x1 (eager) K={K:2d} backward", *eager_of(stock_bwd), 4.0 * P * C + 2.0 * K * P))
    us = {f[0]: [] for f in forms}
    for _ in range(rounds):
        for label, g, reps, _ in forms:
            t = time_graph(g, reps)
            us[label].append(t / 20 if reps == 1 else t)     # an eager form is 20 calls per invocation
    for label, _, _, nbytes in forms:
        v = sorted(us[label])
        med = statistics.median(v)
        lines.append(f"{label}  {med:8.2f} us [{v[0]:.2f} .. {v[-1]:.2f}]  {nbytes / 1e6:6.1f} MB  {nbytes / med / 1e3:6.0f} GB/s")
    del keep
    return {k: statistics.median(v) for k, v in us.items()}


def step_rows(lines, rounds, iters, classes):
    gen = torch.Generator().manual_seed(1)
    img = torch.randn(B, 3, S, S, generator=gen).cuda()
    steps = []
    for K in classes:
        torch.manual_seed(0)
        m = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=K)
        m.run_dtype = torch.bfloat16
        m = m.cuda().train()
        gs = unet_zoo_amd.GraphedStep(m, MulticlassLoss.ce_dice(), lr=1e-4, weight_decay=1e-5, max_norm=1.0)
        y = torch.randint(0, K, (B, S, S), generator=gen).int().cuda()
        for _ in range(5):
            gs(img, y)
        torch.cuda.synchronize()
        steps.append((K, gs, y))
    ms = {K: [] for K in classes}
    for _ in range(rounds):
        for K, gs, y in steps:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                gs(img, y)
            e1.record()
            torch.cuda.synchronize()
            ms[K].append(e0.elapsed_time(e1) / iters)
    for K in classes:
        v = sorted(ms[K])
        lines.append(f"step unet bf16 B=16 256x256 num_classes={K:2d}  {statistics.median(v):.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}] per step "
                     f"({rounds} windows of {iters} steps, interleaved)   tree: {os.path.relpath(os.path.abspath(ARGS.root))}")


class _Lines:
    def __init__(self, out, mode):
        self.f = None
        if out:
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            self.f = open(out, mode)

    def append(self, line):
        print(line, flush=True)
        if self.f:
            self.f.write(line + "\n")
            self.f.flush()


def main():
    if not torch.cuda.is_available():
        sys.exit("tools/head_wide_bench.py measures on the GPU; none is visible")
    p = torch.cuda.get_device_properties(0)
    lines = _Lines(ARGS.out, "a" if ARGS.append else "w")
    lines.append(f"# tools/head_wide_bench.py on {p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs), "
                 f"{datetime.date.today()}; median [min .. max] over {ARGS.rounds} interleaved rounds; one process")
    if not ARGS.steps_only:
        lines.append(f"# kernels: bf16, P = {B} * {S} * {S}, C = {C}; us per call inside a hipGraph of 20 calls")
        kernel_rows(lines, ARGS.rounds)
    if not ARGS.kernels_only:
        step_rows(lines, ARGS.rounds, ARGS.iters, [int(k) for k in ARGS.classes.split(",")])


if __name__ == "__main__":
    main()
