#!/usr/bin/env python3
"""GpuAugment (uz_augment.hip) measured, in ONE process on one GPU:

(a) uz_augment_apply (with the uz_augment_params launch in front of it, as GpuAugment issues them) at B = 16, 3 x 256 x 256
    with a 1-channel fp32 mask: the per-call time of a hipGraph of 20 back-to-back calls (median of five windows: no host
    launch rate in the number), of uz_augment_apply alone and of the draw + uz_augment_params + uz_augment_apply, for a rotation + scaling + translation + jitter and for the same with a 4 x 4 displacement
    grid; beside it the bytes the launch must move (picture and mask read once and written once) and the time those bytes take
    at the 6.3 TB/s a float4 copy reaches on this GPU.  The 33.5 MB of one call fit the 256 MB Infinity Cache, so back-to-back
    calls can run above that roof; the figure says what the launch costs, not what HBM delivers.
(b) the unet training step, B = 16, 256 x 256, bf16, from GraphedStep with and without `augment=`: `iters` steps per
    window, three windows each, the two steps ALTERNATING window by window; median [min .. max].

(c) with --trace DIR: the augmentation kernels' own durations from the csv a run of (a)'s first setting under
    `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/augbench.py --kernel-only` left in DIR (a run of its
    own: tracing slows the host): median [min .. max] over the graph replays, no kernel boundary in the number.

    python tools/augbench.py [--iters 30] [--out profiles/augment_256_b16.txt] [--kernel-only] [--trace DIR]
"""
import argparse
import csv
import datetime
import glob
import os
import re
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import unet_zoo_amd  # noqa: E402
from unet_zoo_amd import GpuAugment, ops  # noqa: E402

SHAPE = (16, 3, 256, 256)
ROOF_TBS = 6.3
AUG = dict(hflip=0.5, vflip=0.5, rotate=15.0, scale=(0.9, 1.1), translate=0.05, brightness=0.1, contrast=0.1)


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


def kernel_rows(lines, first_only=False):
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(SHAPE, generator=gen).cuda()
    t = (torch.rand((SHAPE[0], 1) + SHAPE[2:], generator=gen) > 0.5).float().cuda()
    nbytes = 2 * 4 * (x.numel() + t.numel())
    floor = nbytes / (ROOF_TBS * 1e12) * 1e6
    for name, kw in (("warp + jitter", AUG), ("warp + jitter + 4x4 grid", dict(AUG, grid_distort=(4, 3.0))))[:1 if first_only else 2]:
        aug = GpuAugment(**kw)
        bound = aug.bind(x, t)
        us = graph_us(bound.run)
        ap = graph_us(lambda: ops.augment_apply(bound.desc, bound.image, bound.mask, bound.params, bound.disp, bound.out_image,
                                                bound.out_mask))
        lines.append(f"{'x'.join(map(str, SHAPE)):14s} + 1-channel mask  {name:26s} hipGraph of 20: {ap[0]:7.2f} us [{ap[1]:.2f} .. {ap[2]:.2f}] per "
                     f"call (uz_augment_apply alone, a kernel boundary included) | {nbytes / 1e6:.2f} MB = {nbytes / ap[0] / 1e6:.2f} TB/s; at the "
                     f"{ROOF_TBS} TB/s copy roof {floor:.2f} us (x {ap[0] / floor:.2f})")
        lines.append(f"{'x'.join(map(str, SHAPE)):14s} + 1-channel mask  {name:26s} hipGraph of 20: {us[0]:7.2f} us [{us[1]:.2f} .. {us[2]:.2f}] per "
                     f"call (the draw + params + apply) | {nbytes / 1e6:.2f} MB = {nbytes / us[0] / 1e6:.2f} TB/s; at the {ROOF_TBS} TB/s copy roof "
                     f"{floor:.2f} us (x {us[0] / floor:.2f})")


def step_rows(iters, lines):
    gen = torch.Generator().manual_seed(1)
    img = torch.randn(SHAPE, generator=gen).cuda()
    mask = (torch.rand((SHAPE[0], 1) + SHAPE[2:], generator=gen) > 0.5).float().cuda()
    steps = {}
    for name, aug in (("without augment", None), ("with augment=GpuAugment(...)", GpuAugment(**AUG))):
        torch.manual_seed(0)
        m = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=1)
        m.run_dtype = torch.bfloat16
        m = m.cuda().train()
        step = unet_zoo_amd.GraphedStep(m, lr=1e-4, weight_decay=1e-5, augment=aug)
        for _ in range(5):
            step(img, mask)
        steps[name] = (step, [])
    torch.cuda.synchronize()
    for _ in range(3):
        for step, ms in steps.values():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                step(img, mask)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / iters)
    for name, (step, ms) in steps.items():
        ms.sort()
        lines.append(f"step {name:30s} {ms[1]:.3f} ms [{ms[0]:.3f} .. {ms[2]:.3f}]  loss {step.loss.item():.6f}  {step.describe()}")


def trace_rows(trace_dir, lines):
    d = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "augment_" in r["Kernel_Name"]:
                d.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    if not d:
        sys.exit(f"no augmentation kernel in the kernel traces under {trace_dir}")
    nbytes = 2 * 4 * (SHAPE[0] * SHAPE[1] + SHAPE[0]) * SHAPE[2] * SHAPE[3]
    for k, v in sorted(d.items()):
        v.sort()
        med = v[len(v) // 2]
        rate = f" | {nbytes / 1e6:.2f} MB = {nbytes / med / 1e6:.2f} TB/s of the {ROOF_TBS} TB/s copy roof" if "apply" in k else ""
        name = re.search(r"augment_\w+(<[^>]*>)?", k).group(0)
        lines.append(f"kernel trace  {name:34s} n = {len(v):4d}  {med:6.2f} us [{v[0]:.2f} .. {v[-1]:.2f}]{rate}")


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
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--trace", default=None, help="summarise the augmentation kernels of a rocprofv3 csv kernel trace and stop")
    a = ap.parse_args()
    if a.trace:
        lines = _Lines(a.out)
        lines.append(f"# tools/augbench.py --trace: kernel durations of `rocprofv3 --kernel-trace -- python tools/augbench.py --kernel-only` "
                     f"(warp + jitter, no displacement grid), {datetime.date.today()}")
        trace_rows(a.trace, lines)
        return
    if not torch.cuda.is_available():
        sys.exit("tools/augbench.py measures on the GPU; none is visible")
    p = torch.cuda.get_device_properties(0)
    lines = _Lines(a.out)
    lines.append(f"# tools/augbench.py on {p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs), "
                 f"{datetime.date.today()}; median [min .. max]; one process")
    kernel_rows(lines, first_only=a.kernel_only)
    if a.kernel_only:
        return
    lines.append(f"# unet train step, B = 16, 256 x 256, bf16, GraphedStep, ms per step over {a.iters} steps, three windows each, alternating")
    step_rows(a.iters, lines)


if __name__ == "__main__":
    main()
