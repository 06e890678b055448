#!/usr/bin/env python3
"""BoundaryLoss (uz_boundary_loss.hip) measured, in ONE process on one GPU:

(a) the stand-alone uz_boundary_loss call (five launches, the base criterion's launches NOT included) on fp32 logits with
    gradients, B = 16, 256 x 256: binary (16, 1, 256, 256) with one map against compact discs, against a ONE-PIXEL target
    (every pixel looks at one row), against TWO pixels in the first and the last row (the worst case of the outward column
    search: the rows that hold the target span the picture, so every pixel walks until its distance is reached) and against
    an all-empty batch (the common case in medical batches: no search at all), and class indices with K = 8 (16, 8, 256, 256) against seven discs per
    image; the per-call time of a hipGraph of 20 back-to-back calls, median of five windows.
(b) the unet GraphedStep at B = 16, 3 x 256 x 256, bf16: RegionLoss.dice() against BoundaryLoss(RegionLoss.dice()) on the
    same targets; `iters` replays per window, three windows each, the two steps ALTERNATING window by window.
(c) the host yardstick: scipy.ndimage.distance_transform_edt of the same targets on this machine's CPU, one Python thread --
    what a data loader would pay per batch (and could not do after GpuAugment).
(d) with --trace DIR: the kernels' own durations from the csv a run of (a) under
    `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/boundary_bench.py --kernel-only` left in DIR.

    python tools/boundary_bench.py [--iters 30] [--out profiles/boundary_loss_bench.txt] [--kernel-only] [--trace DIR]
"""
import argparse
import csv
import datetime
import glob
import os
import re
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import unet_zoo_amd  # noqa: E402
from unet_zoo_amd import BoundaryLoss, MulticlassLoss, RegionLoss, ops  # noqa: E402

B, HW, K = 16, 256, 8
CASES = ("binary compact discs", "binary one-pixel target", "binary two pixels, top + bottom", "binary all-empty batch",
         "class K=8 compact discs")


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


def discs(rng, n, classes):
    """(n, HW, HW) int64 labels: one disc per class 1 .. classes at a seeded place"""
    yy, xx = np.mgrid[:HW, :HW]
    lab = np.zeros((n, HW, HW), dtype=np.int64)
    for i in range(n):
        for c in range(1, classes + 1):
            cy, cx, r = rng.uniform(30, HW - 30), rng.uniform(30, HW - 30), rng.uniform(8, 40 if classes == 1 else 22)
            lab[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = c
    return lab


def cases():
    """name -> (criterion, logits, target) on the device, in the order of CASES"""
    rng = np.random.RandomState(0)
    gen = torch.Generator().manual_seed(0)
    xb = torch.randn(B, 1, HW, HW, generator=gen)
    one = torch.zeros(B, 1, HW, HW)
    one[:, 0, HW - 1, HW // 2] = 1.0
    two = torch.zeros(B, 1, HW, HW)
    two[:, 0, 0, 0] = two[:, 0, HW - 1, HW - 1] = 1.0
    out = {
        CASES[0]: (BoundaryLoss(RegionLoss.dice()), xb, torch.from_numpy(discs(rng, B, 1)[:, None]).float()),
        CASES[1]: (BoundaryLoss(RegionLoss.dice()), xb, one),
        CASES[2]: (BoundaryLoss(RegionLoss.dice()), xb, two),
        CASES[3]: (BoundaryLoss(RegionLoss.dice()), xb, torch.zeros(B, 1, HW, HW)),
        CASES[4]: (BoundaryLoss(MulticlassLoss.ce_dice()), torch.randn(B, K, HW, HW, generator=gen),
                   torch.from_numpy(discs(rng, B, K - 1)).int()),
    }
    return {k: (c, x.cuda().contiguous(), t.cuda().contiguous()) for k, (c, x, t) in out.items()}


def kernel_rows(lines, data):
    for name, (crit, x, t) in data.items():
        # one full call builds the plan and leaves the base's value and gradient; the timed call is uz_boundary_loss alone, on
        # those buffers (its gradient buffer is rewritten in place every time: the values drift, the work does not)
        base_loss, _, dl = crit._base_launch((x,), t, (1.0,), 0, (True,))
        crit.direct(x, t)
        desc, items, ws, sd2 = crit._plan(1, x.shape, x.device, 0)
        items[0].logits, items[0].dlogits, items[0].weight = x.data_ptr(), dl[0].data_ptr(), 1.0
        scales, out, bl = crit._scales_on(x.device), torch.empty(2, device=x.device), base_loss.detach().reshape(1).clone()
        us = graph_us(lambda: ops.boundary_loss(desc, items, t, scales, bl, out, sd2, ws))
        torch.cuda.synchronize()
        s = sd2.cpu()
        lines.append(f"{name:31s} hipGraph of 20: {us[0]:8.2f} us [{us[1]:.2f} .. {us[2]:.2f}] per call (5 launches) | "
                     f"{s.shape[0]} planes, {int((s != 0).flatten(1).any(1).sum())} searched, max |sd2| {int(s.abs().max())}, "
                     f"boundary term {float(crit.term):+.4f}")


def step_rows(iters, lines):
    gen = torch.Generator().manual_seed(1)
    img = torch.randn(B, 3, HW, HW, generator=gen).cuda()
    target = torch.from_numpy(discs(np.random.RandomState(1), B, 1)[:, None]).float().cuda()
    steps = {}
    for label, crit in (("RegionLoss.dice()", RegionLoss.dice()), ("BoundaryLoss(RegionLoss.dice())", BoundaryLoss(RegionLoss.dice()))):
        torch.manual_seed(0)
        m = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=1)
        m.run_dtype = torch.bfloat16
        step = unet_zoo_amd.GraphedStep(m.cuda().train(), crit, lr=1e-4)
        for _ in range(5):
            step(img, target)
        steps[label] = (step, [])
    torch.cuda.synchronize()
    for _ in range(3):
        for step, ms in steps.values():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                loss = step(img, target)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / iters)
    for label, (step, ms) in steps.items():
        ms.sort()
        lines.append(f"step unet bf16 {label:34s} {ms[1]:.3f} ms [{ms[0]:.3f} .. {ms[2]:.3f}] per step  {step.describe()}")
    a, b = (sorted(v[1])[1] for v in steps.values())
    lines.append(f"step unet bf16 difference of the medians: {1e3 * (b - a):+.1f} us per step ({100.0 * (b - a) / a:+.2f} %)")


def host_rows(lines, data):
    try:
        from scipy import ndimage as ndi
    except ImportError:
        lines.append("host yardstick: scipy is not installed on this machine; not measured")
        return
    for name, (_, x, t) in data.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        th = t.cpu().numpy()
        t1 = time.perf_counter()
        if th.dtype.kind == "f":
            planes = [th[n, c] > 0.5 for n in range(th.shape[0]) for c in range(th.shape[1])]
        else:
            planes = [th[n] == c for n in range(th.shape[0]) for c in range(1, x.shape[1])]
        for G in planes:
            if G.any() and not G.all():
                ndi.distance_transform_edt(~G) * ~G - (ndi.distance_transform_edt(G) - 1) * G
        t2 = time.perf_counter()
        lines.append(f"host {name:31s} copy back {1e3 * (t1 - t0):7.2f} ms + scipy distance_transform_edt {1e3 * (t2 - t1):8.2f} ms "
                     f"for {len(planes)} planes, one Python thread")


def trace_rows(trace_dir, lines):
    """the cases of (a) run one after the other with the same number of calls each: a kernel's launches in time order fall
    into as many equal groups as cases use it (rows and loss are one instantiation per mode: four binary cases, one class)"""
    d = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "boundary_" in r["Kernel_Name"]:
                d.setdefault(r["Kernel_Name"], []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    if not d:
        sys.exit(f"no boundary kernel in the kernel traces under {trace_dir}")
    for k, v in sorted(d.items()):
        v.sort()
        name = re.search(r"boundary_\w+(<[^>]*>)?", k).group(0)
        mine = CASES[:4] if name.endswith("<0>") else CASES[4:] if name.endswith("<1>") else CASES
        if len(v) % len(mine):
            sys.exit(f"{name}: {len(v)} launches do not split into {len(mine)} cases")
        n = len(v) // len(mine)
        cols = []
        for c, case in enumerate(mine):
            us = sorted(t for _, t in v[c * n:(c + 1) * n])
            cols.append(f"{case} {us[n // 2]:8.2f} [{us[0]:.2f} .. {us[-1]:.2f}]")
        lines.append(f"kernel trace  {name:28s} n = {n:4d} per case, us  " + " | ".join(cols))


class _Lines:
    """every line goes to the screen and to the output file as soon as it exists"""

    def __init__(self, out, mode="w"):
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--trace", default=None, help="summarise the boundary kernels of a rocprofv3 csv kernel trace and stop")
    a = ap.parse_args()
    if a.trace:
        lines = _Lines(a.out, "a")
        lines.append(f"# tools/boundary_bench.py --trace: kernel durations of `rocprofv3 --kernel-trace -- python tools/boundary_bench.py "
                     f"--kernel-only`, {datetime.date.today()}")
        trace_rows(a.trace, lines)
        return
    if not torch.cuda.is_available():
        sys.exit("tools/boundary_bench.py measures on the GPU; none is visible")
    p = torch.cuda.get_device_properties(0)
    lines = _Lines(a.out)
    lines.append(f"# tools/boundary_bench.py on {p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs), "
                 f"{datetime.date.today()}; median [min .. max]; one process")
    data = cases()
    kernel_rows(lines, data)
    if a.kernel_only:
        return
    lines.append(f"# unet GraphedStep, B = 16, 3 x 256 x 256, bf16, ms per step over {a.iters} replays, three windows each, alternating")
    step_rows(a.iters, lines)
    lines.append("# host yardstick on this machine's CPU (for orientation)")
    host_rows(lines, data)


if __name__ == "__main__":
    main()
