#!/usr/bin/env python3
"""LovaszLoss (uz_lovasz_loss.hip) measured, in ONE process on one GPU:

(a) the stand-alone uz_lovasz_loss call (19 launches, the base criterion's launches NOT included) on fp32 logits with
    gradients: binary (16, 1, 256, 256), per image, with early-training logits (every error positive: all 2^20 elements are
    ranked), late-training logits (about 5 % ranked) and all-empty targets; class indices with K = 8 (16, 8, 256, 256); and
    seven maps of (8, 1, 512, 512) in one call (u2net); the per-call time of a hipGraph of 20 back-to-back calls, median of five
    windows.
(b) the unet GraphedStep at B = 16, 3 x 256 x 256, bf16: RegionLoss.dice() against LovaszLoss(RegionLoss.dice()) against the
    same loss as an eager Python callable on torch.sort (the only route without this criterion: the step splits into a
    forward graph, the eager criterion and backward graphs); `iters` steps per window, three windows each, the three steps
    ALTERNATING window by window.
(c) with --trace DIR: the kernels' own durations from the csv a run of (a) under
    `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/lovasz_bench.py --kernel-only` left in DIR.

    python tools/lovasz_bench.py [--iters 30] [--out profiles/lovasz_loss_bench.txt] [--kernel-only] [--trace DIR]
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
from unet_zoo_amd import LovaszLoss, MulticlassLoss, RegionLoss, ops  # noqa: E402

B, HW, K = 16, 256, 8
CASES = ("binary early (all ranked)", "binary late (5 % ranked)", "binary all-empty targets", "class K=8", "seven maps 8x1x512x512")
CLASS_CASE = 3


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


def blobs(gen, shape):
    """a float mask of smooth blobs: a blurred noise field above its 70 % quantile"""
    z = torch.nn.functional.avg_pool2d(torch.randn(shape, generator=gen), 31, 1, 15)
    return (z > z.flatten(1).quantile(0.7, dim=1).reshape(-1, 1, 1, 1)).float()


def cases():
    """name -> (criterion, [logits], target) on the device, in the order of CASES"""
    gen = torch.Generator().manual_seed(0)
    t = blobs(gen, (B, 1, HW, HW))
    s = 2.0 * t - 1.0
    early = 0.3 * torch.randn(B, 1, HW, HW, generator=gen)                          # |x| < 1: every e = 1 - x s > 0
    margin = 1.0 + 2.0 * torch.randn(B, 1, HW, HW, generator=gen).abs()
    wrong = torch.rand(B, 1, HW, HW, generator=gen) < 0.05
    late = s * torch.where(wrong, 0.5 * torch.randn(B, 1, HW, HW, generator=gen), margin)
    labels = torch.randint(0, K, (B, HW // 16, HW // 16), generator=gen).repeat_interleave(16, 1).repeat_interleave(16, 2)
    t7 = blobs(gen, (8, 1, 512, 512))
    out = {
        CASES[0]: (LovaszLoss(RegionLoss.dice()), [early], t),
        CASES[1]: (LovaszLoss(RegionLoss.dice()), [late], t),
        CASES[2]: (LovaszLoss(RegionLoss.dice()), [early], torch.zeros(B, 1, HW, HW)),
        CASES[3]: (LovaszLoss(MulticlassLoss.ce_dice()), [torch.randn(B, K, HW, HW, generator=gen)], labels.int()),
        CASES[4]: (LovaszLoss(RegionLoss.dice()), [torch.randn(8, 1, 512, 512, generator=gen) for _ in range(7)], t7),
    }
    return {k: (c, [x.cuda().contiguous() for x in xs], t.cuda().contiguous()) for k, (c, xs, t) in out.items()}


def kernel_rows(lines, data):
    for name, (crit, xs, t) in data.items():
        # one full call builds the plan and leaves the base's value and gradients; the timed call is uz_lovasz_loss alone, on
        # those buffers (the gradient buffers are rewritten in place every time: the values drift, the work does not)
        n = len(xs)
        base_loss, _, dl = crit._base_launch(tuple(xs), t, (1.0,) * n, n - 1, (True,) * n)
        crit.direct(xs if n > 1 else xs[0], t)
        desc, items, ws, errors, ranks = crit._plan(n, xs[0].shape, t.device, n - 1)
        for it, x, d in zip(items, xs, dl):
            it.logits, it.dlogits, it.weight = x.data_ptr(), d.data_ptr(), 1.0
        scales, out, bl = crit._scales_on(t.device), torch.empty(2, device=t.device), base_loss.detach().reshape(1).clone()
        us = graph_us(lambda: ops.lovasz_loss(desc, items, t, scales, bl, out, errors, ranks, ws))
        torch.cuda.synchronize()
        ranked = int((ranks >= 0).sum())
        lines.append(f"{name:27s} hipGraph of 20: {us[0]:8.2f} us [{us[1]:.2f} .. {us[2]:.2f}] per call (19 launches) | "
                     f"{n} map(s), {ranks.shape[0]} segments of {ranks.shape[1]}, {100.0 * ranked / ranks.numel():.1f} % of the main "
                     f"map ranked, workspace {ws.numel() * 8 / 2 ** 20:.1f} MiB, V {float(crit.term):.4f}")


def eager_lovasz_hinge(out, t):
    """the Lovasz hinge per image as a user writes it today: torch.sort, cumsum, Jaccard, differences"""
    n = out.shape[0]
    x, b = out.float().reshape(n, -1), t.reshape(n, -1) > 0.5
    e = 1.0 - x * torch.where(b, 1.0, -1.0)
    es, perm = torch.sort(e, dim=1, descending=True)
    bs = torch.gather(b.float(), 1, perm)
    G = bs.sum(1, keepdim=True)
    J = 1.0 - (G - bs.cumsum(1)) / (G + (1.0 - bs).cumsum(1))
    g = torch.cat([J[:, :1], J[:, 1:] - J[:, :-1]], dim=1)
    return (torch.relu(es) * g).sum(1).mean()


def step_rows(iters, lines):
    gen = torch.Generator().manual_seed(1)
    img = torch.randn(B, 3, HW, HW, generator=gen).cuda()
    target = blobs(gen, (B, 1, HW, HW)).cuda()
    dice = RegionLoss.dice()
    steps = {}
    for label, crit in (("RegionLoss.dice()", RegionLoss.dice()), ("LovaszLoss(RegionLoss.dice())", LovaszLoss(RegionLoss.dice())),
                        ("eager callable: dice + torch.sort hinge", lambda out, t: dice(out, t) + eager_lovasz_hinge(out, t))):
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
                step(img, target)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / iters)
    for label, (step, ms) in steps.items():
        ms.sort()
        lines.append(f"step unet bf16 {label:40s} {ms[1]:.3f} ms [{ms[0]:.3f} .. {ms[2]:.3f}] per step  {step.describe()}")
    a, b, c = (sorted(v[1])[1] for v in steps.values())
    lines.append(f"step unet bf16 fused Lovasz over dice alone: {1e3 * (b - a):+.1f} us per step ({100.0 * (b - a) / a:+.2f} %)")
    lines.append(f"step unet bf16 fused Lovasz against the eager callable: {1e3 * (b - c):+.1f} us per step ({100.0 * (b - c) / c:+.2f} %)")


def trace_rows(trace_dir, lines):
    """the cases of (a) run one after the other with the same number of calls each: a kernel's launches in time order fall
    into as many equal groups as cases use it (keys and grad are one kernel per mode: four binary cases, one class)"""
    d = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "lovasz_" in r["Kernel_Name"]:
                d.setdefault(r["Kernel_Name"], []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    if not d:
        sys.exit(f"no lovasz kernel in the kernel traces under {trace_dir}")
    binary = [c for i, c in enumerate(CASES) if i != CLASS_CASE]
    for k, v in sorted(d.items()):
        v.sort()
        name = re.search(r"lovasz_\w+", k).group(0)
        mine = binary if "_binary_" in name else [CASES[CLASS_CASE]] if "_class_" in name else CASES
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
    ap.add_argument("--trace", default=None, help="summarise the lovasz kernels of a rocprofv3 csv kernel trace and stop")
    a = ap.parse_args()
    if a.trace:
        lines = _Lines(a.out, "a")
        lines.append(f"# tools/lovasz_bench.py --trace: kernel durations of `rocprofv3 --kernel-trace -- python tools/lovasz_bench.py "
                     f"--kernel-only`, {datetime.date.today()}")
        trace_rows(a.trace, lines)
        return
    if not torch.cuda.is_available():
        sys.exit("tools/lovasz_bench.py measures on the GPU; none is visible")
    p = torch.cuda.get_device_properties(0)
    lines = _Lines(a.out)
    lines.append(f"# tools/lovasz_bench.py on {p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs), "
                 f"{datetime.date.today()}; median [min .. max]; one process")
    data = cases()
    kernel_rows(lines, data)
    if a.kernel_only:
        return
    lines.append(f"# unet GraphedStep, B = 16, 3 x 256 x 256, bf16, ms per step over {a.iters} steps, three windows each, alternating")
    step_rows(a.iters, lines)


if __name__ == "__main__":
    main()
