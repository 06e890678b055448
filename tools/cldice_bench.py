#!/usr/bin/env python3
"""ClDiceLoss (uz_cldice_loss.hip) measured, in ONE process on one GPU:

(a) the stand-alone uz_cldice_loss call (6 launches with gradients, the base criterion's launches NOT included) on fp32 logits:
    binary (16, 1, 256, 256) at iterations 3 and 10; class indices with K = 8 (16, 8, 256, 256, background excluded); and seven
    maps of (8, 1, 512, 512) in one call (u2net); the per-call time of a hipGraph of 10 back-to-back calls, median of five
    windows.  Each case also without gradient buffers (4 launches: what GraphedEval pays).
(b) the unet GraphedStep at B = 16, 3 x 256 x 256, bf16: RegionLoss.dice() against ClDiceLoss(RegionLoss.dice()) against the
    same loss as an eager Python callable on max_pool2d (the only route without this criterion: the step splits into a
    forward graph, the eager criterion and backward graphs); `iters` steps per window, three windows each, the three steps
    ALTERNATING window by window.

    python tools/cldice_bench.py [--iters 30] [--out profiles/cldice_loss_bench.txt] [--kernel-only]
"""
import argparse
import datetime
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import unet_zoo_amd  # noqa: E402
from unet_zoo_amd import ClDiceLoss, MulticlassLoss, RegionLoss, ops  # noqa: E402

B, HW, K = 16, 256, 8
CASES = ("binary iterations=3", "binary iterations=10", "class K=8 iterations=3", "seven maps 8x1x512x512 iterations=3")


def graph_us(fn, reps=10, windows=5, replays=5):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    for _ in range(2):
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


def vessels(gen, shape):
    """a float mask of thin curved structures: the zero crossings of a blurred noise field, 2-3 pixels wide"""
    z = F.avg_pool2d(torch.randn(shape, generator=gen), 15, 1, 7)
    z = z / z.flatten(1).std(dim=1).reshape(-1, 1, 1, 1)
    return (z.abs() < 0.08).float()


def cases():
    """name -> (criterion, [logits], target) on the device, in the order of CASES: mid-training logits, the target's sign
    times a margin plus noise"""
    gen = torch.Generator().manual_seed(0)
    t = vessels(gen, (B, 1, HW, HW))
    x = (2.0 * t - 1.0) * 2.0 + 1.5 * torch.randn(B, 1, HW, HW, generator=gen)
    labels = (vessels(gen, (B, 1, HW, HW))[:, 0] * torch.randint(1, K, (B, HW // 32, HW // 32), generator=gen)
              .repeat_interleave(32, 1).repeat_interleave(32, 2)).int()
    t7 = vessels(gen, (8, 1, 512, 512))
    out = {
        CASES[0]: (ClDiceLoss(RegionLoss.dice(), iterations=3), [x], t),
        CASES[1]: (ClDiceLoss(RegionLoss.dice(), iterations=10), [x], t),
        CASES[2]: (ClDiceLoss(MulticlassLoss.ce_dice(), iterations=3), [torch.randn(B, K, HW, HW, generator=gen)], labels),
        CASES[3]: (ClDiceLoss(RegionLoss.dice(), iterations=3),
                   [(2.0 * t7 - 1.0) * 2.0 + 1.5 * torch.randn(8, 1, 512, 512, generator=gen) for _ in range(7)], t7),
    }
    return {k: (c, [v.cuda().contiguous() for v in xs], t.cuda().contiguous()) for k, (c, xs, t) in out.items()}


def kernel_rows(lines, data):
    for name, (crit, xs, t) in data.items():
        # one full call builds the plan and leaves the base's value and gradients; the timed call is uz_cldice_loss alone, on
        # those buffers (the gradient buffers are rewritten in place every time: the values drift, the work does not)
        n = len(xs)
        base_loss, _, dl = crit._base_launch(tuple(xs), t, (1.0,) * n, n - 1, (True,) * n)
        crit.direct(xs if n > 1 else xs[0], t)
        desc, items, ws, probs, skeleton, tskel = crit._plan(n, xs[0].shape, t.device, n - 1)
        scales, out, bl = crit._scales_on(t.device), torch.empty(2, device=t.device), base_loss.detach().reshape(1).clone()
        res = []
        for grads in (True, False):
            for it, x, d in zip(items, xs, dl):
                it.logits, it.dlogits, it.weight = x.data_ptr(), (d.data_ptr() if grads else None), 1.0
            res.append(graph_us(lambda: ops.cldice_loss(desc, items, t, scales, bl, out, probs, skeleton, tskel, ws)))
        torch.cuda.synchronize()
        grid, units = ops.cldice_grid(desc)
        (us, lo, hi), (us0, lo0, hi0) = res
        lines.append(f"{name:36s} hipGraph of 10: {us:9.2f} us [{lo:.2f} .. {hi:.2f}] per call with gradients (6 launches), "
                     f"{us0:9.2f} us [{lo0:.2f} .. {hi0:.2f}] without (4 launches) | {n} map(s), {units} units on {grid} workgroups, "
                     f"workspace {ws.numel() * 8 / 2 ** 20:.1f} MiB, V {float(crit.term):.4f}")


def eager_soft_skel(a, iterations):
    def erode(v):
        return torch.min(-F.max_pool2d(-v, (3, 1), (1, 1), (1, 0)), -F.max_pool2d(-v, (1, 3), (1, 1), (0, 1)))

    def opened(v):
        return F.max_pool2d(erode(v), (3, 3), (1, 1), (1, 1))
    s = F.relu(a - opened(a))
    for _ in range(iterations):
        a = erode(a)
        d = F.relu(a - opened(a))
        s = s + F.relu(d - s * d)
    return s


def eager_cldice(out, t, iterations=3, smooth=1.0):
    """soft clDice over the batch as a user writes it today (the paper's published form)"""
    p = torch.sigmoid(out.float())
    sp, st = eager_soft_skel(p, iterations), eager_soft_skel(t, iterations)
    tprec = ((sp * t).sum() + smooth) / (sp.sum() + smooth)
    tsens = ((st * p).sum() + smooth) / (st.sum() + smooth)
    return 1.0 - 2.0 * tprec * tsens / (tprec + tsens)


def step_rows(iters, lines):
    gen = torch.Generator().manual_seed(1)
    img = torch.randn(B, 3, HW, HW, generator=gen).cuda()
    target = vessels(gen, (B, 1, HW, HW)).cuda()
    dice = RegionLoss.dice()
    steps = {}
    for label, crit in (("RegionLoss.dice()", RegionLoss.dice()), ("ClDiceLoss(RegionLoss.dice())", ClDiceLoss(RegionLoss.dice())),
                        ("eager callable: dice + max_pool2d clDice", lambda out, t: dice(out, t) + 0.5 * eager_cldice(out, t))):
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
        lines.append(f"step unet bf16 {label:42s} {ms[1]:.3f} ms [{ms[0]:.3f} .. {ms[2]:.3f}] per step  {step.describe()}")
    (a, sa), (b, sb), (c, sc) = ((sorted(v[1])[1], max(v[1]) - min(v[1])) for v in steps.values())
    lines.append(f"step unet bf16 fused clDice over dice alone: {1e3 * (b - a):+.1f} us per step ({100.0 * (b - a) / a:+.2f} %)")
    lines.append(f"step unet bf16 fused clDice against the eager callable: {1e3 * (b - c):+.1f} us per step ({100.0 * (b - c) / c:+.2f} %); "
                 f"spread of the three windows: {1e3 * sa:.1f} / {1e3 * sb:.1f} / {1e3 * sc:.1f} us")


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
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/cldice_bench.py measures on the GPU; none is visible")
    p = torch.cuda.get_device_properties(0)
    lines = _Lines(a.out)
    lines.append(f"# tools/cldice_bench.py on {p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs), "
                 f"{datetime.date.today()}; median [min .. max]; one process")
    data = cases()
    kernel_rows(lines, data)
    if a.kernel_only:
        return
    lines.append(f"# unet GraphedStep, B = 16, 3 x 256 x 256, bf16, ms per step over {a.iters} steps, three windows each, alternating")
    step_rows(a.iters, lines)


if __name__ == "__main__":
    main()
