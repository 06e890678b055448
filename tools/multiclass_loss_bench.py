#!/usr/bin/env python3
"""MulticlassLoss (uz_class_loss) measured, in ONE process on one GPU:

(a) `MulticlassLoss.ce_dice().direct` on fp32 logits of (16, 9, 256, 256) and (16, 4, 256, 256) with int32 labels: the
    median of `calls` single calls issued from Python (events around each call), and the per-call time of a hipGraph of
    20 back-to-back calls (median of five windows: no host launch rate in the number), with and without the gradient;
    yardstick 1: the same loss and its gradient from torch ops (F.cross_entropy + softmax Dice + autograd.grad), eager, the
    median of `calls` calls; yardstick 2: the bytes the three launches must move -- x read twice, the labels read twice,
    dlogits written once -- at the 4.3 TB/s the sister kernel's pass reaches on this GPU.
(b) the unet training step at num_classes = 8, B = 16, 256 x 256, bf16 from GraphedStep with MulticlassLoss.ce_dice() on
    class-index labels and, beside it, with "bce_dice" on the one-hot masks of the same labels: `iters` steps, three
    windows, median [min .. max].  (8, not Synapse's 9: unet's 1x1 head kernel, uz_outconv_fwd, takes at most 8 output
    channels; the loss kernel's own K = 9 figures are in (a).)

    python tools/multiclass_loss_bench.py [--calls 30] [--iters 30] [--out profiles/multiclass_loss_bench.txt]
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
from unet_zoo_amd import MulticlassLoss  # noqa: E402

SHAPES = [(16, 9, 256, 256), (16, 4, 256, 256)]
YARD_TBS = 4.3
STEP_CLASSES = 8


def each_call_us(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out), min(out), max(out)


def graph_us(fn, reps=20, windows=5, replays=10):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
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


def torch_ce_dice(x, y, w_ce=0.4, w_dice=0.6, smooth=1e-5):
    """the published recipe with torch ops: 0.4 CE + 0.6 Dice (squared probabilities, batch sums), and its gradient"""
    leaf = x.detach().requires_grad_(True)
    K = x.shape[1]
    ce = F.cross_entropy(leaf, y)
    p = torch.softmax(leaf, dim=1)
    onehot = F.one_hot(y, K).permute(0, 3, 1, 2).to(p.dtype)
    I = (p * onehot).sum((0, 2, 3))
    S = (p * p).sum((0, 2, 3))
    T = onehot.sum((0, 2, 3))
    dice = (1 - (2 * I + smooth) / (S + T + smooth)).mean()
    loss = w_ce * ce + w_dice * dice
    (g,) = torch.autograd.grad(loss, leaf)
    return loss.detach(), g


def kernel_rows(calls, lines):
    for shape in SHAPES:
        N, K, H, W = shape
        gen = torch.Generator().manual_seed(0)
        x = (3.0 * torch.randn(shape, generator=gen)).cuda()
        y64 = torch.randint(0, K, (N, H, W), generator=gen).cuda()
        y = y64.int()
        crit = MulticlassLoss.ce_dice()
        bytes_grad = (3 * K * 4 + 2 * 4) * N * H * W
        bytes_nograd = (K * 4 + 4) * N * H * W

        def with_grad():
            return crit.direct(x, y)

        def no_grad():
            with torch.no_grad():
                return crit.loss_and_dice(x, y)

        loss, _, (g,) = with_grad()
        ref_loss, ref_g = torch_ce_dice(x, y64)
        torch.cuda.synchronize()
        lines.append(f"# {shape} fp32, int32 labels: loss {loss.item():.6f} (torch ops {ref_loss.item():.6f}), "
                     f"max |grad - torch grad| / max |grad| {((g - ref_g).abs().max() / ref_g.abs().max()).item():.2e}")
        rows = []
        for name, fn, nbytes in (("class_grad", with_grad, bytes_grad), ("class_nograd", no_grad, bytes_nograd)):
            py = each_call_us(fn, 10, calls)
            gr = graph_us(fn)
            rows.append((name, py, gr, nbytes))
        yard = each_call_us(lambda: torch_ce_dice(x, y64), 10, calls)
        for name, py, gr, nbytes in rows:
            floor = nbytes / (YARD_TBS * 1e12) * 1e6
            lines.append(f"{'x'.join(map(str, shape)):16s} {name:13s} python {py[0]:8.2f} us [{py[1]:.2f} .. {py[2]:.2f}] | hipGraph of 20 "
                         f"{gr[0]:8.2f} us [{gr[1]:.2f} .. {gr[2]:.2f}] | {nbytes / 1e6:8.2f} MB = {nbytes / gr[0] / 1e3:7.1f} GB/s; "
                         f"at {YARD_TBS} TB/s {floor:6.2f} us (x {gr[0] / floor:.2f})")
        lines.append(f"{'x'.join(map(str, shape)):16s} {'torch_ops':13s} python {yard[0]:8.2f} us [{yard[1]:.2f} .. {yard[2]:.2f}] "
                     f"(eager F.cross_entropy + softmax Dice + autograd.grad) = {yard[0] / rows[0][1][0]:.1f} x class_grad from Python, "
                     f"{yard[0] / rows[0][2][0]:.1f} x its graphed time")
        del x, y, y64, g, ref_g
        torch.cuda.empty_cache()


def step_rows(iters, lines):
    gen = torch.Generator().manual_seed(1)
    img = torch.randn(16, 3, 256, 256, generator=gen).cuda()
    y = torch.randint(0, STEP_CLASSES, (16, 256, 256), generator=gen).cuda()
    onehot = F.one_hot(y, STEP_CLASSES).permute(0, 3, 1, 2).float().contiguous()
    for name, crit, target in (("bce_dice on one-hot masks", "bce_dice", onehot), ("MulticlassLoss.ce_dice()", MulticlassLoss.ce_dice(), y)):
        torch.manual_seed(0)
        m = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=STEP_CLASSES)
        m.run_dtype = torch.bfloat16
        m = m.cuda().train()
        step = unet_zoo_amd.GraphedStep(m, crit, lr=1e-4, weight_decay=1e-5)
        for _ in range(5):
            step(img, target)
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                step(img, target)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / iters)
        ms.sort()
        lines.append(f"step {name:28s} {ms[1]:.3f} ms [{ms[0]:.3f} .. {ms[2]:.3f}]  loss {step.loss.item():.6f}  dice {step.dice.item():.4f}  "
                     f"{step.describe()}")
        del step, m
        torch.cuda.empty_cache()


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
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/multiclass_loss_bench.py measures on the GPU; none is visible")
    p = torch.cuda.get_device_properties(0)
    lines = _Lines(a.out)
    lines.append(f"# tools/multiclass_loss_bench.py on {p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs), "
             f"{datetime.date.today()}; calls {a.calls}, median [min .. max]; one process")
    kernel_rows(a.calls, lines)
    if not a.skip_step:
        lines.append(f"# unet (num_classes = {STEP_CLASSES}) train step, B = 16, 256 x 256, bf16, GraphedStep, ms per step over {a.iters} steps, three windows")
        step_rows(a.iters, lines)


if __name__ == "__main__":
    main()
