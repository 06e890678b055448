#!/usr/bin/env python3
"""ConfusionMetrics (uz_confusion.hip) measured, in ONE process on one GPU:

(a) the stand-alone metric call (three launches) on fp32 logits (16, 1, 256, 256) against float masks with B = 256 bins, once
    with the logits of a trained model (nearly every pixel in an end bin) and once with noise (every bin of a wave distinct: the
    worst case of the one-add-per-distinct-bin loop), and on (16, 4, 256, 256) against int32 labels: the per-call time of a
    hipGraph of 20 back-to-back calls, median of five windows (no host launch rate in the number).
(b) GraphedEval per batch at B = 16, 3 x 256 x 256, unet, bf16, in three forms, `iters` calls per window, five windows each:
      none      confusion=None -- measured TWICE, before and after the other forms: that pair is the noise band
      in-graph  confusion=ConfusionMetrics(bins=256)
      eager     confusion=None, then the same counts formed with torch after the replay (bucketize / argmax + bincount)
    with "bce_dice" against float masks (binary mode), and with num_classes = 4 and MulticlassLoss.ce_dice() against int32 labels
    (class mode).  The eager counts are compared with the in-graph ones before anything is timed.
The last lines say whether the in-graph form beats the eager one, and by how much against the noise band.

    python tools/confusion_bench.py [--iters 30] [--out profiles/confusion_metrics_bench.txt] [--kernel-only]
"""
import argparse
import datetime
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import unet_zoo_amd  # noqa: E402
from unet_zoo_amd import ConfusionMetrics, MulticlassLoss  # noqa: E402

B, HW, K, BINS = 16, 256, 4, 256
WINDOWS = 5


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


def kernel_rows(lines):
    rng = np.random.RandomState(0)
    gen = torch.Generator().manual_seed(0)
    t1, p1 = discs(rng, B, 1), discs(rng, B, 1)
    tk, pk = discs(rng, B, K - 1), discs(rng, B, K - 1)
    onehot = torch.nn.functional.one_hot(torch.from_numpy(pk), K).permute(0, 3, 1, 2).float()
    data = {
        "binary 16x1x256x256 trained": (torch.from_numpy(np.where(p1 > 0, 9.0, -9.0)[:, None]).float(), torch.from_numpy(t1[:, None]).float()),
        "binary 16x1x256x256 noise": (2.0 * torch.randn(B, 1, HW, HW, generator=gen), torch.from_numpy(t1[:, None]).float()),
        "class  16x4x256x256 trained": (4.0 * onehot + torch.rand(B, K, HW, HW, generator=gen), torch.from_numpy(tk).int()),
        "class  16x4x256x256 noise": (torch.randn(B, K, HW, HW, generator=gen), torch.from_numpy(tk).int())}
    for name, (x, t) in data.items():
        x, t = x.cuda().contiguous(), t.cuda().contiguous()
        m = ConfusionMetrics(bins=BINS)
        us = graph_us(lambda: m(x, t))
        torch.cuda.synchronize()
        nbytes = 4 * (x.numel() + t.numel())
        occupied = f", {int((m.hist.sum((0, 1, 2)) > 0).sum())} of {BINS} bins occupied" if m.hist is not None else ""
        lines.append(f"{name:30s} hipGraph of 20: {us[0]:8.2f} us [{us[1]:.2f} .. {us[2]:.2f}] per call (3 launches), "
                     f"{nbytes / 1e6:.1f} MB read: {nbytes / us[0] / 1e3:.0f} GB/s{occupied}")


def eager_binary(ev, target, edges):
    """counts (N, C, 4) and hist (N, C, 2, B) of the static logits with torch, as a user without ConfusionMetrics forms them"""
    x = ev.outputs.float()
    N, C = x.shape[:2]
    nb = edges.numel() + 1
    plane = torch.arange(N * C, device=x.device).view(N, C, 1, 1)
    pred, targ = x > 0, target > 0.5
    code = 2 * (~pred).long() + (~targ).long()                    # TP, FP, FN, TN
    counts = torch.bincount((plane * 4 + code).flatten(), minlength=N * C * 4).view(N, C, 4)
    bins = torch.bucketize(x, edges, right=True)
    hist = torch.bincount((plane * 2 * nb + targ.long() * nb + bins).flatten(), minlength=N * C * 2 * nb).view(N, C, 2, nb)
    return counts, hist


def eager_class(ev, target):
    """the (N, K, K) matrices of the static logits with torch"""
    x = ev.outputs.float()
    N, Kc = x.shape[:2]
    pred = x.argmax(1)
    y = target.long()
    valid = (y >= 0) & (y < Kc)
    img = torch.arange(N, device=x.device).view(N, 1, 1).expand_as(y)
    idx = (img * Kc + y) * Kc + pred
    return torch.bincount(idx[valid], minlength=N * Kc * Kc).view(N, Kc, Kc)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def eval_rows(iters, lines):
    gen = torch.Generator().manual_seed(1)
    img = torch.randn(B, 3, HW, HW, generator=gen).cuda()
    rng = np.random.RandomState(1)
    verdicts = []
    for name, classes, crit, target in (
            ("unet bce_dice, binary mode", 1, lambda: "bce_dice", torch.from_numpy(discs(rng, B, 1)[:, None]).float().cuda()),
            (f"unet K={K} ce_dice, class mode", K, MulticlassLoss.ce_dice, torch.from_numpy(discs(rng, B, K - 1)).int().cuda())):
        torch.manual_seed(0)
        m = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=classes)
        m.run_dtype = torch.bfloat16
        m = m.cuda().eval()
        if classes == 1:      # an untrained head is negative everywhere: move its bias to the logits' median, so that the
            with torch.no_grad():    # histogram is the spread one of an early epoch and not one bin
                m.out.conv.bias -= m(img).float().median()
        plain = unet_zoo_amd.GraphedEval(m, crit())
        cm = ConfusionMetrics(bins=BINS)
        graphed = unet_zoo_amd.GraphedEval(m, crit(), confusion=cm)
        edges = cm.edges.cuda()

        def none():
            plain(img, target)

        def in_graph():
            graphed(img, target)

        def eager():
            plain(img, target)
            return eager_binary(plain, target, edges) if classes == 1 else eager_class(plain, target)

        for _ in range(5):
            none(), in_graph(), eager()
        torch.cuda.synchronize()
        got = eager()
        if classes == 1:
            same = torch.equal(got[0], graphed.confusion[0]) and torch.equal(got[1], graphed.confusion[1])
        else:
            same = torch.equal(got, graphed.confusion[0])
        if not same:
            sys.exit(f"{name}: the eager counts differ from the in-graph ones")
        forms = (("none (first)", none), ("in-graph confusion=", in_graph), ("eager torch counts", eager), ("none (last)", none))
        ms = {}
        for label, fn in forms:
            ms[label] = sorted(window(fn, iters) for _ in range(WINDOWS))
            v = ms[label]
            lines.append(f"eval {name:32s} {label:22s} {statistics.median(v):.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}] per batch")
        med = {k: statistics.median(v) for k, v in ms.items()}
        base = 0.5 * (med["none (first)"] + med["none (last)"])
        both = ms["none (first)"] + ms["none (last)"]
        band = max(both) - min(both)
        add_g, add_e = med["in-graph confusion="] - base, med["eager torch counts"] - base
        verdicts.append(f"{name}: in-graph adds {1e3 * add_g:+.1f} us per batch, eager adds {1e3 * add_e:+.1f} us, noise band of the two "
                        f"`none` runs {1e3 * band:.1f} us (all ten windows); in-graph is {1e3 * (add_e - add_g):.1f} us per batch "
                        f"{'faster' if add_e > add_g else 'slower'} than eager, "
                        f"{'above' if abs(add_e - add_g) > band else 'INSIDE'} the noise band; counts equal in both forms")
        del plain, graphed
        torch.cuda.empty_cache()
    lines.append("# verdict")
    for v in verdicts:
        lines.append(v)


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
        sys.exit("tools/confusion_bench.py measures on the GPU; none is visible")
    p = torch.cuda.get_device_properties(0)
    lines = _Lines(a.out)
    lines.append(f"# tools/confusion_bench.py on {p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs), "
                 f"{datetime.date.today()}; median [min .. max]; one process")
    kernel_rows(lines)
    if a.kernel_only:
        return
    lines.append(f"# GraphedEval per batch, B = 16, 3 x 256 x 256, unet, bf16, ms per batch over {a.iters} calls, {WINDOWS} windows per form, in the "
                 f"order shown")
    eval_rows(a.iters, lines)


if __name__ == "__main__":
    main()
