#!/usr/bin/env python3
"""SurfaceMetrics (uz_surface.hip) measured, in ONE process on one GPU:

(a) the stand-alone metric call (seven launches) on fp32 logits: binary (16, 1, 256, 256) against float masks and class
    indices (16, 9, 256, 256) against int32 labels, each with compact blobs and with ragged, noise-like masks (the worst
    perimeter: an early-training prediction); the per-call time of a hipGraph of 20 back-to-back calls, median of five
    windows (no host launch rate in the number), and the surface pixels the column pass queried.
(b) GraphedEval replays at B = 16, 3 x 256 x 256, bf16, with and without `surface=`: unet with "bce_dice" and swin_unet_v2
    (num_classes = 8: the models' head kernel takes at most 8 channels) with MulticlassLoss.ce_dice(); `iters` replays per
    window, three windows each, the two objects ALTERNATING window by window; median [min .. max].
(c) the host yardstick: the maps of (a) copied back and scipy's binary_erosion + distance_transform_edt + numpy.percentile
    per pair on this machine's CPU, one process, one thread of Python -- or the statement that scipy is not installed.
(d) with --trace DIR: the kernels' own durations from the csv a run of (a) under
    `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/surface_bench.py --kernel-only` left in DIR (a run of
    its own: tracing slows the host): the per-launch split, median [min .. max] per kernel.

    python tools/surface_bench.py [--iters 30] [--out profiles/surface_metrics_bench.txt] [--kernel-only] [--trace DIR]
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
from unet_zoo_amd import MulticlassLoss, SurfaceMetrics  # noqa: E402

B, HW, K = 16, 256, 9
EVAL_K = 8       # the 1x1 head kernel of the models takes at most 8 output channels; the metric's own K = 9 figures are in (a)


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
    """name -> (logits, target) on the device: compact = discs, moved a little between prediction and target; ragged = the
    same target against logits of pure noise"""
    rng = np.random.RandomState(0)
    gen = torch.Generator().manual_seed(0)
    out = {}
    t1, p1 = discs(rng, B, 1), discs(rng, B, 1)
    out["binary 16x1x256x256 compact"] = (torch.from_numpy(np.where(p1 > 0, 2.0, -2.0)[:, None]).float(), torch.from_numpy(t1[:, None]).float())
    out["binary 16x1x256x256 ragged"] = (torch.randn(B, 1, HW, HW, generator=gen), torch.from_numpy(t1[:, None]).float())
    tk, pk = discs(rng, B, K - 1), discs(rng, B, K - 1)
    onehot = torch.nn.functional.one_hot(torch.from_numpy(pk), K).permute(0, 3, 1, 2).float()
    out["class  16x9x256x256 compact"] = (4.0 * onehot + torch.rand(B, K, HW, HW, generator=gen), torch.from_numpy(tk).int())
    out["class  16x9x256x256 ragged"] = (torch.randn(B, K, HW, HW, generator=gen), torch.from_numpy(tk).int())
    return {k: (x.cuda().contiguous(), t.cuda().contiguous()) for k, (x, t) in out.items()}


def kernel_rows(lines, data):
    for name, (x, t) in data.items():
        m = SurfaceMetrics()
        us = graph_us(lambda: m(x, t))
        torch.cuda.synchronize()
        st = m.stats.cpu()
        valid = int((st[..., 5] == 0).sum())
        lines.append(f"{name:30s} hipGraph of 20: {us[0]:8.2f} us [{us[1]:.2f} .. {us[2]:.2f}] per call (7 launches) | "
                     f"{st.shape[0] * st.shape[1]} pairs, {valid} valid, {int(st[..., :2].sum())} surface pixels queried, "
                     f"mean hd95 of the valid {float(m.hdq[st[..., 5] == 0].mean()):.3f} px")


def eval_rows(iters, lines):
    gen = torch.Generator().manual_seed(1)
    img = torch.randn(B, 3, HW, HW, generator=gen).cuda()
    rng = np.random.RandomState(1)
    for name, kw, crit, target in (
            ("unet bce_dice", dict(num_classes=1), lambda: "bce_dice", torch.from_numpy(discs(rng, B, 1)[:, None]).float().cuda()),
            ("swin_unet_v2 K=8 ce_dice", dict(num_classes=EVAL_K, image_size=HW, window_size=8), MulticlassLoss.ce_dice,
             torch.from_numpy(discs(rng, B, EVAL_K - 1)).int().cuda())):
        model = name.split()[0]
        evs = {}
        for label, surf in (("without surface", None), ("with surface=SurfaceMetrics()", SurfaceMetrics())):
            torch.manual_seed(0)
            m = unet_zoo_amd.create_model(model, in_channels=3, **kw)
            m.run_dtype = torch.bfloat16
            m = m.cuda().eval()
            if model == "unet":      # an untrained head is negative everywhere: move its bias to the logits' median, so that the
                with torch.no_grad():    # prediction is the ragged mask of an early epoch and not an empty one
                    m.out.conv.bias -= m(img).float().median()
            ev = unet_zoo_amd.GraphedEval(m, crit(), surface=surf)
            for _ in range(5):
                ev(img, target)
            evs[label] = (ev, [])
        torch.cuda.synchronize()
        for _ in range(3):
            for ev, ms in evs.values():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    ev(img, target)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / iters)
        for label, (ev, ms) in evs.items():
            ms.sort()
            extra = ""
            if ev.surface is not None:
                st = ev.surface[1]
                extra = f"  {int((st[..., 5] == 0).sum())} of {st.shape[0] * st.shape[1]} pairs valid, {int(st[..., :2].sum())} surface pixels"
            lines.append(f"eval {name:26s} {label:30s} {ms[1]:.3f} ms [{ms[0]:.3f} .. {ms[2]:.3f}] per batch  loss {ev.loss.item():.6f}{extra}")
        del evs
        torch.cuda.empty_cache()


def host_rows(lines, data):
    try:
        from scipy import ndimage as ndi
    except ImportError:
        lines.append("host yardstick: scipy is not installed on this machine; not measured")
        return
    cross = ndi.generate_binary_structure(2, 1)
    for name, (x, t) in data.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        xh, th = x.cpu().numpy(), t.cpu().numpy()
        t1 = time.perf_counter()
        if th.dtype.kind == "f":
            pairs = [(xh[n, c] > 0, th[n, c] > 0.5) for n in range(xh.shape[0]) for c in range(xh.shape[1])]
        else:
            pred = xh.argmax(1)
            pairs = [(pred[n] == c, th[n] == c) for n in range(xh.shape[0]) for c in range(1, xh.shape[1])]
        done = 0
        for A, Bm in pairs:
            if not A.any() or not Bm.any():
                continue
            sa, sb = A & ~ndi.binary_erosion(A, cross), Bm & ~ndi.binary_erosion(Bm, cross)
            d = np.concatenate([ndi.distance_transform_edt(~sb)[sa], ndi.distance_transform_edt(~sa)[sb]])
            np.percentile(d, 95.0), d.max(), d.mean()
            done += 1
        t2 = time.perf_counter()
        lines.append(f"host {name:30s} copy back {1e3 * (t1 - t0):7.2f} ms + scipy erosion / EDT / numpy.percentile {1e3 * (t2 - t1):8.2f} ms "
                     f"for {len(pairs)} pairs ({done} valid), one Python thread")


def trace_rows(trace_dir, lines):
    """the four cases of (a) run one after the other with the same number of calls each: a kernel's launches in time order
    fall into as many equal groups as cases use it (the codes kernel is one instantiation per mode: two cases each)"""
    d = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "surface_" in r["Kernel_Name"]:
                d.setdefault(r["Kernel_Name"], []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    if not d:
        sys.exit(f"no surface kernel in the kernel traces under {trace_dir}")
    names = ["binary compact", "binary ragged", "class compact", "class ragged"]
    for k, v in sorted(d.items()):
        v.sort()
        name = re.search(r"surface_\w+(<[^>]*>)?", k).group(0)
        mine = names[:2] if name.endswith("<0>") else names[2:] if name.endswith("<1>") else names
        if len(v) % len(mine):
            sys.exit(f"{name}: {len(v)} launches do not split into {len(mine)} cases")
        n = len(v) // len(mine)
        cols = []
        for c, case in enumerate(mine):
            us = sorted(t for _, t in v[c * n:(c + 1) * n])
            cols.append(f"{case} {us[n // 2]:8.2f} [{us[0]:.2f} .. {us[-1]:.2f}]")
        lines.append(f"kernel trace  {name:26s} n = {n:4d} per case, us  " + " | ".join(cols))


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
    ap.add_argument("--trace", default=None, help="summarise the surface kernels of a rocprofv3 csv kernel trace and stop")
    a = ap.parse_args()
    if a.trace:
        lines = _Lines(a.out, "a")
        lines.append(f"# tools/surface_bench.py --trace: kernel durations of `rocprofv3 --kernel-trace -- python tools/surface_bench.py "
                     f"--kernel-only`, {datetime.date.today()}")
        trace_rows(a.trace, lines)
        return
    if not torch.cuda.is_available():
        sys.exit("tools/surface_bench.py measures on the GPU; none is visible")
    p = torch.cuda.get_device_properties(0)
    lines = _Lines(a.out)
    lines.append(f"# tools/surface_bench.py on {p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs), "
                 f"{datetime.date.today()}; median [min .. max]; one process")
    data = cases()
    kernel_rows(lines, data)
    if a.kernel_only:
        return
    lines.append(f"# GraphedEval replay, B = 16, 3 x 256 x 256, bf16, ms per batch over {a.iters} replays, three windows each, alternating")
    eval_rows(a.iters, lines)
    lines.append("# host yardstick on this machine's CPU (for orientation)")
    host_rows(lines, data)


if __name__ == "__main__":
    main()
