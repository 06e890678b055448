#!/usr/bin/env python3
"""MaskPostprocess / GraphedPredict (uz_postproc.hip, uz_tta.hip) measured, in ONE process on one GPU:

(a) the stand-alone post-process call on fp32 logits: binary (16, 1, 256, 256) and class (16, 9, 256, 256), each with compact
    discs and with a ragged, noise-like map (an early-epoch prediction) -- the inputs of tools/surface_bench.py -- with and
    without fill_holes; the per-call time of a hipGraph of 20 back-to-back calls, median of five windows.
(b) GraphedPredict replays on unet at B = 16, 3 x 256 x 256, bf16: 1, 2 and 4 views, each with and without the post-process;
    `iters` replays per window, three windows each, the objects ALTERNATING window by window; median [min .. max].
(c) the host path it replaces, on the maps of (a): copy back, then ndimage.label + numpy.bincount (+ binary_fill_holes) per
    plane on this machine's CPU, one Python thread -- or the statement that scipy is not installed.
(d) with --trace DIR: the kernels' own durations from the csv a run of (a) under
    `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/postproc_bench.py --kernel-only` left in DIR.

    python tools/postproc_bench.py [--iters 30] [--out profiles/postproc_bench.txt] [--kernel-only] [--trace DIR]
"""
import argparse
import csv
import datetime
import glob
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import unet_zoo_amd  # noqa: E402
from surface_bench import B, HW, K, _Lines, discs, graph_us  # noqa: E402  (the same inputs and the same timing loop)
from unet_zoo_amd import GraphedPredict, MaskPostprocess  # noqa: E402

SETTINGS = dict(min_area=16, keep_largest=1)


def cases():
    """name -> fp32 logits on the device: compact = discs; ragged = pure noise"""
    rng = np.random.RandomState(0)
    gen = torch.Generator().manual_seed(0)
    out = {}
    p1 = discs(rng, B, 1)
    out["binary 16x1x256x256 compact"] = torch.from_numpy(np.where(p1 > 0, 2.0, -2.0)[:, None]).float()
    out["binary 16x1x256x256 ragged"] = torch.randn(B, 1, HW, HW, generator=gen)
    pk = discs(rng, B, K - 1)
    onehot = torch.nn.functional.one_hot(torch.from_numpy(pk), K).permute(0, 3, 1, 2).float()
    out["class  16x9x256x256 compact"] = 4.0 * onehot + torch.rand(B, K, HW, HW, generator=gen)
    out["class  16x9x256x256 ragged"] = torch.randn(B, K, HW, HW, generator=gen)
    return {k: x.cuda().contiguous() for k, x in out.items()}


def kernel_rows(lines, data):
    for name, x in data.items():
        for fill in (False, True):
            pp = MaskPostprocess(fill_holes=fill, **SETTINGS)
            us = graph_us(lambda: pp(x))
            torch.cuda.synchronize()
            pp.check()
            st = pp.stats.cpu()
            launches = 18 + (4 if fill else 0) + (1 if x.shape[1] > 1 else 0)
            lines.append(f"{name:30s} fill_holes={int(fill)} hipGraph of 20: {us[0]:8.2f} us [{us[1]:.2f} .. {us[2]:.2f}] per call "
                         f"({launches} launches) | {st.shape[0] * st.shape[1]} planes, {int(st[..., 0].sum())} components found, "
                         f"{int(st[..., 1].sum())} kept, {int(st[..., 4].sum())} pixels filled")


def predict_rows(iters, lines):
    gen = torch.Generator().manual_seed(1)
    img = torch.randn(B, 3, HW, HW, generator=gen).cuda()
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=1)
    m.run_dtype = torch.bfloat16
    m = m.cuda().eval()
    with torch.no_grad():      # an untrained head is negative everywhere: move its bias to the logits' median, so that the
        m.out.conv.bias -= m(img).float().median()     # prediction is the ragged mask of an early epoch and not an empty one
    objs = {}
    for tta in ((), ("hflip",), ("hflip", "vflip", "hvflip")):
        for label, pp in (("postprocess=None", None), ("MaskPostprocess(fill_holes, min_area=16, keep_largest=1)",
                                                      MaskPostprocess(fill_holes=True, **SETTINGS))):
            pred = GraphedPredict(m, tta=tta, postprocess=pp)
            for _ in range(3):
                pred(img)
            objs[(1 + len(tta), label)] = (pred, [])
    torch.cuda.synchronize()
    for _ in range(3):
        for pred, ms in objs.values():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                pred(img)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / iters)
    for (views, label), (pred, ms) in objs.items():
        ms.sort()
        pred.check()
        extra = f"  mask pixels {int(pred.mask.sum())}"
        if pred.stats is not None:
            extra += f", {int(pred.stats[..., 0].sum())} components found, {int(pred.stats[..., 1].sum())} kept"
        lines.append(f"predict unet {views} view(s) {label:58s} {ms[1]:.3f} ms [{ms[0]:.3f} .. {ms[2]:.3f}] per batch{extra}")


def host_rows(lines, data):
    try:
        from scipy import ndimage as ndi
    except ImportError:
        lines.append("host yardstick: scipy is not installed on this machine; not measured")
        return
    for name, x in data.items():
        for fill in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            xh = x.cpu().numpy()
            t1 = time.perf_counter()
            if xh.shape[1] == 1:
                planes = [xh[n, 0] > 0 for n in range(xh.shape[0])]
            else:
                am = xh.argmax(1)
                planes = [am[n] == c for n in range(xh.shape[0]) for c in range(1, xh.shape[1])]
            for p in planes:
                if fill:
                    p = ndi.binary_fill_holes(p)
                lab, n = ndi.label(p)
                area = np.bincount(lab.ravel(), minlength=n + 1)[1:]
                if n:
                    best = int(np.argmax(area))
                    keep = (lab == best + 1) & (area[best] >= SETTINGS["min_area"])
                    ndi.label(keep)
            t2 = time.perf_counter()
            lines.append(f"host {name:30s} fill_holes={int(fill)} copy back {1e3 * (t1 - t0):7.2f} ms + scipy label / bincount"
                         f"{' / binary_fill_holes' if fill else ''} {1e3 * (t2 - t1):8.2f} ms for {len(planes)} planes, one Python thread")


def trace_rows(trace_dir, lines):
    """the eight cases of (a) run one after the other with the same number of calls each: per kernel, median [min .. max] of all
    its launches and their share of the summed kernel time"""
    d = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "postproc_" in r["Kernel_Name"]:
                name = re.search(r"postproc_\w+(<[^>]*>)?", r["Kernel_Name"]).group(0)
                d.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    if not d:
        sys.exit(f"no postproc kernel in the kernel traces under {trace_dir}")
    total = sum(sum(v) for v in d.values())
    for name, v in sorted(d.items(), key=lambda kv: -sum(kv[1])):
        v.sort()
        lines.append(f"kernel trace  {name:34s} n = {len(v):5d}, us  {v[len(v) // 2]:8.2f} [{v[0]:.2f} .. {v[-1]:.2f}]  "
                     f"{100.0 * sum(v) / total:5.1f} % of the kernel time")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--trace", default=None, help="summarise the postproc kernels of a rocprofv3 csv kernel trace and stop")
    a = ap.parse_args()
    if a.trace:
        lines = _Lines(a.out, "a")
        lines.append(f"# tools/postproc_bench.py --trace: kernel durations of `rocprofv3 --kernel-trace -- python tools/postproc_bench.py "
                     f"--kernel-only`, all eight cases of (a) together, {datetime.date.today()}")
        trace_rows(a.trace, lines)
        return
    if not torch.cuda.is_available():
        sys.exit("tools/postproc_bench.py measures on the GPU; none is visible")
    p = torch.cuda.get_device_properties(0)
    lines = _Lines(a.out)
    lines.append(f"# tools/postproc_bench.py on {p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs), "
                 f"{datetime.date.today()}; median [min .. max]; one process; settings {SETTINGS}")
    data = cases()
    kernel_rows(lines, data)
    if a.kernel_only:
        return
    lines.append(f"# GraphedPredict replay, unet, B = 16, 3 x 256 x 256, bf16, ms per batch over {a.iters} replays, three windows each, alternating")
    predict_rows(a.iters, lines)
    lines.append("# the host path it replaces, on this machine's CPU (for orientation)")
    host_rows(lines, data)


if __name__ == "__main__":
    main()
