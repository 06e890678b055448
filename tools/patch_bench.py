#!/usr/bin/env python3
"""PatchSampler (uz_patch.hip) measured, in ONE process on one GPU: unet bf16, B = 16, 256 x 256 patches from a pool of
1024 x 1024 pictures (uint8, three channels, a one-channel fp32 mask).

(a) the sampler alone: the per-call time of a hipGraph of 20 back-to-back pool.run() calls (torch.rand + uz_patch_draw +
    uz_patch_cut; median of five windows, no host launch rate in the number) and of uz_patch_cut alone, beside the bytes the
    cut must move (the patches written as fp32, the picture windows read as uint8, the mask windows as fp32);
    uz_patch_index, once per pool, timed by events around one call.
(b) the training step, ms per step over `iters` steps, three windows each, the three forms ALTERNATING window by window:
      source=     GraphedStep(model, source=pool): step()
      ready       the same GraphedStep code fed a ready device batch (one fixed set of patches): step(x, t) -- the difference to
                  `source=` is the feature's cost
      eager       the same sampling rule written with eager torch (torch.nonzero of the picture's mask and indexing per patch,
                  the coordinates read on the host), then step(x, t)

    python tools/patch_bench.py [--iters 30] [--pool 32] [--out profiles/patch_sampler_bench.txt]
"""
import argparse
import datetime
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import unet_zoo_amd  # noqa: E402
from unet_zoo_amd import PatchSampler, ops  # noqa: E402
from unet_zoo_amd.data import IMAGENET_MEAN, IMAGENET_STD  # noqa: E402

B, C, HW, WIN, POS = 16, 3, 1024, 256, 1.0 / 3.0


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


def make_pool(M):
    """uint8 pictures and blob masks (four discs per picture, about 9 % foreground), made on the device from a seed"""
    gen = torch.Generator(device="cuda").manual_seed(0)
    images = torch.randint(0, 256, (M, C, HW, HW), generator=gen, device="cuda", dtype=torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(HW, device="cuda"), torch.arange(HW, device="cuda"), indexing="ij")
    masks = torch.zeros((M, 1, HW, HW), device="cuda")
    for m in range(M):
        for _ in range(4):
            cy, cx, r = (float(v) for v in torch.rand(3, generator=gen, device="cuda"))
            masks[m, 0] += ((yy - cy * HW) ** 2 + (xx - cx * HW) ** 2 < (40 + 90 * r) ** 2).float()
    return images, (masks > 0).float()


class EagerSampler:
    """the rule of uz_patch_draw / uz_patch_cut with eager torch: per patch a picture, with probability pos a foreground pixel
    from torch.nonzero of its mask, a window around it, the crop and the normalisation; the coordinates go through the host"""

    def __init__(self, images, masks):
        self.images, self.masks = images, masks
        mean = torch.tensor(IMAGENET_MEAN, device="cuda").view(1, C, 1, 1)
        std = torch.tensor(IMAGENET_STD, device="cuda").view(1, C, 1, 1)
        self.scale, self.shift = 1.0 / (255.0 * std), -mean / std

    def __call__(self):
        M = self.images.shape[0]
        u = torch.rand((B, 8)).tolist()
        xs, ts = [], []
        for b in range(B):
            m = min(M - 1, int(u[b][0] * M))
            y0, x0 = min(HW - WIN, int(u[b][4] * (HW - WIN + 1))), min(HW - WIN, int(u[b][5] * (HW - WIN + 1)))
            if u[b][1] < POS:
                nz = torch.nonzero(self.masks[m, 0] > 0.5)
                if nz.shape[0]:
                    py, px = nz[min(nz.shape[0] - 1, int(u[b][3] * nz.shape[0]))].tolist()
                    y0 = min(max(py - min(WIN - 1, int(u[b][4] * WIN)), 0), HW - WIN)
                    x0 = min(max(px - min(WIN - 1, int(u[b][5] * WIN)), 0), HW - WIN)
            xs.append(self.images[m, :, y0:y0 + WIN, x0:x0 + WIN])
            ts.append(self.masks[m, :, y0:y0 + WIN, x0:x0 + WIN])
        return torch.stack(xs).float() * self.scale + self.shift, torch.stack(ts)


def sampler_rows(pool, lines):
    d = pool.desc
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ops.patch_index(d, pool.masks, pool.index)
    torch.cuda.synchronize()
    e0.record()
    ops.patch_index(d, pool.masks, pool.index)
    e1.record()
    torch.cuda.synchronize()
    lines.append(f"uz_patch_index  {d.M} x {d.P} planes of {d.H} x {d.W}: {e0.elapsed_time(e1) * 1e3:.1f} us (two launches, once per pool; "
                 f"{pool.masks.numel() * 4 / 1e6:.1f} MB of mask read)")
    px = B * WIN * WIN
    nbytes = px * (4 * C + 4) + px * (C + 4)          # written fp32 picture + mask; read uint8 picture + fp32 mask
    cut = graph_us(lambda: ops.patch_cut(d, pool.images, pool.masks, pool.coords, pool.norm, pool.out_image, pool.out_mask))
    run = graph_us(pool.run)
    lines.append(f"uz_patch_cut    {B} x {C} x {WIN} x {WIN} + 1-channel mask, hipGraph of 20: {cut[0]:7.2f} us [{cut[1]:.2f} .. {cut[2]:.2f}] per "
                 f"call (a kernel boundary included) | {nbytes / 1e6:.2f} MB = {nbytes / cut[0] / 1e6:.2f} TB/s")
    lines.append(f"pool.run()      torch.rand + uz_patch_draw + uz_patch_cut,   hipGraph of 20: {run[0]:7.2f} us [{run[1]:.2f} .. {run[2]:.2f}] per call")


def step_rows(pool, iters, lines):
    def model():
        torch.manual_seed(0)
        m = unet_zoo_amd.create_model("unet", in_channels=C, num_classes=1)
        m.run_dtype = torch.bfloat16
        return m.cuda().train()

    x, t = (v.clone() for v in pool())
    eager = EagerSampler(pool.images, pool.masks)
    s_src = unet_zoo_amd.GraphedStep(model(), lr=1e-4, weight_decay=1e-5, source=pool)
    s_ready = unet_zoo_amd.GraphedStep(model(), lr=1e-4, weight_decay=1e-5)
    s_eager = unet_zoo_amd.GraphedStep(model(), lr=1e-4, weight_decay=1e-5)
    forms = {"source=pool: step()": (s_src, lambda: s_src()),
             "ready device batch: step(x, t)": (s_ready, lambda: s_ready(x, t)),
             "eager torch sampling, then step(x, t)": (s_eager, lambda: s_eager(*eager()))}
    for _, fn in forms.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(3):
        for name, (_, fn) in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / iters)
    for name, (step, _) in forms.items():
        ms = sorted(times[name])
        lines.append(f"step {name:40s} {ms[1]:.3f} ms [{ms[0]:.3f} .. {ms[2]:.3f}]  loss {step.loss.item():.6f}")
    src, ready, eag = (sorted(times[k])[1] for k in forms)
    lines.append(f"# source= costs {1e3 * (src - ready):+.1f} us per step over the ready batch ({100 * (src - ready) / ready:+.2f} %); the eager "
                 f"sampling costs {eag - ready:+.3f} ms per step ({100 * (eag - ready) / ready:+.1f} %)")
    lines.append(f"# {s_src.describe()}")


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
    ap.add_argument("--pool", type=int, default=32, help="pictures in the pool")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/patch_bench.py measures on the GPU; none is visible")
    p = torch.cuda.get_device_properties(0)
    lines = _Lines(a.out)
    lines.append(f"# tools/patch_bench.py on {p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs), "
                 f"{datetime.date.today()}; median [min .. max]; one process")
    images, masks = make_pool(a.pool)
    pool = PatchSampler(images, masks, window=(WIN, WIN), batch=B, pos=POS, jitter=1.0)
    lines.append(f"# pool: {a.pool} pictures {C} x {HW} x {HW} uint8 + 1-channel fp32 mask ({float(masks.mean()) * 100:.1f} % foreground), "
                 f"{(images.numel() + 4 * masks.numel()) / 1e6:.0f} MB on the device; {pool!r}")
    sampler_rows(pool, lines)
    lines.append(f"# unet train step, B = {B}, {WIN} x {WIN}, bf16, GraphedStep, ms per step over {a.iters} steps, three windows each, alternating")
    step_rows(pool, a.iters, lines)


if __name__ == "__main__":
    main()
