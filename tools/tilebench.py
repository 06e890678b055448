#!/usr/bin/env python3
"""SlidingWindowPredict (uz_tile.hip) measured, in ONE process on one GPU.  Workload: unet bf16, input (2, 3, 1024, 1024), window
256, overlap 0.5, tile_batch 16, Gaussian weights: 2 x 49 tiles, 7 forwards (6 of 16 tiles, 1 of 2).

(a) the replay of SlidingWindowPredict's hipGraph;
(b) the same tiling on the host side of torch: Python slicing (and F.pad where the image is smaller than the window), the
    model's eager forward per tile batch, sigmoid, `+=` of w p and w into two accumulators per tile, one division, `> 0.5`;
    the same model, the same kernels inside the forward -- what differs is the work around the forwards and the launch path;
(c) the share of (a) spent in uz_tile_gather + uz_tile_blend: the kernels' own durations from the per-op timers of
    ops._Timed over one eager pass of the captured pipeline, against the replay time of (a).

`iters` calls per window, `repeats` windows each, (a) and (b) ALTERNATING window by window; median [min .. max] per call.

    python tools/tilebench.py [--iters 20] [--repeats 5] [--out profiles/tiled_1024_unet_bench.txt]
"""
import argparse
import datetime
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import unet_zoo_amd  # noqa: E402
from unet_zoo_amd import SlidingWindowPredict, ops  # noqa: E402

SHAPE, WINDOW, OVERLAP, TILE_BATCH = (2, 3, 1024, 1024), (256, 256), 0.5, 16


def host_tiling(model, x, ys, xs, w2d):
    """sliding-window inference as a torch user writes it around the model's eager forward"""
    th, tw = WINDOW
    N, _, H, W = x.shape
    ph, pw = max(th - H, 0), max(tw - W, 0)
    cv = F.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2)) if ph or pw else x
    where = [(n, y, x0) for n in range(N) for y in ys for x0 in xs]
    num = den = None
    with torch.no_grad():
        for t0 in range(0, len(where), TILE_BATCH):
            part = where[t0:t0 + TILE_BATCH]
            batch = torch.stack([cv[n, :, y:y + th, x0:x0 + tw] for n, y, x0 in part])
            p = torch.sigmoid(model(batch).float())
            if num is None:
                num = torch.zeros((N, p.shape[1]) + tuple(cv.shape[2:]), device=x.device)
                den = torch.zeros((N, 1) + tuple(cv.shape[2:]), device=x.device)
            for k, (n, y, x0) in enumerate(part):
                num[n, :, y:y + th, x0:x0 + tw] += w2d * p[k]
                den[n, :, y:y + th, x0:x0 + tw] += w2d
    prob = (num / den)[:, :, ph // 2:ph // 2 + H, pw // 2:pw // 2 + W]
    return prob, prob > 0.5


def window_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    torch.manual_seed(0)
    model = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=1)
    model.run_dtype = torch.bfloat16
    model = model.cuda().eval()
    x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(1)).cuda()
    pred = SlidingWindowPredict(model, window=WINDOW, overlap=OVERLAP, tile_batch=TILE_BATCH)
    pred(x)
    torch.cuda.synchronize()
    plan = pred.plan
    gh, gw = ops.tile_weights(WINDOW[0]).cuda(), ops.tile_weights(WINDOW[1]).cuda()
    w2d = torch.clamp(gh[:, None] * gw[None, :], min=1e-3)

    def replay():
        pred(x)

    def host():
        host_tiling(model, x, plan["ys"], plan["xs"], w2d)

    prob_h, mask_h = host_tiling(model, x, plan["ys"], plan["xs"], w2d)
    torch.cuda.synchronize()
    diff = float((prob_h - pred.prob).abs().max())
    differ = int((mask_h != pred.mask.bool()).sum())
    for fn in (replay, host):                                   # warm-up
        window_ms(fn, 3)
    ms = {"replay": [], "host": []}
    for _ in range(args.repeats):
        ms["replay"].append(window_ms(replay, args.iters))
        ms["host"].append(window_ms(host, args.iters))

    # (c) the kernels' own time over one eager pass of the captured pipeline
    g = pred._graphs[tuple(x.shape)]
    shares = []
    for _ in range(3):
        ops.profile_begin()
        pred._pipeline(g)
        prof = ops.profile_end()
        shares.append({k: (v["ms"], v["launches"]) for k, v in prof.items() if k in ("tile_gather", "tile_blend", "tta_merge", "mask_decide")})

    def row(v):
        return f"{statistics.median(v):8.3f} ms [{min(v):.3f} .. {max(v):.3f}]"

    med = statistics.median(ms["replay"])
    lines = [f"# tools/tilebench.py  {datetime.datetime.now().isoformat(timespec='seconds')}  {torch.cuda.get_device_name(0)}",
             f"# unet bf16, input {SHAPE}, window {WINDOW}, overlap {OVERLAP}, tile_batch {TILE_BATCH}, gaussian weights, no TTA: "
             f"{plan['tiles']} tiles, {plan['forwards']} forwards; {args.iters} calls per window, {args.repeats} windows, alternating",
             f"SlidingWindowPredict replay          {row(ms['replay'])} per call",
             f"host-side tiling around eager fwd    {row(ms['host'])} per call   ({statistics.median(ms['host']) / med:.2f} x the replay)",
             f"host-side prob against the replay's: largest difference {diff:.3e}, {differ} of {mask_h.numel()} mask pixels differ"]
    for name in ("tile_gather", "tile_blend", "tta_merge", "mask_decide"):
        v = [s[name][0] for s in shares if name in s]
        if v:
            lines.append(f"kernel time per call, {name:12s} {statistics.median(v) * 1e3:9.1f} us [{min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f}] "
                         f"in {shares[0][name][1]} launches")
    tile = statistics.median([s["tile_gather"][0] + s["tile_blend"][0] for s in shares])
    lines.append(f"uz_tile_gather + uz_tile_blend: {tile * 1e3:.1f} us = {100.0 * tile / med:.2f} % of the replay")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
