#!/usr/bin/env python3
"""RegionLoss (uz_region_loss) measured: (a) the call itself against uz_bce_dice, on one map of (16, 1, 256, 256) and on
seven maps of (8, 1, 512, 512); (b) the unet training step at B = 16, 256 x 256, bf16 from GraphedStep with "bce_dice", with
RegionLoss(), and with the same BCE + soft Dice written as a torch callable -- the eager route RegionLoss replaces.

    python tools/region_loss_bench.py [--iters 50] [--out profiles/region_loss_bench.txt]

Every measurement runs in a child process of its own under `timeout`; the first one that fails ends the run.
(a) times a hipGraph of `reps` back-to-back calls between two events (no host launch rate in the number) and, beside it,
the same calls issued from Python (what an eager training loop sees).  uz_bce_dice handles one map per call: the seven-map
row is seven calls, the route loss_and_dice takes.  Bytes are what the algorithm must move: 5 * 4 * n per map with a
gradient (x and t read twice, dlogits written), 2 * 4 * n without; for uz_bce_dice 3 * 4 * n / 2 * 4 * n.
(b) times `iters` whole steps (graph replays; the callable row also runs its criterion eagerly between them), three windows,
median [min .. max].  The callable row is the baseline; the "bce_dice" row shows what the region term costs.
"""
import argparse
import datetime
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNEL_CASES = {"one_map": (1, (16, 1, 256, 256)), "seven_maps": (7, (8, 1, 512, 512))}
STEP_CASES = ("bce_dice", "region", "callable")


def _device():
    import torch
    p = torch.cuda.get_device_properties(0)
    return f"{p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs)"


def _window(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _stats(fn, warmup, iters, windows=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = sorted(_window(fn, iters) for _ in range(windows))
    return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}


def step_kernel(case, warmup, iters, reps=20):
    import torch
    from unet_zoo_amd import RegionLoss
    from unet_zoo_amd.loss import loss_and_dice, loss_and_dice_direct
    n_maps, shape = KERNEL_CASES[case]
    g = torch.Generator().manual_seed(0)
    maps = [(3.0 * torch.randn(shape, generator=g)).cuda() for _ in range(n_maps)]
    t = (torch.rand(shape, generator=g) > 0.7).float().cuda()
    outs = maps[0] if n_maps == 1 else maps
    crit = RegionLoss()
    n = maps[0].numel()
    routes = {
        "region_grad": (lambda: crit.direct(outs, t), 5 * 4 * n * n_maps),
        "region_nograd": (lambda: crit.loss_and_dice(outs, t), 2 * 4 * n * n_maps),
        "bce_dice_grad": (lambda: loss_and_dice_direct(outs, t), 3 * 4 * n * n_maps),
        "bce_dice_nograd": (lambda: loss_and_dice(outs, t), 2 * 4 * n * n_maps),
    }
    res = {"case": case, "maps": n_maps, "shape": list(shape), "device": _device(), "routes": {}}
    with torch.no_grad():
        for name, (fn, nbytes) in routes.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(reps):
                    keep = fn()      # (the results stay alive until the capture ends)
            st = _stats(graph.replay, warmup, iters)
            eager = _stats(fn, warmup, iters)
            us = 1e3 * st["median"] / reps
            res["routes"][name] = {"graph_us": round(us, 2), "graph_us_min": round(1e3 * st["min"] / reps, 2),
                                   "graph_us_max": round(1e3 * st["max"] / reps, 2), "python_us": round(1e3 * eager["median"], 2),
                                   "bytes": nbytes, "gbps": round(nbytes / (us * 1e-6) / 1e9, 1)}
            del graph, keep
    return res


def torch_bce_dice(out, t):
    """RegionLoss()'s formula with torch ops: BCEWithLogits + mean over images of 1 - (I + 1) / (I + (S - I) / 2 + (T - I) / 2 + 1)"""
    import torch
    import torch.nn.functional as F
    p = torch.sigmoid(out)
    pf, tf = p.flatten(1), t.flatten(1)
    inter, sp, st = (pf * tf).sum(1), pf.sum(1), tf.sum(1)
    ti = (inter + 1.0) / (inter + 0.5 * (sp - inter) + 0.5 * (st - inter) + 1.0)
    return F.binary_cross_entropy_with_logits(out, t) + (1.0 - ti).mean()


def step_train(case, B, S, warmup, iters):
    import torch
    import unet_zoo_amd
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=1)
    m.run_dtype = torch.bfloat16
    m = m.cuda().train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 3, S, S, generator=g).cuda()
    t = (torch.rand(B, 1, S, S, generator=g) > 0.7).float().cuda()
    crit = {"bce_dice": "bce_dice", "region": unet_zoo_amd.RegionLoss(), "callable": torch_bce_dice}[case]
    gs = unet_zoo_amd.GraphedStep(m, crit, lr=1e-4)
    st = _stats(lambda: gs(x, t), warmup, iters)
    return {"case": case, "batch": B, "size": S, "dtype": "bf16", "device": _device(),
            "loss": round(float(gs.loss.item()), 6), "launch": gs.describe(),
            "ms": round(st["median"], 4), "ms_min": round(st["min"], 4), "ms_max": round(st["max"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-timeout", type=int, default=180)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)     # child: "kernel:<case>" or "train:<case>"
    a = ap.parse_args()
    if a.step is not None:
        kind, case = a.step.split(":")
        r = step_kernel(case, a.warmup, a.iters) if kind == "kernel" else step_train(case, a.batch, a.size, a.warmup, a.iters)
        print("REGION_BENCH " + json.dumps(r), flush=True)
        return 0
    lines = []
    for step in [f"kernel:{c}" for c in KERNEL_CASES] + [f"train:{c}" for c in STEP_CASES]:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--batch",
               str(a.batch), "--size", str(a.size), "--iters", str(a.iters), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        got = [l for l in p.stdout.split("\n") if l.startswith("REGION_BENCH ")]
        if p.returncode != 0 or not got:
            print(f"step {step} failed (exit {p.returncode}); nothing more is started on the GPU\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            return 1
        r = json.loads(got[0][len("REGION_BENCH "):])
        if not lines:
            lines.append(f"# tools/region_loss_bench.py on {r['device']}, {datetime.date.today().isoformat()}; "
                         f"iters {a.iters}, warmup {a.warmup}, three windows: median [min .. max]")
        new = []
        if step.startswith("kernel:"):
            new.append(f"# {r['maps']} map(s) of {tuple(r['shape'])} fp32: us per call over all maps (hipGraph of 20 calls | issued from Python), "
                       f"GB/s = algorithm bytes / graph time")
            for name, v in r["routes"].items():
                new.append(f"{r['case']:11s} {name:16s} {v['graph_us']:9.2f} us [{v['graph_us_min']:.2f} .. {v['graph_us_max']:.2f}] | "
                           f"python {v['python_us']:9.2f} us   {v['bytes'] / 1e6:8.2f} MB  {v['gbps']:8.1f} GB/s")
        else:
            if step == f"train:{STEP_CASES[0]}":
                new.append(f"# unet train step, B = {r['batch']}, {r['size']} x {r['size']}, bf16, GraphedStep, ms per step")
            new.append(f"step {r['case']:9s} {r['ms']:8.3f} ms [{r['ms_min']:.3f} .. {r['ms_max']:.3f}]  loss {r['loss']:.6f}  {r['launch']}")
        lines += new
        print("\n".join(new), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
