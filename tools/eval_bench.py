#!/usr/bin/env python3
"""Evaluation pass, ms per batch, three routes -- eager eval, GraphedEval(fold_bn=False), GraphedEval(fold_bn=True) -- for
unet, attention_unet and nested_unet at B = 16, 256 x 256, bf16; and, per Conv -> BN -> ReLU layer shape of unet, the one
launch of uz_conv_igemm_bnact against the two it replaces (uz_conv_igemm + uz_bn_relu_apply), in the same process.

    python tools/eval_bench.py [--batch 16] [--size 256] [--iters 30] [--out FILE]

Every GPU step runs in a child process of its own under `timeout` (a model's three routes; the layer table); the first step
that fails ends the run.  Timing, for the models and the layer table alike: two CUDA events around `iters` back-to-back calls
from Python after `warmup` calls.  The layer rows therefore include the host's launch rate: the two-launch side makes two
wrapper calls per iteration, which can weigh on the 30-50 us rows; the whole-model numbers come from graph replays and do not
have that term.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODELS = ("unet", "attention_unet", "nested_unet")


def _time(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def step_model(name, B, S, warmup, iters):
    import torch
    import unet_zoo_amd
    from unet_zoo_amd.loss import loss_and_dice
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model(name, in_channels=3, num_classes=1)
    m.run_dtype = torch.bfloat16
    m = m.cuda().eval()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 3, S, S, generator=g).cuda()
    t = (torch.rand(B, 1, S, S, generator=g) > 0.5).float().cuda()

    def eager():
        with torch.no_grad():
            loss_and_dice(m(x), t)

    res = {"model": name, "batch": B, "size": S, "dtype": "bf16"}
    res["eager_ms"] = round(_time(eager, warmup, iters), 4)
    for fold in (False, True):
        ev = unet_zoo_amd.GraphedEval(m, "bce_dice", fold_bn=fold)
        res["graphed_fold_ms" if fold else "graphed_ms"] = round(_time(lambda: ev(x, t), warmup, iters), 4)
        if fold:
            res["folded_layers"], res["unfolded_layers"] = ev.folded_layers, ev.unfolded_layers
    return res


def unet_layers(B, S):
    """(H, Cin, Cout, ldy) of unet's Conv -> BN -> ReLU layers without a pool, first layer aside"""
    out, c, h = [], 64, S
    for _ in range(4):                       # encoder: first convolution of each DoubleConv (the second one is pooled)
        if c > 64:
            out.append((h, c // 2, c, c))
        c, h = 2 * c, h // 2
    out += [(h, c // 2, c, c), (h, c, c, c)]  # bottleneck
    for _ in range(4):                       # decoder: cat(skip, up) -> c/2 -> c/2
        h, c = 2 * h, c // 2
        out += [(h, 2 * c, c, c), (h, c, c, c)]
    return out


def step_layers(B, S, warmup, iters):
    import torch
    from ctypes import byref
    from unet_zoo_amd import _lib as L, ops
    dt = torch.bfloat16
    lib = L.load()
    rows = []
    for (H, Cin, Cout, ldy) in unet_layers(B, S):
        x = ops.new_act(B, H, H, Cin, dt, "cuda")
        x.buf.normal_()
        wp = (torch.randn(Cout, 9 * Cin, device="cuda") * 0.05).to(dt)
        bias, sc, sh = torch.randn(Cout, device="cuda"), torch.rand(Cout, device="cuda") + 0.5, torch.randn(Cout, device="cuda")
        raw, act = ops.new_act(B, H, H, Cout, dt, "cuda"), ops.new_act(B, H, H, Cout, dt, "cuda")
        d = L.ConvDesc(L.dtype_code(dt), B, H, H, H, H, Cin, x.ld, Cout, act.ld, 9, L.TAPS_CONV, 1, L.STORE_PLAIN, 0, 0, 0)
        row = {"H": H, "Cin": Cin, "Cout": Cout, "kernel": ops.conv_kernel_name(d, True),
               "supported": int(lib.uz_conv_igemm_bnact_supported(byref(d)))}

        def two():
            ops.conv_igemm(x, wp, bias, raw, ntaps=9)
            ops.bn_relu_apply(raw, sc, sh, act, reverse=True)

        def one():
            ops.conv_igemm_bnact(x, wp, bias, sc, sh, True, act, ntaps=9)

        row["two_launch_us"] = round(1e3 * _time(two, warmup, iters), 2)
        if row["supported"]:
            row["folded_us"] = round(1e3 * _time(one, warmup, iters), 2)
        rows.append(row)
    return {"layers": rows, "batch": B, "size": S, "dtype": "bf16"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)     # child: one model's routes, or "layers"
    a = ap.parse_args()
    if a.step is not None:
        r = step_layers(a.batch, a.size, a.warmup, a.iters) if a.step == "layers" else step_model(a.step, a.batch, a.size, a.warmup, a.iters)
        print("EVAL_BENCH " + json.dumps(r), flush=True)
        return 0
    lines = []
    for step in MODELS + ("layers",):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--batch",
               str(a.batch), "--size", str(a.size), "--iters", str(a.iters), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        got = [l for l in p.stdout.split("\n") if l.startswith("EVAL_BENCH ")]
        if p.returncode != 0 or not got:
            print(f"step {step} failed (exit {p.returncode}); nothing more is started on the GPU\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            return 1
        r = json.loads(got[0][len("EVAL_BENCH "):])
        if step == "layers":
            lines.append(f"# unet layer shapes, B = {a.batch}, {a.size} x {a.size}, bf16: uz_conv_igemm + uz_bn_relu_apply vs uz_conv_igemm_bnact (us)")
            for row in r["layers"]:
                f = f"{row['folded_us']:9.2f}" if "folded_us" in row else "      n/a"
                lines.append(f"{row['H']:4d}^2 {row['Cin']:5d} -> {row['Cout']:5d}  {row['kernel']:34s} two launches {row['two_launch_us']:9.2f}  "
                             f"folded {f}  supported {row['supported']}")
        else:
            lines.append(f"{r['model']:16s} B={r['batch']} {r['size']}^2 bf16  eager {r['eager_ms']:8.3f} ms  graphed {r['graphed_ms']:8.3f} ms  "
                         f"graphed+fold {r['graphed_fold_ms']:8.3f} ms  (folded {r['folded_layers']}, two-launch {r['unfolded_layers']} layers)")
        print(lines[-1] if step != "layers" else "\n".join(lines[-len(r["layers"]) - 1:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
