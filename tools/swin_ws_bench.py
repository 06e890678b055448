"""swin_unet_v2 at B=16 256x256 in bf16 with window_size 16 beside window_size 8 on one device: train-step time (eager
forward + backward, median of --steps after --warmup), the winattn_* kernel times of one profiled step (ops.profile_begin /
profile_end: kernel begin to kernel end), and the wide window-attention core alone against the same core evaluated with
torch ops in bf16 (the roll -> partition -> cosine attention -> reverse restatement of the kernel tests) on the stage-0
shape B=16, 64x64 tokens, 3 heads, window 16, shift 8.

    python tools/swin_ws_bench.py [--steps 20] [--warmup 5] [--out profiles/swin_ws16_256_b16_bench.txt]

bench.py measures the flagship configuration (window 8) and takes no window size; this script leaves it alone."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import unet_zoo_amd  # noqa: E402
from oracle import torch_ref  # noqa: E402
from unet_zoo_amd import ops  # noqa: E402
from unet_zoo_amd.ops import Act  # noqa: E402

DEV = "cuda"


def _events(fn, n, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def model_step(ws, steps, warmup, lines):
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model("swin_unet_v2", image_size=256, in_channels=3, num_classes=1, window_size=ws)
    m.run_dtype = torch.bfloat16
    m = m.to(DEV).train()
    x, mask = torch_ref.synthetic_batch(16, 3, 256, 256, seed=1)
    x, mask = x.to(DEV), mask.to(DEV)

    def step():
        for p in m.parameters():
            p.grad = None
        F.binary_cross_entropy_with_logits(m(x), mask).backward()

    ms = _events(step, steps, warmup)
    ops.profile_begin()
    step()
    prof = ops.profile_end()
    lines.append(f"window {ws:2d}: train step (eager forward + backward, B=16 256x256 bf16) {ms:8.3f} ms, median of {steps}")
    for fam in ("winattn_fwd", "winattn_bwd"):
        if fam in prof:
            p = prof[fam]
            lines.append(f"window {ws:2d}:   {fam}: {p['ms']:8.3f} ms in {p['launches']} launches of one step")
    del m
    torch.cuda.empty_cache()


def _core_ref(qkv, tau, bias, heads, ws, shift, mask):
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    d = C // heads
    xs = torch.roll(qkv, shifts=(-shift, -shift), dims=(1, 2)) if shift > 0 else qkv
    xw = xs.view(B, H // ws, ws, W // ws, ws, C3).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C3)
    B_, N, _ = xw.shape
    t = xw.reshape(B_, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    q, k, v = t[0] * d ** -0.5, t[1], t[2]
    attn = torch.einsum("bhqd,bhkd->bhqk", q, k) / torch.maximum(
        q.norm(dim=-1, keepdim=True) * k.norm(dim=-1, keepdim=True).transpose(-2, -1), torch.tensor(1e-6, device=qkv.device, dtype=qkv.dtype))
    attn = attn / torch.clip(tau.unsqueeze(0)[:, :, :N, :N], min=0.01) + bias.unsqueeze(0)
    if shift > 0:
        nW = mask.shape[0]
        attn = (attn.view(B_ // nW, nW, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, N, N)
    o = (attn.softmax(-1) @ v).transpose(1, 2).reshape(B_, N, C)
    o = o.view(B, H // ws, W // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    return torch.roll(o, shifts=(shift, shift), dims=(1, 2)) if shift > 0 else o


def core(steps, warmup, lines):
    B, H, W, heads, ws, shift = 16, 64, 64, 3, 16, 8
    C, N, dt = 32 * heads, ws * ws, torch.bfloat16
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B, H, W, 3 * C, generator=g).to(dt).to(DEV)
    dout = torch.randn(B, H, W, C, generator=g).to(dt).to(DEV)
    tau = (torch.rand(heads, N, N, generator=g) * 1.5 + 0.005).to(DEV)
    bias = (torch.randn(heads, N, N, generator=g) * 0.5).to(DEV)
    qa, da = Act(qkv.view(-1, 3 * C), 0, 3 * C, B, H, W), Act(dout.view(-1, C), 0, C, B, H, W)
    out, dq = ops.new_act(B, H, W, C, dt, DEV), ops.new_act(B, H, W, 3 * C, dt, DEV)
    state = {}

    def fwd():
        state["lse"] = ops.winattn_fwd(qa, tau, bias, out, heads, ws, shift)

    def bwd():
        ops.winattn_bwd(qa, tau, bias, out, state["lse"], da, dq, heads, ws, shift)

    tf = _events(fwd, steps, warmup)
    tb = _events(bwd, steps, warmup)
    mask = torch_ref.swin_attention_mask(H, W, ws, shift).to(DEV).to(dt)
    qr = qkv.clone().requires_grad_(True)
    tr, br = tau.to(dt).requires_grad_(True), bias.to(dt).requires_grad_(True)

    def torch_fb():
        qr.grad = tr.grad = br.grad = None
        _core_ref(qr, tr, br, heads, ws, shift, mask).backward(dout)

    tt = _events(torch_fb, max(3, steps // 4), 2)
    lines.append(f"core, B=16 64x64 tokens, 3 heads, window 16, shift 8, bf16: wide kernels forward {tf:.3f} ms + backward "
                 f"(with the row sums) {tb:.3f} ms = {tf + tb:.3f} ms; the same core with torch ops in bf16, forward + backward "
                 f"{tt:.3f} ms ({tt / (tf + tb):.1f}x)")
    return tf + tb, tt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"# tools/swin_ws_bench.py --steps {a.steps} --warmup {a.warmup}; {torch.cuda.get_device_name(0)}, one process, one device"]
    mine, theirs = core(a.steps, a.warmup, lines)
    for ws in (16, 8):
        model_step(ws, a.steps, a.warmup, lines)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not mine < theirs:
        print("the wide kernels are SLOWER than the torch-op core")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
