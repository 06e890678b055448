"""GPU: layernorm_kernel and ln_head_kernel of uz_swin.hip where every workgroup makes SEVERAL trips.

Both kernels walk `for (t0 = blockIdx.x * tpb; t0 < P; t0 += gridDim.x * tpb)` on a grid of min(ceil(P / tpb), 8 * CUs)
workgroups and leave one dgamma / dbeta (dw / db) partial row per workgroup.  The other LayerNorm tests have 30 tokens:
one workgroup, one trip, one partial row.  Here uz_set_cu_reserve(128) puts the cap at 8 * 128 = 1024 workgroups and every
case has P > 2 * 1024 * tpb tokens with P % tpb != 0: at least two trips per workgroup, the last one partial, and 1024
partial rows.  References: F.layer_norm on the addressing restated in torch, float64 on the CPU, on dtype-rounded inputs;
tolerances: those of the 30-token tests (test_swin_gpu.py, test_mit_gpu.py).

tpb = 4 waves * (64 / lpt) tokens per wave * unroll, from ln_lpt / ln_its / ln_unroll / ln_grid (ln_head_lpt / ln_head_unroll)
of uz_swin.hip, restated in _ln_plan / _head_plan below; chunks = C / (4 fp32 | 8 bf16):
  C = 96  fp32: 24 chunks -> 8 per lane-third -> lpt 8,  its 3, unroll 1 fwd / 2 bwd: tpb  32 /  64
  C = 96  bf16: 12 chunks -> 4               -> lpt 4,  its 3,                        tpb  64 / 128
  C = 384 fp32: 96 chunks -> 32              -> lpt 32, its 3,                        tpb   8 /  16
  C = 384 bf16: 48 chunks -> 16              -> lpt 16, its 3,                        tpb  16 /  32
  C = 64  fp32: 16 chunks -> 6 -> lpt 8, its 2, unroll 1 / 2: tpb 32 / 64;  bf16: 8 -> 3 -> lpt 4, its 2: tpb 64 / 128
  head K = 1 (three chunks per lane, unroll 1 / 2): as C = 96: 32 / 64 fp32, 64 / 128 bf16
  head K = 3 (one chunk per lane, unroll 2 both ways): fp32 lpt 32: tpb 16; bf16 lpt 16: tpb 32
The backward's tpb is pinned to the library through uz_layernorm_bwd_rows / uz_ln_head_bwd_workspace_bytes on a probe shape;
the forward has no such query, its figure stands on the restatement alone."""
from ctypes import byref

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from unet_zoo_amd import _lib as L
from unet_zoo_amd import ops
from unet_zoo_amd.ops import Act

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
RESERVE = 128
CAP = 8 * (256 - RESERVE)


@pytest.fixture(autouse=True)
def _restore():
    yield
    L.set_cu_reserve(0)


def rnd(dt, t):
    return t.to(dt).float()


def relerr(a, b):
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30)).item()


def tokens_to_act(t, dt):
    """(B, H, W, C) -> Act"""
    B, H, W, C = t.shape
    return Act(t.reshape(B * H * W, C).to(dt).to(DEV).contiguous(), 0, C, B, H, W)


def _pow2(cc):
    l = 1
    while l < cc and l < 64:
        l <<= 1
    return l


def _ln_plan(C, dt, bwd):
    chunks = C // (8 if dt == BF16 else 4)
    lpt = _pow2((chunks + 2) // 3)
    its = -(-chunks // lpt)
    unroll = 1 if its > 3 else ((2 if bwd else 1) if its > 1 else 4)
    return 4 * (64 // lpt) * unroll


def _head_plan(C, dt, K, bwd):
    its = 3 if K == 1 else 1
    lpt = _pow2(-(-(C // (8 if dt == BF16 else 4)) // its))
    return 4 * (64 // lpt) * (1 if (K == 1 and not bwd) else 2)


def _desc(dt, B, Ho, Wo, C, ldx, mode, r, act=0):
    return L.LnDesc(L.dtype_code(dt), B, Ho, Wo, C, ldx, C, C, C, ldx, mode, r, 1e-5, act)


def _assert_walking(P, tf, tb, rows, probe_rows):
    """the case is in the walking regime under the reserve, and the restated backward tpb is the library's"""
    assert probe_rows == 11                                    # a probe of 10 * tb + 1 tokens: ceil(P / tpb) workgroups
    assert P > 2 * CAP * max(tf, tb)                           # every workgroup makes at least two trips, both ways
    assert P % tf != 0 and P % tb != 0                         # and the last trip is partial
    assert rows == CAP                                         # one partial row per workgroup, the grid is the cap


def _addressed(x, mode, r, c):
    """the (B, Ho, Wo, C) token map the kernel normalises, from x as it lies in memory"""
    if mode == L.LN_MERGE:
        return torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
    if mode == L.LN_EXPAND:
        B, H, W, _ = x.shape
        return x.view(B, H, W, r, r, c).permute(0, 1, 3, 2, 4, 5).reshape(B, H * r, W * r, c)
    return x


# name: (mode, C of the normalised token, r, residual + per-image scale, GELU, {dtype: (B, Ho, Wo) of the normalised map}).
# P = B Ho Wo is the smallest convenient count over 2 * 1024 * tpb_bwd with a ragged tail for both tpb:
LN_CASES = {
    # 2 * 1024 * 64 = 131072 < 3 * 210 * 210 = 132300 (% 64 = % 32 = 12); 2 * 1024 * 128 = 262144 < 3 * 297 * 295 = 262845
    # (% 128 = % 64 = 61); an image (44100 / 87615 tokens) is no multiple of tpb either: trips cross image boundaries
    "plain96_res_scale": (L.LN_PLAIN, 96, 1, True, False, {F32: (3, 210, 210), BF16: (3, 297, 295)}),
    # 2 * 1024 * 16 = 32768 < 3 * 105 * 105 = 33075 (% 16 = % 8 = 3); 2 * 1024 * 32 = 65536 < 3 * 149 * 147 = 65709 (% 32 = % 16 = 13)
    "plain384": (L.LN_PLAIN, 384, 1, False, False, {F32: (3, 105, 105), BF16: (3, 149, 147)}),
    # the benchmark's 1M-token LayerNorm: x is (3, 105, 105, 4 * 96) -> 132300 tokens; (3, 149, 147, 384) -> 262836 (% 128 = % 64 = 52)
    "expand2_96": (L.LN_EXPAND, 96, 2, False, False, {F32: (3, 210, 210), BF16: (3, 298, 294)}),
    # x is (3, 210, 210, 96) / (3, 298, 294, 96), normalised as 33075 / 65709 tokens of 384
    "merge384": (L.LN_MERGE, 384, 1, False, False, {F32: (3, 105, 105), BF16: (3, 149, 147)}),
    # act(norm1(.)) of MISSFormer: tpb as C = 96
    "gelu64": (L.LN_PLAIN, 64, 1, False, True, {F32: (3, 210, 210), BF16: (3, 297, 295)}),
}


def _ln_tols(dt, gelu):
    """(out, dx, parameter gradients): test_layernorm_plain_with_residual_and_drop_scale's.  With GELU the parameter
    gradients get test_layernorm_with_gelu_forward_backward's 2e-4; out and dx keep the plain figures, which is tighter than
    that test's 5e-6 / 2e-5 (fp32) and 2e-2 (bf16 dx): the kernel's erf (Abramowitz-Stegun 7.1.26, |error| < 1.5e-7) moves
    z * cdf(z) by less than 7.5e-8 of |z| and the derivative by about as much, an order under 2e-6 / 1e-5"""
    return (2e-6, 1e-5, 2e-4 if gelu else 1e-4) if dt == F32 else (1e-2, 1e-2, 2e-4 if gelu else 1e-4)


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(LN_CASES))
def test_layernorm_with_several_trips_per_workgroup(dt, name):
    mode, C, r, res_scale, gelu, shapes = LN_CASES[name]
    B, Ho, Wo = shapes[dt]
    P = B * Ho * Wo
    g = torch.Generator().manual_seed(len(name) + C)
    if mode == L.LN_MERGE:
        xs = (B, 2 * Ho, 2 * Wo, C // 4)
    elif mode == L.LN_EXPAND:
        xs = (B, Ho // r, Wo // r, r * r * C)
    else:
        xs = (B, Ho, Wo, C)
    x = rnd(dt, torch.randn(xs, generator=g) * 2 + 0.5)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.1
    dy = rnd(dt, torch.randn(B, Ho, Wo, C, generator=g))
    res = rnd(dt, torch.randn(B, Ho, Wo, C, generator=g)) if res_scale else None
    sb = torch.tensor([0.0, 1.0 / 0.9, 0.37]) if res_scale else None       # distinct per image; 0 = a dropped path
    assert x.numel() * (2 if dt == BF16 else 4) < 64 << 20

    xa, ga = tokens_to_act(x, dt), tokens_to_act(dy, dt)
    ra = tokens_to_act(res, dt) if res_scale else None
    gd, bd = gamma.to(DEV), beta.to(DEV)
    sbd = sb.to(DEV) if res_scale else None
    lib = L.load()

    def run():
        out = ops.new_act(B, Ho, Wo, C, dt, DEV)
        dx = ops.new_act(*xs, dt, DEV)
        out.buf.fill_(float("nan"))
        dx.buf.fill_(float("nan"))
        stats = ops.layernorm_fwd(xa, gd, bd, out, mode=mode, r=r, res=ra, image_scale=sbd, gelu=gelu)
        dgam, dbet = ops.layernorm_bwd(xa, gd, stats, ga, dx, mode=mode, r=r, image_scale=sbd, gelu_beta=bd if gelu else None)
        return out.buf, stats, dx.buf, dgam, dbet

    full_chip = run()
    L.set_cu_reserve(RESERVE)
    tf, tb = _ln_plan(C, dt, False), _ln_plan(C, dt, True)
    rows = L.check_count(lib.uz_layernorm_bwd_rows(byref(_desc(dt, B, Ho, Wo, C, xa.ld, mode, r, int(gelu)))), "rows")
    probe = L.check_count(lib.uz_layernorm_bwd_rows(byref(_desc(dt, 1, 1, 10 * tb + 1, C, C, L.LN_PLAIN, 1, int(gelu)))), "rows")
    _assert_walking(P, tf, tb, rows, probe)
    got = run()
    again = run()
    names = ("out", "stats", "dx", "dgamma", "dbeta")
    fails = []
    for n, a, b, c in zip(names, got, again, full_chip):
        if not bool(torch.isfinite(a).all()):
            fails.append(f"{n}: {int((~torch.isfinite(a)).sum())} elements not finite (tokens nobody wrote?)")
        if not torch.equal(a, b):
            fails.append(f"{n}: two identical launches differ")
        if n in ("out", "stats", "dx") and not torch.equal(a, c):
            fails.append(f"{n}: differs between a grid of 2048 and of 1024 workgroups ({int((a != c).sum())} elements)")

    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ref = F.layer_norm(_addressed(x64, mode, r, C), (C,), g64, b64, 1e-5)
    if gelu:
        ref = F.gelu(ref)
    if res_scale:
        ref = res.double() + ref * sb.double().view(B, 1, 1, 1)
    ref.backward(dy.double())
    t_out, t_dx, t_par = _ln_tols(dt, gelu)
    for n, a, b, tol in (("out", got[0].float().cpu().reshape(ref.shape), ref.detach(), t_out),
                         ("dx", got[2].float().cpu().reshape(xs), x64.grad, t_dx),
                         ("dgamma", got[3].cpu(), g64.grad, t_par), ("dbeta", got[4].cpu(), b64.grad, t_par)):
        e = relerr(a, b)
        print(f"  {n} vs float64: {e:.3e} (tolerance {tol:g})")
        if not e < tol:
            fails.append(f"{n} vs float64: {e:.3e} >= {tol:g}")
    assert not fails, "\n".join(fails)


# (K, bias, mode, r, {dtype: (B, Ho, Wo)}): C = 96.
HEAD_CASES = {
    # the tail of swin_unet_v2 (4x4 expand): tpb 32 / 64 fp32, 64 / 128 bf16.  x is (3, 53, 53, 16 * 96) -> 134832 tokens > 131072
    # (% 64 = 48, % 32 = 16); (3, 75, 73, 1536) -> 262800 > 262144 (% 128 = 16, % 64 = 16)
    "K1_expand4": (1, False, L.LN_EXPAND, 4, {F32: (3, 212, 212), BF16: (3, 300, 292)}),
    # one chunk per lane: tpb 16 fp32, 32 bf16, both ways.  Plain tokens: 16 r^2 tokens per input pixel leave no ragged tail under
    # the 4x4 expand.  3 * 105 * 105 = 33075 > 32768 (% 16 = 3); 3 * 149 * 147 = 65709 > 65536 (% 32 = 13)
    "K3_plain_bias": (3, True, L.LN_PLAIN, 1, {F32: (3, 105, 105), BF16: (3, 149, 147)}),
}


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(HEAD_CASES))
def test_layernorm_head_with_several_trips_per_workgroup(dt, name):
    """uz_ln_head_fwd / bwd: tolerances of test_layernorm_with_1x1_head_fused (logits 2e-6 fp32 / 1e-5 bf16 -- x is exact in
    both --, dx 1e-5 / 1e-2, dgamma / dbeta / dw 1e-4, db 1e-5)"""
    K, bias, mode, r, shapes = HEAD_CASES[name]
    C = 96
    B, Ho, Wo = shapes[dt]
    P = B * Ho * Wo
    g = torch.Generator().manual_seed(61 + K)
    xs = (B, Ho // r, Wo // r, r * r * C)
    x = rnd(dt, torch.randn(xs, generator=g) * 2 + 0.5)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.1
    w = torch.randn(K, C, generator=g) * 0.2
    b = torch.randn(K, generator=g) if bias else None
    dlog = torch.randn(B, K, Ho, Wo, generator=g)
    assert x.numel() * (2 if dt == BF16 else 4) < 64 << 20
    xa = tokens_to_act(x, dt)
    gd, bd, wd, dld = gamma.to(DEV), beta.to(DEV), w.to(DEV), dlog.to(DEV)
    bb = b.to(DEV) if bias else None
    lib = L.load()
    assert ops.ln_head_supported(C, K, dt)

    def run():
        dx = ops.new_act(*xs, dt, DEV)
        dx.buf.fill_(float("nan"))
        logits, stats = ops.ln_head_fwd(xa, gd, bd, wd, bb, B, Ho, Wo, C, mode=mode, r=r)
        dgam, dbet, dw, db = ops.ln_head_bwd(xa, gd, bd, wd, stats, dld, dx, mode=mode, r=r)
        return logits, stats, dx.buf, dgam, dbet, dw, db

    full_chip = run()
    L.set_cu_reserve(RESERVE)
    tf, tb = _head_plan(C, dt, K, False), _head_plan(C, dt, K, True)
    row_bytes = (K * C + K) * 4
    wsb = L.check_count(lib.uz_ln_head_bwd_workspace_bytes(byref(_desc(dt, B, Ho, Wo, C, xa.ld, mode, r)), K), "workspace")
    probe = L.check_count(lib.uz_ln_head_bwd_workspace_bytes(byref(_desc(dt, 1, 1, 10 * tb + 1, C, C, L.LN_PLAIN, 1)), K), "workspace")
    assert wsb % row_bytes == 0 and probe % row_bytes == 0
    _assert_walking(P, tf, tb, wsb // row_bytes, probe // row_bytes)
    got = run()
    again = run()
    names = ("logits", "stats", "dx", "dgamma", "dbeta", "dw", "db")
    fails = []
    for n, a, b_, c in zip(names, got, again, full_chip):
        if n == "db" and not bias:
            continue                                           # written all the same, but nothing to hold it against
        if not bool(torch.isfinite(a).all()):
            fails.append(f"{n}: {int((~torch.isfinite(a)).sum())} elements not finite (tokens nobody wrote?)")
        if not torch.equal(a, b_):
            fails.append(f"{n}: two identical launches differ")
        if n in ("logits", "stats", "dx") and not torch.equal(a, c):
            fails.append(f"{n}: differs between a grid of 2048 and of 1024 workgroups ({int((a != c).sum())} elements)")

    x64 = x.double().requires_grad_(True)
    g64, b64, w64 = (t.double().requires_grad_(True) for t in (gamma, beta, w))
    bias64 = b.double().requires_grad_(True) if bias else None
    tok = F.layer_norm(_addressed(x64, mode, r, C), (C,), g64, b64, 1e-5)
    ref = F.conv2d(tok.permute(0, 3, 1, 2), w64.view(K, C, 1, 1), bias64)
    ref.backward(dlog.double())
    checks = [("logits", got[0].cpu(), ref.detach(), 2e-6 if dt == F32 else 1e-5),
              ("dx", got[2].float().cpu().reshape(xs), x64.grad, 1e-5 if dt == F32 else 1e-2),
              ("dgamma", got[3].cpu(), g64.grad, 1e-4), ("dbeta", got[4].cpu(), b64.grad, 1e-4),
              ("dw", got[5].cpu(), w64.grad, 1e-4)]
    if bias:
        checks.append(("db", got[6].cpu(), bias64.grad, 1e-5))
    for n, a, b_, tol in checks:
        e = relerr(a, b_)
        print(f"  {n} vs float64: {e:.3e} (tolerance {tol:g})")
        if not e < tol:
            fails.append(f"{n} vs float64: {e:.3e} >= {tol:g}")
    assert not fails, "\n".join(fails)
