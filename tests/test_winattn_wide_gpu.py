"""GPU: the window-attention wide kernels of uz_winattn.hip, windows of 65 .. 256 tokens (window_size 9 .. 16).

Kernel level, in the scheme of tests/test_swin_gpu.py::test_window_attention_core_forward_backward: the reference is a
float64 restatement of the reference model's roll -> partition -> cosine attention -> reverse -> roll back and its autograd
on the dtype-rounded operands; out, dqkv, d(bias) and d(tau) are held, `tau[:, 0, 1] = 0.002` (under the 0.01 clip) must
give an exactly-zero d(tau).  Tolerances are the project's figures for the 64-token kernels (fp32: 1e-5 out, 2e-4
gradients; bf16: 1e-2 out, 2e-2 gradients, 5e-2 d(tau)), relative to the reference's maximum.

The walk test follows tests/test_winattn_walk_gpu.py: 192 windows of 256 tokens, more than any of the grids holds, bit for
bit on out / lse / dqkv against launches image by image, against the same launch under uz_set_cu_reserve(128) and against
itself; d(bias) / d(tau), whose partition into partial rows depends on the grid, to 1e-5."""
from ctypes import byref

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import torch_ref
from unet_zoo_amd import _lib as L
from unet_zoo_amd import ops
from unet_zoo_amd.ops import Act
from winattn_ref import attention_core_ref as _attention_core_ref, grid as _grid  # tests/winattn_ref.py (pytest puts this directory on sys.path)

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
NUM_CU = 256
# resident workgroups per CU the grids are sized by: UZ_WIDE_SLOTS_* of csrc/uz_winattn.hip
SLOTS = {("fwd", torch.float32): 2, ("fwd", torch.bfloat16): 2, ("bwd", torch.float32): 1, ("bwd", torch.bfloat16): 2}
PARTIAL_BYTES = 64 << 20     # UZ_WIDE_PARTIAL_BYTES: cap of one launch's d(bias) / d(tau) partial rows

# (B, H, W, heads, ws, shift, Nt)
CASES = [
    (1, 16, 16, 3, 16, 0, 256),    # one full 256-token window
    (1, 32, 32, 3, 16, 8, 256),    # four shifted windows, all nine mask regions
    (2, 24, 24, 6, 12, 6, 144),    # N = 144
    (1, 9, 18, 6, 9, 4, 81),       # odd N, H != W
    (1, 15, 15, 3, 15, 7, 256),    # N = 225 inside a 256^2 tau: last tile partial, Nt > N
    (1, 20, 10, 12, 10, 5, 100),   # N = 100
]
IDS = [f"B{c[0]}-{c[1]}x{c[2]}-h{c[3]}-ws{c[4]}-s{c[5]}" for c in CASES]


@pytest.fixture(autouse=True)
def _restore():
    yield
    L.set_cu_reserve(0)


def rnd(dt, t):
    return t.to(dt).float()


def relerr(a, b):
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30)).item()


def _operands(case, dt):
    B, H, W, heads, ws, shift, Nt = case
    C, N = heads * 32, ws * ws
    g = torch.Generator().manual_seed(1000 * heads + 10 * ws + shift)
    qkv = rnd(dt, torch.randn(B, H, W, 3 * C, generator=g))
    tau = torch.rand(heads, Nt, Nt, generator=g) * 1.5 + 0.005
    tau[:, 0, 1] = 0.002                                        # below the 0.01 clip: zero tau gradient there
    bias = torch.randn(heads, N, N, generator=g) * 0.5
    dout = rnd(dt, torch.randn(B, H, W, C, generator=g))
    return qkv, tau, bias, dout


class _Dev:
    """the operands of a case on the device"""

    def __init__(self, case, dt, qkv, tau, bias, dout):
        B, H, W, heads, ws, shift, Nt = case
        self.case, self.dt, self.C = case, dt, 32 * heads
        self.qkv = qkv.reshape(B * H * W, -1).to(dt).to(DEV).contiguous()
        self.dout = dout.reshape(B * H * W, -1).to(dt).to(DEV).contiguous()
        self.tau, self.bias = tau.to(DEV).contiguous(), bias.to(DEV).contiguous()

    def bwd_rows(self, nb):
        B, H, W, heads, ws, shift, Nt = self.case
        d = L.WinAttnDesc(L.dtype_code(self.dt), nb, H, W, self.C, heads, ws, shift, Nt, 3 * self.C, self.C, 32 ** -0.5)
        return L.check_count(L.load().uz_winattn_bwd_rows(byref(d)), "uz_winattn_bwd_rows")

    def launch(self, b0=0, nb=None, fwd=None):
        """forward and backward of images [b0, b0 + nb) in one launch each; out and dqkv are NaN before the launches.
        fwd = (out, lse) of a launch over all images: the backward then reads those rows instead of its own forward's"""
        B, H, W, heads, ws, shift, Nt = self.case
        nb = B if nb is None else nb
        C, wpi = self.C, (H // ws) * (W // ws)
        r0, r1 = b0 * H * W, (b0 + nb) * H * W
        qa, da = Act(self.qkv[r0:r1], 0, 3 * C, nb, H, W), Act(self.dout[r0:r1], 0, C, nb, H, W)
        out, dq = ops.new_act(nb, H, W, C, self.dt, DEV), ops.new_act(nb, H, W, 3 * C, self.dt, DEV)
        out.buf.fill_(float("nan"))
        dq.buf.fill_(float("nan"))
        lse = ops.winattn_fwd(qa, self.tau, self.bias, out, heads, ws, shift)
        bo, bl = out, lse
        if fwd is not None:
            bo, bl = Act(fwd[0][r0:r1], 0, C, nb, H, W), fwd[1][b0 * wpi:(b0 + nb) * wpi]
        dbias, dtau = ops.winattn_bwd(qa, self.tau, self.bias, bo, bl, da, dq, heads, ws, shift)
        return out.buf, lse, dq.buf, dbias, dtau


def _tols(dt):
    """out, dqkv, dbias, dtau, each relative to the reference's maximum"""
    return (1e-5, 2e-4, 2e-4, 2e-4) if dt == torch.float32 else (1e-2, 2e-2, 2e-2, 5e-2)


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wide_window_attention_core_forward_backward(dt, case):
    """Every figure is printed before anything is asserted."""
    B, H, W, heads, ws, shift, Nt = case
    N, P = ws * ws, B * H * W
    qkv, tau, bias, dout = _operands(case, dt)
    q, t, b = (x.double().requires_grad_(True) for x in (qkv, tau, bias))
    ref = _attention_core_ref(q, t, b, heads, ws, shift)
    ref.backward(dout.double())
    dev = _Dev(case, dt, qkv, tau, bias, dout)
    out, lse, dq, dbias, dtau = dev.launch()
    fails = []
    for name, x in zip(("out", "lse", "dqkv", "dbias", "dtau"), (out, lse, dq, dbias, dtau)):
        if not bool(torch.isfinite(x).all()):
            fails.append(f"{name}: {int((~torch.isfinite(x)).sum())} elements not finite (unwritten?)")
    want = (ref.detach().reshape(P, -1), q.grad.reshape(P, -1), b.grad, t.grad[:, :N, :N])
    for name, g_, r_, tol in zip(("out", "dqkv", "dbias", "dtau"), (out, dq, dbias, dtau), want, _tols(dt)):
        e = relerr(g_.float().cpu(), r_)
        print(f"  {name} vs float64: {e:.3e} (tolerance {tol:g})")
        if not e < tol:
            fails.append(f"{name} vs float64: {e:.3e} >= {tol:g}")
    # lse against the float64 scores' log-sum-exp is implied by out and the gradients (the backward recomputes P from it)
    if float(dtau[:, 0, 1].abs().max()) != 0.0:
        fails.append("dtau under the 0.01 clip is not exactly zero")
    assert not fails, "\n".join(fails)


# ---- the walk --------------------------------------------------------------------------------------------------
WALK = (12, 64, 64, 3, 16, 8, 256)       # 192 windows of 256 tokens


def _rows(nwin, heads, N, slots, num_cu=NUM_CU):
    """the backward's grid = rows of `partial`: the fitted grid, capped so that the rows stay within PARTIAL_BYTES"""
    return min(_grid(nwin, heads, slots, num_cu), max(1, PARTIAL_BYTES // (2 * heads * N * N * 4)))


def _assert_walking(dev, num_cu=NUM_CU):
    B, H, W, heads, ws, shift, Nt = dev.case
    nwin, N = B * (H // ws) * (W // ws), ws * ws
    for key, slots in SLOTS.items():
        assert nwin > _grid(nwin, heads, slots, num_cu), key
    rows = dev.bwd_rows(B)
    assert rows == _rows(nwin, heads, N, SLOTS[("bwd", dev.dt)], num_cu) and nwin > rows
    assert rows * 2 * heads * N * N * 4 <= PARTIAL_BYTES
    return nwin


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
def test_wide_windows_walked_by_a_workgroup_are_the_windows_of_single_image_launches(dt):
    """192 windows: the forward's 96 workgroups take two each, the backward's 42 (the 64 MiB cap of the partial rows) four
    or five; under a reserve of 128 CUs the forward has 64 workgroups of three, the fp32 backward 39.  A single image has
    16 windows: one per workgroup in every kernel.  No CPU reference at this size (the cases above hold the arithmetic)."""
    case = WALK
    B, H, W, heads, ws, shift, Nt = case
    wpi, hw = (H // ws) * (W // ws), H * W
    dev = _Dev(case, dt, *_operands(case, dt))
    nwin = _assert_walking(dev)
    assert nwin == 192
    for slots in SLOTS.values():
        assert _grid(wpi, heads, slots) == wpi          # the single-image launches do not walk
    full = dev.launch()
    again = dev.launch()
    fails = []
    for name, t in zip(("out", "lse", "dqkv", "dbias", "dtau"), full):
        if not bool(torch.isfinite(t).all()):
            fails.append(f"{name}: {int((~torch.isfinite(t)).sum())} elements not finite (an unwritten window?)")
    for name, a, b in zip(("out", "lse", "dqkv", "dbias", "dtau"), full, again):
        if not torch.equal(a, b):
            fails.append(f"{name}: two identical launches differ")
    sb, st = torch.zeros_like(full[3], dtype=torch.float64), torch.zeros_like(full[4], dtype=torch.float64)
    for b in range(B):
        o, l, dq, dbias, dtau = dev.launch(b, 1, fwd=(full[0], full[1]))
        for name, got, want in (("out", full[0][b * hw:(b + 1) * hw], o), ("lse", full[1][b * wpi:(b + 1) * wpi], l),
                                ("dqkv", full[2][b * hw:(b + 1) * hw], dq)):
            if not torch.equal(got, want):
                fails.append(f"{name} of image {b}: full launch != single-image launch ({int((got != want).sum())} elements)")
        sb += dbias.double()
        st += dtau.double()
    for name, got, want in (("dbias", full[3], sb), ("dtau", full[4], st)):
        e = relerr(got, want)
        print(f"  {name} full launch vs float64 sum of the per-image launches: {e:.3e}")
        if not e < 1e-5:
            fails.append(f"{name}: full launch vs sum of the per-image launches {e:.3e} >= 1e-5")
    if float(full[4][:, 0, 1].abs().max()) != 0.0:
        fails.append("dtau under the 0.01 clip is not exactly zero")
    L.set_cu_reserve(128)
    _assert_walking(dev, 128)
    half = dev.launch()
    for name, a, b in zip(("out", "lse", "dqkv"), full, half):
        if not torch.equal(a, b):
            fails.append(f"{name}: differs under a reserve of 128 CUs ({int((a != b).sum())} elements)")
    for name, a, b in (("dbias", full[3], half[3]), ("dtau", full[4], half[4])):
        e = relerr(b, a)
        print(f"  {name} under a reserve of 128 CUs: {e:.3e}")
        if not e < 1e-5:
            fails.append(f"{name} under a reserve of 128 CUs: {e:.3e} >= 1e-5")
    assert not fails, "\n".join(fails)
