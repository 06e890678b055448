"""GPU: the window-attention kernels of uz_winattn.hip where a workgroup walks SEVERAL windows.

The four kernels (winattn_fwd_kernel / winattn_bwd_kernel in fp32, winattn_fwd_mfma2_kernel / winattn_bwd_mfma_kernel in
bf16) are persistent: attn_grid_x() caps the x-grid at 256 * slots / heads workgroups (slots = resident workgroups per CU,
1 .. 3) and a workgroup handles windows blockIdx.x, blockIdx.x + gridDim.x, ...  The other kernel-level tests have at most
8 windows -- one trip through that loop.  Here every case has more windows than any of the four grids holds, and is held
  1. against a float64 restatement of the reference (roll -> partition -> cosine attention -> reverse -> roll back) and its
     autograd, on the same dtype-rounded operands, with the tolerances of test_swin_gpu.py;
  2. bit for bit against the same kernels launched image by image (few or one window per workgroup): a window's out / lse /
     dqkv rows depend on its own tokens, tau, bias and its position inside its image only;
  3. bit for bit against the same launch under uz_set_cu_reserve(128) (half the grid, twice the windows per workgroup);
  4. bit for bit against itself (two launches).
d bias / d tau are sums over windows whose partition into per-workgroup partial rows depends on the grid: 1e-5 between
regimes (the figure of test_cu_reserve_gpu.py for grid-dependent fp32 partial sums)."""
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
# resident workgroups per CU of the kernel that serves (direction, dtype): ATTN_SLOTS_* of uz_winattn.hip
SLOTS = {("fwd", torch.float32): 2, ("fwd", torch.bfloat16): 3, ("bwd", torch.float32): 1, ("bwd", torch.bfloat16): 2}

# (heads, ws, shift, B, H, W, Nt); windows per workgroup at full chip as "grid: count x windows", in the order
# fp32 forward / bf16 forward / fp32 backward / bf16 backward (cap = 256 * slots / heads, per = ceil(nwin / cap),
# grid = ceil(nwin / per); workgroup i takes windows i, i + grid, ...)
CASES = [
    # 768 windows, N = 16, uneven deal: 154: 152x5 + 2x4 / 256: all 3 / 77: 75x10 + 2x9 / 154: 152x5 + 2x4; mask region
    # ids of windows that are not a workgroup's first
    (3, 4, 2, 3, 64, 64, 16),
    # 300 windows, N = 49 (padded key / query rows carried across trips): 150: all 2 / 150: all 2 / 75: all 4 / 150: all 2
    (3, 7, 3, 3, 70, 70, 49),
    # 320 windows, N = 64, the benchmark's stage-1 form: 160: all 2 / 160: all 2 / 80: all 4 / 160: all 2
    (3, 8, 4, 5, 64, 64, 64),
    # the same without the mask
    (3, 8, 0, 5, 64, 64, 64),
    # 144 windows, H != W (window index <-> (image, row, column) under the walk): 72: all 2 / 72: all 2 / 36: all 4 / 72: all 2
    (6, 4, 2, 3, 16, 48, 16),
    # 80 windows, deep stage, few workgroups: 40: all 2 / 40: all 2 / 20: all 4 / 40: all 2
    (12, 7, 3, 5, 28, 28, 49),
    # 36 windows, bottleneck form, N = 4 inside a 7x7 tau: 18: all 2 / 18: all 2 / 9: all 4 / 18: all 2
    (24, 2, 0, 9, 4, 4, 49),
]
IDS = [f"h{c[0]}-ws{c[1]}-s{c[2]}-B{c[3]}-{c[4]}x{c[5]}" for c in CASES]
STAGE1, BOTTLENECK = CASES[2], CASES[6]


@pytest.fixture(autouse=True)
def _restore():
    yield
    L.set_cu_reserve(0)


def rnd(dt, t):
    return t.to(dt).float()


def relerr(a, b):
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30)).item()


def _reference64(qkv, tau, bias, dout, case):
    """out, dqkv as (P, C) / (P, 3C), dbias, dtau[:, :N, :N]: float64 on the CPU"""
    heads, ws, shift, B, H, W, Nt = case
    N = ws * ws
    q, t, b = (x.double().requires_grad_(True) for x in (qkv, tau, bias))
    o = _attention_core_ref(q, t, b, heads, ws, shift)
    o.backward(dout.double())
    P = B * H * W
    return o.detach().reshape(P, -1), q.grad.reshape(P, -1), b.grad, t.grad[:, :N, :N]


# where the norm-clamp construction of test_window_attention_backward_follows_the_norm_clamp_of_the_reference sits inside
# its image: (row, column) of the three queries scaled by 1e-5 and of the zero query row
TINY = [(0, 3), (20, 17), (63, 63)]
ZERO = (33, 5)


def _operands(case, dt, clamp_img=None):
    heads, ws, shift, B, H, W, Nt = case
    C, N = heads * 32, ws * ws
    g = torch.Generator().manual_seed(1000 * heads + 10 * ws + shift)
    qkv = torch.randn(B, H, W, 3 * C, generator=g)
    if clamp_img is not None:
        qkv[clamp_img, :, :, C:2 * C] *= 1e-2                   # small keys
        for y, x in TINY:
            qkv[clamp_img, y, x, :C] *= 1e-5                    # tiny (non-zero) queries: |scale q||k| ~ 5e-7 < 1e-6
        qkv[clamp_img, ZERO[0], ZERO[1], :C] = 0                # a zero query row
    qkv = rnd(dt, qkv)
    tau = torch.rand(heads, Nt, Nt, generator=g) * 1.5 + 0.005
    tau[:, 0, 1] = 0.002                                        # below the 0.01 clip: zero tau gradient there
    bias = torch.randn(heads, N, N, generator=g) * 0.5
    dout = rnd(dt, torch.randn(B, H, W, C, generator=g))
    return qkv, tau, bias, dout


class _Dev:
    """the operands of a case on the device"""

    def __init__(self, case, dt, qkv, tau, bias, dout):
        heads, ws, shift, B, H, W, Nt = case
        self.case, self.dt, self.C = case, dt, 32 * heads
        self.qkv = qkv.reshape(B * H * W, -1).to(dt).to(DEV).contiguous()
        self.dout = dout.reshape(B * H * W, -1).to(dt).to(DEV).contiguous()
        self.tau, self.bias = tau.to(DEV).contiguous(), bias.to(DEV).contiguous()

    def desc(self, nb):
        heads, ws, shift, B, H, W, Nt = self.case
        return L.WinAttnDesc(L.dtype_code(self.dt), nb, H, W, self.C, heads, ws, shift, Nt, 3 * self.C, self.C, 32 ** -0.5)

    def bwd_rows(self, nb):
        return L.check_count(L.load().uz_winattn_bwd_rows(byref(self.desc(nb))), "uz_winattn_bwd_rows")

    def launch(self, b0=0, nb=None, fwd=None):
        """forward and backward of images [b0, b0 + nb) in one launch each; out and dqkv are NaN before the launches.
        fwd = (out, lse) of a launch over all images: the backward then reads those rows instead of its own forward's"""
        heads, ws, shift, B, H, W, Nt = self.case
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


def _assert_walking(dev, num_cu=NUM_CU):
    """some workgroup of each of the four kernels handles two or more windows (and the backward's own row query agrees)"""
    heads, ws, shift, B, H, W, Nt = dev.case
    nwin = B * (H // ws) * (W // ws)
    assert nwin > 768 // heads                                 # 768 / heads >= 256 * slots / heads, every kernel's cap
    for key, slots in SLOTS.items():
        assert nwin > _grid(nwin, heads, slots, num_cu), key
    rows = dev.bwd_rows(B)
    assert rows == _grid(nwin, heads, SLOTS[("bwd", dev.dt)], num_cu) and nwin > rows
    return nwin


def _tols(dt):
    """test_window_attention_core_forward_backward's: out, dqkv, dbias, dtau, each relative to the reference's maximum"""
    return (1e-5, 2e-4, 2e-4, 2e-4) if dt == torch.float32 else (1e-2, 2e-2, 2e-2, 5e-2)


def _bitwise_against_images(dev, full, fails):
    """check 2: B launches of one image each.  Returns nothing; appends to fails."""
    heads, ws, shift, B, H, W, Nt = dev.case
    wpi, hw = (H // ws) * (W // ws), H * W
    one_window = {k: _grid(wpi, heads, s) == wpi for k, s in SLOTS.items() if k[1] == dev.dt}
    sb, st = torch.zeros_like(full[3], dtype=torch.float64), torch.zeros_like(full[4], dtype=torch.float64)
    for b in range(B):
        o, l, dq, dbias, dtau = dev.launch(b, 1, fwd=(full[0], full[1]))
        for name, got, want in (("out", full[0][b * hw:(b + 1) * hw], o), ("lse", full[1][b * wpi:(b + 1) * wpi], l),
                                ("dqkv", full[2][b * hw:(b + 1) * hw], dq)):
            if not torch.equal(got, want):
                fails.append(f"{name} of image {b}: full launch != single-image launch "
                             f"({int((got != want).sum())} elements, one window per workgroup there: {one_window})")
        sb += dbias.double()
        st += dtau.double()
    for name, got, want in (("dbias", full[3], sb), ("dtau", full[4], st)):
        e = relerr(got, want)
        print(f"  {name} full launch vs float64 sum of the per-image launches: {e:.3e}")
        if not e < 1e-5:
            fails.append(f"{name}: full launch vs sum of the per-image launches {e:.3e} >= 1e-5")
    return one_window


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_several_windows_per_workgroup_against_float64_and_against_single_image_launches(dt, case):
    """Checks 1, 2 and 4 of the module docstring; every figure is printed before anything is asserted.

    The per-image launches of check 2 have one window per workgroup in every kernel for the ws 8, 12-head and 24-head cases
    (64, 16, 4 windows per image).  Where an image still has more windows than a grid (256 windows per image of the first
    case in all kernels but the bf16 forward; the fp32 backward's 85- / 42-workgroup grid with 100 / 48 windows per image)
    the single-image launch walks too, with another deal (2 - 4 windows per workgroup, other neighbours): the comparison is
    kept, it is then walk against walk.  It is never skipped and never a tolerance."""
    heads, ws, shift, B, H, W, Nt = case
    N = ws * ws
    qkv, tau, bias, dout = _operands(case, dt)
    dev = _Dev(case, dt, qkv, tau, bias, dout)
    _assert_walking(dev)
    full = dev.launch()
    again = dev.launch()
    fails = []
    for name, t in zip(("out", "lse", "dqkv", "dbias", "dtau"), full):
        if not bool(torch.isfinite(t).all()):
            fails.append(f"{name}: {int((~torch.isfinite(t)).sum())} elements not finite (an unwritten window?)")
    for name, a, b in zip(("out", "lse", "dqkv", "dbias", "dtau"), full, again):
        if not torch.equal(a, b):
            fails.append(f"{name}: two identical launches differ")
    ref = _reference64(qkv, tau, bias, dout, case)
    got = (full[0], full[2], full[3], full[4])
    for name, g_, r_, tol in zip(("out", "dqkv", "dbias", "dtau"), got, ref, _tols(dt)):
        e = relerr(g_.cpu(), r_)
        print(f"  {name} vs float64: {e:.3e} (tolerance {tol:g})")
        if not e < tol:
            fails.append(f"{name} vs float64: {e:.3e} >= {tol:g}")
    if float(full[4][:, 0, 1].abs().max()) != 0.0:
        fails.append("dtau under the 0.01 clip is not exactly zero")
    one_window = _bitwise_against_images(dev, full, fails)
    if (heads, ws) in ((3, 8), (12, 7), (24, 2)):
        assert all(one_window.values()), one_window
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", [STAGE1, BOTTLENECK], ids=[IDS[2], IDS[6]])
def test_half_the_grid_gives_the_same_windows(dt, case):
    """uz_set_cu_reserve(128): cap = 128 * slots / heads.  Windows per workgroup (fp32 fwd / bf16 fwd / fp32 bwd / bf16 bwd):
    3 heads, 320 windows: 80: all 4 / 107: 106x3 + 1x2 / 40: all 8 / 80: all 4; 24 heads, 36 windows: 9: all 4 / 12: all 3 /
    5: 1x8 + 4x7 / 9: all 4."""
    heads, ws, shift, B, H, W, Nt = case
    dev = _Dev(case, dt, *_operands(case, dt))
    nwin = _assert_walking(dev)
    base = dev.launch()
    rows0 = dev.bwd_rows(B)
    L.set_cu_reserve(128)
    _assert_walking(dev, 128)
    rows = dev.bwd_rows(B)
    assert rows < rows0 and -(-nwin // rows) >= 2 * (nwin // rows0)
    half = dev.launch()
    for name, a, b in zip(("out", "lse", "dqkv"), base, half):
        assert bool(torch.isfinite(b).all()), name
        assert torch.equal(a, b), name
    for name, a, b in (("dbias", base[3], half[3]), ("dtau", base[4], half[4])):
        assert relerr(b, a) < 1e-5, name


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("clamp_img", [4, 1])
def test_norm_clamp_windows_between_ordinary_windows_of_the_same_workgroup(dt, clamp_img):
    """State that must not leak from one window to the next (sCorrK, sRk, sRkMax, sCnt, the prefetch registers): the
    3-head / ws 8 / shift 4 case with the construction of test_window_attention_backward_follows_the_norm_clamp_of_the_reference
    in one image -- all keys at 1e-2, three queries at 1e-5 (norm products ~5e-7 under the 1e-6 clamp, the backward's slow
    path), a zero query row, a tau entry under the 0.01 clip.
    clamp_img = 4, the last image (windows 256 .. 319): the slow path runs in every workgroup's LAST trip, after ordinary
    windows (bf16 backward, 160 workgroups: windows i, i + 160; fp32 backward, 80: i, i + 80, i + 160, i + 240).
    clamp_img = 1 (windows 64 .. 127): ordinary windows FOLLOW a clamped one in the same workgroup, which the last image
    cannot give -- its windows are the end of every walk.
    dq of the clamped queries carries the clamp's 1e6 factor and dk of the small-key image 1e2: they are compared by
    themselves, and everything else by itself; the three parts partition dqkv."""
    case = STAGE1
    heads, ws, shift, B, H, W, Nt = case
    C, N, hw = 32 * heads, ws * ws, H * W
    qkv, tau, bias, dout = _operands(case, dt, clamp_img)
    nq = qkv[clamp_img, TINY[0][0], TINY[0][1], :32].norm() * 32 ** -0.5
    nk = qkv[clamp_img, 0, 4, C:C + 32].norm()
    assert 0 < nq * nk < 1e-6
    dev = _Dev(case, dt, qkv, tau, bias, dout)
    _assert_walking(dev)
    out, lse, dq, dbias, dtau = dev.launch()
    again = dev.launch()
    r_out, r_dq, r_dbias, r_dtau = _reference64(qkv, tau, bias, dout, case)
    fails = []
    for name, a, b in zip(("out", "lse", "dqkv", "dbias", "dtau"), (out, lse, dq, dbias, dtau), again):
        if not bool(torch.isfinite(a).all()):
            fails.append(f"{name}: not finite")
        if not torch.equal(a, b):
            fails.append(f"{name}: two identical launches differ")
    t_out, t_dq, t_db, t_dt = _tols(dt)
    part = torch.zeros(B * hw, 3 * C, dtype=torch.int8)        # 0: the rest, 1: dq of the clamped queries, 2: dk of the image
    part[clamp_img * hw:(clamp_img + 1) * hw, C:2 * C] = 2
    for y, x in TINY + [ZERO]:                                 # the zero row's pairs are clamped too: the same 1e6 factor
        part[clamp_img * hw + y * W + x, :C] = 1
    gq = dq.double().cpu()
    assert int((part == 0).sum() + (part == 1).sum() + (part == 2).sum()) == part.numel()
    for name, sel in (("the rest of dqkv", part == 0), ("dq of the clamped queries", part == 1), ("dk of the small-key image", part == 2)):
        a, b = gq[sel], r_dq[sel]
        e = ((a - b).abs().max() / b.abs().max()).item()
        print(f"  {name}: {e:.3e} (tolerance {t_dq:g}), reference maximum {b.abs().max().item():.3e}")
        if not e < t_dq:
            fails.append(f"{name}: {e:.3e} >= {t_dq:g}")
    for name, g_, r_, tol in (("out", out, r_out, t_out), ("dbias", dbias, r_dbias, t_db), ("dtau", dtau, r_dtau, t_dt)):
        e = relerr(g_.cpu(), r_)
        print(f"  {name} vs float64: {e:.3e} (tolerance {tol:g})")
        if not e < tol:
            fails.append(f"{name} vs float64: {e:.3e} >= {tol:g}")
    if float(dtau[:, 0, 1].abs().max()) != 0.0:
        fails.append("dtau under the 0.01 clip is not exactly zero")
    _bitwise_against_images(dev, (out, lse, dq, dbias, dtau), fails)
    assert not fails, "\n".join(fails)
