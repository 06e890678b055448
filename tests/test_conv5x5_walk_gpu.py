"""GPU: the 5x5 convolution family of uz_conv5x5.hip where its workgroups walk: several trips of conv5_kernel's tile loop,
wgrad5_kernel at the pixel split its plan asks for, and the BatchNorm + ELU passes beyond one workgroup.

conv5_kernel is persistent over M: c5_plan caps grid_m at 2 * 256 / tiles_n and the kernel runs
`for (tile = blockIdx.x; tile < a.tiles_m; tile += gridDim.x)`.  What only a later trip executes: the statistics registers
s1 / s2 that live across trips, the reuse of LDS stage 0 by the next trip's store_step(0), m0 = tile * BM on a tile that is
not blockIdx.x, and a partial last tile reached on a late trip.  tests/test_conv5x5_gpu.py stops at 15 tiles, the model tests
at 64: one trip.  Here every conv case asserts, before it compares anything, that
  * uz_conv5x5_grid_m() is the cap of the plan as restated in _c5_plan() below,
  * ceil(M / 128) >= 2 * grid_m + 1: every workgroup makes at least two trips and some make three,
  * M % 128 != 0: the last trip of some workgroup is a partial tile.
The plan is sized by the hardware's CU count, not by uz_set_cu_reserve(): one test asserts that.

References:
  1. integer operands (x from {-1, 0, 1}, thinned weights from {-1, 0, 1}, integer bias; {-2..2} for the weight gradient):
     every fp32 sum is exact whatever the order, so F.conv2d / conv2d_weight in fp32 on the CPU is the float64 result, and
     the kernel's result must be that value rounded once to the run dtype, bit for bit.  A norm-relative bound cannot see one
     wrong pixel in 131572 (sqrt(1 / 131572) = 0.0028 < 2^-8); torch.equal can;
  2. statistics rows summed in float64 against the float64 column sums of the reference, exactly: the test first asserts
     from the reference alone that sum |y| < 2^24, sum y^2 < 2^24 and max |y| <= 256 in every column, so no fp32 partial sum
     and no bf16 store can round however the tiles are dealt to workgroups;
  3. normal operands, one case per instantiation: float64 on dtype-rounded inputs, to the bounds tests/test_conv5x5_gpu.py
     derives from the formats (1e-4 fp32, 2^-8 bf16, of the norm) and the max-error-over-max-magnitude bounds of
     tests/test_gemm_dma_walk_gpu.py (1e-5 fp32, 1.2e-2 bf16);
  4. BatchNorm + ELU: the float64 autograd oracle of test_conv5x5_gpu.py::test_bn_elu_forward_and_backward and its bounds
     (1e-4 fp32, 2^-7 bf16: up to three chained bf16 roundings; dgamma / dbeta against the sum of their terms' magnitudes),
     each applied to the norm and to max error over max magnitude."""
import functools
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
DT_IDS = ["fp32", "bf16"]
SENTINEL = -77.0                 # exact in bf16; no case can produce it where it is looked for
CUS_HW = 256                     # UZ_NUM_CU_HW: these plans do not follow uz_set_cu_reserve()
BM = 128

MAP_33K = (2, 130, 127)          # M = 33020 = 257 * 128 + 124
MAP_66K = (2, 182, 181)          # M = 65884 = 514 * 128 + 92
MAP_131K = (2, 259, 254)         # M = 131572 = 1027 * 128 + 116


@pytest.fixture(autouse=True)
def _restore():
    yield
    L.set_cu_reserve(0)


@pytest.fixture(scope="module", autouse=True)
def _free_references():
    yield
    _int_conv.cache_clear()


def cdiv(a, b):
    return -(-a // b)


def _id(dt):
    return DT_IDS[DTYPES.index(dt)]


def ints(g, shape, lo=-1, hi=1):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def nhwc(t):
    """(N, C, H, W) -> (N H W, C)"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def _round_store(prod64, dt, bias=None):
    """the exact sum rounded once to the run dtype"""
    y = (prod64 + bias.double()) if bias is not None else prod64
    return y.to(dt)


def _where(got, ref, gm):
    """which rows of a (M, n) result differ, as 128-row tiles and trips (tile // grid_m): a fault of the walk shows in
    trips >= 1 only"""
    bad = (got != ref).any(1).nonzero().flatten()
    if bad.numel() == 0:
        return "equal"
    tiles = torch.unique(bad // BM)
    trips = torch.unique(tiles // gm).tolist()
    return (f"{bad.numel()} of {got.shape[0]} rows differ, in {tiles.numel()} tiles of {BM} rows (first {tiles[:6].tolist()}), "
            f"trips {trips} of a grid of {gm}; max |diff| {(got.double() - ref.double()).abs().max().item():g}")


def _assert_sums_exact(ref):
    """precondition of the exact statistics check, from the reference alone: no fp32 partial sum of a column can round, and
    every value is an integer that bf16 holds"""
    r = ref.double()
    assert r.abs().sum(0).max().item() < 2 ** 24, r.abs().sum(0).max().item()
    assert (r * r).sum(0).max().item() < 2 ** 24, (r * r).sum(0).max().item()
    assert r.abs().max().item() <= 256, r.abs().max().item()


def _check_stats(stats, ref, gm):
    """partial rows (gm, 2, n) of sum y and sum y^2 over the STORED values, summed in float64: exact"""
    assert stats.shape == (gm, 2, ref.shape[1]), (tuple(stats.shape), gm)
    _assert_sums_exact(ref)
    s = stats.double().sum(0).cpu()
    r = ref.double()
    assert torch.equal(s[0], r.sum(0)), f"sum y: {(s[0] - r.sum(0)).abs().max().item():g} off"
    assert torch.equal(s[1], (r * r).sum(0)), f"sum y^2: {(s[1] - (r * r).sum(0)).abs().max().item():g} off"


def _close2(what, got, ref, tol_norm, tol_max=None):
    """the bound on the norm, and on max error over max magnitude; prints what it saw"""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    tol_max = tol_norm if tol_max is None else tol_max
    en = ((got - ref).norm() / (ref.norm() + 1e-300)).item()
    em = ((got - ref).abs().max() / (ref.abs().max() + 1e-300)).item()
    print(f"    {what}: norm {en:.3e} (bound {tol_norm:.3e}), max/max {em:.3e} (bound {tol_max:.3e})")
    assert en <= tol_norm, (what, en, tol_norm)
    assert em <= tol_max, (what, em, tol_max)


def _close_sum(what, got, ref, scale, tol):
    """a sum of rounded terms: |got - ref| <= tol * sum |term|, per element"""
    got, ref, scale = got.double().cpu(), ref.double().cpu(), scale.double().cpu()
    worst = ((got - ref).abs() / (scale + 1e-300)).max().item()
    print(f"    {what}: err / sum|terms| {worst:.3e} (bound {tol:.3e})")
    assert worst <= tol, (what, worst, tol)


# ---- 1. conv5_kernel over several trips ----------------------------------------------------------------------------------
def _c5_plan(M, Nout):
    """(bn, tiles_m, grid_m) as c5_plan of uz_conv5x5.hip decides:
        p->bn = Nout <= 32 ? 32 : (Nout <= 64 ? 64 : 128);      <128,32,4,1> / <128,64,2,2> / <128,128,2,2>
        p->tiles_m = ceil(M / 128);  p->tiles_n = ceil(Nout / bn);
        cap = 2 * UZ_NUM_CU_HW / tiles_n (at least 1);  p->grid_m = min(tiles_m, cap)"""
    bn = 32 if Nout <= 32 else (64 if Nout <= 64 else 128)
    tiles_n = cdiv(Nout, bn)
    cap = max(1, 2 * CUS_HW // tiles_n)
    tiles_m = cdiv(M, BM)
    return bn, tiles_m, min(tiles_m, cap)


def _c5_desc(dt, shape, Cin, ldx, Nout, ldy, k):
    N, H, W = shape
    return L.Conv5Desc(L.dtype_code(dt), N, H, W, Cin, ldx, Nout, ldy, k)


def _assert_walks(d, bn_want):
    """the plan is the restated one, every workgroup makes at least two trips, some three, one of them over a partial tile;
    returns grid_m"""
    M = d.N * d.H * d.W
    gm = L.check_count(L.load().uz_conv5x5_grid_m(byref(d)), "uz_conv5x5_grid_m")
    bn, tiles_m, grid = _c5_plan(M, d.Nout)
    assert bn == bn_want, (bn, bn_want)
    assert gm == grid, (gm, grid)
    assert tiles_m >= 2 * gm + 1, (tiles_m, gm)
    assert M % BM != 0
    return gm


def _pack5(w):
    """(Nout, Cin, k, k) -> [Nout][tap * Cin + c], the kernel's flat reduction index (UZ_PACK_CONV_FWD)"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


# name: (Cin, Nout, ldy, k, map, bn, weight density, bias, statistics, dtypes)
CONV = {
    # <128,32,4,1>; K = 800: a bf16 K-step (64) spans two taps, an fp32 one (32) is one tap
    "lu32": (32, 32, 32, 5, MAP_131K, 32, 1 / 8, True, True, DTYPES),
    # <128,64,2,2>
    "lu64": (64, 64, 64, 5, MAP_131K, 64, 1 / 16, True, True, DTYPES),
    # 32 -> num_classes = 3 into an 8-column zero-padded buffer: columns 3..7 keep their zeros
    "out3": (32, 3, 8, 5, MAP_131K, 32, 1 / 8, True, False, DTYPES),
    # the output layer's input gradient: the same kernel on the 8-column gradient, K = 200 = 3 * 64 + 8 = 6 * 32 + 8: partial
    # last K-step, eight (bf16) or four (fp32) taps per step
    "dgrad8": (8, 32, 32, 5, MAP_131K, 32, 1 / 2, False, False, DTYPES),
    # K = 400: an fp32 K-step spans two taps too
    "cin16": (16, 32, 32, 5, MAP_131K, 32, 1 / 8, True, True, [F32]),
    # k = 1, 8 -> 16: one K-step, `more` is never true, every trip is load_step(0) / store_step(0) alone
    "adapter": (8, 16, 16, 1, MAP_131K, 32, 1.0, True, True, DTYPES),
    # <128,128,2,2>, two N tiles (cap 256), the second one partial (200 = 128 + 72)
    "n200": (32, 200, 200, 5, MAP_66K, 128, 1 / 4, True, True, DTYPES),
    # four N tiles, cap 128
    "n512": (32, 512, 512, 5, MAP_33K, 128, 1 / 2, True, True, DTYPES),
}
CONV_PARAMS = [pytest.param(n, dt, id=f"{n}-{_id(dt)}") for n, c in CONV.items() for dt in c[9]]


@functools.lru_cache(maxsize=2)
def _int_conv(name):
    """integer operands of a case and its exact product (M, Nout) in float64, shared by the dtypes (which follow each other)"""
    Cin, Nout, _, k, (N, H, W), _, density, with_bias, _, _ = CONV[name]
    g = torch.Generator().manual_seed(Cin * 1000 + Nout + k)
    x = ints(g, (N, Cin, H, W))
    w = ints(g, (Nout, Cin, k, k))
    if density < 1.0:
        w = w * (torch.rand(w.shape, generator=g) < density).float()
    b = ints(g, (Nout,), -3, 3) if with_bias else None
    prod = F.conv2d(x, w, None, padding=k // 2)          # fp32 on integers with |sum| <= 1600: exact
    return nhwc(x), _pack5(w), b, nhwc(prod).double()


@pytest.mark.parametrize("name,dt", CONV_PARAMS)
def test_conv5_is_exact_on_integers_over_several_trips(name, dt):
    Cin, Nout, ldy, k, shape, bn, _, with_bias, want_stats, _ = CONV[name]
    N, H, W = shape
    x, wp, b, prod = _int_conv(name)
    ref = _round_store(prod, dt, b)
    gm = _assert_walks(_c5_desc(dt, shape, Cin, Cin, Nout, ldy, k), bn)
    xa = Act(x.to(dt).to(DEV), 0, Cin, N, H, W)
    wd, bd = wp.to(dt).to(DEV), (b.to(DEV) if with_bias else None)

    def run():
        buf = torch.zeros((N * H * W, ldy), dtype=dt, device=DEV)
        buf[:, :Nout] = SENTINEL
        return buf, ops.conv5x5(xa, wd, bd, Act(buf, 0, Nout, N, H, W), ksize=k, want_stats=want_stats)

    ybuf, stats = run()
    got = ybuf.cpu()
    assert torch.equal(got[:, :Nout], ref), _where(got[:, :Nout], ref, gm)
    assert bool((got[:, Nout:] == 0).all())               # the zero padding of a thin layer's buffer
    if want_stats:
        _check_stats(stats, ref, gm)
    else:
        assert stats is None
    ybuf2, stats2 = run()
    assert torch.equal(ybuf2, ybuf) and (not want_stats or torch.equal(stats2, stats))


def test_conv5_plan_does_not_follow_the_cu_reserve():
    """the number of statistics rows is fixed per shape: the grid is sized by the hardware's CU count"""
    descs = [(_c5_desc(dt, c[4], c[0], c[0], c[1], c[2], c[3]), c[5]) for c in CONV.values() for dt in c[9]]
    full = [_assert_walks(d, bn) for d, bn in descs]
    L.set_cu_reserve(128)
    assert L.get_cu_reserve() == 128
    assert [_assert_walks(d, bn) for d, bn in descs] == full


def test_conv5_channel_windows_of_wider_buffers_over_several_trips():
    """lu32 in bf16: x a window of a wider buffer (ldx > Cin), y a window of a wider buffer (ldy > Nout); with statistics.
    Nothing outside y's window changes"""
    dt = BF16
    Cin, Nout, _, k, shape, bn, *_ = CONV["lu32"]
    N, H, W = shape
    x, wp, b, prod = _int_conv("lu32")
    ref = _round_store(prod, dt, b)
    ldx, xo, ldy, yo = Cin + 40, 24, Nout + 96, 64
    xbuf = torch.full((N * H * W, ldx), 5.0)                  # a neighbour read by mistake would show in every sum
    xbuf[:, xo:xo + Cin] = x
    gm = _assert_walks(_c5_desc(dt, shape, Cin, ldx, Nout, ldy, k), bn)
    xa = Act(xbuf.to(dt).to(DEV), xo, Cin, N, H, W)
    ybuf = torch.full((N * H * W, ldy), SENTINEL, dtype=dt, device=DEV)
    stats = ops.conv5x5(xa, wp.to(dt).to(DEV), b.to(DEV), Act(ybuf, yo, Nout, N, H, W), want_stats=True)
    got = ybuf.cpu()
    assert torch.equal(got[:, yo:yo + Nout], ref), _where(got[:, yo:yo + Nout], ref, gm)
    assert bool((got[:, :yo] == SENTINEL).all()) and bool((got[:, yo + Nout:] == SENTINEL).all())
    _check_stats(stats, ref, gm)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", ["lu32", "lu64", "n200"])
def test_conv5_normal_operands_against_float64_over_several_trips(name, dt):
    """one case per instantiation: randn operands rounded to the run dtype, float64 on the CPU"""
    Cin, Nout, _, k, shape, bn, *_ = CONV[name]
    N, H, W = shape
    g = torch.Generator().manual_seed(Cin + Nout)
    x = torch.randn(N, Cin, H, W, generator=g).to(dt)
    w = (torch.randn(Nout, Cin, k, k, generator=g) / (5.0 * Cin ** 0.5)).to(dt)
    b = torch.randn(Nout, generator=g)
    gm = _assert_walks(_c5_desc(dt, shape, Cin, Cin, Nout, Nout, k), bn)
    xa = Act(nhwc(x).to(DEV), 0, Cin, N, H, W)
    y = ops.new_act(N, H, W, Nout, dt, DEV)
    y.buf.fill_(float("nan"))
    stats = ops.conv5x5(xa, _pack5(w).to(DEV), b.to(DEV), y, want_stats=True)
    ref = nhwc(F.conv2d(x.double(), w.double(), b.double(), padding=2))
    _close2("y vs float64", y.buf, ref, 1e-4 if dt == F32 else 2.0 ** -8, 1e-5 if dt == F32 else 1.2e-2)
    # sums of the stored values, against sum |y| and sum y^2: a thread's partial is a chain of 16 TM <= 32 additions per trip
    # over three trips, then one shuffle and WM <= 4 rows in LDS: ~100 roundings of 2^-24 = 6e-6 of the sum of magnitudes at
    # the very worst, under the 1e-5 asked here
    assert stats.shape == (gm, 2, Nout)
    s = stats.double().sum(0).cpu()
    yd = y.buf.double().cpu()
    assert ((s[0] - yd.sum(0)).abs() <= 1e-5 * yd.abs().sum(0)).all()
    assert ((s[1] - (yd * yd).sum(0)).abs() <= 1e-5 * (yd * yd).sum(0)).all()


# ---- 2. wgrad5_kernel at its unclipped split ---------------------------------------------------------------------------
def _w5_plan(dt, P, Ci, Cj):
    """(wanted split, split before the chunk is rounded, chunk, split, BKP) as w5_plan of uz_conv5x5.hip decides:
        b = (Ci <= 32 && Cj <= 32) ? 32 : 64;  base = ceil(Ci / b) * ceil(Cj / b) * 25;
        split = ceil(4 * UZ_NUM_CU_HW / base), clipped to min(64, max(1, P / (4 * BKP)));
        chunk = ceil(P / split) rounded up to BKP;  split = ceil(P / chunk)"""
    bkp = 64 if dt == BF16 else 32
    b = 32 if (Ci <= 32 and Cj <= 32) else 64
    base = cdiv(Ci, b) * cdiv(Cj, b) * 25
    want = cdiv(4 * CUS_HW, base)
    split0 = max(1, min(want, 64, max(1, P // (4 * bkp))))
    chunk = cdiv(cdiv(P, split0), bkp) * bkp
    return want, split0, chunk, cdiv(P, chunk), bkp


# name: (map, Ci, CiOut, Cj, dtypes)
WGRAD = {
    # 39 ranges of 320 pixels; W = 67 > BKP: the single-wrap branch of `rw += BKP`; image boundaries inside a K-step
    "c32": ((3, 61, 67), 32, 32, 32, DTYPES),
    "c64": ((3, 61, 67), 64, 64, 64, DTYPES),                 # the 64-wide tile
    "c128": ((3, 61, 67), 128, 128, 128, DTYPES),             # 2 x 2 tiles, split 11
    "c64x32": ((3, 61, 67), 64, 64, 32, DTYPES),              # channel tail inside the tile
    "out3": ((3, 61, 67), 8, 3, 32, DTYPES),                  # the output layer: L an 8-column zero-padded gradient
    # W = 2 * BKP + 2 (bf16); 3 x 3 tiles so that the wanted split (5) fits 1560 pixels unclipped
    "w130": ((2, 6, 130), 192, 192, 192, DTYPES),
    "map131k": (MAP_131K, 32, 32, 32, DTYPES),                # 41 ranges of 3264 pixels (bf16), 51 K-steps each
}


def _wgrad_operands(name):
    (N, H, W), Ci, CiOut, Cj, _ = WGRAD[name]
    g = torch.Generator().manual_seed(Ci * 100 + Cj + H)
    dy = ints(g, (N, CiOut, H, W), -2, 2)
    x = ints(g, (N, Cj, H, W), -2, 2)
    assert 4 * N * H * W < 2 ** 24                            # |sum| <= 4 P: every fp32 sum is exact
    ref = torch.nn.grad.conv2d_weight(x, (CiOut, Cj, 5, 5), dy, padding=2)
    L8 = torch.zeros((N * H * W, Ci))
    L8[:, :CiOut] = nhwc(dy)
    return L8, nhwc(x), ref


def _assert_unclipped(dt, shape, Ci, ldl, Cj, ldr, CiOut):
    N, H, W = shape
    P = N * H * W
    want, split0, chunk, split, bkp = _w5_plan(dt, P, Ci, Cj)
    assert split0 == want, (split0, want)                     # the plan's own split, not the clip to P / (4 BKP)
    assert split == cdiv(P, chunk) and split >= 2
    assert (P % chunk) % bkp != 0, (P, chunk, bkp)            # the last range ends inside a K-step
    d = L.Wgrad5Desc(L.dtype_code(dt), N, H, W, Ci, ldl, Cj, ldr, 5, CiOut, Cj)
    wsb = L.check_count(L.load().uz_wgrad5x5_workspace_bytes(byref(d)), "uz_wgrad5x5_workspace_bytes")
    assert wsb == split * 25 * Ci * Cj * 4, (wsb, split)


@pytest.mark.parametrize("name,dt", [pytest.param(n, dt, id=f"{n}-{_id(dt)}") for n, c in WGRAD.items() for dt in c[4]])
def test_wgrad5_is_exact_on_integers_at_its_unclipped_split(name, dt):
    shape, Ci, CiOut, Cj, _ = WGRAD[name]
    N, H, W = shape
    Lt, Rt, ref = _wgrad_operands(name)
    _assert_unclipped(dt, shape, Ci, Ci, Cj, Cj, CiOut)
    la = Act(Lt.to(dt).to(DEV), 0, Ci, N, H, W)
    ra = Act(Rt.to(dt).to(DEV), 0, Cj, N, H, W)
    dw = ops.wgrad5x5(la, ra, (CiOut, Cj, 5, 5))
    got = dw.cpu()
    assert torch.equal(got, ref), (f"{(got != ref).sum().item()} of {ref.numel()} differ, taps "
                                   f"{torch.unique((got != ref).nonzero()[:, 2:], dim=0)[:6].tolist()}, "
                                   f"max |diff| {(got - ref).abs().max().item():g}")
    assert torch.equal(ops.wgrad5x5(la, ra, (CiOut, Cj, 5, 5)), dw)


def test_wgrad5_channel_windows_of_poisoned_buffers():
    """bf16, both operands windows of wider buffers full of NaN: the clamped loads stay inside the windows"""
    dt = BF16
    shape, Ci, CiOut, Cj, _ = WGRAD["c32"]
    N, H, W = shape
    Lt, Rt, ref = _wgrad_operands("c32")
    ldl, lo, ldr, ro = Ci + 40, 24, Cj + 16, 8
    lbuf = torch.full((N * H * W, ldl), float("nan"))
    lbuf[:, lo:lo + Ci] = Lt
    rbuf = torch.full((N * H * W, ldr), float("nan"))
    rbuf[:, ro:ro + Cj] = Rt
    _assert_unclipped(dt, shape, Ci, ldl, Cj, ldr, CiOut)
    dw = ops.wgrad5x5(Act(lbuf.to(dt).to(DEV), lo, Ci, N, H, W), Act(rbuf.to(dt).to(DEV), ro, Cj, N, H, W), (Ci, Cj, 5, 5))
    got = dw.cpu()
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, ref), f"max |diff| {(got - ref).abs().max().item():g}"


# ---- 3. BatchNorm + ELU passes beyond one workgroup -----------------------------------------------------------------------
# (act1, act2, res, out2) as test_conv5x5_gpu.py names them
COMBOS = {"lu": (True, False, False, False), "res_do": (True, True, True, True)}


def _be_vec(dt, C, lds):
    vec = 8 if dt == BF16 else 4
    return vec if C % vec == 0 and all(ld % vec == 0 for ld in lds) else 1


def _be_reduce_shape(CC, P):
    """(bx, by, gx, gy) as be_reduce_shape decides: bx = the power of two >= CC, at most 64; by = 256 / bx;
    gy = ceil(CC / bx); gx = ceil(P / (8 by)) capped at 2 * UZ_NUM_CU_HW / gy: one partial row per gx"""
    bx = 1
    while bx < CC and bx < 64:
        bx <<= 1
    by = 256 // bx
    gy = cdiv(CC, bx)
    gx = max(1, min(cdiv(P, by * 8), max(1, 2 * CUS_HW // gy)))
    return bx, by, gx, gy


def _be_grid(total):
    """workgroups of 256 threads of the three element passes: ceil(total / 256) capped at 8 * UZ_NUM_CU_HW"""
    return max(1, min(cdiv(total, 256), 8 * CUS_HW))


def _elu_ref(t, on):
    return F.elu(t) if on else t


def _rnd(t, dt):
    return t.to(dt).double()


def _bn_elu_case(shape, C, ld, dt, combo, windows=False):
    """forward and backward of one BatchNorm + ELU block against the float64 autograd oracle; returns
    (V, (bx, by, rows, gy), workgroups of an element pass, its elements) for the caller's assertions on the plan"""
    act1, act2, has_res, has_out2 = COMBOS[combo]
    N, H, W = shape
    P = N * H * W
    g = torch.Generator().manual_seed(C * 7 + P)
    mk = lambda: torch.randn(P, C, generator=g)   # noqa: E731
    nan = float("nan")

    def as_act(t, width=ld, off=0, fill=0.0):
        buf = torch.full((P, width), fill, dtype=dt, device=DEV)
        buf[:, off:off + C] = t.to(DEV)
        return Act(buf, off, C, N, H, W)

    def outside(a, fill):
        """everything but a's window still holds `fill`"""
        rest = torch.cat([a.buf[:, :a.off], a.buf[:, a.off + C:]], 1)
        return bool((rest == fill).all())

    # g0 carries a mean: dbeta and dgamma are then of the order of the sum of their terms' magnitudes, which is what their
    # bound is taken against -- with zero-mean gradients a partial row that went missing would hide under that bound in bf16
    x, res, g0, g1, g2 = mk() * 1.5 + 0.3, mk(), mk() + 0.75, mk(), mk()
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    mask = (torch.rand(N, C, generator=g) >= 0.5).float() * 2.0
    xa = as_act(x)
    xs = xa.buf[:, :C].double()
    stats = torch.stack([xs.sum(0), (xs * xs).sum(0)]).float().reshape(1, 2, C).contiguous()
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    vec = ops.bn_finalize(stats, P, gamma.to(DEV), beta.to(DEV), 1e-5, 0.1, rm, rv)
    zero = torch.zeros(P, C)
    if windows:      # VNet's up path: out and the dropped skip copy are the halves of one concat buffer
        assert has_res and has_out2 and ld == C
        cat = torch.full((P, 2 * C), nan, dtype=dt, device=DEV)
        out, out2 = Act(cat, 0, C, N, H, W), Act(cat, C, C, N, H, W)
        ra = as_act(res, C + 40, 24, nan)
        g0a = as_act(g0, C + 16, 8, nan)
        dx, gres = as_act(zero, C + 24, 16, SENTINEL), as_act(zero, C + 8, 8, SENTINEL)
        dx.buf[:, dx.off:dx.off + C] = SENTINEL
        gres.buf[:, gres.off:gres.off + C] = SENTINEL
    else:
        out, out2 = as_act(zero), (as_act(zero) if has_out2 else None)
        ra = as_act(res) if has_res else None
        g0a = as_act(g0)
        dx, gres = as_act(zero), (as_act(zero) if has_res else None)
    g1a, g2a = as_act(g1), (as_act(g2) if has_out2 else None)
    mdev = mask.to(DEV) if has_out2 else None
    ops.bn_elu_apply(xa, vec[0], vec[1], out, act1=act1, act2=act2, res=ra, out2=out2, mask2=mdev)

    # float64 oracle on the (rounded) operands, gradients by autograd THROUGH the batch statistics
    xr = _rnd(x, dt).requires_grad_(True)
    rr = _rnd(res, dt).requires_grad_(True)
    gm, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    mean, var = xr.mean(0), xr.var(0, unbiased=False)
    xhat = (xr - mean) / torch.sqrt(var + 1e-5)
    bnout = xhat * gm + bt
    bnout.retain_grad()
    o = _elu_ref(_elu_ref(bnout, act1) + (rr if has_res else 0.0), act2)
    mfull = mask.double().repeat_interleave(H * W, dim=0)
    tol = 1e-4 if dt == F32 else 2.0 ** -7
    _close2("out", out.buf[:, out.off:out.off + C], o.detach(), tol)
    if has_out2:
        _close2("out2", out2.buf[:, out2.off:out2.off + C], (o * mfull).detach(), tol)
    G = _rnd(g0, dt) + _rnd(g1, dt) + (_rnd(g2, dt) * mfull if has_out2 else 0.0)
    o.backward(G)

    d = L.BnEluBwdDesc(L.dtype_code(dt), N, H * W, C, xa.ld, out.ld, g0a.ld, g1a.ld, g2a.ld if g2a is not None else 0,
                       dx.ld, gres.ld if gres is not None else 0, int(act1) | (2 if act2 else 0))
    V = _be_vec(dt, C, [getattr(d, n) for n in ("ldx", "ldo", "ldg0", "ldg1", "ldg2", "lddx", "ldgres")])
    shape_r = _be_reduce_shape(C // V, P)
    assert L.check_count(L.load().uz_bn_elu_bwd_rows(byref(d)), "uz_bn_elu_bwd_rows") == shape_r[2]

    sums = torch.empty((2, C), dtype=torch.float64, device=DEV)
    dgamma, dbeta = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    runs = []
    for _ in range(2):
        ops.bn_elu_bwd(xa, vec, out, g0a, g1a, g2a, mdev, sums, dx, gres, dgamma, dbeta, act1=act1, act2=act2)
        torch.cuda.synchronize()
        runs.append((dx.buf.clone(), dgamma.clone(), dbeta.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    _close2("dx", dx.buf[:, dx.off:dx.off + C], xr.grad, tol)
    _close_sum("dgamma", dgamma, gm.grad, (bnout.grad * xhat.detach()).abs().sum(0), tol)
    _close_sum("dbeta", dbeta, bt.grad, bnout.grad.abs().sum(0), tol)
    if has_res:
        _close2("gres", gres.buf[:, gres.off:gres.off + C], rr.grad, tol)
    if windows:
        assert outside(dx, SENTINEL) and outside(gres, SENTINEL)
        # the halves of the concat buffer after the backward pass has read one of them: both as the forward left them
        _close2("out (after)", cat[:, :C], o.detach(), tol)
        _close2("out2 (after)", cat[:, C:], (o * mfull).detach(), tol)
    return V, shape_r, _be_grid(P * (C // V)), P * (C // V)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("combo", ["res_do", "lu"])
@pytest.mark.parametrize("C", [32, 256])
def test_bn_elu_several_partial_rows(C, combo, dt):
    shape = (2, 37, 41)
    V, (bx, by, rows, gy), _, _ = _bn_elu_case(shape, C, C, dt, combo)
    P = shape[0] * shape[1] * shape[2]
    assert V == (8 if dt == BF16 else 4) and gy == 1
    assert rows >= 2 and cdiv(P, rows * by) > 1, (rows, by)          # several rows, several pixels per thread


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_bn_elu_channel_windows_of_a_concat_buffer(dt):
    V, (bx, by, rows, gy), _, _ = _bn_elu_case((2, 37, 41), 32, 32, dt, "res_do", windows=True)
    assert V == (8 if dt == BF16 else 4) and rows >= 2


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_bn_elu_strided_element_passes(dt):
    """P * C / V = 1052576 vector elements >= 2 * (8 * 256 workgroups * 256 threads): every thread of the three element
    passes strides at least once, some twice"""
    C = 64 if dt == BF16 else 32
    V, (bx, by, rows, gy), grid, total = _bn_elu_case(MAP_131K, C, C, dt, "res_do")
    assert grid == 8 * CUS_HW and total >= 2 * grid * 256, (grid, total)
    assert rows == 2 * CUS_HW


def test_bn_elu_thin_path_strides():
    """C = 1 in 8-column buffers (the num_classes-wide output layer), scalar path: 525312 elements, 1024 more than the
    8 * 256 * 256 threads of an element pass"""
    V, (bx, by, rows, gy), grid, total = _bn_elu_case((2, 513, 512), 1, 8, BF16, "lu")
    assert V == 1 and (bx, by) == (1, 256)
    assert grid == 8 * CUS_HW and total > grid * 256, (grid, total)
    assert rows >= 2


def test_bn_elu_two_channel_groups():
    """fp32, C = 512: 128 channel chunks, blockIdx.y in {0, 1}"""
    V, (bx, by, rows, gy), _, _ = _bn_elu_case((2, 9, 11), 512, 512, F32, "lu")
    assert V == 4 and (bx, gy) == (64, 2) and rows >= 2
