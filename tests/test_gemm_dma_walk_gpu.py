"""GPU: gemm_dma_kernel of uz_gemm_dma.hip where every workgroup makes SEVERAL trips through its tile loop.

The kernel's workgroups are persistent: uz_gemm_dma_plan / gemm_nt_plan cap grid_m at CUs / tiles_n (twice that for the
two-stage form) and the kernel runs `for (tile = blockIdx.x; tile < a.tiles_m; tile += gridDim.x)`.  What only a second trip
executes: the bf16 epilogue's prefetch of the next tile's first PRE K slabs under the staging area (PRE from SC_OFF against
STAGE: <128,256,3> 1, <64,256,3> 2, <64,256,2> 1, <128,128,2> 0), the `pre` the next trip skips by, the s_waitcnt vmcnt counts
that assume exactly those loads in flight, the barrier at the top of a trip, and the statistics / BatchNorm-backward sums that
live in registers across trips.  The other tests of this kernel (test_ops_gpu.py, test_c_ref_gpu.py, test_c_ref_r5_gpu.py,
test_gemm_splitk_gpu.py, test_token_attention_gpu.py) stay at M <= 4096: tiles_m <= grid_m, one trip.

Here uz_set_cu_reserve(128) leaves the plans 128 CUs, and every case asserts, before it compares anything, that
  * the library names the LDS-DMA GEMM for the descriptor and asks for no workspace (not the split-K form, one tile each),
  * uz_conv_igemm_grid_m() is the cap of the plan as restated in _plan() below, for the instantiation the case claims,
  * ceil(M / bm) >= 2 * grid_m + 1: every workgroup makes at least two trips and some make three,
  * M % 256 != 0 and M % 128 != 0: the last trip of some workgroup is a partial tile.
uz_gemm_nt has no query; its cases stand on the restatement of gemm_nt_plan alone (the same rule with
per = tiles_n * batch * batch2 in place of tiles_n).

References:
  1. integer operands (x, w from {-1, 0, 1}, integer bias and residual): every fp32 sum is exact whatever the order, so the
     result must be the float64 product rounded once to the run dtype, bit for bit; the residual a separate add of the
     stored result (as test_gemm_splitk_gpu.py);
  2. statistics / BNRED partial rows summed in float64 against the float64 column sums of the reference, exactly: the test
     first asserts from the reference alone that sum |y| and sum y^2 (sum |dz y|) of every column stay below 2^24, so no fp32
     partial sum can round however the tiles are dealt to workgroups;
  3. normal operands, one case per instantiation: float64 on dtype-rounded inputs to the tolerances of
     test_token_attention_gpu.py for this kernel (1e-5 fp32, 1.2e-2 bf16, max error over max magnitude), and bit for bit
     against the same call under uz_set_cu_reserve(0) -- the same tiles on half as many trips.

No case for the <128,128,4> form: both plans take it only when bn == 128 and 2 * ceil(M / 256) * per <= CUs (per = tiles_n,
times the matrix count for uz_gemm_nt).  Then
    tiles_m = ceil(M / 128) <= 2 * ceil(M / 256) <= floor(CUs / per) = cap,
so grid_m = tiles_m: the form never walks and its PRE = 2 branch cannot be reached through the ABI."""
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
RESERVE = 128
CUS = 256 - RESERVE
SENTINEL = -77.0                 # exact in bf16; no case can produce it where it is looked for


@pytest.fixture(autouse=True)
def _restore():
    yield
    L.set_cu_reserve(0)


@pytest.fixture(scope="module", autouse=True)
def _free_references():
    yield
    _int_1x1.cache_clear()
    _gather_case.cache_clear()


def cdiv(a, b):
    return -(-a // b)


def relerr(a, b):
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30)).item()


def _plan(dt, M, Nout, Cin, ntaps=1, *, cus=CUS, mats=1, shuffle_co=None):
    """(bn, bm, nst, tiles_m, grid_m) as uz_gemm_dma_plan and gemm_nt_plan (mats = batch * batch2) of uz_gemm_dma.hip decide:
        p->bn = Nout <= 64 ? 64 : 128;     shuffle store: Co % 128 == 0 -> 128, Co % 64 == 0 -> 64, else (bf16) as above
        p->tiles_n = (Nout + p->bn - 1) / p->bn;                        per = tiles_n [* batch * batch2]
        p->bm = (p->bn == 128 && ((M + 255) / 256) * per * 2 <= UZ_NUM_CU) ? 128 : 256;
        nsteps = ntaps * ((Cin + 8 * vec - 1) / (8 * vec));             vec = 8 bf16, 4 fp32
        p->nst = p->bm == 128 ? 4 : 3;
        if (p->bn == 128 && nsteps <= 2) { p->bm = 128; p->nst = 2; }
        if (p->bn == 64 && nsteps <= 2) p->nst = 2;
        p->tiles_m = (M + p->bm - 1) / p->bm;
        cap = (p->nst == 2 ? 2 : 1) * UZ_NUM_CU / per;                   (at least 1)
        p->grid_m = min(tiles_m, cap)"""
    bn = 64 if Nout <= 64 else 128
    if shuffle_co is not None:
        bn = 128 if shuffle_co % 128 == 0 else (64 if shuffle_co % 64 == 0 else bn)
    per = cdiv(Nout, bn) * mats
    bm = 128 if (bn == 128 and cdiv(M, 256) * per * 2 <= cus) else 256
    nsteps = ntaps * cdiv(Cin, 64 if dt == BF16 else 32)
    nst = 4 if bm == 128 else 3
    if nsteps <= 2:
        bm, nst = (128 if bn == 128 else bm), 2
    tiles_m = cdiv(M, bm)
    cap = max(1, (2 if nst == 2 else 1) * cus // per)
    return bn, bm, nst, tiles_m, min(tiles_m, cap)


def _assert_walks(d, dt, form, *, shuffle_co=None):
    """the descriptor is an unsplit LDS-DMA GEMM of the instantiation `form` = (bn, bm, nst) under the reserve in force, and
    every workgroup makes at least two trips, some three, one of them over a partial tile; returns (bm, grid_m)"""
    lib = L.load()
    M = d.N * d.H * d.W
    name = ops.conv_kernel_name(d)
    assert name.startswith("gemm_dma"), name
    assert L.check_count(lib.uz_conv_igemm_workspace_bytes(byref(d)), "workspace") == 0
    gm = L.check_count(lib.uz_conv_igemm_grid_m(byref(d)), "grid_m")
    bn, bm, nst, tiles_m, grid = _plan(dt, M, d.Nout, d.Cin, d.ntaps, shuffle_co=shuffle_co)
    assert (bn, bm, nst) == form, ((bn, bm, nst), form)
    assert gm == grid, (gm, grid)
    assert tiles_m >= 2 * gm + 1, (tiles_m, gm)
    assert M % 256 != 0 and M % 128 != 0
    return bm, gm


def _where(got, ref, bm, gm):
    """which rows of a (M, n) result differ, as tiles and trips: a wrong prefetch shows in trips >= 1 only"""
    bad = (got != ref).any(1).nonzero().flatten()
    if bad.numel() == 0:
        return "equal"
    tiles = torch.unique(bad // bm)
    trips = torch.unique(tiles // gm).tolist()
    return (f"{bad.numel()} of {got.shape[0]} rows differ, in {tiles.numel()} tiles of {bm} rows (first {tiles[:6].tolist()}), "
            f"trips {trips} of a grid of {gm}; max |diff| {(got.double() - ref.double()).abs().max().item():g}")


def ints(g, shape, lo=-1, hi=1):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _round_store(prod64, dt, bias=None, res=None):
    """the exact sum rounded once to the run dtype; the residual a separate add of the stored result"""
    y = (prod64 + bias.double()) if bias is not None else prod64
    y = y.to(dt)
    if res is not None:
        y = (y.float() + res.float()).to(dt)
    return y


def _assert_sums_exact(ref, sq_of=None):
    """precondition of the exact statistics check, from the reference alone: no fp32 partial sum of a column can round"""
    r = ref.double()
    other = r if sq_of is None else sq_of.double()
    assert r.abs().sum(0).max().item() < 2 ** 24 and (r * other).abs().sum(0).max().item() < 2 ** 24


def _check_stats(stats, ref, gm):
    """partial rows (gm, 2, n) of sum y and sum y^2 over the STORED values, summed in float64: exact"""
    assert stats.shape == (gm, 2, ref.shape[1])
    _assert_sums_exact(ref)
    s = stats.double().sum(0).cpu()
    r = ref.double()
    assert torch.equal(s[0], r.sum(0)), f"sum y: {(s[0] - r.sum(0)).abs().max().item():g} off"
    assert torch.equal(s[1], (r * r).sum(0)), f"sum y^2: {(s[1] - (r * r).sum(0)).abs().max().item():g} off"


def _desc(dt, N, H, W, Hin, Win, Cin, ldx, Nout, ldy, ntaps=1, taps=L.TAPS_CONV, dil=1, store=L.STORE_PLAIN, co=0, Hd=0, Wd=0):
    return L.ConvDesc(L.dtype_code(dt), N, H, W, Hin, Win, Cin, ldx, Nout, ldy, ntaps, taps, dil, store, co, Hd, Wd)


def nhwc(t):
    """(N, C, H, W) -> (N H W, C)"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


# ---- 1x1 products: cases a - e and j --------------------------------------------------------------------------------------
MAP_33K = (2, 130, 127)          # M = 33020 = 128 * 256 + 252 = 257 * 128 + 124
MAP_66K = (2, 182, 181)          # M = 65884 = 257 * 256 + 92
MAP_131K = (2, 259, 254)         # M = 131572 = 513 * 256 + 244


@functools.lru_cache(maxsize=1)
def _int_1x1(Cin, Nout, shape):
    """integer operands of a 1x1 product and its float64 result, shared by the variants of a shape (which follow each other)"""
    N, H, W = shape
    g = torch.Generator().manual_seed(Cin * 1000 + Nout)
    x = ints(g, (N * H * W, Cin))
    w = ints(g, (Nout, Cin))
    b = ints(g, (Nout,), -3, 3)
    r = ints(g, (N * H * W, Nout), -8, 8)
    return x, w, b, r, x.double() @ w.double().t()


# name: (Cin, Nout, map, (bn, bm, nst), bias, want_stats, res, dtypes)
ONE_BY_ONE = {
    # a: <128,256,3>, PRE = 1; three slabs in bf16 (all of them in the ring: the prefetched stage 0 lies under no stage in use), six in fp32
    "a_bias": (192, 256, MAP_33K, (128, 256, 3), True, False, False, DTYPES),
    "a_stats": (192, 256, MAP_33K, (128, 256, 3), False, True, False, DTYPES),
    "a_res": (192, 256, MAP_33K, (128, 256, 3), True, False, True, DTYPES),
    # b: partial last K slab (200 = 3 * 64 + 8 = 6 * 32 + 8), partial last N tile (200 = 128 + 72), partial last M tile
    "b_ragged_stats": (200, 200, MAP_33K, (128, 256, 3), True, True, False, DTYPES),
    "b_ragged_res": (200, 200, MAP_33K, (128, 256, 3), True, False, True, DTYPES),
    # c: <128,128,2>, PRE = 0, two workgroups per CU: one slab (bf16 Cin 64; fp32 Cin 32) and two (bf16 Cin 96; fp32 Cin 64)
    "c_cin64_stats": (64, 256, MAP_33K, (128, 128, 2), True, True, False, DTYPES),
    "c_cin64_res": (64, 256, MAP_33K, (128, 128, 2), True, False, True, DTYPES),
    "c_cin96_stats": (96, 256, MAP_33K, (128, 128, 2), True, True, False, [BF16]),
    "c_cin32_stats": (32, 256, MAP_33K, (128, 128, 2), True, True, False, [F32]),
    # d: <64,256,3>, PRE = 2 with nsteps = 3 (bf16) / 6 (fp32)
    "d_stats": (192, 64, MAP_66K, (64, 256, 3), True, True, False, DTYPES),
    "d_res": (192, 64, MAP_66K, (64, 256, 3), True, False, True, DTYPES),
    # e: <64,256,2>, PRE = 1: nsteps = 1 never issues a second stage (K = 32: the im2col'd first convolution), nsteps = 2
    # issues it at the top of the next trip (bf16 K = 128; fp32 K = 64)
    "e_k32_stats": (32, 64, MAP_131K, (64, 256, 2), True, True, False, DTYPES),
    "e_k128_stats": (128, 64, MAP_131K, (64, 256, 2), True, True, False, [BF16]),
    "e_k128_res": (128, 64, MAP_131K, (64, 256, 2), True, False, True, [BF16]),
    "e_k64_stats": (64, 64, MAP_131K, (64, 256, 2), True, True, False, [F32]),
}
ONE_BY_ONE_PARAMS = [pytest.param(n, dt, id=f"{n}-{DT_IDS[DTYPES.index(dt)]}") for n, c in ONE_BY_ONE.items() for dt in c[7]]


@pytest.mark.parametrize("name,dt", ONE_BY_ONE_PARAMS)
def test_1x1_product_is_exact_on_integers_over_several_trips(name, dt):
    Cin, Nout, shape, form, with_bias, want_stats, with_res, _ = ONE_BY_ONE[name]
    N, H, W = shape
    x, w, b, r, prod = _int_1x1(Cin, Nout, shape)
    ref = _round_store(prod, dt, b if with_bias else None, r if with_res else None)
    L.set_cu_reserve(RESERVE)
    bm, gm = _assert_walks(_desc(dt, N, H, W, H, W, Cin, Cin, Nout, Nout), dt, form)
    xa = Act(x.to(dt).to(DEV), 0, Cin, N, H, W)
    ra = Act(r.to(dt).to(DEV), 0, Nout, N, H, W) if with_res else None
    wd, bd = w.to(dt).to(DEV), (b.to(DEV) if with_bias else None)
    y = ops.new_act(N, H, W, Nout, dt, DEV)
    y.buf.fill_(SENTINEL)
    stats = ops.conv_igemm(xa, wd, bd, y, ntaps=1, want_stats=want_stats, res=ra)
    got = y.buf.cpu()
    assert torch.equal(got, ref), _where(got, ref, bm, gm)
    if want_stats:
        _check_stats(stats, ref, gm)
    y2 = ops.new_act(N, H, W, Nout, dt, DEV)
    stats2 = ops.conv_igemm(xa, wd, bd, y2, ntaps=1, want_stats=want_stats, res=ra)
    assert torch.equal(y2.buf, y.buf) and (not want_stats or torch.equal(stats2, stats))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_channel_windows_of_wider_buffers_over_several_trips(dt):
    """case j on shape a: x a window of a wider buffer (ldx > Cin), y a window of a concat buffer (ldy > Nout); with
    statistics.  Nothing outside y's window changes"""
    Cin, Nout, (N, H, W) = 192, 256, MAP_33K
    x, w, b, _, prod = _int_1x1(Cin, Nout, MAP_33K)
    ref = _round_store(prod, dt, b)
    ldx, xo, ldy, yo = Cin + 40, 24, Nout + 96, 64
    xbuf = torch.full((N * H * W, ldx), 5.0)                  # a neighbour read by mistake would show in every sum
    xbuf[:, xo:xo + Cin] = x
    L.set_cu_reserve(RESERVE)
    bm, gm = _assert_walks(_desc(dt, N, H, W, H, W, Cin, ldx, Nout, ldy), dt, (128, 256, 3))
    xa = Act(xbuf.to(dt).to(DEV), xo, Cin, N, H, W)
    ybuf = torch.full((N * H * W, ldy), SENTINEL, dtype=dt, device=DEV)
    y = Act(ybuf, yo, Nout, N, H, W)
    stats = ops.conv_igemm(xa, w.to(dt).to(DEV), b.to(DEV), y, ntaps=1, want_stats=True)
    got = ybuf.cpu()
    assert torch.equal(got[:, yo:yo + Nout], ref), _where(got[:, yo:yo + Nout], ref, bm, gm)
    assert bool((got[:, :yo] == SENTINEL).all()) and bool((got[:, yo + Nout:] == SENTINEL).all())
    _check_stats(stats, ref, gm)


# ---- pixel-shuffle store: case f -----------------------------------------------------------------------------------------
# name: (Cin, Co, map, {dtype: (bn, bm, nst)})
SHUFFLE = {
    # ConvTranspose 128 -> 64: Co % 64 == 0 -> bn 64, four N tiles of one sub-pixel each; two slabs in bf16 (<64,256,2>), four in fp32
    "convt_128_64": (128, 64, MAP_33K, {F32: (64, 256, 3), BF16: (64, 256, 2)}),
    # Co = 96: bn 128, three N tiles that straddle sub-pixels (bf16 only: the per-chunk store); M = 21630 = 84 * 256 + 126
    "convt_192_96": (192, 96, (2, 105, 103), {BF16: (128, 256, 3)}),
}


@pytest.mark.parametrize("name,dt", [pytest.param(n, dt, id=f"{n}-{DT_IDS[DTYPES.index(dt)]}")
                                      for n, c in SHUFFLE.items() for dt in DTYPES if dt in c[3]])
def test_pixel_shuffle_store_over_several_trips(name, dt):
    """ConvTranspose2d(k2, s2) forward into a destination one row and one column larger than 2H x 2W: out_row per trip, the
    sub-pixel decided per chunk; the pad row and column keep the sentinel"""
    Cin, Co, (N, H, W), forms = SHUFFLE[name]
    g = torch.Generator().manual_seed(Cin + Co)
    x = ints(g, (N, Cin, H, W))
    w = ints(g, (Cin, Co, 2, 2))
    b = ints(g, (Co,), -3, 3)
    ref = F.conv_transpose2d(x, w, b, stride=2).double().to(dt)       # (N, Co, 2H, 2W); fp32 on integers: exact
    Hd, Wd = 2 * H + 1, 2 * W + 1
    L.set_cu_reserve(RESERVE)
    d = _desc(dt, N, H, W, H, W, Cin, Cin, 4 * Co, Co, store=L.STORE_SHUFFLE2X2, co=Co, Hd=Hd, Wd=Wd)
    bm, gm = _assert_walks(d, dt, forms[dt], shuffle_co=Co)
    xa = Act(nhwc(x).to(dt).to(DEV), 0, Cin, N, H, W)
    wp = ops.pack_weights(w.to(DEV), L.PACK_CONVT_FWD, dt)
    y = ops.new_act(N, Hd, Wd, Co, dt, DEV)
    y.buf.fill_(SENTINEL)
    ops.conv_igemm(xa, wp, b.repeat(4).to(DEV), y, ntaps=1, store_mode=L.STORE_SHUFFLE2X2, nout=4 * Co, co=Co)
    got = y.buf.cpu().view(N, Hd, Wd, Co)
    want = ref.permute(0, 2, 3, 1)
    inner = got[:, :2 * H, :2 * W]
    if not torch.equal(inner, want):
        # rows of the GEMM: coarse pixel m owns fine pixels (2h + a, 2w + b)
        per_m = (inner != want).any(3).view(N, H, 2, W, 2).any(4).any(2).reshape(-1, 1)
        raise AssertionError(_where(per_m.float(), torch.zeros_like(per_m, dtype=torch.float32), bm, gm))
    assert bool((got[:, 2 * H] == SENTINEL).all()) and bool((got[:, :, 2 * W] == SENTINEL).all())


# ---- 2x2 gather with the BatchNorm-backward reduction: case g --------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _gather_case():
    """gradient of a ConvTranspose2d(256 -> 64, k2, s2) output on a (2 * 130 + 1) x (2 * 127 + 1) grid (the last row and
    column belong to no coarse pixel) and the input gradient over the 2 x 130 x 127 coarse pixels"""
    N, H, W = MAP_33K
    Co, Ci = 64, 256
    g = torch.Generator().manual_seed(7)
    gy = ints(g, (N, Co, 2 * H + 1, 2 * W + 1))
    w = ints(g, (Ci, Co, 2, 2))
    dx = F.conv2d(gy[:, :, :2 * H, :2 * W], w, None, stride=2)        # fp32 on integers: exact
    return gy, w, nhwc(dx).double()


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_conv_transpose_input_gradient_over_several_trips(dt):
    """UZ_TAPS_GATHER2X2, four taps: the tap offsets are recomputed by every issue(), the prefetching one included"""
    N, H, W = MAP_33K
    Co, Ci = 64, 256
    gy, w, prod = _gather_case()
    ref = _round_store(prod, dt)
    L.set_cu_reserve(RESERVE)
    d = _desc(dt, N, H, W, 2 * H + 1, 2 * W + 1, Co, Co, Ci, Ci, ntaps=4, taps=L.TAPS_GATHER2X2)
    bm, gm = _assert_walks(d, dt, (128, 256, 3))
    ga = Act(nhwc(gy).to(dt).to(DEV), 0, Co, N, 2 * H + 1, 2 * W + 1)
    wp = ops.pack_weights(w.to(DEV), L.PACK_CONVT_DGRAD, dt)
    dx = ops.new_act(N, H, W, Ci, dt, DEV)
    dx.buf.fill_(SENTINEL)
    stats = ops.conv_igemm(ga, wp, None, dx, ntaps=4, taps_mode=L.TAPS_GATHER2X2, want_stats=True)
    got = dx.buf.cpu()
    assert torch.equal(got, ref), _where(got, ref, bm, gm)
    _check_stats(stats, ref, gm)


def test_bn_backward_sums_in_the_input_gradient_over_several_trips():
    """uz_conv_igemm_bnred on the same product (bf16): the sums of dz = g * [relu(bn(y)) > 0] and of dz * xhat accumulate in
    registers across trips, one partial row per workgroup; bn_y is loaded between the prefetch and the store.  The four
    channel vectors are given directly: scale = +-1 and shift = 0.5 on integer y leave the mask no ties; integer mean and a
    power of two for invstd make invstd * (sum dz y - mean sum dz) exact"""
    dt = BF16
    N, H, W = MAP_33K
    Co, Ci = 64, 256
    gy, w, prod = _gather_case()
    ref = _round_store(prod, dt)
    g = torch.Generator().manual_seed(8)
    bn_y = ints(g, (N * H * W, Ci), -3, 3)
    scale = ints(g, (Ci,), 0, 1) * 2 - 1
    shift = torch.full((Ci,), 0.5)
    mean = ints(g, (Ci,), -2, 2)
    invstd = 2.0 ** ints(g, (Ci,), -2, 1)
    dz = torch.where(bn_y * scale + shift > 0, ref.float(), torch.zeros(())).double()
    _assert_sums_exact(dz, sq_of=bn_y)
    assert (mean.double() * dz.sum(0)).abs().max().item() < 2 ** 24
    L.set_cu_reserve(RESERVE)
    d = _desc(dt, N, H, W, 2 * H + 1, 2 * W + 1, Co, Co, Ci, Ci, ntaps=4, taps=L.TAPS_GATHER2X2)
    bm, gm = _assert_walks(d, dt, (128, 256, 3))
    assert L.load().uz_conv_igemm_bnred_supported(byref(d))
    ga = Act(nhwc(gy).to(dt).to(DEV), 0, Co, N, 2 * H + 1, 2 * W + 1)
    wp = ops.pack_weights(w.to(DEV), L.PACK_CONVT_DGRAD, dt)
    plain = ops.new_act(N, H, W, Ci, dt, DEV)
    ops.conv_igemm(ga, wp, None, plain, ntaps=4, taps_mode=L.TAPS_GATHER2X2)
    fused = ops.new_act(N, H, W, Ci, dt, DEV)
    fused.buf.fill_(SENTINEL)
    ya = Act(bn_y.to(dt).to(DEV), 0, Ci, N, H, W)
    vec = torch.stack([scale, shift, mean, invstd]).to(DEV)
    part = ops.conv_igemm(ga, wp, None, fused, ntaps=4, taps_mode=L.TAPS_GATHER2X2, bnred=(ya, vec))
    assert part is not None and part.shape == (gm, 2, Ci)
    got = fused.buf.cpu()
    assert torch.equal(got, ref), _where(got, ref, bm, gm)
    assert torch.equal(fused.buf, plain.buf)
    s = part.double().sum(0).cpu()
    want0 = dz.sum(0)
    want1 = invstd.double() * ((dz * bn_y.double()).sum(0) - mean.double() * want0)
    assert torch.equal(s[0], want0), f"sum dz: {(s[0] - want0).abs().max().item():g} off"
    assert torch.equal(s[1], want1), f"sum dz xhat: {(s[1] - want1).abs().max().item():g} off"


# ---- nine taps: cases h and i -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("form", ["stride2", "dilated2"])
def test_nine_tap_products_over_several_trips(form, dt):
    """h: UZ_TAPS_CONV_S2 (Conv2d k3 s2 p1) on odd Hin x Win: zero rows at the right and bottom border on later trips too.
    i: the dilated form (dilation 2, padding 2), unsplit.  Both with statistics; F.conv2d in fp32 on integers is exact"""
    N, H, W = MAP_33K
    Cin, Nout = 64, 256
    g = torch.Generator().manual_seed(len(form))
    if form == "stride2":
        Hin, Win, taps, dil = 2 * H - 1, 2 * W - 1, L.TAPS_CONV_S2, 1
    else:
        Hin, Win, taps, dil = H, W, L.TAPS_CONV, 2
    x = ints(g, (N, Cin, Hin, Win))
    w = ints(g, (Nout, Cin, 3, 3))
    b = ints(g, (Nout,), -3, 3)
    if form == "stride2":
        prod = F.conv2d(x, w, None, stride=2, padding=1)
    else:
        prod = F.conv2d(x, w, None, padding=2, dilation=2)
    assert prod.shape == (N, Nout, H, W)
    ref = _round_store(nhwc(prod).double(), dt, b)
    L.set_cu_reserve(RESERVE)
    bm, gm = _assert_walks(_desc(dt, N, H, W, Hin, Win, Cin, Cin, Nout, Nout, ntaps=9, taps=taps, dil=dil), dt, (128, 256, 3))
    xa = Act(nhwc(x).to(dt).to(DEV), 0, Cin, N, Hin, Win)
    wp = ops.pack_weights(w.to(DEV), L.PACK_CONV_FWD, dt)
    y = ops.new_act(N, H, W, Nout, dt, DEV)
    y.buf.fill_(SENTINEL)
    stats = ops.conv_igemm(xa, wp, b.to(DEV), y, ntaps=9, dil=dil, taps_mode=taps, want_stats=True)
    got = y.buf.cpu()
    assert torch.equal(got, ref), _where(got, ref, bm, gm)
    _check_stats(stats, ref, gm)


# ---- normal operands, one case per instantiation: reference 3 ---------------------------------------------------------------
# name: ({dtype: Cin}, Nout, map, (bn, bm, nst))
RANDOM = {
    "128x256x3": ({F32: 192, BF16: 192}, 256, MAP_33K, (128, 256, 3)),
    "128x128x2": ({F32: 64, BF16: 96}, 256, MAP_33K, (128, 128, 2)),
    "64x256x3": ({F32: 192, BF16: 192}, 64, MAP_66K, (64, 256, 3)),
    "64x256x2": ({F32: 64, BF16: 128}, 64, MAP_131K, (64, 256, 2)),
}


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", list(RANDOM))
def test_normal_operands_against_float64_and_against_half_as_many_trips(name, dt):
    """a tile's value must not depend on which trip computed it: the launch under the reserve equals the launch on the whole
    chip (the same tiles, half as many trips) bit for bit, statistics apart (their rows are summed in another order)"""
    cins, Nout, (N, H, W), form = RANDOM[name]
    Cin = cins[dt]
    g = torch.Generator().manual_seed(Cin + Nout)
    x = torch.randn(N * H * W, Cin, generator=g).to(dt)
    w = (torch.randn(Nout, Cin, generator=g) * 0.1).to(dt)
    b = torch.randn(Nout, generator=g)
    xa = Act(x.to(DEV), 0, Cin, N, H, W)
    wd, bd = w.to(DEV), b.to(DEV)

    def run():
        y = ops.new_act(N, H, W, Nout, dt, DEV)
        y.buf.fill_(float("nan"))
        return y.buf, ops.conv_igemm(xa, wd, bd, y, ntaps=1, want_stats=True)

    full_chip, _ = run()
    L.set_cu_reserve(RESERVE)
    bm, gm = _assert_walks(_desc(dt, N, H, W, H, W, Cin, Cin, Nout, Nout), dt, form)
    got, stats = run()
    assert torch.equal(got, full_chip), _where(got.cpu(), full_chip.cpu(), bm, gm)
    ref = x.double() @ w.double().t() + b.double()
    e = relerr(got.cpu(), ref)
    tol = 1e-5 if dt == F32 else 1.2e-2
    print(f"  y vs float64: {e:.3e} (tolerance {tol:g})")
    assert e < tol, e
    # sums of the stored values, against sum |y| and sum y^2: a thread's partial is a chain of at most 32 additions per trip
    # (fp32 path; 16 in bf16) over three trips, then 4 (bf16: 64) more in the workgroup: ~100 roundings of 2^-24 = 6e-6 of
    # the sum of magnitudes at the very worst, under the 1e-5 asked here
    s = stats.double().sum(0).cpu()
    yd = got.double().cpu()
    assert ((s[0] - yd.sum(0)).abs() <= 1e-5 * yd.abs().sum(0)).all()
    assert ((s[1] - (yd * yd).sum(0)).abs() <= 1e-5 * (yd * yd).sum(0)).all()


# ---- uz_gemm_nt: case k -----------------------------------------------------------------------------------------------------
# name: (batch, batch2, M, N, K, row padding, (bn, bm, nst), cap)
NT = {
    # per = 2 * 16 = 32: cap 4, nine tiles of 256 rows (2100 = 8 * 256 + 52)
    "b16_2100x256x192": (16, 1, 2100, 256, 192, 16, (128, 256, 3), 4),
    # per = 128: cap 1 -- ONE workgroup walks the whole matrix (700 = 2 * 256 + 188)
    "b128_700x64x192": (128, 1, 700, 64, 192, 0, (64, 256, 3), 1),
    # the same with at most two slabs: the two-stage form, cap 2, five tiles (1100 = 4 * 256 + 76)
    "b128_1100x64x64": (128, 1, 1100, 64, 64, 8, (64, 256, 2), 2),
    # 4 images x 8 heads side by side in the channels of one token map (q k^T of an attention): per = 2 * 32, the two-stage form
    # with 128-row tiles, cap 4, nine tiles (1100 = 8 * 128 + 76); N = 136 leaves a partial N tile
    "b4_h8_1100x136x64": (4, 8, 1100, 136, 64, 8, (128, 128, 2), 4),
}


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", list(NT))
def test_gemm_nt_is_exact_on_integers_over_several_trips(name, dt):
    """the bz / bh base offsets combined with the walk; bias + residual; padded row strides keep their sentinel.  uz_gemm_nt
    has no plan query: the walk stands on _plan(), the restatement of gemm_nt_plan"""
    batch, heads, M, N, K, pad, form, cap = NT[name]
    g = torch.Generator().manual_seed(M + N + K)
    L.set_cu_reserve(RESERVE)
    bn, bm, nst, tiles_m, gm = _plan(dt, M, N, K, mats=batch * heads)
    assert (bn, bm, nst) == form and gm == cap, ((bn, bm, nst), gm)
    assert tiles_m >= 2 * gm + 1 and M % 256 != 0 and M % 128 != 0
    ldy = N + pad
    bias = ints(g, (N,), -3, 3)
    if heads == 1:
        ldx = ldw = K + pad
        x = ints(g, (batch, M, ldx))
        w = ints(g, (batch, N, ldw))
        prod = torch.matmul(x[..., :K].double(), w[..., :K].double().transpose(1, 2))              # (batch, M, N)
        strides = dict(xb=M * ldx, wb=N * ldw, yb=M * ldy, resb=M * ldy)
        lead = (batch,)
    else:
        ldx = ldw = heads * K
        x = ints(g, (batch, M, heads, K))
        w = ints(g, (batch, N, heads, K))
        prod = torch.einsum("bmhk,bnhk->bhmn", x.double(), w.double())                             # (batch, heads, M, N)
        strides = dict(xb=M * ldx, wb=N * ldw, yb=heads * M * ldy, resb=heads * M * ldy,
                       batch2=heads, xb2=K, wb2=K, yb2=M * ldy, resb2=M * ldy)
        lead = (batch, heads)
    res = ints(g, lead + (M, ldy), -8, 8)
    ref = _round_store(prod, dt, bias, res[..., :N])
    xd, wd, rd = x.to(dt).to(DEV), w.to(dt).to(DEV), res.to(dt).to(DEV)
    y = torch.full(lead + (M, ldy), SENTINEL, dtype=dt, device=DEV)
    ops.gemm_nt(dt, batch, M, N, K, xd.data_ptr(), ldx, strides.pop("xb"), wd.data_ptr(), ldw, strides.pop("wb"),
                y.data_ptr(), ldy, strides.pop("yb"), bias=bias.to(DEV), res_ptr=rd.data_ptr(), ldres=ldy, **strides)
    got = y.cpu()
    if not torch.equal(got[..., :N], ref):
        bad = (got[..., :N] != ref).any(-1).nonzero()
        raise AssertionError(f"{bad.shape[0]} rows differ; first (matrix ..., row): {bad[:6].tolist()}; "
                             f"tiles of {bm} rows, {gm} workgroups per matrix")
    if pad:
        assert bool((got[..., N:] == SENTINEL).all())          # nothing written beyond the N columns
