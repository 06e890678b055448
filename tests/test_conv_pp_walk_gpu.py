"""GPU: conv3x3_pp_kernel of uz_conv3x3_pp.hip where every workgroup makes SEVERAL trips through its tile loop, all five tile
configurations and all four epilogue / input forms, held bit for bit to exact references (helpers, case table and the
restated plan: tests/conv_pp_ref.py; their own checks: tests/test_conv_pp_walk.py).

The kernel's workgroups are persistent: uz_pp_plan caps grid_m at UZ_NUM_CU / tiles_n and the kernel runs
`for (tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x)`.  What only a second trip executes: compute_avoff() of the next
tile in a tile's last slab and the halo requests of that tile's first slab from phase() with `last && has_next`; issue_b() of
slab cbeg on the wrap; the `first` branch of the counted waits, wait_vmcnt<NW0 + NSTORE> / <NN + NSTORE>, which allows for
exactly NSTORE epilogue stores of the previous tile in flight; apar and bslot carried over a tile boundary; decode() of a
tile that is not blockIdx.x; the running BatchNorm sums parked in the staging strip between epilogues; the ACT form's
(scale, shift) in the 16 spare bytes of the staging rows across epilogues; the XF form's table reload
xf_table(last ? cbeg : c + 1); wait_nonext on the last slab of a late trip over a ragged tile.  The other tests of this kernel
hold what walks to 2e-2 of the maximum and 3e-3 of a sum, and their one exact case makes one trip.

Here uz_set_cu_reserve(128) leaves the plan 128 CUs, and every case asserts, before it compares anything, that
  * the library names conv3x3_<cfg>_bf16[_up2] for the descriptor -- the configuration the case claims, not the split-K
    form -- and asks for no workspace,
  * uz_conv_igemm_grid_m() is the grid of pp_plan(), the restatement of uz_pp_plan(),
  * ntiles >= 2 * grid_m + 1: every workgroup makes at least two trips and some make three (pp128w16: grid_m + 1 <= ntiles
    <= 2 * grid_m, see below); the map is ragged in the directions the table says,
  * the preconditions of exactness hold for the reference (conv_pp_ref.assert_exact_preconditions).
Every case launches twice into fresh buffers and the two must be equal bit for bit: a miscounted wait is a race.

Slabs per tile (Cin / 32): with one, first == last in every slab -- the wrap issues the next tile's slab from the only slab,
the NSTORE branch and the next tile's halo requests fall in the same phases; two; three or four have a middle slab that is
neither.  pp512 (NPH = 9, DPH = 4) and pp256 (NPH = 3, DPH = 2, as the other three) take all three counts, the rest one and two.

(configuration, form) pairs and the cases that hold them -- ntiles / grid_m under the reserve in brackets:
  (a) plain forward, bias + statistics, x and y channel windows of wider buffers (x's neighbours hold 5.0, y's the sentinel):
      pp512 [224 / 64] Cin 32, 64, 96 -> 200 and 64 -> 136;  pp512x64 [260 / 128] 32 -> 40, 64 -> 64;
      pp256 [240 / 64] Cin 32, 64, 128 -> 200 and [330 / 64] 64 -> 256;  pp256w16 [130 / 64] Cin 32, 64 -> 136 and
      [66 / 32] 64 -> 512;  pp128w16 [256 / 128] Cin 32, 64 -> 128 and [100 / 64] 32 -> 256
  (b) the nearest x2 upsampled read (TAPS_CONV_UP2):  pp512 64 -> 200, pp512x64 32 -> 40, pp256 64 -> 200
  (c) fused BatchNorm-backward sums:  pp512 64 -> 136, pp512x64 32 -> 40, pp256 128 -> 200, pp256w16 64 -> 136,
      pp128w16 64 -> 128
  (d) eval-mode epilogue, with and without the ReLU:  pp512 96 -> 200, pp512x64 32 -> 40, pp256 64 -> 200, pp256w16 32 -> 136,
      pp128w16 32 -> 128
  (e) input transform (pp512x64, the only configuration with an XF form):  32 -> 40, 64 -> 64, 128 -> 40, and 64 -> 64 upsampled
  (f) normal operands against float64 and against the launch without a reserve:  one 64-channel case per configuration

Not reachable through the ABI:
  * pp128w16 never makes a third trip.  It is chosen only when tiles256 * tiles_n <= 128 (tiles256: the 256-pixel tiles of the
    pp256 / pp256w16 plan it replaces), a 256-pixel tile splits into at most two 128-pixel ones, so
        ntiles <= 2 * tiles256 <= 2 * floor(128 / tiles_n) <= 2 * cap      (cap = (256 - reserve) / tiles_n, reserve <= 128).
    Without a reserve cap = 256 / tiles_n >= ntiles: it walks only while a reserve is set.  Its cases ask for two trips.
  * the split-K form launches grid = (ntiles, tiles_n, ksplit): one tile per workgroup, it never walks
    (tests/test_conv_pp_gpu.py keeps it).
The second-generation kernels of uz_conv3x3.hip (direct, resident, res64) have a tile loop of their own: their test of this
kind is tests/test_conv_direct_walk_gpu.py."""
from ctypes import byref

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import conv_pp_ref as R  # tests/conv_pp_ref.py (pytest puts this directory on sys.path)
from unet_zoo_amd import _lib as L
from unet_zoo_amd import ops
from unet_zoo_amd.ops import Act

DEV = "cuda"
BF16 = torch.bfloat16
SENTINEL = R.SENTINEL
XPAD, XOFF = 40, 24              # x: channels [24, 24 + Cin) of a buffer 40 channels wider
YPAD, YOFF = 96, 64              # y: channels [64, 64 + Nout) of a buffer 96 channels wider


@pytest.fixture(autouse=True)
def _restore():
    yield
    L.set_cu_reserve(0)


@pytest.fixture(scope="module", autouse=True)
def _free_references():
    yield
    R.int_operands.cache_clear()


def _params(cases):
    return [pytest.param(c, id=R.case_id(c)) for c in cases]


def _taps(c):
    return L.TAPS_CONV_UP2 if c.up else L.TAPS_CONV


def _in_hw(c):
    _, H, W = R.MAPS[c.map].shape
    return (H // 2, W // 2) if c.up else (H, W)


def _assert_walks(c, ldx, ldy):
    """under the reserve in force: the library's plan for the case's descriptor is the restated one, unsplit, and it walks;
    returns the plan"""
    lib = L.load()
    assert L.get_cu_reserve() == R.RESERVE
    N, H, W = R.MAPS[c.map].shape
    Hi, Wi = _in_hw(c)
    d = L.ConvDesc(L.UZ_BF16, N, H, W, Hi, Wi, c.cin, ldx, c.nout, ldy, 9, _taps(c), 1, L.STORE_PLAIN, 0, 0, 0)
    plan = R.case_plan(c)
    want = R.kernel_name(R.MAPS[c.map].cfg, c.up)
    assert ops.conv_kernel_name(d) == want and ops.conv_kernel_name(d, with_workspace=True) == want
    assert L.check_count(lib.uz_conv_igemm_workspace_bytes(byref(d)), "workspace") == 0
    gm = L.check_count(lib.uz_conv_igemm_grid_m(byref(d)), "grid_m")
    assert gm == plan.grid_m, (gm, plan)
    R.assert_walks(c, plan)
    print(f"    {want}: {plan.ntiles} tiles / grid of {plan.grid_m} x {plan.tiles_n}, {c.cin // R.KU} slabs")
    return plan, d


def _x_act(c, x, window=False, fill=5.0):
    """the NHWC input of a case on the device; window: inside a wider buffer whose other channels hold `fill` -- a neighbour
    read by mistake shows in every sum"""
    N = R.MAPS[c.map].shape[0]
    Hi, Wi = _in_hw(c)
    rows = R.nhwc(x)
    if not window:
        return Act(rows.to(BF16).to(DEV), 0, c.cin, N, Hi, Wi)
    buf = torch.full((rows.shape[0], c.cin + XPAD), fill)
    buf[:, XOFF:XOFF + c.cin] = rows
    return Act(buf.to(BF16).to(DEV), XOFF, c.cin, N, Hi, Wi)


def _y_window(c, fill):
    N, H, W = R.MAPS[c.map].shape
    buf = torch.full((N * H * W, c.nout + YPAD), fill, dtype=BF16, device=DEV)
    return buf, Act(buf, YOFF, c.nout, N, H, W)


def _split(buf, c):
    """(the window, everything else) of a (P, Nout + YPAD) buffer, on the CPU"""
    t = buf.cpu()
    return t[:, YOFF:YOFF + c.nout], torch.cat([t[:, :YOFF], t[:, YOFF + c.nout:]], 1)


def _weights(c, o):
    wp = ops.pack_weights(o.w[:c.nout].contiguous().to(DEV), L.PACK_CONV_FWD, BF16)
    return wp, o.b[:c.nout].contiguous().to(DEV)


# ---- (a), (b): plain forward, bias + statistics ----------------------------------------------------------------------------------
def _plain_forward(c):
    shape = R.MAPS[c.map].shape
    o = R.operands(c)
    ref64 = R.plain_ref(c)
    R.assert_exact_preconditions(ref64)
    ref = ref64.to(BF16)
    L.set_cu_reserve(R.RESERVE)
    plan, _ = _assert_walks(c, c.cin + XPAD, c.nout + YPAD)
    xa = _x_act(c, o.x, window=True)
    wp, bd = _weights(c, o)

    def run():
        ybuf, y = _y_window(c, SENTINEL)
        return ybuf, ops.conv_igemm(xa, wp, bd, y, ntaps=9, want_stats=True, taps_mode=_taps(c))

    ybuf, stats = run()
    got, rest = _split(ybuf, c)
    R.assert_same(got, ref, shape, plan)
    assert bool((rest == SENTINEL).all())
    R.check_stats(stats, ref64, plan)
    ybuf2, stats2 = run()
    assert torch.equal(ybuf2, ybuf) and torch.equal(stats2, stats)


@pytest.mark.parametrize("c", _params(R.PLAIN))
def test_plain_forward_is_exact_over_several_trips(c):
    _plain_forward(c)


@pytest.mark.parametrize("c", _params(R.UP2))
def test_upsampled_read_is_exact_over_several_trips(c):
    """TAPS_CONV_UP2: the reference is F.interpolate(nearest, x2), then the convolution"""
    _plain_forward(c)


# ---- (c): fused BatchNorm-backward sums ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", _params(R.BNRED))
def test_bn_backward_sums_are_exact_over_several_trips(c):
    """uz_conv_igemm_bnred: the sums of dz = g * [relu(bn(y)) > 0] and of dz * ((y - mean) * invstd) -- the per-element form of
    the epilogue, sq2[e] += dz * ((yv - bmu[e]) * bis[e]) -- live in the staging strip between the epilogues of a workgroup's
    tiles; bn_y is loaded in the epilogue, behind wait_vmcnt<0>"""
    shape = R.MAPS[c.map].shape
    N, H, W = shape
    o = R.operands(c)
    ref64 = R.plain_ref(c, with_bias=False)
    R.assert_exact_preconditions(ref64)
    br = R.bnred_operands(c, ref64)
    ref = ref64.to(BF16)
    L.set_cu_reserve(R.RESERVE)
    plan, d = _assert_walks(c, c.cin, c.nout)
    assert L.load().uz_conv_igemm_bnred_supported(byref(d)) == 1
    xa = _x_act(c, o.x)
    wp, _ = _weights(c, o)
    ya = Act(br.bn_y.to(BF16).to(DEV), 0, c.nout, N, H, W)
    vec = br.vec.to(DEV)
    plain = ops.new_act(N, H, W, c.nout, BF16, DEV)
    plain.buf.fill_(SENTINEL)
    ops.conv_igemm(xa, wp, None, plain, ntaps=9, taps_mode=_taps(c))

    def run():
        fused = ops.new_act(N, H, W, c.nout, BF16, DEV)
        fused.buf.fill_(SENTINEL)
        return fused.buf, ops.conv_igemm(xa, wp, None, fused, ntaps=9, taps_mode=_taps(c), bnred=(ya, vec))

    fbuf, part = run()
    assert part is not None
    R.assert_same(fbuf.cpu(), ref, shape, plan, "gradient")
    assert torch.equal(fbuf, plain.buf)
    R.check_sums(part, br.want0, br.want1, plan, ("sum dz", "sum dz xhat"))
    fbuf2, part2 = run()
    assert torch.equal(fbuf2, fbuf) and torch.equal(part2, part)


# ---- (d): eval-mode epilogue --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("c", _params(R.BNACT))
def test_eval_mode_epilogue_is_exact_over_several_trips(c, relu):
    """uz_conv_igemm_bnact: relu?(fma(conv + bias, scale, shift)), rounded once.  The (scale, shift) of a wave's channels wait in
    the spare 16 bytes of its staging rows from the prologue on: an epilogue that overwrote them would show in the next tile
    of the same workgroup, which is a later trip"""
    shape = R.MAPS[c.map].shape
    o = R.operands(c)
    scale, shift = R.act_vectors(c)
    ref64 = R.act_ref(R.plain_ref(c), scale, shift, relu)
    R.assert_exact_preconditions(ref64, sums=False)
    ref = ref64.to(BF16)
    L.set_cu_reserve(R.RESERVE)
    plan, d = _assert_walks(c, c.cin + XPAD, c.nout + YPAD)
    assert L.load().uz_conv_igemm_bnact_supported(byref(d)) == 1
    xa = _x_act(c, o.x, window=True)
    wp, bd = _weights(c, o)
    sc, sh = scale.to(DEV), shift.to(DEV)

    def run():
        ybuf, y = _y_window(c, float("nan"))
        ops.conv_igemm_bnact(xa, wp, bd, sc, sh, bool(relu), y, ntaps=9, taps_mode=_taps(c))
        return ybuf

    ybuf = run()
    got, rest = _split(ybuf, c)
    assert bool(torch.isfinite(got).all()), R._where(torch.nan_to_num(got, nan=SENTINEL), ref, shape, plan)
    assert bool(torch.isnan(rest).all())
    R.assert_same(got, ref, shape, plan)
    got2, rest2 = _split(run(), c)
    assert torch.equal(got2, got) and bool(torch.isnan(rest2).all())


# ---- (e): input transform -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", _params(R.XF))
def test_input_transform_is_exact_over_several_trips(c):
    """uz_conv_igemm_xf: x integers in -2..2 read through relu(x * scale + shift), scale from {+-1, +-2}, shift from {1, 2, 3}:
    integers in 0..7, and a zero pad that was transformed would be shift > 0.  Against F.conv2d on the transformed activation
    (zero-padded AFTER the transform), and bit for bit, statistics included, against uz_bn_relu_apply followed by the plain
    launch"""
    shape = R.MAPS[c.map].shape
    N = shape[0]
    Hi, Wi = _in_hw(c)
    o = R.operands(c)
    ref64 = R.plain_ref(c)
    R.assert_exact_preconditions(ref64)
    ref = ref64.to(BF16)
    L.set_cu_reserve(R.RESERVE)
    plan, _ = _assert_walks(c, c.cin, c.nout + YPAD)
    xa = _x_act(c, o.x)
    raw = xa.buf.clone()
    assert ops.conv_xform_supported(xa, c.nout, c.nout + YPAD, upsample=c.up)
    wp, bd = _weights(c, o)
    sc, sh = o.scale.to(DEV), o.shift.to(DEV)

    def run(x, xform):
        ybuf, y = _y_window(c, SENTINEL)
        return ybuf, ops.conv_igemm(x, wp, bd, y, ntaps=9, want_stats=True, taps_mode=_taps(c), xform=xform)

    ybuf, stats = run(xa, (sc, sh))
    got, rest = _split(ybuf, c)
    R.assert_same(got, ref, shape, plan)
    assert bool((rest == SENTINEL).all())
    R.check_stats(stats, ref64, plan)
    # the two launches it replaces
    a = ops.new_act(N, Hi, Wi, c.cin, BF16, torch.device(DEV), False)
    ops.bn_relu_apply(xa, sc, sh, a)
    ybuf0, stats0 = run(a, None)
    R.assert_same(got, _split(ybuf0, c)[0], shape, plan, "fused against apply-then-convolve")
    assert torch.equal(ybuf0, ybuf) and torch.equal(stats0, stats)
    ybuf2, stats2 = run(xa, (sc, sh))
    assert torch.equal(ybuf2, ybuf) and torch.equal(stats2, stats)
    assert torch.equal(xa.buf, raw)                  # the raw input is left as it was


# ---- (f): normal operands -------------------------------------------------------------------------------------------------------------------
# 16-pixel tiles of a wave (PT = TH / WM * TW / 16) and its waves along the pixels (WM), per configuration
PT_WM = {"pp512": (8, 4), "pp512x64": (4, 8), "pp256": (4, 4), "pp256w16": (4, 4), "pp128w16": (2, 4)}


@pytest.mark.parametrize("c", _params(R.NORMAL))
def test_normal_operands_against_float64_and_against_fewer_trips(c):
    """randn operands rounded to bf16 against float64 on the rounded operands, to the bound tests/test_conv_pp_gpu.py applies
    to this kernel (2e-2, max error over max magnitude) and the format-derived one of tests/test_conv5x5_gpu.py (2^-8 of the
    norm).  And a tile's value must not depend on which trip computed it: the launch under the reserve equals the launch on
    the whole chip bit for bit (uz_pp_plan: "the summation order, hence the rounding of the result, must not depend on that
    setting"; "an output's K order does not depend on its tile") -- whatever configuration the whole chip gets"""
    shape = R.MAPS[c.map].shape
    N, H, W = shape
    g = torch.Generator().manual_seed(c.cin + c.nout + H)
    x = torch.randn(N, c.cin, H, W, generator=g).to(BF16)
    w = (torch.randn(c.nout, c.cin, 3, 3, generator=g) * 0.05).to(BF16)
    b = torch.randn(c.nout, generator=g)
    xa = _x_act(c, x.float())
    wp = ops.pack_weights(w.float().to(DEV), L.PACK_CONV_FWD, BF16)
    bd = b.to(DEV)

    def run():
        y = ops.new_act(N, H, W, c.nout, BF16, DEV)
        y.buf.fill_(float("nan"))
        return y.buf, ops.conv_igemm(xa, wp, bd, y, ntaps=9, want_stats=True)

    d = L.ConvDesc(L.UZ_BF16, N, H, W, H, W, c.cin, c.cin, c.nout, c.nout, 9, L.TAPS_CONV, 1, L.STORE_PLAIN, 0, 0, 0)
    name_full = ops.conv_kernel_name(d, with_workspace=True)
    gm_full = L.check_count(L.load().uz_conv_igemm_grid_m(byref(d)), "grid_m")
    assert name_full.startswith("conv3x3_pp") and not name_full.endswith("_splitk"), name_full
    full_chip, _ = run()
    L.set_cu_reserve(R.RESERVE)
    plan, _ = _assert_walks(c, c.cin, c.nout)
    print(f"    whole chip: {name_full}, grid of {gm_full}; reserve {R.RESERVE}: {ops.conv_kernel_name(d)}, grid of {plan.grid_m}")
    got, stats = run()
    assert bool(torch.isfinite(got).all())
    R.assert_same(got.cpu(), full_chip.cpu(), shape, plan, "reserve 128 against the whole chip")
    got2, stats2 = run()
    assert torch.equal(got2, got) and torch.equal(stats2, stats)
    ref = R.nhwc(F.conv2d(x.double(), w.double(), b.double(), padding=1))
    yd = got.double().cpu()
    e_max = ((yd - ref).abs().max() / ref.abs().max()).item()
    e_norm = ((yd - ref).norm() / ref.norm()).item()
    print(f"    y vs float64: max/max {e_max:.3e} (bound 2e-2), norm {e_norm:.3e} (bound {2.0 ** -8:.3e})")
    assert e_max < 2e-2, e_max
    assert e_norm <= 2.0 ** -8, e_norm
    # Sums of the STORED values, against sum |y| and sum y^2.  The epilogue's chain for one channel of one lane: a round is 32
    # pixels, of which a lane adds 4 (k = 0 .. 3); PT / 2 rounds per tile; at most ceil(ntiles / grid_m) trips; then the
    # fixed-order sum over the 8 lanes x WM waves that own the channel.  pp512: 4 * 4 * 4 trips + 32 = 96 additions,
    # pp512x64: 4 * 2 * 3 + 64 = 88, pp256 (330 / 64: 6 trips): 4 * 2 * 6 + 32 = 80, pp256w16: 4 * 2 * 3 + 32 = 56,
    # pp128w16: 4 * 1 * 2 + 32 = 40 -- each at most 2^-24 of the sum of magnitudes (one more for the square): 96 * 2^-24
    # = 5.7e-6 at the very worst, under the 1e-5 asked here (the argument of tests/test_gemm_dma_walk_gpu.py)
    pt, wm = PT_WM[plan.cfg]
    chain = 4 * (pt // 2) * R.cdiv(plan.ntiles, plan.grid_m) + 8 * wm
    assert (chain + 1) * 2.0 ** -24 < 1e-5, chain
    assert tuple(stats.shape) == (plan.grid_m, 2, c.nout)
    s = stats.double().sum(0).cpu()
    assert ((s[0] - yd.sum(0)).abs() <= 1e-5 * yd.abs().sum(0)).all()
    assert ((s[1] - (yd * yd).sum(0)).abs() <= 1e-5 * (yd * yd).sum(0)).all()
