"""GPU: the two persistent kernels of uz_conv3x3.hip -- conv3x3_direct_kernel in its three forms (weights resident in LDS,
streaming with 64 and with 128 output channels) and conv3x3_res64_kernel -- where every workgroup makes SEVERAL trips through
its tile loop, both tile shapes and both dtypes, held bit for bit to exact references (helpers, case table and the restated
plan: tests/conv_direct_ref.py, on tests/conv_pp_ref.py; their own checks: tests/test_conv_direct_walk.py).

uz_direct_plan caps grid_m at UZ_NUM_CU / tiles_n and both kernels run
`for (tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x)`.  What only a second trip executes:
  resident   the next tile's halo patch issued into buffer (it + 1) & 1 during the current tile; a prefetched tile preceded by
             a barrier alone; cbuf = it & 1
  streaming  pre / has_next; the next tile's first halo pieces issued from the last slab (nxt, buffer (ncb + par) & 1) and its
             first weight pair from the last double-step (slot pair (ndbl + dpar) & 1); the counted wait_vmcnt<NSTORE> at d == 0
             of a prefetched tile, which assumes exactly NPASS buffer stores of the previous epilogue in flight (hence the
             out-of-image lanes that store to OOB); par = (ncb + par) & 1 and dpar = (ndbl + dpar) & 1 carried across tiles;
             the C staging in cbuf / cpair, the two buffers that do NOT hold the prefetch; sq1 / sq2 in registers across tiles
  res64      the late waves issue the next patch into (it + 1) & 1 and run epilogue(pimg, ph0, pw0) of the PREVIOUS tile, half
             a tile behind; the trailing `if (late && it > 0) epilogue(...)`; the early waves do not wait at the top of a trip;
             per-thread statistics parked in sStat between epilogues
The other tests of these kernels stay at a few tiles per launch, and to 2e-2 (bf16) or 2e-5 (fp32) of the maximum.

Here uz_set_cu_reserve(128) leaves the plan 128 CUs, and every case asserts, before it compares anything, that
  * the library names the kernel the case claims -- conv3x3_direct_<dt>_bn<bn>[_resident][_up2] or conv3x3_res64_<dt>[_up2] --
    with and without a workspace, and asks for no workspace,
  * uz_conv_igemm_grid_m() is the grid of direct_plan(), the restatement of uz_direct_plan(),
  * ntiles >= 2 * grid_m + 1: every workgroup makes at least two trips and some make three; the map is ragged both ways,
  * the preconditions of exactness hold for the reference (conv_pp_ref.assert_exact_preconditions).

Slabs per tile (ncb = ceil(Cin / 64) in bf16, ceil(Cin / 32) in fp32), streaming form: one to four give every combination of
the two carried parities -- ncb odd flips `par`, even keeps it; ndbl = ceil(9 ncb / 2) = 5, 9, 14, 18 flips, flips, keeps,
keeps `dpar`.  The bf16 streaming form cannot have one slab (Cin <= 64 goes to res64 or to the resident form), so flip / flip
is held by fp32 alone; the counted wait is bf16's alone (`sizeof(T) == 2`).

Instantiations and the cases that hold them -- map (N, H, W): tiles / grid_m under the reserve; A16 (129, 12, 20): 258 / 128,
A32 (65, 12, 40): 260 / 128, B32 (33, 20, 40): 198 / 64, B16 (33, 20, 20): 132 / 64 (res64: 132 / 42 and 198 / 32):
  (a) plain forward, bias + statistics, x and y channel windows of wider buffers (x's neighbours hold 5.0, three cases once
      more with NaN; y's the sentinel), the statistics compared row by row, i.e. per workgroup:
      fp32 resident   A16 32 -> 64;  A32 32 -> 40;  A32 32 -> 40 upsampled
      fp32 stream64   A16 64 -> 64 (2 slabs);  A32 96 -> 40 (3);  A32 128 -> 64 (4)
      fp32 stream128  B32 32 -> 200 (1);  B32 64 -> 200 (2);  B16 96 -> 136 (3);  B16 128 -> 200 (4)
      bf16 resident   A16 64 -> 64;  A32 64 -> 64;  A32 64 -> 32;  A32 64 -> 64 upsampled
      bf16 stream64   A16 128 -> 64 (2);  A32 72 -> 40 (2, the last slab 8 channels);  A32 192 -> 40 (3);  A32 256 -> 32 (4)
      bf16 stream128  B32 72 -> 200 (2, partial);  B16 128 -> 200 (2);  B32 136 -> 200 (3, partial);  B16 192 -> 136 (3);
                      B16 256 -> 200 (4);  B32 72 -> 200 upsampled
      res64           A16 16 -> 64;  A32 48 -> 40;  A32 32 -> 32;  B16 64 -> 136 (three N tiles);  B32 40 -> 200 (four);
                      A32 32 -> 32 upsampled
  (b) fused BatchNorm-backward sums (BNRED; bf16, not res64):  resident A32 64 -> 64;  stream64 A16 128 -> 64;
      stream128 B32 136 -> 200 and B16 192 -> 136
  (c) eval-mode epilogue (ACT), with and without the ReLU:  fp32 resident A16 32 -> 64;  fp32 stream128 B32 64 -> 200;
      bf16 resident A32 64 -> 32;  bf16 stream64 A32 192 -> 40;  bf16 stream128 B16 128 -> 200
  (d) normal operands against float64 and against the launch without a reserve:  one case per (dtype, form)

Not reachable through the ABI:
  * the `ybytes == 0` path of the streaming epilogue (st16 instead of the buffer store, and wait_vmcnt<0> instead of the counted
    wait) needs an output tensor of 2 GiB or more;
  * the bn flip to 64 (bn == 128 && ntiles * tn <= UZ_NUM_CU / 2) implies ntiles <= cap, one trip per workgroup: the flipped
    plan never walks (tests/test_conv_direct_walk.py holds the rule itself);
  * the UZ_ABLATE / UZ_KFLAGS variants (the 16x16x32 and three-deep res64, the no-prefetch and no-late switches) exist in the
    ablation build only.
Not instantiated, so not listed: BNRED in fp32 or on res64, ACT on res64."""
from ctypes import byref

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import conv_direct_ref as R  # tests/conv_direct_ref.py (pytest puts this directory on sys.path)
from unet_zoo_amd import _lib as L
from unet_zoo_amd import ops
from unet_zoo_amd.ops import Act

DEV = "cuda"
BF16, F32 = R.BF16, R.F32
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


def _desc(c, ldx, ldy):
    N, H, W = R.MAPS[c.map].shape
    Hi, Wi = _in_hw(c)
    return L.ConvDesc(L.dtype_code(c.dt), N, H, W, Hi, Wi, c.cin, ldx, c.nout, ldy, 9, _taps(c), 1, L.STORE_PLAIN, 0, 0, 0)


def _assert_walks(c, ldx, ldy):
    """under the reserve in force: the library's plan for the case's descriptor is the restated one, and it walks; returns
    the plan and the descriptor"""
    lib = L.load()
    assert L.get_cu_reserve() == R.RESERVE
    d = _desc(c, ldx, ldy)
    plan = R.case_plan(c)
    want = R.case_kernel_name(c)
    assert ops.conv_kernel_name(d) == want and ops.conv_kernel_name(d, with_workspace=True) == want, ops.conv_kernel_name(d)
    assert L.check_count(lib.uz_conv_igemm_workspace_bytes(byref(d)), "workspace") == 0
    gm = L.check_count(lib.uz_conv_igemm_grid_m(byref(d)), "grid_m")
    assert gm == plan.grid_m, (gm, plan)
    R.assert_walks(c, plan)
    print(f"    {want}: {plan.ntiles} tiles / grid of {plan.grid_m} x {plan.tiles_n}, {plan.slabs} slabs")
    return plan, d


def _x_act(c, x, window=False, fill=5.0):
    """the NHWC input of a case on the device; window: inside a wider buffer whose other channels hold `fill` -- a neighbour
    read by mistake shows in every sum"""
    N = R.MAPS[c.map].shape[0]
    Hi, Wi = _in_hw(c)
    rows = R.nhwc(x)
    if not window:
        return Act(rows.to(c.dt).to(DEV), 0, c.cin, N, Hi, Wi)
    buf = torch.full((rows.shape[0], c.cin + XPAD), fill)
    buf[:, XOFF:XOFF + c.cin] = rows
    return Act(buf.to(c.dt).to(DEV), XOFF, c.cin, N, Hi, Wi)


def _y_window(c, fill):
    N, H, W = R.MAPS[c.map].shape
    buf = torch.full((N * H * W, c.nout + YPAD), fill, dtype=c.dt, device=DEV)
    return buf, Act(buf, YOFF, c.nout, N, H, W)


def _split(buf, c):
    """(the window, everything else) of a (P, Nout + YPAD) buffer, on the CPU"""
    t = buf.cpu()
    return t[:, YOFF:YOFF + c.nout], torch.cat([t[:, :YOFF], t[:, YOFF + c.nout:]], 1)


def _weights(c, o):
    wp = ops.pack_weights(o.w[:c.nout].contiguous().to(DEV), L.PACK_CONV_FWD, c.dt)
    return wp, o.b[:c.nout].contiguous().to(DEV)


# ---- (a): plain forward, bias + statistics ---------------------------------------------------------------------------------
def _plain_forward(c, fill=5.0):
    shape = R.MAPS[c.map].shape
    o = R.operands(c)
    ref64 = R.plain_ref(c)
    R.assert_exact_preconditions(ref64)
    ref = ref64.to(c.dt)                             # rounded once to the run dtype (which changes nothing)
    L.set_cu_reserve(R.RESERVE)
    plan, _ = _assert_walks(c, c.cin + XPAD, c.nout + YPAD)
    xa = _x_act(c, o.x, window=True, fill=fill)
    wp, bd = _weights(c, o)

    def run():
        ybuf, y = _y_window(c, SENTINEL)
        return ybuf, ops.conv_igemm(xa, wp, bd, y, ntaps=9, want_stats=True, taps_mode=_taps(c))

    ybuf, stats = run()
    got, rest = _split(ybuf, c)
    R.assert_same(got, ref, shape, plan)
    assert bool((rest == SENTINEL).all())
    R.check_rows(stats, ref64, shape, plan)          # every workgroup's rows, not only their total
    ybuf2, stats2 = run()
    assert torch.equal(ybuf2, ybuf) and torch.equal(stats2, stats)


@pytest.mark.parametrize("c", _params(R.PLAIN))
def test_plain_forward_is_exact_over_several_trips(c):
    """up2: the reference is F.interpolate(nearest, x2), then the convolution"""
    _plain_forward(c)


@pytest.mark.parametrize("c", _params(R.NAN_NEIGHBOURS))
def test_plain_forward_next_to_nan_neighbours(c):
    """the channels beside x's window hold NaN (as in tests/test_ops_gpu.py): a partial last slab, or a Cin below the slab,
    must come from the `ch < Cin` range check, never from memory -- 0 * NaN would show in every output"""
    _plain_forward(c, fill=float("nan"))


# ---- (b): fused BatchNorm-backward sums ------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", _params(R.BNRED))
def test_bn_backward_sums_are_exact_over_several_trips(c):
    """uz_conv_igemm_bnred: the sums of dz = g * [relu(bn(y)) > 0] and of dz * ((y - mean) * invstd) -- the per-element form of
    the epilogue, sq2[e] += dz * ((yv - bmu[e]) * bis[e]) -- live in sq1 / sq2 across the epilogues of a workgroup's tiles;
    bn_y of a tile is requested at the top of its epilogue, among the prefetched pieces of the next tile"""
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


# ---- (c): eval-mode epilogue -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("c", _params(R.ACT))
def test_eval_mode_epilogue_is_exact_over_several_trips(c, relu):
    """uz_conv_igemm_bnact: relu?(fma(conv + bias, scale, shift)), rounded once; scales are powers of two and shifts integers,
    so the result is exact.  bf16 keeps (scale, shift) in an LDS table behind the weight slots from the prologue on, fp32 in
    registers: an epilogue's staging (or a prefetch) that reached them would show from the next tile of the workgroup on.
    What no case may write holds NaN here: -77 is a value this epilogue can produce"""
    shape = R.MAPS[c.map].shape
    o = R.operands(c)
    scale, shift = R.act_vectors(c)
    ref64 = R.act_ref(R.plain_ref(c), scale, shift, relu)
    R.assert_exact_preconditions(ref64, sums=False)
    ref = ref64.to(c.dt)
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


# ---- (d): normal operands --------------------------------------------------------------------------------------------------
def tol(dt):
    """restated from tests/test_ops_gpu.py (its tol(dt), applied there to these kernels through relerr(): max error over max
    magnitude) -- restated, not imported, so that this file does not collect that module's tests a second time"""
    return 2e-5 if dt == torch.float32 else 2e-2


@pytest.mark.parametrize("c", _params(R.NORMAL))
def test_normal_operands_against_float64_and_against_fewer_trips(c):
    """randn operands rounded to the run dtype against float64 F.conv2d on the rounded operands, to the bound
    tests/test_ops_gpu.py holds these kernels to.  And a tile's value must not depend on which trip computed it: the launch
    under the reserve equals the launch on the whole chip bit for bit (an output's K order does not depend on its tile) -- the
    same kernel by name, on a grid twice as wide or wider"""
    shape = R.MAPS[c.map].shape
    N, H, W = shape
    g = torch.Generator().manual_seed(c.cin + c.nout + H)
    x = torch.randn(N, c.cin, H, W, generator=g).to(c.dt)
    w = (torch.randn(c.nout, c.cin, 3, 3, generator=g) * 0.05).to(c.dt)
    b = torch.randn(c.nout, generator=g)
    xa = _x_act(c, x.float())
    wp = ops.pack_weights(w.float().to(DEV), L.PACK_CONV_FWD, c.dt)
    bd = b.to(DEV)

    def run():
        y = ops.new_act(N, H, W, c.nout, c.dt, DEV)
        y.buf.fill_(float("nan"))
        return y.buf, ops.conv_igemm(xa, wp, bd, y, ntaps=9, want_stats=True)

    d = _desc(c, c.cin, c.nout)
    name_full = ops.conv_kernel_name(d, with_workspace=True)
    gm_full = L.check_count(L.load().uz_conv_igemm_grid_m(byref(d)), "grid_m")
    assert name_full == R.case_kernel_name(c), name_full     # both reserves: the same kernel (the CPU file: from the plan)
    full_chip, _ = run()
    L.set_cu_reserve(R.RESERVE)
    plan, _ = _assert_walks(c, c.cin, c.nout)
    assert gm_full >= 2 * plan.grid_m or gm_full == plan.ntiles, (gm_full, plan)
    print(f"    whole chip: grid of {gm_full}; reserve {R.RESERVE}: grid of {plan.grid_m}")
    got, stats = run()
    assert bool(torch.isfinite(got).all())
    R.assert_same(got.cpu(), full_chip.cpu(), shape, plan, "reserve 128 against the whole chip")
    got2, stats2 = run()
    assert torch.equal(got2, got) and torch.equal(stats2, stats)
    ref = R.nhwc(F.conv2d(x.double(), w.double(), b.double(), padding=1))
    yd = got.double().cpu()
    e_max = ((yd - ref).abs().max() / ref.abs().max()).item()
    print(f"    y vs float64: max/max {e_max:.3e} (bound {tol(c.dt):g})")
    assert e_max < tol(c.dt), e_max
