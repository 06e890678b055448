"""CPU: the ground tests/test_conv_pp_walk_gpu.py stands on, checked without a GPU (helpers: tests/conv_pp_ref.py).

  * every case of the table gets the configuration it claims from pp_plan() -- the restatement of uz_pp_plan() -- under
    cus = 128, unsplit; every workgroup makes at least two trips through the tile loop and some make three (pp128w16: two at
    the most, see the GPU file's docstring); its map is ragged the way the table says;
  * pp_plan() agrees with the library's own host-side queries (uz_conv_igemm_kernel_name / _grid_m / _workspace_bytes answer
    without a device) under a reserve of 128 CUs and of none;
  * the preconditions of exactness hold for every reference: a bf16 store and an fp32 sum of any order leave it unchanged;
  * the comparators see planted faults of the kind a wrong schedule leaves -- one bf16 ulp in one output of a trip-2 tile, a
    tile never stored, one tile lost from a workgroup's running sums, a halo row read from memory instead of zero padding --
    and name the tile and the trip; the first of them passes the 2e-2 bound of tests/test_conv_pp_gpu.py (asserted here)."""
from ctypes import byref

import pytest
import torch
import torch.nn.functional as F

import conv_pp_ref as R  # tests/conv_pp_ref.py (pytest puts this directory on sys.path)
from unet_zoo_amd import _lib as L
from unet_zoo_amd import ops

CASES = [pytest.param(c, id=R.case_id(c)) for c in R.ALL_CASES]


@pytest.fixture(autouse=True)
def _restore():
    yield
    L.set_cu_reserve(0)


@pytest.fixture(scope="module", autouse=True)
def _free_references():
    yield
    R.int_operands.cache_clear()


def _desc(c, ldx=None, ldy=None):
    N, H, W = R.MAPS[c.map].shape
    Hi, Wi = (H // 2, W // 2) if c.up else (H, W)
    return L.ConvDesc(L.UZ_BF16, N, H, W, Hi, Wi, c.cin, ldx or c.cin, c.nout, ldy or c.nout, 9,
                      L.TAPS_CONV_UP2 if c.up else L.TAPS_CONV, 1, L.STORE_PLAIN, 0, 0, 0)


@pytest.mark.parametrize("c", CASES)
def test_case_walks_under_the_restated_plan(c):
    R.assert_walks(c, R.case_plan(c))


@pytest.mark.parametrize("c", CASES)
def test_restated_plan_is_the_library_plan(c):
    """the host-side queries need no device; windows of wider buffers (ldx > Cin, ldy > Nout) change nothing"""
    lib = L.load()
    for reserve in (R.RESERVE, 0):
        L.set_cu_reserve(reserve)
        plan = R.case_plan(c, R.CUS_HW - reserve)
        for d in (_desc(c), _desc(c, c.cin + 40, c.nout + 96)):
            assert ops.conv_kernel_name(d) == R.kernel_name(plan.cfg, c.up), (reserve, plan)
            assert ops.conv_kernel_name(d, with_workspace=True) == R.kernel_name(plan.cfg, c.up)
            assert L.check_count(lib.uz_conv_igemm_grid_m(byref(d)), "grid_m") == plan.grid_m, (reserve, plan)
            assert L.check_count(lib.uz_conv_igemm_workspace_bytes(byref(d)), "workspace") == 0


def test_restated_plan_on_the_shapes_the_suite_names():
    """the branches no walking case takes: the split-K rule, the plain pp256 / pp256w16 without a reserve, no plan at all
    (shapes of tests/test_conv_pp_gpu.py)"""
    lib = L.load()
    # N, H, W, Cin, Nout, up, cfg, ksplit
    for N, H, W, Cin, Nout, up, cfg, ks in [(16, 16, 16, 1024, 512, False, "pp256w16", 4), (2, 32, 32, 512, 256, False, "pp256", 4),
                                            (2, 12, 14, 544, 136, False, "pp256w16", 4), (1, 32, 64, 1024, 128, True, "pp256", 8),
                                            (16, 16, 16, 512, 1024, False, "pp128w16", 1), (3, 128, 256, 64, 128, False, "pp512", 1),
                                            (16, 32, 32, 256, 512, False, "pp256", 1), (70, 16, 16, 64, 512, False, "pp256w16", 1),
                                            (1, 32, 32, 64, 64, False, None, 1), (2, 64, 64, 16, 128, False, None, 1)]:
        plan = R.pp_plan(N, H, W, Cin, Nout, R.CUS_HW, up)
        d = L.ConvDesc(L.UZ_BF16, N, H, W, H // 2 if up else H, W // 2 if up else W, Cin, Cin, Nout, Nout, 9,
                       L.TAPS_CONV_UP2 if up else L.TAPS_CONV, 1, L.STORE_PLAIN, 0, 0, 0)
        name = ops.conv_kernel_name(d, with_workspace=True)
        if cfg is None:
            assert plan is None and not name.startswith("conv3x3_pp"), name
            continue
        assert (plan.cfg, plan.ksplit) == (cfg, ks), plan
        assert name == R.kernel_name(cfg, up) + ("_splitk" if ks > 1 else "")
        assert L.check_count(lib.uz_conv_igemm_grid_m(byref(d)), "grid_m") == plan.grid_m
        assert lib.uz_conv_igemm_workspace_bytes(byref(d)) == (ks * N * H * W * Nout * 4 if ks > 1 else 0)


def _case_refs(c):
    """every exact reference the GPU file forms for a case, as (name, float64 tensor, whether statistics are formed of it)"""
    out = [("conv + bias", R.plain_ref(c), True)]
    if c.kind == "int":
        pre = R.plain_ref(c)
        scale, shift = R.act_vectors(c)
        out += [("gradient", R.plain_ref(c, with_bias=False), True)]
        out += [(f"bnact relu={relu}", R.act_ref(pre, scale, shift, relu), False) for relu in (0, 1)]
    return out


@pytest.mark.parametrize("c", CASES)
def test_preconditions_of_exactness(c):
    for name, ref, sums in _case_refs(c):
        got = R.assert_exact_preconditions(ref, sums)
        assert not sums or got[1] < 2 ** 23, (name, got)              # with room: half of what the exact sums allow
    if c.kind == "int":
        R.bnred_operands(c, R.plain_ref(c, with_bias=False))          # asserts its own 2^22 bounds
    else:
        o = R.operands(c)
        a = torch.relu(o.x * o.scale.view(1, -1, 1, 1) + o.shift.view(1, -1, 1, 1))
        assert a.min().item() == 0 and a.max().item() == 7 and torch.equal(a.to(R.BF16).float(), a)
        assert set(o.scale.abs().tolist()) <= {1.0, 2.0} and o.shift.min().item() >= 1


def test_fp32_convolution_on_integers_is_the_float64_one():
    """once, on the smallest case: F.conv2d in fp32 is exact on these operands"""
    c = min((c for c in R.ALL_CASES if c.kind == "int" and not c.up), key=lambda c: R.operands(c).prod.numel() * c.cin)
    o = R.operands(c)
    want = R.nhwc(F.conv2d(o.x.double(), o.w.double(), None, padding=1))
    assert torch.equal(o.prod.double(), want)


# ---- planted faults ---------------------------------------------------------------------------------------------------------
FAULT_CASE = R.PLAIN[1]          # pp512, two slabs, 224 tiles on a grid of 64: trips 0 .. 3


def _fault_ground():
    c = FAULT_CASE
    shape, plan = R.MAPS[c.map].shape, R.case_plan(c)
    ref64 = R.plain_ref(c)
    tiles = R.tile_of_pixels(shape, plan)
    return c, shape, plan, ref64, ref64.to(R.BF16), tiles


def _weak(got, ref):
    """the bound tests/test_conv_pp_gpu.py applies: max error over max magnitude below 2e-2"""
    return ((got.double() - ref.double()).abs().max() / ref.double().abs().max()).item() < 2e-2


def test_comparator_passes_the_reference_itself():
    c, shape, plan, ref64, ref, tiles = _fault_ground()
    R.assert_same(ref.clone(), ref, shape, plan)
    assert R._where(ref.clone(), ref, shape, plan) == "equal"
    R.check_stats(R.stats_rows(ref64, shape, plan).float(), ref64, plan)


def test_comparator_sees_one_ulp_in_a_tile_of_trip_2():
    c, shape, plan, ref64, ref, tiles = _fault_ground()
    tile = 2 * plan.grid_m + 5
    pix = int((tiles == tile).nonzero()[3])
    ch = 131                                         # the second N tile
    got = ref.clone()
    bits = got.view(torch.int16)
    bits[pix, ch] += 1                               # the next bf16
    assert got[pix, ch] != ref[pix, ch] and _weak(got, ref)
    with pytest.raises(AssertionError) as e:
        R.assert_same(got, ref, shape, plan)
    msg = str(e.value)
    assert "1 of 104640 pixels differ in 1 of 224" in msg and "trips [2] of a grid of 64" in msg, msg
    assert str(R.decode(tile, shape, plan)) in msg and "first [131]" in msg, msg


def test_comparator_sees_a_tile_left_at_the_sentinel():
    c, shape, plan, ref64, ref, tiles = _fault_ground()
    tile = plan.grid_m + 17                          # trip 1; an interior tile: 512 pixels
    got = ref.clone()
    got[tiles == tile] = R.SENTINEL
    with pytest.raises(AssertionError) as e:
        R.assert_same(got, ref, shape, plan)
    msg = str(e.value)
    assert "512 of 104640 pixels differ in 1 of 224" in msg and "trips [1]" in msg and str(R.decode(tile, shape, plan)) in msg, msg


def test_statistics_check_sees_one_tile_missing_from_a_workgroup():
    c, shape, plan, ref64, ref, tiles = _fault_ground()
    rows = R.stats_rows(ref64, shape, plan)
    tile = 3 * plan.grid_m + 2                       # the last trip of workgroup 2
    part = ref64[tiles == tile]
    rows[tile % plan.grid_m, 0] -= part.sum(0)
    rows[tile % plan.grid_m, 1] -= (part * part).sum(0)
    with pytest.raises(AssertionError, match="sum y: .* of 200 channels off"):
        R.check_stats(rows.float(), ref64, plan)


def test_comparator_sees_a_halo_row_without_zero_padding():
    """tile (image 1, tile row 0, tile column 0) of a later trip computed with its top halo row read from memory -- the last
    row of image 0 -- instead of zeros"""
    c, shape, plan, ref64, ref, tiles = _fault_ground()
    N, H, W = shape
    o = R.operands(c)
    im = 2
    tile = im * R.cdiv(H, plan.th) * R.cdiv(W, plan.tw)
    assert R.decode(tile, shape, plan) == (im, 0, 0) and tile // plan.grid_m == 1
    xin = torch.cat([o.x[im - 1:im, :, -1:, :], o.x[im:im + 1, :, :2, :]], 2)                 # rows -1, 0, 1 of the image
    row0 = F.conv2d(F.pad(xin, (1, 1, 0, 0)), o.w[:c.nout], o.b[:c.nout], padding=0)          # (1, Nout, 1, W): output row 0
    got = ref.clone().view(N, H, W, c.nout)
    got[im, 0, :plan.tw] = row0[0, :, 0, :plan.tw].t().to(R.BF16)
    got = got.view(-1, c.nout)
    with pytest.raises(AssertionError) as e:
        R.assert_same(got, ref, shape, plan)
    msg = str(e.value)
    assert "in 1 of 224" in msg and "trips [1]" in msg and f"[({im}, 0, 0)]" in msg, msg
