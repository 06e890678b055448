"""CPU: the ground tests/test_conv_direct_walk_gpu.py stands on, checked without a GPU (helpers: tests/conv_direct_ref.py).

  * every case of the table gets the form (resident / stream / res64), tile and bn it claims from direct_plan() -- the
    restatement of uz_direct_plan() -- under UZ_NUM_CU = 128; its bf16 cases are declined by conv_pp_ref.pp_plan(); every
    workgroup makes at least two trips through the tile loop and some make three (ntiles >= 2 * grid_m + 1); it resolves to
    the same form, tile and bn, hence the same kernel name, at 256 CUs; its map is ragged the way the table says;
  * direct_plan() gives what a handful of descriptors worked by hand must get -- the bn flip to 64 when ntiles * tn <= CUs / 2
    and the Cin == 64 && Nout <= 64 exclusion from res64 among them -- and agrees with the library's own host-side queries
    (uz_conv_igemm_kernel_name / _grid_m / _workspace_bytes answer without a device) on those and on every case, under a
    reserve of 128 CUs and of none;
  * the preconditions of exactness hold for every reference the GPU file forms: rounding to bf16 changes nothing, sum |y| and
    sum y^2 stay below 2^24 per channel, the bnred_operands() bounds hold.  These are conditions on the inputs, not
    measurements: a case that fails one gets another input, never another bound;
  * the comparators see planted faults of the kind a wrong walk leaves -- one tile of a late trip altered, one tile's sums
    moved from one workgroup's rows to another's (which leaves the totals as they were) -- and name the trip."""
from ctypes import byref

import pytest
import torch
import torch.nn.functional as F

import conv_direct_ref as R  # tests/conv_direct_ref.py (pytest puts this directory on sys.path)
import conv_pp_ref as P
from unet_zoo_amd import _lib as L
from unet_zoo_amd import ops

BF16, F32 = R.BF16, R.F32
CASES = [pytest.param(c, id=R.case_id(c)) for c in R.ALL_CASES]


@pytest.fixture(autouse=True)
def _restore():
    yield
    L.set_cu_reserve(0)


@pytest.fixture(scope="module", autouse=True)
def _free_references():
    yield
    R.int_operands.cache_clear()


def _desc(dt, N, H, W, Cin, Nout, up=False, ldx=None, ldy=None):
    Hi, Wi = (H // 2, W // 2) if up else (H, W)
    return L.ConvDesc(L.dtype_code(dt), N, H, W, Hi, Wi, Cin, ldx or Cin, Nout, ldy or Nout, 9,
                      L.TAPS_CONV_UP2 if up else L.TAPS_CONV, 1, L.STORE_PLAIN, 0, 0, 0)


def _assert_library_agrees(d, dt, plan, up):
    lib = L.load()
    want = R.kernel_name(dt, plan.form, plan.bn, up)
    assert ops.conv_kernel_name(d) == want and ops.conv_kernel_name(d, with_workspace=True) == want, (plan, ops.conv_kernel_name(d))
    assert L.check_count(lib.uz_conv_igemm_grid_m(byref(d)), "grid_m") == plan.grid_m, plan
    assert L.check_count(lib.uz_conv_igemm_workspace_bytes(byref(d)), "workspace") == 0


@pytest.mark.parametrize("c", CASES)
def test_case_walks_under_the_restated_plan(c):
    N, H, W = R.MAPS[c.map].shape
    plan = R.case_plan(c)
    R.assert_walks(c, plan)
    if c.dt == BF16:
        for cus in (R.CUS, R.CUS_HW):
            assert P.pp_plan(N, H, W, c.cin, c.nout, cus, c.up) is None
    full = R.case_plan(c, R.CUS_HW)                  # the whole chip: the same kernel, so a launch without the reserve compares
    assert (full.form, full.tw, full.th, full.bn, full.slabs) == (plan.form, plan.tw, plan.th, plan.bn, plan.slabs), (full, plan)
    assert R.kernel_name(c.dt, full.form, full.bn, c.up) == R.case_kernel_name(c)


def test_the_table_covers_every_instantiation():
    """every (dtype, form, bn, TW) of the plain forward, every slab count 1 .. 4 of the fp32 streaming forms and 2 .. 4 of the
    bf16 ones, a channel tail, a partial slab and an upsampled read per kernel family"""
    have = {(c.dt, c.form, c.bn, R.MAPS[c.map].tw) for c in R.PLAIN}
    want = {(dt, form, bn, tw) for dt in (F32, BF16) for form, bn in (("resident", 64), ("stream", 64), ("stream", 128))
            for tw in (16, 32)} | {(BF16, "res64", 64, 16), (BF16, "res64", 64, 32)}
    assert have == want, have ^ want
    for dt, lo in ((F32, 1), (BF16, 2)):
        for bn in (64, 128):
            slabs = {c.slabs for c in R.PLAIN if (c.dt, c.form, c.bn) == (dt, "stream", bn)}
            # the 64-channel fp32 form with one slab is the resident one
            assert slabs >= set(range(2 if bn == 64 else lo, 5)), (dt, bn, slabs)
    assert {c.slabs for c in R.PLAIN if c.dt == F32 and c.form == "stream"} == {1, 2, 3, 4}
    for fam in ("resident", "stream", "res64"):
        cs = [c for c in R.PLAIN if c.form == fam]
        assert any(c.up for c in cs) and any(c.nout % c.bn for c in cs), fam
    assert any(c.cin % 64 for c in R.PLAIN if c.dt == BF16 and c.form == "stream")          # a partial last slab
    assert {(c.form, c.bn, R.MAPS[c.map].tw) for c in R.BNRED} == {("resident", 64, 32), ("stream", 64, 16), ("stream", 128, 32),
                                                                 ("stream", 128, 16)}
    assert {(c.dt, c.form, c.bn) for c in R.ACT} == {(F32, "resident", 64), (F32, "stream", 128), (BF16, "resident", 64),
                                                     (BF16, "stream", 64), (BF16, "stream", 128)}
    assert {(c.dt, c.form) for c in R.NORMAL} == {(dt, f) for dt in (F32, BF16) for f in ("resident", "stream")} | {(BF16, "res64")}


@pytest.mark.parametrize("c", CASES)
def test_restated_plan_is_the_library_plan(c):
    """the host-side queries need no device; windows of wider buffers (ldx > Cin, ldy > Nout) change nothing"""
    N, H, W = R.MAPS[c.map].shape
    for reserve in (R.RESERVE, 0):
        L.set_cu_reserve(reserve)
        plan = R.case_plan(c, R.CUS_HW - reserve)
        for d in (_desc(c.dt, N, H, W, c.cin, c.nout, c.up), _desc(c.dt, N, H, W, c.cin, c.nout, c.up, c.cin + 40, c.nout + 96)):
            _assert_library_agrees(d, c.dt, plan, c.up)


# dt, (N, H, W), Cin, Nout, up, UZ_NUM_CU -> (form, tw, th, bn, ntiles, tiles_n, grid_m, slabs), each worked by hand from the rule
HAND = [
    # 16 x 16 tiles: 2 * 1 * 2 = 4 of them; Nout 64 -> bn 64; Cin 64 != 32 -> streaming, two slabs
    (F32, (2, 12, 20), 64, 64, False, 256, ("stream", 16, 16, 64, 4, 1, 4, 2)),
    # the same in bf16: Cin == 64 && Nout <= 64 is excluded from res64 and Cin == bk: resident
    (BF16, (2, 12, 20), 64, 64, False, 256, ("resident", 16, 16, 64, 4, 1, 4, 1)),
    # one more output chunk and the exclusion no longer holds: res64, two N tiles of 64
    (BF16, (2, 12, 20), 64, 72, False, 256, ("res64", 16, 16, 64, 4, 2, 4, 1)),
    (BF16, (2, 12, 20), 32, 64, False, 256, ("res64", 16, 16, 64, 4, 1, 4, 1)),
    # 8 x 32 tiles: 4 * 1 = 4; Nout 200 -> bn 128, tn 2; 4 * 2 <= 128 -> bn 64; Cin == 32: resident; four N tiles, cap 64
    (F32, (1, 32, 32), 32, 200, False, 256, ("resident", 32, 8, 64, 4, 4, 4, 1)),
    # 16 * 4 = 64 tiles, tn 2: 128 <= 256 / 2 flips to bn 64 (four N tiles, cap 64) ...
    (F32, (16, 32, 32), 64, 200, False, 256, ("stream", 32, 8, 64, 64, 4, 64, 2)),
    # ... and 128 <= 128 / 2 does not: bn 128, two N tiles, cap 64
    (F32, (16, 32, 32), 64, 200, False, 128, ("stream", 32, 8, 128, 64, 2, 64, 2)),
    # 17 <= W <= 31 is not the ping-pong kernel's; 2 * 2 * 2 = 8 tiles, tn 2: 16 <= 128 -> bn 64, four N tiles
    (BF16, (2, 20, 20), 128, 200, False, 256, ("stream", 16, 16, 64, 8, 4, 8, 2)),
    # Cin % 32 != 0 is not the ping-pong kernel's either: 3 * 4 * 2 = 24 tiles x tn 1 -> no flip question, bn 64; 72 / 64: 2 slabs
    (BF16, (3, 32, 64), 72, 64, True, 256, ("stream", 32, 8, 64, 24, 1, 24, 2)),
    # a walk: 129 * 1 * 2 = 258 tiles on 128 CUs
    (F32, (129, 12, 20), 32, 64, False, 128, ("resident", 16, 16, 64, 258, 1, 128, 1)),
    # fp32 takes Cin in multiples of 4: 12 channels are one partial slab of the streaming form
    (F32, (1, 16, 16), 12, 8, False, 256, ("stream", 16, 16, 64, 1, 1, 1, 1)),
    # the ping-pong kernel takes it / the channel multiples fail
    (BF16, (3, 128, 256), 64, 128, False, 256, None),
    (BF16, (1, 16, 16), 12, 64, False, 256, None),
    (F32, (1, 16, 16), 32, 6, False, 256, None),
]


@pytest.mark.parametrize("dt,shape,cin,nout,up,cus,want", HAND)
def test_restated_plan_on_hand_worked_descriptors(dt, shape, cin, nout, up, cus, want):
    N, H, W = shape
    plan = R.direct_plan(dt, N, H, W, cin, nout, cus, up)
    assert (None if plan is None else tuple(plan)) == want
    if plan is None:
        if cin % (8 if dt == BF16 else 4) == 0 and nout % (8 if dt == BF16 else 4) == 0:
            L.set_cu_reserve(R.CUS_HW - cus)
            assert ops.conv_kernel_name(_desc(dt, N, H, W, cin, nout, up)).startswith("conv3x3_pp")
        return
    L.set_cu_reserve(R.CUS_HW - cus)
    _assert_library_agrees(_desc(dt, N, H, W, cin, nout, up), dt, plan, up)


def _case_refs(c):
    """every exact reference the GPU file may form for a case, as (name, float64 tensor, whether statistics are formed of it)"""
    pre = R.plain_ref(c)
    scale, shift = R.act_vectors(c)
    return ([("conv + bias", pre, True), ("gradient", R.plain_ref(c, with_bias=False), True)]
            + [(f"act relu={relu}", R.act_ref(pre, scale, shift, relu), False) for relu in (0, 1)])


@pytest.mark.parametrize("c", CASES)
def test_preconditions_of_exactness(c):
    for name, ref, sums in _case_refs(c):
        got = R.assert_exact_preconditions(ref, sums)
        assert not sums or got[1] < 2 ** 23, (name, got)              # with room: half of what the exact sums allow
    if c.dt == BF16 and c.form != "res64":
        R.bnred_operands(c, R.plain_ref(c, with_bias=False))          # asserts its own 2^22 bounds
    o = R.operands(c)
    for t in (o.x, o.w, o.b):
        assert torch.equal(t.to(BF16).float(), t)


def test_fp32_convolution_on_integers_is_the_float64_one():
    """once, on the smallest case: F.conv2d in fp32 is exact on these operands"""
    c = min((c for c in R.ALL_CASES if not c.up), key=lambda c: R.MAPS[c.map].shape[0] * c.cin)
    o = R.operands(c)
    want = R.nhwc(F.conv2d(o.x.double(), o.w.double(), None, padding=1))
    assert torch.equal(o.prod.double(), want)


# ---- planted faults ---------------------------------------------------------------------------------------------------------
FAULT_CASE = next(c for c in R.PLAIN if (c.dt, c.form, c.map, c.cin, c.nout) == (F32, "stream", "B32", 32, 200))   # 198 / 64: trips 0 .. 3


def _fault_ground():
    c = FAULT_CASE
    shape, plan = R.MAPS[c.map].shape, R.case_plan(c)
    ref64 = R.plain_ref(c)
    return c, shape, plan, ref64, R.tile_of_pixels(shape, plan)


def test_comparators_pass_the_reference_itself():
    c, shape, plan, ref64, tiles = _fault_ground()
    for dt in (BF16, F32):
        R.assert_same(ref64.to(dt), ref64.to(dt), shape, plan)
    rows = R.stats_rows(ref64, shape, plan).float()
    R.check_rows(rows, ref64, shape, plan)
    R.check_stats(rows, ref64, plan)


@pytest.mark.parametrize("trip", [1, 2, 3])
def test_comparator_names_the_trip_of_an_altered_tile(trip):
    """one tile of a late trip altered -- here: computed without its bias, as a tile whose accumulators started from the
    wrong values would be -- is reported with that trip and that tile alone"""
    c, shape, plan, ref64, tiles = _fault_ground()
    tile = trip * plan.grid_m + 5
    assert tile < plan.ntiles
    o = R.operands(c)
    ref = ref64.float()
    got = ref.clone()
    got[tiles == tile] -= o.b[:c.nout]
    with pytest.raises(AssertionError) as e:
        R.assert_same(got, ref, shape, plan)
    msg = str(e.value)
    assert f"in 1 of {plan.ntiles} 8 x 32 tiles" in msg and f"trips [{trip}] of a grid of {plan.grid_m}" in msg, msg
    assert str(R.decode(tile, shape, plan)) in msg, msg


def test_comparator_sees_one_ulp_in_a_tile_of_the_last_trip():
    c, shape, plan, ref64, tiles = _fault_ground()
    tile = plan.ntiles - 1                            # the ragged corner tile of the last image
    pix = int((tiles == tile).nonzero()[-1])
    ref = ref64.to(BF16)
    got = ref.clone()
    got.view(torch.int16)[pix, 199] += 1              # the next bf16, in the channel tail of the second N tile
    assert got[pix, 199] != ref[pix, 199]
    with pytest.raises(AssertionError) as e:
        R.assert_same(got, ref, shape, plan)
    msg = str(e.value)
    assert f"1 of {ref.shape[0]} pixels differ in 1 of 198" in msg and "trips [3]" in msg and "first [199]" in msg, msg


def test_rows_check_sees_a_tile_moved_between_workgroups():
    """the sums of one tile of trip 2 credited to the neighbouring workgroup: the totals are what they were, so
    check_stats() passes; the rows are not, and check_rows() names both workgroups"""
    c, shape, plan, ref64, tiles = _fault_ground()
    rows = R.stats_rows(ref64, shape, plan)
    tile = 2 * plan.grid_m + 9
    part = ref64[tiles == tile]
    for k, v in enumerate((part.sum(0), (part * part).sum(0))):
        rows[9, k] -= v
        rows[10, k] += v
    R.check_stats(rows.float(), ref64, plan)
    with pytest.raises(AssertionError, match=r"2 of 64 workgroups differ \(first \[9, 10\]\); workgroup 9, ") as e:
        R.check_rows(rows.float(), ref64, shape, plan)
    assert "(2, " in str(e.value)                     # the parts of workgroup 9's tiles are listed by trip


def test_rows_check_sees_one_tile_missing_from_a_workgroup():
    c, shape, plan, ref64, tiles = _fault_ground()
    rows = R.stats_rows(ref64, shape, plan)
    tile = 3 * plan.grid_m + 2                        # the last trip of workgroup 2
    part = ref64[tiles == tile]
    rows[2, 0] -= part.sum(0)
    rows[2, 1] -= (part * part).sum(0)
    with pytest.raises(AssertionError, match=r"1 of 64 workgroups differ \(first \[2\]\)"):
        R.check_rows(rows.float(), ref64, shape, plan)
    with pytest.raises(AssertionError, match="sum y"):
        R.check_stats(rows.float(), ref64, plan)
