"""CPU: the ground tests/test_wgrad_walk_gpu.py stands on, checked without a GPU (helper: tests/wgrad_walk_cases.py).

  * the launch plans of the weight-gradient family as restated in wgrad_walk_cases.py agree with the library's host-side
    queries (uz_wgrad_kernel_name, uz_wgrad_split, uz_wgrad_workspace_bytes, uz_wgrad_batched_workspace_bytes,
    uz_wgrad_multi_workspace_bytes answer without a device) for every case of the GPU file, under no reserve and under every
    reserve a case uses (and 37 and 128 besides);
  * every case reaches the loop state it exists for -- kernel family, slab count, K-steps of every pixel range, XCD remap on /
    off, a range that starts inside an image or a 128-wide row, a ragged last row -- and says so (run with -s to read it);
  * the tables as a whole cover what the issue lists: per one-tap tile nu in {1, 2, 3, 4, odd >= 5, even >= 6} and a last range
    of one step after full ones; per reduction form the slab counts around its two-splits-per-pass loop.

A case that stops reaching its state after a change of a plan fails here, in milliseconds, and not silently on the GPU."""
import ctypes
from ctypes import byref

import pytest

import wgrad_walk_cases as C  # tests/wgrad_walk_cases.py (pytest puts this directory on sys.path)
from unet_zoo_amd import _lib as L

RESERVES = sorted({0, 37, 128} | {c.reserve for c in C.PRODUCT_CASES} | {c.reserve for c in C.REDUCE_CASES}
                  | {c.reserve for c in C.BATCHED_CASES})


@pytest.fixture(autouse=True)
def _restore():
    yield
    L.set_cu_reserve(0)


def cdesc(d):
    return L.WgradDesc(L.UZ_BF16 if d.dt == "bf16" else L.UZ_F32, d.N, d.H, d.W, d.Hr, d.Wr, d.Ci, d.ldl, d.Cj, d.ldr, d.ntaps,
                       d.mode, d.dil)


def lib_name(d):
    buf = ctypes.create_string_buffer(96)
    L.check_count(L.load().uz_wgrad_kernel_name(byref(cdesc(d)), buf, 96), "uz_wgrad_kernel_name")
    return buf.value.decode()


def _agrees(d, reserve):
    lib = L.load()
    L.set_cu_reserve(reserve)
    cus = C.CUS_HW - reserve
    p = C.plan(d, cus)
    assert lib_name(d) == p["name"], (reserve, p)
    assert L.check_count(lib.uz_wgrad_split(byref(cdesc(d))), "uz_wgrad_split") == p["nslabs"], (reserve, p)
    assert L.check_count(lib.uz_wgrad_workspace_bytes(byref(cdesc(d))), "workspace") == C.workspace_bytes(d, cus), (reserve, p)


@pytest.mark.parametrize("c", [pytest.param(c, id=c.id) for c in C.PRODUCT_CASES])
def test_restated_plan_is_the_library_plan(c):
    """also with both operands as windows of wider buffers, as the GPU file hands them over"""
    for reserve in RESERVES:
        _agrees(c.d, reserve)
        _agrees(c.d._replace(ldl=c.d.Ci + 40, ldr=c.d.Cj + 24), reserve)


@pytest.mark.parametrize("c", [pytest.param(c, id=c.id) for c in C.PRODUCT_CASES])
def test_product_case_reaches_its_state(c):
    L.set_cu_reserve(c.reserve)
    assert lib_name(c.d) == c.name
    print("\n  " + C.check_claims(c, C.plan(c.d, C.CUS_HW - c.reserve)))


def test_one_tap_cases_cover_the_step_counts():
    """per tile: nu in {1, 2, 3, 4, an odd value >= 5, an even value >= 6}, nu = 1 as the whole problem and as the last range
    after full ones; ragged last rows of 1 and 63 pixels; two reserves that split one problem differently"""
    for tile in (C.T64, C.T128):
        cs = [c for c in C.PRODUCT_CASES if c.name == tile + "1tap"]
        nus = {n for c in cs for n in c.claims["nus"]}
        assert {1, 2, 3, 4} <= nus and any(n >= 5 and n % 2 for n in nus) and any(n >= 6 and n % 2 == 0 for n in nus), (tile, nus)
        assert any(c.claims["nus"] == [1] for c in cs)
        assert any(len(c.claims["nus"]) > 1 and c.claims["nus"][-1] == 1 and c.claims["nus"][0] > 1 for c in cs)
    assert {1, 63} <= {c.claims.get("ragged") for c in C.PRODUCT_CASES if c.name.endswith("1tap")}
    a, b = [c for c in C.PRODUCT_CASES if c.id.startswith("1tap128-512x512")]
    assert a.d == b.d and a.reserve != b.reserve and a.claims["nus"] != b.claims["nus"]


def test_gather_and_nine_tap_cases_cover_their_states():
    for fam in ("gather9", "dilated9"):
        for tile in (C.T64, C.T128):
            cs = [c for c in C.PRODUCT_CASES if c.name == tile + fam]
            nus = {n for c in cs for n in c.claims["nus"]}
            assert any(n % 2 for n in nus) and any(n % 2 == 0 for n in nus), (tile, fam, nus)
            assert any(c.claims.get("mid_image") and c.d.N > 1 for c in cs), (tile, fam)
        assert any(c.claims["nus"][-1] < c.claims["nus"][0] for c in C.PRODUCT_CASES if c.name.endswith(fam)), fam
    s2 = [c for c in C.PRODUCT_CASES if c.name.endswith("gather9")]
    assert any(c.d.Hr % 2 and c.d.Wr % 2 and len(c.claims["nus"]) > 1 for c in s2)
    assert any(c.claims["nus"][-1] < c.claims["nus"][0] for c in s2)
    assert {c.d.dil for c in C.PRODUCT_CASES if c.name.endswith("dilated9")} == {2, 8}
    names = {c.name for c in C.PRODUCT_CASES}
    assert {C.T128 + "3tap", "wgrad3x3_bf16_128x64_9tap", "wgrad3x3_bf16_64x128_9tap", C.T64 + "9tap"} <= names
    three = [c for c in C.PRODUCT_CASES if c.name.endswith("3tap")]
    assert {c.claims["remap"] for c in three} == {True, False} and any(c.claims.get("mid_row") for c in three)
    short = {(c.d.W, c.d.H) for c in C.PRODUCT_CASES if c.name.endswith(("3tap", "9tap"))}
    assert {(16, 4), (16, 8), (16, 12), (32, 2), (32, 4), (32, 8)} <= short and any(w == 64 for w, h in short) \
        and any(w == 128 and h <= 4 for w, h in short)
    for fam in ("3tap", "9tap"):
        assert any(c.d.mode == C.CONV_UP2 for c in C.PRODUCT_CASES if c.name.endswith(fam))


def test_generic_cases_cover_their_states():
    gen = [c for c in C.PRODUCT_CASES if c.name.startswith(("wgrad_fp32", "wgrad_bf16"))]
    assert {c.name for c in gen} == {"wgrad_fp32_64x64", "wgrad_fp32_128x128", "wgrad_bf16_64x64", "wgrad_bf16_128x128"}
    for dt in ("fp32", "bf16"):
        assert any("img_wraps" in c.claims and c.d.dt == dt for c in gen)
        assert any(c.claims.get("ragged_chunks") and c.d.dt == dt for c in gen)
    f32 = [c.d for c in gen if c.d.dt == "fp32"]
    assert {5, 7} <= {d.W for d in f32}
    assert {(C.CONV, 1), (C.CONV, 9), (C.CONV_UP2, 9), (C.GATHER2X2, 4)} <= {(d.mode, d.ntaps) for d in f32}
    assert any(d.dil == 2 for d in f32) and any(d.dil > max(d.H, d.W) for d in f32)
    assert {(0, 0), (1, 1)} <= {(d.Hr - 2 * d.H, d.Wr - 2 * d.W) for d in f32 if d.mode == C.GATHER2X2}
    assert {8, 12, 20} <= {c.d.W for c in gen if c.d.dt == "bf16"}


@pytest.mark.parametrize("c", [pytest.param(c, id=c.id) for c in C.REDUCE_CASES])
def test_reduction_case_gets_its_form_and_slab_count(c):
    for reserve in RESERVES:
        _agrees(c.d, reserve)
    L.set_cu_reserve(c.reserve)
    n = L.check_count(L.load().uz_wgrad_split(byref(cdesc(c.d))), "uz_wgrad_split")
    assert n == c.nslabs and C.reduce_form(c.d, n) == c.form, (n, C.reduce_form(c.d, n))
    print(f"\n  {c.id}: {c.form}, nslabs {n}, Ci Cj {c.d.Ci * c.d.Cj}, planned by {lib_name(c.d)}")


def test_reduction_cases_cover_the_loop_edges():
    """ZG = 4: {1, 2 | 3, 4, 5, 8, 9, 30 | 31}; ZG = 16: {32, 40, 48, >= 56} (32 = 2 ZG, 40 = 2 ZG + tail, 48 = 3 ZG); the flat form
    with Ci Cj = 64 and with a workgroup across a tap boundary; Ci Cj % 64 != 0 on every element-wise form"""
    by = {}
    for c in C.REDUCE_CASES:
        by.setdefault(c.form, set()).add(c.nslabs)
    assert {1, 2, 4, 5, 8, 9} <= by["reduce<9,4>"] and by["reduce<9,4>"] & {30, 31}
    for f in ("reduce<9,16>", "flat<9,16>"):
        assert {32, 40, 48} <= by[f] and max(by[f]) >= 56
    for f in ("reduce<4,4>", "reduce<1,4>"):
        assert {1, 3, 4, 5, 8, 9} <= by[f]
    flat = [c.d.Ci * c.d.Cj for c in C.REDUCE_CASES if c.form == "flat<9,16>"]
    assert 64 in flat and any(256 % n and n < 256 for n in flat) and all(n <= 64 * 128 for n in flat)
    assert all(c.d.Ci * c.d.Cj > 64 * 128 for c in C.REDUCE_CASES if c.form == "reduce<9,16>")
    for f in ("reduce<9,4>", "reduce<9,16>", "reduce<4,4>", "reduce<1,4>"):
        assert any((c.d.Ci * c.d.Cj) % 64 and c.d.dt == "fp32" for c in C.REDUCE_CASES if c.form == f), f
    assert all(any(c.random for c in C.REDUCE_CASES if c.form == f) for f in by)


@pytest.mark.parametrize("c", [pytest.param(c, id=c.id) for c in C.BATCHED_CASES])
def test_batched_case_reaches_its_state(c):
    lib = L.load()
    d = C.batched_desc(c)
    for reserve in RESERVES:
        L.set_cu_reserve(reserve)
        got = L.check_count(lib.uz_wgrad_batched_workspace_bytes(byref(cdesc(d)), c.batch * c.heads), "workspace")
        assert got == C.batched_workspace_bytes(d, c.batch * c.heads, C.CUS_HW - reserve), reserve
    print("\n  " + C.check_batched_claims(c))


def test_batched_cases_cover_their_states():
    cs = C.BATCHED_CASES
    assert any(len(c.nus) == 1 and c.gap for c in cs) and any(len(c.nus) > 1 for c in cs)
    assert any(c.heads > 1 and c.C != c.KV and len(c.nus) > 1 for c in cs) and any(c.forced for c in cs)


@pytest.mark.parametrize("c", [pytest.param(c, id=c.id) for c in C.MULTI_CASES])
def test_multi_case_reaches_its_state(c):
    lib = L.load()
    ds = C.multi_descs(c)
    arr = (L.WgradItem * len(ds))()
    for i, d in enumerate(ds):
        arr[i] = L.WgradItem(cdesc(d), None, None, None)
    for reserve in RESERVES:
        L.set_cu_reserve(reserve)
        got = L.check_count(lib.uz_wgrad_multi_workspace_bytes(arr, len(ds)), "workspace")
        assert got == C.multi_plan(ds, C.CUS_HW - reserve)[1], reserve
    print("\n  " + C.check_multi_claims(c)[0])


def test_phase1_and_random_cases_cover_every_main_kernel_form():
    forms = {c.name for c in C.PRODUCT_CASES}
    assert {c.name for c in C.PRODUCT_CASES if c.phase1} == forms
    assert {c.name for c in C.PRODUCT_CASES if c.random} == forms
