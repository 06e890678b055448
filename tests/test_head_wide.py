"""CPU: the wide 1x1 head's entries (uz_head_wide_*, uz_head_wide.hip) as far as they go without a GPU -- the support
predicate over its edges, the workspace query, the grid's independence of the CU reserve, and the refusals, which come
with a message naming the entry before anything is launched."""
import ctypes

import pytest

from unet_zoo_amd import _lib

F32, BF16 = _lib.UZ_F32, _lib.UZ_BF16


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_exports_are_declared(lib):
    for name in ("uz_head_wide_supported", "uz_head_wide_grid", "uz_head_wide_fwd", "uz_head_wide_bwd_workspace_bytes",
                 "uz_head_wide_bwd"):
        assert name in _lib.EXPORTS and hasattr(lib, name)


@pytest.mark.parametrize("dtype,vec", [(F32, 4), (BF16, 8)], ids=["fp32", "bf16"])
def test_supported_over_the_edges(lib, dtype, vec):
    for K in (0, 1, 32, 33):
        for C in (4, 8, 12, 512, 520):
            want = int(1 <= K <= 32 and C % vec == 0 and C <= 512)
            assert lib.uz_head_wide_supported(dtype, C, K) == want, (dtype, C, K)
    assert lib.uz_head_wide_supported(7, 64, 9) == 0 and lib.uz_head_wide_supported(dtype, 0, 9) == 0
    assert lib.uz_head_wide_supported(dtype, -8, 9) == 0


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_workspace_is_positive_and_non_decreasing_in_k_and_c(lib, dtype):
    N, HW = 3, 1000
    last_k = 0
    for K in (1, 8, 9, 16, 17, 32):
        last_c = 0
        for C in (8, 16, 32, 64, 96, 128, 256, 512):
            b = lib.uz_head_wide_bwd_workspace_bytes(dtype, N, HW, C, K)
            assert b > 0 and b % 4 == 0 and b >= last_c, (K, C, b, last_c)
            last_c = b
        b64 = lib.uz_head_wide_bwd_workspace_bytes(dtype, N, HW, 64, K)
        assert b64 >= last_k
        last_k = b64
    assert lib.uz_head_wide_bwd_workspace_bytes(dtype, N, HW, 64, 33) == -1
    assert b"uz_head_wide_bwd_workspace_bytes" in lib.uz_last_error_string()
    assert lib.uz_head_wide_bwd_workspace_bytes(dtype, 1 << 16, 1 << 15, 64, 9) == -1      # N * HW = 2^31


def test_grid_does_not_follow_the_cu_reserve(lib):
    shapes = [(BF16, 16, 256 * 256, 64, 19), (F32, 2, 64 * 96, 64, 9), (BF16, 3, 35, 8, 32), (F32, 16, 512 * 512, 512, 32)]
    try:
        assert lib.uz_set_cu_reserve(0) == 0
        g0 = [lib.uz_head_wide_grid(*s) for s in shapes]
        w0 = [lib.uz_head_wide_bwd_workspace_bytes(*s) for s in shapes]
        assert lib.uz_set_cu_reserve(128) == 0
        assert [lib.uz_head_wide_grid(*s) for s in shapes] == g0
        assert [lib.uz_head_wide_bwd_workspace_bytes(*s) for s in shapes] == w0      # the partial rows: the backward's grid
    finally:
        lib.uz_set_cu_reserve(0)
    assert all(g >= 1 for g in g0) and g0[2] == 1          # 105 pixels: one tile
    assert g0[0] == g0[3]                                   # both saturate the persistent grid
    assert lib.uz_head_wide_grid(BF16, 16, 65536, 64, 33) == -1 and b"uz_head_wide_grid" in lib.uz_last_error_string()


def test_bad_arguments_are_refused_before_any_launch(lib):
    buf = (ctypes.c_float * 4096)()       # host memory: a call that got as far as a launch would fail differently
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(dtype=BF16, x=p, ldx=64, N=1, HW=16, C=64, w=p, b=p, K=9, out=p):
        return lib.uz_head_wide_fwd(dtype, x, ldx, N, HW, C, w, b, K, out, None)

    def bwd(dtype=BF16, x=p, ldx=64, N=1, HW=16, C=64, w=p, K=9, g=p, dx=None, lddx=0, dw=p, db=p, ws=p):
        return lib.uz_head_wide_bwd(dtype, x, ldx, N, HW, C, w, K, g, dx, lddx, dw, db, ws, None)

    for call, name in ((fwd, b"uz_head_wide_fwd"), (bwd, b"uz_head_wide_bwd")):
        for kw, word in (({"K": 33}, b"K=33"), ({"K": 0}, b"K=0"), ({"ldx": 56}, b"ldx=56"), ({"x": None}, b"null pointer"),
                         ({"w": None}, b"null pointer"), ({"C": 520, "ldx": 520}, b"C=520"), ({"C": 12, "ldx": 16}, b"C=12"),
                         ({"dtype": 5}, b"bad dtype"), ({"N": 1 << 16, "HW": 1 << 15}, b"2^31"), ({"N": 0}, b"bad shape")):
            rc = call(**kw)
            msg = lib.uz_last_error_string()
            assert rc != 0 and name in msg and word in msg, (name, kw, rc, msg)
    assert fwd(out=None) != 0 and fwd(b=None) != 0
    assert bwd(g=None) != 0 and bwd(dw=None) != 0 and bwd(db=None) != 0 and bwd(ws=None) != 0
    assert bwd(dx=p, lddx=56) != 0 and b"lddx=56" in lib.uz_last_error_string()


def test_engine_routes_by_class_count():
    from unet_zoo_amd import ops
    assert ops.HEAD_NARROW_MAX_K == 8 and ops.HEAD_WIDE_MAX_K == 32
