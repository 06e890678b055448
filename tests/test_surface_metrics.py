"""CPU: SurfaceMetrics' surface and the checker of its GPU tests.

tests/surface_ref.py (numpy, brute force over surface-pixel pairs) is pinned against scipy: its surface against
binary_erosion with the cross, its distances against distance_transform_edt, its percentile against numpy.percentile.  Also
here: fixed cases with answers derived by hand, the argument checks of SurfaceMetrics, the refusals of the three ABI entries
(the library loads without a GPU), the workspace size and the exports."""
import ctypes
import math

import numpy as np
import pytest
import torch

import surface_ref as R  # tests/surface_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from unet_zoo_amd import _lib
from unet_zoo_amd.surface import SurfaceMetrics


# ---- the reference against scipy -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(24))
def test_reference_equals_scipy(seed):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(1000 + seed)
    H, W = int(rng.randint(5, 71)), int(rng.randint(5, 71))
    A, B = R.blobs((H, W), 2 * seed, count=1 + seed % 3), R.blobs((H, W), 2 * seed + 1, count=1 + (seed // 3) % 3)
    if seed % 3 == 0:                                   # a third of the pairs: ragged masks
        A ^= rng.rand(H, W) < 0.05
        B ^= rng.rand(H, W) < 0.05
    if not A.any() or not B.any():
        A[H // 2, W // 2] = B[0, 0] = True
    q = [95.0, 50.0, 100.0, 37.5][seed % 4]
    spacing = [1.0, 0.75][seed % 2]
    cross = ndi.generate_binary_structure(2, 1)
    sa, sb = A & ~ndi.binary_erosion(A, cross), B & ~ndi.binary_erosion(B, cross)
    assert np.array_equal(R.surface(A), sa) and np.array_equal(R.surface(B), sb)
    dab = ndi.distance_transform_edt(~sb)[sa]
    dba = ndi.distance_transform_edt(~sa)[sb]
    both = np.concatenate([dab, dba])
    want = (spacing * both.max(), spacing * np.percentile(both, q), spacing * 0.5 * (dab.mean() + dba.mean()))
    got, stats = R.pair(A, B, q, spacing)
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-12 * abs(w), (g, w)
    assert stats[0] == sa.sum() and stats[1] == sb.sum() and stats[5] == 0 and stats[6] == A.sum() and stats[7] == B.sum()
    assert stats[2] == round(both.max() ** 2)


# ---- fixed cases, derived by hand -------------------------------------------------------------------------------------------
def _one(shape, *pixels):
    m = np.zeros(shape, dtype=bool)
    for p in pixels:
        m[p] = True
    return m


def test_single_pixel_against_single_pixel():
    # (1, 2) against (4, 6): d2 = 9 + 16 = 25 both ways, n = 2: every statistic is 5 pixels
    (hd, hdq, assd), st = R.pair(_one((7, 9), (1, 2)), _one((7, 9), (4, 6)), 95.0, 2.0)
    assert (hd, hdq, assd) == (10.0, 10.0, 10.0)
    assert st.tolist() == [1, 1, 25, 25, 25, 0, 1, 1]


def test_identical_masks_are_at_distance_zero():
    A = R.blobs((23, 31), 7)
    (hd, hdq, assd), st = R.pair(A, A.copy())
    assert (hd, hdq, assd) == (0.0, 0.0, 0.0) and st[2:6].tolist() == [0, 0, 0, 0] and st[0] == st[1] > 0


def test_full_picture_mask_has_the_frame_as_its_surface():
    H, W = 9, 12
    full = np.ones((H, W), dtype=bool)
    frame = full.copy()
    frame[1:-1, 1:-1] = False
    assert np.array_equal(R.surface(full), frame)
    # against the centre pixel (4, 6): the farthest frame pixel is a corner, (0, 0): 16 + 36; the centre pixel is 4 from row 0
    (hd, hdq, assd), st = R.pair(full, _one((H, W), (4, 6)), 100.0)
    assert st[0] == 2 * H + 2 * W - 4 and st[1] == 1 and st[6] == H * W
    assert st[2] == 52 and hd == math.sqrt(52.0) and hdq == hd
    d = np.sqrt(((np.argwhere(frame) - np.array([4, 6])) ** 2).sum(1))
    assert abs(assd - 0.5 * (d.mean() + 4.0)) < 1e-14


def test_one_row_picture():
    # 1 x W: every pixel of a mask is a surface pixel (rows above and below are outside the picture)
    A, B = np.zeros((1, 20), dtype=bool), np.zeros((1, 20), dtype=bool)
    A[0, 2:5] = True          # 2, 3, 4
    B[0, 10:12] = True        # 10, 11
    (hd, hdq, assd), st = R.pair(A, B, 50.0)
    # A -> B: 8, 7, 6;  B -> A: 6, 7;  sorted d: 6 6 7 7 8, n = 5, r = 2: the median is 7
    assert st.tolist() == [3, 2, 64, 49, 49, 0, 3, 2]
    assert (hd, hdq) == (8.0, 7.0) and abs(assd - 0.5 * (7.0 + 6.5)) < 1e-15


def test_states_and_the_class_formulation():
    A = R.blobs((12, 12), 3)
    Z = np.zeros_like(A)
    for a, b, state in ((Z, A, 1), (A, Z, 2), (Z, Z, 3)):
        vals, st = R.pair(a, b)
        assert vals == (0.0, 0.0, 0.0) and st[5] == state and st[2:5].tolist() == [0, 0, 0]
    # classes(): an ignored pixel is in no mask, ties go to the lowest class
    logits = np.zeros((1, 3, 4, 4))
    logits[0, 2, :2] = 1.0
    labels = np.full((1, 4, 4), 2)
    labels[0, 0, 0] = -100
    labels[0, 3, 3] = 7
    out, st = R.classes(logits, labels)
    assert st[0, :, 5].tolist() == [3, 0] and st[0, 1, 6] == 7 and st[0, 1, 7] == 14      # class 1 nowhere; class 2: 8 - 1, 16 - 2


# ---- SurfaceMetrics' own checks (no GPU) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,word", [
    (dict(percentile=0.0), "percentile"), (dict(percentile=100.5), "percentile"), (dict(percentile=float("nan")), "percentile"),
    (dict(percentile="x"), "percentile"), (dict(spacing=0.0), "spacing"), (dict(spacing=-1.0), "spacing"),
    (dict(spacing=float("inf")), "spacing"), (dict(ignore_index=2 ** 31), "ignore_index"), (dict(ignore_index=1.5), "ignore_index"),
    (dict(ignore_index=True), "ignore_index")])
def test_constructor_refuses_bad_arguments_by_name(kw, word):
    with pytest.raises(ValueError, match=word):
        SurfaceMetrics(**kw)


def test_call_refuses_bad_tensors_before_any_kernel():
    m = SurfaceMetrics()
    x = torch.zeros(2, 3, 16, 16)
    with pytest.raises(ValueError, match="logits"):
        m(torch.zeros(2, 16, 16), torch.zeros(2, 16, 16))
    with pytest.raises(ValueError, match="logits"):
        m(x.double(), torch.zeros(2, 3, 16, 16))
    with pytest.raises(ValueError, match="target of shape"):
        m(x, torch.zeros(2, 1, 16, 16))
    with pytest.raises(ValueError, match="target of shape"):
        m(x, torch.zeros(2, 16, 8, dtype=torch.int64))
    with pytest.raises(ValueError, match="K = 1"):
        m(torch.zeros(2, 1, 16, 16), torch.zeros(2, 16, 16, dtype=torch.int64))
    with pytest.raises(ValueError, match="target must be"):
        m(x, torch.zeros(2, 3, 16, 16, dtype=torch.bool))
    with pytest.raises(ValueError, match="at most 4096"):
        m(torch.zeros(1, 1, 1, 4097), torch.zeros(1, 1, 1, 4097))
    with pytest.raises(RuntimeError, match="no call yet"):
        m.hd
    with pytest.raises(_lib.HipLibraryError):                              # good arguments on the CPU: no fallback
        m({"d0": x, "d1": x}, torch.zeros(2, 3, 16, 16))
    with pytest.raises(TypeError, match="SurfaceMetrics"):
        unet_zoo_amd.GraphedEval(unet_zoo_amd.create_model("unet"), surface=object())


# ---- the ABI without a GPU ---------------------------------------------------------------------------------------------------
def _desc(mode=_lib.SURFACE_BINARY, N=2, C=1, H=16, W=16, first=0, ign=-100, q=95.0, spacing=1.0):
    return _lib.SurfaceDesc(mode, N, C, H, W, first, ign, 0, q, spacing)


CLS = _lib.SURFACE_CLASS


@pytest.mark.parametrize("kw,word", [
    (dict(mode=2), b"mode"), (dict(mode=-1), b"mode"), (dict(N=0), b"shape"), (dict(C=0), b"shape"), (dict(H=0), b"shape"),
    (dict(W=-3), b"shape"), (dict(H=4097), b"above 4096"), (dict(W=4097), b"above 4096"),
    (dict(mode=CLS, C=1, first=0), b"K ="), (dict(mode=CLS, C=33, first=1), b"K ="), (dict(mode=CLS, C=3, first=3), b"first_class"),
    (dict(mode=CLS, C=3, first=-1), b"first_class"), (dict(q=0.0), b"q outside"), (dict(q=100.0001), b"q outside"),
    (dict(q=float("nan")), b"q outside"), (dict(spacing=0.0), b"spacing"), (dict(spacing=-2.0), b"spacing"),
    (dict(spacing=float("inf")), b"spacing"), (dict(spacing=float("nan")), b"spacing"),
    (dict(N=128, C=1, H=4096, W=4096), b"too large"), (dict(mode=CLS, N=8, C=16, first=1, H=4096, W=4096), b"too large")])
def test_bad_descriptor_is_rejected_without_a_gpu(kw, word):
    lib = _lib.load()
    d = _desc(**kw)
    assert lib.uz_surface_workspace_bytes(ctypes.byref(d)) == -1 and word in lib.uz_last_error_string()
    assert lib.uz_surface_grid(ctypes.byref(d), None) == -1 and word in lib.uz_last_error_string()
    # the launch entry point makes the same check before it touches a pointer
    assert lib.uz_surface_metrics(ctypes.byref(d), None, None, None, None, None, None) == -1
    assert word in lib.uz_last_error_string()


def test_null_pointers_misalignment_and_overlaps_are_refused_without_a_gpu():
    lib = _lib.load()
    assert lib.uz_surface_workspace_bytes(None) == -1 and b"null descriptor" in lib.uz_last_error_string()
    assert lib.uz_surface_grid(None, None) == -1 and b"null descriptor" in lib.uz_last_error_string()
    assert lib.uz_surface_metrics(None, None, None, None, None, None, None) == -1 and b"null descriptor" in lib.uz_last_error_string()
    d = _desc()
    good = [0x100000, 0x200000, 0x300000, 0x400000, 0x10000000]          # logits, target, out, stats, workspace: never read
    for k in range(5):
        args = list(good)
        args[k] = None
        assert lib.uz_surface_metrics(ctypes.byref(d), *args, None) == -1 and b"null pointer" in lib.uz_last_error_string()
    for k, off, word in ((0, 2, b"4-byte"), (1, 1, b"4-byte"), (2, 2, b"4-byte"), (3, 4, b"8-byte"), (4, 8, b"16-byte")):
        args = list(good)
        args[k] += off
        assert lib.uz_surface_metrics(ctypes.byref(d), *args, None) == -1 and word in lib.uz_last_error_string()
    nbytes = 4 * 2 * 16 * 16
    ws = lib.uz_surface_workspace_bytes(ctypes.byref(d))
    for a, b, delta in ((1, 0, 0), (1, 0, nbytes - 4), (2, 0, 16), (3, 1, 8), (2, 3, 0), (3, 2, 8), (0, 4, 16), (2, 4, ws - 16),
                        (3, 4, ws // 32 * 16)):
        args = list(good)
        args[a] = good[b] + delta
        assert lib.uz_surface_metrics(ctypes.byref(d), *args, None) == -1 and b"overlap" in lib.uz_last_error_string(), (a, b)


def test_workspace_bytes_are_positive_and_monotone():
    lib = _lib.load()
    last = 0
    for N, C, H, W in ((1, 1, 1, 1), (1, 1, 8, 8), (1, 1, 37, 53), (2, 1, 37, 53), (2, 3, 37, 53), (2, 3, 256, 256), (16, 3, 256, 256)):
        b = lib.uz_surface_workspace_bytes(ctypes.byref(_desc(N=N, C=C, H=H, W=W)))
        assert b > last and b % 16 == 0, (N, C, H, W, b)
        last = b
    last = 0
    for first in (8, 5, 1, 0):                          # more pairs per image: more workspace
        b = lib.uz_surface_workspace_bytes(ctypes.byref(_desc(mode=CLS, N=2, C=9, H=64, W=64, first=first)))
        assert b > last
        last = b


def test_launch_plan_caps_the_grid():
    lib = _lib.load()
    units = ctypes.c_int(0)
    assert lib.uz_surface_grid(ctypes.byref(_desc(N=2, C=1, H=37, W=53)), ctypes.byref(units)) == 32 and units.value == 2 * 2 * 8
    grid = lib.uz_surface_grid(ctypes.byref(_desc(N=4, C=4, H=130, W=131)), ctypes.byref(units))
    assert units.value == 2 * 16 * 67 and 0 < grid < units.value      # the walk case of tests/test_surface_metrics_gpu.py


def test_exports():
    assert unet_zoo_amd.SurfaceMetrics is SurfaceMetrics and "SurfaceMetrics" in unet_zoo_amd.__all__
    for name in ("uz_surface_workspace_bytes", "uz_surface_grid", "uz_surface_metrics"):
        assert name in _lib.EXPORTS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("uz_surface_workspace_bytes", "uz_surface_grid", "uz_surface_metrics"):
        assert getattr(raw, name)
    assert ctypes.sizeof(_lib.SurfaceDesc) == 48
