"""CPU: MaskPostprocess' reference and the checker of its GPU tests.

tests/postproc_ref.py (numpy + scipy.ndimage) is pinned to answers derived by hand and to the property that the label plane
is ndimage.label of the mask.  Also here: the union-find core of the kernels as a stand-alone host program under the address
and undefined-behaviour sanitizers (tests/postproc_core_main.cpp, a child process; nothing is loaded into Python), the
refusals of the ABI entries (the library loads without a GPU) and the argument checks of MaskPostprocess and GraphedPredict."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import postproc_ref as R  # tests/postproc_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from unet_zoo_amd import _lib, ops
from unet_zoo_amd.postprocess import MaskPostprocess
from unet_zoo_amd.predict import GraphedPredict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference, by hand ----------------------------------------------------------------------------------------------------
def test_two_components_by_hand():
    p = np.zeros((5, 7), dtype=bool)
    p[0, 5:7] = True                      # area 2, root 5
    p[2:5, 0:3] = True                    # area 9, root 14, box (2, 0) - (4, 2), sum i = 27, sum j = 9
    mask, labels, st, comps = R.plane(p)
    assert st.tolist() == [2, 2, 11, 11, 0, 9, 0, 0]
    assert comps[0].tolist() == [9, 2, 0, 4, 2, 27, 9, 14] and comps[1].tolist() == [2, 0, 5, 0, 6, 0, 11, 5]
    assert not comps[2:].any()
    assert labels[0, 5] == 1 and labels[2, 0] == 2 and np.array_equal(mask, p)      # numbered in raster order, not by area
    mask, labels, st, comps = R.plane(p, keep_largest=1)
    assert st.tolist() == [2, 1, 11, 9, 0, 9, 0, 0] and labels.max() == 1 and labels[2, 0] == 1 and mask.sum() == 9
    assert not comps[1:].any()
    mask, labels, st, comps = R.plane(p, min_area=3)
    assert st[1] == 1 and st[3] == 9
    assert R.plane(p, min_area=2)[2][1] == 2                  # area == min_area stays
    assert R.plane(p, min_area=10)[2].tolist() == [2, 0, 11, 0, 0, 0, 0, 0]


def test_ties_go_to_the_smaller_root_and_connectivity_by_hand():
    p = R.squares(12, 30, [3] * 5)
    for k in (1, 2):
        mask, labels, st, comps = R.plane(p, keep_largest=k)
        assert st[0] == 5 and st[1] == k and comps[:k, 7].tolist() == [31 + 5 * r for r in range(k)]
    cb = R.adversarial()["checkerboard"]
    assert R.plane(cb, 1)[2][:2].tolist() == [33 * 70 // 2, 33 * 70 // 2] and R.plane(cb, 1)[2][5] == 1
    assert R.plane(cb, 2)[2][:2].tolist() == [1, 1]
    d = R.adversarial()["diagonal_touch"]
    assert R.plane(d, 1)[2][0] == 2 and R.plane(d, 2)[2][0] == 1
    for name in ("serpentine", "spiral", "comb_last_row", "comb_last_column", "full"):
        assert R.plane(R.adversarial()[name], 1)[2][0] == 1, name
    assert R.plane(R.adversarial()["corners"], 2)[2][0] == 4 and R.plane(R.adversarial()["empty"])[2].tolist() == [0] * 8


def test_holes_by_hand():
    h = R.holes()
    inner = (20 - 3 - 1) * (40 - 4 - 1)
    st = R.plane(h["ring"], fill_holes=True)[2]
    assert st[4] == inner and st[0] == 1 and st[2] == (18 * 37)
    assert R.plane(h["diagonal_gap"], fill_holes=True)[2][4] == inner          # the background is 4-connected: still a hole
    assert R.plane(h["diagonal_gap"], 2, fill_holes=True)[2][4] == inner       # ... whatever the connectivity
    assert R.plane(h["straight_gap"], fill_holes=True)[2][4] == 0
    assert R.plane(h["u_at_edge"], fill_holes=True)[2][4] == 0
    assert R.plane(h["ring_in_ring"], fill_holes=True)[2][:2].tolist() == [1, 1]
    assert R.plane(h["fill_joins"])[2][0] == 2 and R.plane(h["fill_joins"], fill_holes=True)[2][0] == 1


def test_class_map_by_hand():
    x = np.zeros((1, 3, 9, 9), dtype=np.float32)       # class 0 everywhere (ties to the lowest index)
    x[0, 2, 1:8, 1:8] = 1.0                             # a 7 x 7 square of class 2 ...
    x[0, 2, 3:6, 3:6] = 0.0
    x[0, 1, 3:6, 3:6] = 2.0                             # ... with a 3 x 3 core of class 1
    x[0, 1, 4, 4] = 0.0                                 # ... whose centre is class 0 again
    mask, labels, st, comps, cmap = R.classes(x, fill_holes=True)
    assert st[0, 0].tolist() == [1, 1, 9, 9, 1, 9, 0, 0] and st[0, 1].tolist() == [1, 1, 49, 49, 9, 49, 0, 0]
    assert cmap[0, 4, 4] == 1 and cmap[0, 3, 3] == 1 and cmap[0, 1, 1] == 2 and cmap[0, 0, 0] == 0
    mask, labels, st, comps, cmap = R.classes(x, fill_holes=True, min_area=10)       # class 1 dropped: its pixels are a hole of 2
    assert cmap[0, 4, 4] == 2 and cmap[0, 3, 3] == 2
    assert R.classes(x, include_background=True)[2].shape == (1, 3, 8)


@pytest.mark.parametrize("seed", range(12))
def test_labels_are_ndimage_label_of_the_mask(seed):
    from scipy import ndimage as ndi
    x = R.blobs((1, 1, 37, 150), seed, sigma=1.0 + seed % 3)
    conn = 1 + seed % 2
    mask, labels, st, comps = R.binary(x, connectivity=conn, fill_holes=seed % 3 == 0, min_area=[0, 5][seed % 2], keep_largest=[0, 1, 3][seed % 3])
    want, n = ndi.label(mask[0, 0], structure=R.SQUARE if conn == 2 else R.CROSS)
    assert np.array_equal(labels[0, 0], want) and st[0, 0, 1] == n and st[0, 0, 3] == mask.sum()
    areas = comps[0, 0, :, 0]
    assert (np.diff(areas) <= 0).all() and areas[0] == (st[0, 0, 5] if n else 0)


# ---- the union-find core under the sanitizers (a child process) ------------------------------------------------------------------
def test_union_find_core_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "postproc_core")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    os.path.join(ROOT, "tests", "postproc_core_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout and "runtime error" not in r.stderr


# ---- the ABI without a GPU ------------------------------------------------------------------------------------------------------
def _desc(mode=_lib.POST_BINARY, N=2, C=1, H=16, W=16, first=0, conn=1, fill=0, min_area=0, keep=0, thr=0.0):
    return _lib.PostprocDesc(mode, N, C, H, W, first, conn, fill, min_area, keep, thr, 0)


CLS = _lib.POST_CLASS


@pytest.mark.parametrize("kw,word", [
    (dict(mode=2), b"mode"), (dict(N=0), b"shape"), (dict(C=0), b"shape"), (dict(H=0), b"shape"), (dict(W=-3), b"shape"),
    (dict(H=4097), b"above 4096"), (dict(W=4097), b"above 4096"), (dict(mode=CLS, C=1), b"K ="), (dict(mode=CLS, C=33, first=1), b"K ="),
    (dict(mode=CLS, C=3, first=3), b"first_class"), (dict(mode=CLS, C=3, first=-1), b"first_class"), (dict(conn=0), b"connectivity"),
    (dict(conn=3), b"connectivity"), (dict(fill=2), b"fill_holes"), (dict(min_area=-1), b"min_area"), (dict(keep=-1), b"keep_largest"),
    (dict(keep=9), b"keep_largest"), (dict(thr=float("nan")), b"thr"), (dict(N=128, C=1, H=4096, W=4096), b"too large"),
    (dict(mode=CLS, N=8, C=16, first=1, H=4096, W=4096), b"too large")])
def test_bad_descriptor_is_rejected_without_a_gpu(kw, word):
    lib = _lib.load()
    d = _desc(**kw)
    assert lib.uz_postproc_workspace_bytes(ctypes.byref(d)) == -1 and word in lib.uz_last_error_string()
    assert lib.uz_postproc_grid(ctypes.byref(d), None) == -1 and word in lib.uz_last_error_string()
    assert lib.uz_postproc(ctypes.byref(d), None, None, None, None, None, None, None, None) == -1
    assert word in lib.uz_last_error_string()


def test_null_pointers_misalignment_and_overlaps_are_refused_without_a_gpu():
    lib = _lib.load()
    assert lib.uz_postproc_workspace_bytes(None) == -1 and b"null descriptor" in lib.uz_last_error_string()
    d = _desc()
    good = [0x100000, 0x200000, 0x300000, None, 0x500000, 0x600000, 0x10000000]   # x, mask, labels, class_map, stats, comps, ws
    for k in (0, 1, 4, 5, 6):
        args = list(good)
        args[k] = None
        assert lib.uz_postproc(ctypes.byref(d), *args, None) == -1 and b"null pointer" in lib.uz_last_error_string()
    args = list(good)
    args[3] = 0x700000
    assert lib.uz_postproc(ctypes.byref(d), *args, None) == -1 and b"class_map" in lib.uz_last_error_string()
    for k, off, word in ((0, 2, b"4-byte"), (2, 2, b"4-byte"), (4, 4, b"8-byte"), (5, 4, b"8-byte"), (6, 8, b"16-byte")):
        args = list(good)
        args[k] += off
        assert lib.uz_postproc(ctypes.byref(d), *args, None) == -1 and word in lib.uz_last_error_string()
    for a, b, delta in ((1, 0, 0), (2, 1, 16), (4, 2, 8), (5, 4, 0), (1, 6, 16)):
        args = list(good)
        args[a] = good[b] + delta
        assert lib.uz_postproc(ctypes.byref(d), *args, None) == -1 and b"overlap" in lib.uz_last_error_string(), (a, b)


def test_tta_entries_refuse_bad_descriptors_without_a_gpu():
    lib = _lib.load()
    for kw, word in ((dict(views=0), b"views"), (dict(views=16), b"views"), (dict(dtype=2), b"dtype"), (dict(N=0), b"shape"),
                     (dict(mode=CLS, C=1), b"K =")):
        f = dict(mode=0, N=1, C=1, H=4, W=4, views=1, dtype=0)
        f.update(kw)
        d = _lib.TtaDesc(f["mode"], f["N"], f["C"], f["H"], f["W"], f["views"], f["dtype"], 0)
        assert lib.uz_flip_views(ctypes.byref(d), None, None, None) == -1 and word in lib.uz_last_error_string()
        assert lib.uz_tta_merge(ctypes.byref(d), None, None, None) == -1 and word in lib.uz_last_error_string()
        assert lib.uz_mask_decide(ctypes.byref(d), None, 0.0, 0, None, None, None) == -1 and word in lib.uz_last_error_string()
    assert [lib.uz_tta_num_views(v) for v in (0, 1, 6, 15, 16)] == [-1, 1, 2, 4, -1]
    assert ops.tta_views(()) == 1 and ops.tta_views(("hflip", "vflip")) == 7 and ops.tta_views(("hvflip", "identity")) == 9
    with pytest.raises(ValueError, match="unknown view"):
        ops.tta_views(("rot90",))


def test_workspace_grows_and_the_launch_plan_caps_the_grid():
    lib = _lib.load()
    last = 0
    for N, C, H, W in ((1, 1, 1, 1), (1, 1, 37, 53), (2, 1, 37, 53), (2, 3, 37, 53), (2, 3, 256, 256), (16, 3, 256, 256)):
        b = lib.uz_postproc_workspace_bytes(ctypes.byref(_desc(N=N, C=C, H=H, W=W)))
        assert b > last and b % 16 == 0
        last = b
    units = ctypes.c_int(0)
    assert lib.uz_postproc_grid(ctypes.byref(_desc(N=2, C=3, H=37, W=150)), ctypes.byref(units)) == 132 and units.value == 6 * 22
    grid = lib.uz_postproc_grid(ctypes.byref(_desc(N=4, C=4, H=130, W=261)), ctypes.byref(units))
    assert units.value == 16 * 133 and 0 < grid < units.value      # the walk case of tests/test_postproc_gpu.py


# ---- the Python objects' own checks (no GPU) --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,word", [
    (dict(connectivity=0), "connectivity"), (dict(connectivity=3), "connectivity"), (dict(connectivity=1.0), "connectivity"),
    (dict(min_area=-1), "min_area"), (dict(min_area=2.5), "min_area"), (dict(keep_largest=9), "keep_largest"),
    (dict(keep_largest=-1), "keep_largest"), (dict(keep_largest=True), "keep_largest"), (dict(fill_holes=1), "fill_holes"),
    (dict(include_background="no"), "include_background"), (dict(labels=None), "labels")])
def test_postprocess_constructor_refuses_bad_arguments_by_name(kw, word):
    with pytest.raises(ValueError, match=word):
        MaskPostprocess(**kw)


def test_postprocess_call_refuses_bad_tensors_before_any_kernel():
    pp = MaskPostprocess()
    with pytest.raises(ValueError, match=r"\(N, C, H, W\)"):
        pp(torch.zeros(2, 16, 16))
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        pp(torch.zeros(2, 1, 16, 16, dtype=torch.float64))
    with pytest.raises(ValueError, match="at most 4096"):
        pp(torch.zeros(1, 1, 1, 4097))
    with pytest.raises(ValueError, match="mode must be"):
        pp(torch.zeros(1, 1, 4, 4), mode="multi")
    with pytest.raises(ValueError, match="K = 1"):
        pp(torch.zeros(1, 1, 4, 4), mode="class")
    with pytest.raises(ValueError, match="K = 40"):
        pp(torch.zeros(1, 40, 4, 4))
    with pytest.raises(RuntimeError, match="no call yet"):
        pp.check()
    with pytest.raises(_lib.HipLibraryError):                              # good arguments on the CPU: no fallback
        pp({"d0": torch.zeros(2, 3, 16, 16), "d1": torch.zeros(2, 3, 16, 16)})
    d = pp.describe(_lib.POST_CLASS, (2, 4, 8, 9))
    assert (d.first_class, d.connectivity, d.fill_holes, d.keep_largest) == (1, 1, 0, 0)
    assert MaskPostprocess(include_background=True).describe(_lib.POST_CLASS, (2, 4, 8, 9)).first_class == 0


def test_graphed_predict_constructor_checks():
    model = unet_zoo_amd.create_model("unet")
    with pytest.raises(RuntimeError, match="eval"):                       # a fresh model is in train mode
        GraphedPredict(model)
    with pytest.raises(RuntimeError, match="no CPU path"):                # in eval mode, but on the CPU
        GraphedPredict(model.eval())
    with pytest.raises(ValueError, match="unknown view"):
        GraphedPredict(model, tta=("rot90",))
    with pytest.raises(ValueError, match="sequence"):
        GraphedPredict(model, tta="hflip")
    with pytest.raises(TypeError, match="MaskPostprocess"):
        GraphedPredict(model, postprocess=object())
    with pytest.raises(ValueError, match="mode must be"):
        GraphedPredict(model, mode="multi")
    with pytest.raises(TypeError, match="HipModule"):
        GraphedPredict(torch.nn.Conv2d(1, 1, 1))


def test_exports():
    assert unet_zoo_amd.MaskPostprocess is MaskPostprocess and unet_zoo_amd.GraphedPredict is GraphedPredict
    assert "MaskPostprocess" in unet_zoo_amd.__all__ and "GraphedPredict" in unet_zoo_amd.__all__
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("uz_postproc_workspace_bytes", "uz_postproc_grid", "uz_postproc", "uz_tta_num_views", "uz_flip_views", "uz_tta_merge",
                 "uz_mask_decide"):
        assert name in _lib.EXPORTS and getattr(raw, name)
    assert ctypes.sizeof(_lib.PostprocDesc) == 48 and ctypes.sizeof(_lib.TtaDesc) == 32
