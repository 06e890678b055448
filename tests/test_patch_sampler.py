"""CPU: PatchSampler's surface and the checker of its GPU tests.

tests/patch_ref.py (numpy) is held to a brute force: the k-th foreground pixel against np.flatnonzero of the whole plane, the
cut against slicing; its draws keep their invariants over a few thousand random uniforms.  Also here: the argument checks of
PatchSampler and of GraphedStep(source=), the refusals of the five ABI entries (the library loads without a GPU), the export
and the launch plan's cap."""
import ctypes

import numpy as np
import pytest
import torch

import patch_ref as R  # tests/patch_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from unet_zoo_amd import _lib
from unet_zoo_amd.patches import PatchSampler

NAMES = ("uz_patch_index_bytes", "uz_patch_index", "uz_patch_draw", "uz_patch_cut_grid", "uz_patch_cut")


def test_export():
    assert unet_zoo_amd.PatchSampler is PatchSampler and "PatchSampler" in unet_zoo_amd.__all__
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.EXPORTS and getattr(raw, name)
    assert ctypes.sizeof(_lib.PatchDesc) == 56


# ---- the restatement against a brute force ----------------------------------------------------------------------------------------
def _pool(seed, M=3, H=37, W=41, kind="f2", density=0.2):
    g = np.random.default_rng(seed)
    if kind == "i":
        lab = g.integers(0, 4, (M, H, W)).astype(np.int32) * (g.random((M, H, W)) < density)
        lab[g.random((M, H, W)) < 0.02] = -100          # an ignore index is background
        lab[g.random((M, H, W)) < 0.02] = 7             # so is a class beyond num_classes - 1
        lab[0] = 0                                      # a picture without foreground
        lab[1][lab[1] == 3] = 0                         # class 3 is present in picture 2 only
        return lab.astype(np.int32), 4
    Cm = int(kind[1])
    mask = (g.random((M, Cm, H, W)) < density).astype(np.float32)
    mask[0] = 0.0
    mask[1, 0] = 1.0                                    # a full plane
    mask[mask == 0] = 0.5                               # 0.5 itself is background
    return mask, None


@pytest.mark.parametrize("kind", ["f1", "f3", "i"])
def test_index_is_the_running_count(kind):
    mask, nc = _pool(1, kind=kind)
    idx, fg = R.index(mask, nc), R.planes(mask, nc)
    M, P, H, W = fg.shape
    assert idx.shape == (M, P, H + 1) and idx.dtype == np.int32
    for m in range(M):
        for p in range(P):
            for y in range(H + 1):
                assert idx[m, p, y] == fg[m, p, :y].sum()
    if kind == "i":
        assert idx[0, :, H].sum() == 0 and idx[1, 2, H] == 0 and idx[2, 2, H] > 0
        assert np.array_equal(fg[2, 0], mask[2] == 1)


@pytest.mark.parametrize("kind", ["f2", "i"])
def test_kth_pixel_equals_flatnonzero(kind):
    mask, nc = _pool(2, kind=kind, H=16, W=130)
    idx, fg = R.index(mask, nc), R.planes(mask, nc)
    for m in range(fg.shape[0]):
        for p in range(fg.shape[1]):
            flat = np.flatnonzero(fg[m, p])
            for rank in list(range(0, len(flat), 7)) + ([len(flat) - 1] if len(flat) else []):
                assert R.kth_pixel(idx[m, p], fg[m, p], rank) == divmod(int(flat[rank]), fg.shape[3])


def test_pick_and_anchor():
    assert R.pick(0.0, 5) == 0 and R.pick(np.float32(1) - np.float32(2.0 ** -24), 5) == 4 and R.pick(0.5, 1) == 0
    assert [R.pick(k / 4, 4) for k in range(4)] == [0, 1, 2, 3]
    assert R.pick(np.float32(0.1), 10) == 1          # float32(0.1) lies above 0.1
    for n in (1, 7, 64, 255):
        assert R.anchor(0.123, 0.0, n) == n // 2
        assert R.anchor(0.0, 1.0, n) == 0 and R.anchor(np.float32(1) - np.float32(2.0 ** -24), 1.0, n) == n - 1
        assert R.anchor(0.0, 0.5, n) == int(np.floor(0.25 * n))


@pytest.mark.parametrize("kind,jitter", [("f2", 1.0), ("i", 0.0), ("i", 0.37)])
def test_draw_invariants(kind, jitter):
    M, H, W, h, w, pos = 3, 37, 41, 11, 16, 0.5
    mask, nc = _pool(3, kind=kind)
    idx, fg = R.index(mask, nc), R.planes(mask, nc)
    u = np.random.default_rng(4).random((3000, 8), dtype=np.float32)
    c = R.draw(u, idx, fg, M, H, W, h, w, pos, jitter)
    m, y0, x0, plane = c.T
    assert ((m >= 0) & (m < M)).all() and ((y0 >= 0) & (y0 <= H - h)).all() and ((x0 >= 0) & (x0 <= W - w)).all()
    assert ((plane >= -1) & (plane < fg.shape[1])).all()
    assert (plane[m == 0] == -1).all() and (m == 0).sum() > 500          # no foreground: random mode
    assert (plane[u[:, 1] >= np.float32(pos)] == -1).all()
    fgmode = plane >= 0
    assert np.array_equal(fgmode, (u[:, 1] < np.float32(pos)) & (m != 0))
    for b in np.flatnonzero(fgmode):
        assert idx[m[b], plane[b], H] > 0
        rank = R.pick(u[b, 3], int(idx[m[b], plane[b], H]))
        py, px = divmod(int(np.flatnonzero(fg[m[b], plane[b]])[rank]), W)        # the brute force
        assert y0[b] <= py < y0[b] + h and x0[b] <= px < x0[b] + w
        if jitter == 0.0:          # centred unless the picture's edge is in the way
            assert y0[b] == min(max(py - h // 2, 0), H - h) and x0[b] == min(max(px - w // 2, 0), W - w)
    for b in np.flatnonzero(~fgmode)[:200]:
        assert (y0[b], x0[b]) == (R.pick(u[b, 4], H - h + 1), R.pick(u[b, 5], W - w + 1))
    if kind == "i":
        assert set(plane[m == 1]) <= {-1, 0, 1} and 2 in set(plane[m == 2])      # plane 2 is empty in picture 1


def test_draw_with_indices_and_without_a_mask():
    M, H, W, h, w = 3, 37, 41, 37, 41          # the window is the picture
    mask, nc = _pool(5, kind="f1")
    idx, fg = R.index(mask, nc), R.planes(mask, nc)
    u = np.random.default_rng(6).random((6, 8), dtype=np.float32)
    c = R.draw(u, idx, fg, M, H, W, h, w, 1.0, 1.0, indices=[2, 0, -1, 3, 1, 2])
    assert c[:, 0].tolist() == [2, 0, -1, -1, 1, 2] and not c[:, 1:3].any()
    assert c[:, 3].tolist() == [0, -1, -1, -1, 0, 0]
    c = R.draw(u, None, None, M, H, W, 8, 8, 1.0, 1.0)
    assert (c[:, 3] == -1).all()


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_cut_equals_slicing(dtype):
    g = np.random.default_rng(7)
    M, C, H, W, h, w = 3, 3, 20, 23, 7, 9
    image = g.integers(0, 256, (M, C, H, W)).astype(dtype)
    lab = g.integers(0, 4, (M, H, W)).astype(np.int32)
    coords = np.array([[0, 0, 0, -1], [2, 13, 14, 1], [-1, 0, 0, -1], [1, 5, 3, 0]], dtype=np.int32)
    norm = R.norm_of((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)) if dtype == np.uint8 else None
    x, t = R.cut(image, lab, coords, h, w, norm)
    assert x.shape == (4, C, h, w) and t.shape == (4, h, w) and t.dtype == np.int32
    assert not x[2].any() and not t[2].any()
    want = image[2, :, 13:20, 14:23].astype(np.float64)
    if dtype == np.uint8:
        want = (want / 255.0 - np.array([0.485, 0.456, 0.406])[:, None, None]) / np.array([0.229, 0.224, 0.225])[:, None, None]
        assert np.abs(x[1] - want).max() <= 1e-6          # scale and shift are float32
    else:
        assert np.array_equal(x[1], want)
    assert np.array_equal(t[3], lab[1, 5:12, 3:12])


# ---- the Python side's argument errors --------------------------------------------------------------------------------------------
def test_constructor_refuses_bad_arguments_by_name():
    x, t = torch.zeros(2, 3, 16, 16), torch.zeros(2, 1, 16, 16)
    lab = torch.zeros(2, 16, 16, dtype=torch.int64)
    for args, kw, word in [
            ((torch.zeros(2, 3, 16, 16, dtype=torch.float64), t), {}, "images"), ((torch.zeros(3, 16, 16), None), {}, "images"),
            ((torch.zeros(2, 5, 16, 16), None), {}, "C = 5"), ((x, t), dict(window=(17, 8)), "window"), ((x, t), dict(window=8), "window"),
            ((x, t), dict(window=(8, 8), batch=0), "batch"), ((x, t), dict(window=(8, 8), pos=1.5), "pos"),
            ((x, t), dict(window=(8, 8), jitter=-0.1), "jitter"), ((x, t), dict(window=(8, 8), pos=float("nan")), "pos"),
            ((x, torch.zeros(2, 9, 16, 16)), dict(window=(8, 8)), "masks"), ((x, torch.zeros(2, 1, 16, 8)), dict(window=(8, 8)), "masks"),
            ((x, torch.zeros(2, 1, 16, 16, dtype=torch.float16)), dict(window=(8, 8)), "masks"),
            ((x, torch.zeros(2, 1, 16, 16, dtype=torch.int32)), dict(window=(8, 8), num_classes=3), "masks"),
            ((x, lab), dict(window=(8, 8)), "num_classes"), ((x, lab), dict(window=(8, 8), num_classes=10), "num_classes"),
            ((x, t), dict(window=(8, 8), num_classes=3), "num_classes"), ((x, None), dict(window=(8, 8), num_classes=3), "num_classes"),
            ((x.to(torch.uint8), t), dict(window=(8, 8), mean=(0.5,), std=(0.5,)), "mean / std"),
            ((x.to(torch.uint8), t), dict(window=(8, 8), std=(0.2, 0.0, 0.2)), "mean / std"),
            ((x.to(torch.uint8), t), dict(window=(8, 8), mean=None), "mean / std")]:
        with pytest.raises(ValueError, match=word):
            PatchSampler(*args, **kw)
    if not torch.cuda.is_available():                                      # good arguments without a GPU: no fallback
        with pytest.raises(_lib.HipLibraryError):
            PatchSampler(x, t, window=(8, 8), batch=2)


def test_step_refuses_a_bad_source_and_a_missing_batch():
    model = unet_zoo_amd.create_model("unet")
    with pytest.raises(TypeError, match="PatchSampler"):
        unet_zoo_amd.GraphedStep(model, source=object())
    with pytest.raises(TypeError, match="source="):
        unet_zoo_amd.GraphedStep(model)()
    with pytest.raises(TypeError, match="source="):
        unet_zoo_amd.GraphedStep(model).forward_backward(torch.zeros(1, 3, 16, 16))


# ---- the library's refusals, without a GPU ----------------------------------------------------------------------------------------
def _desc(M=2, C=3, H=16, W=16, ik=_lib.PATCH_IMAGE_F32, mk=_lib.PATCH_MASK_F32, Cm=1, P=1, B=2, h=8, w=8, ui=0, pos=0.5, jitter=1.0):
    return _lib.PatchDesc(M, C, H, W, ik, mk, Cm, P, B, h, w, ui, pos, jitter)


BAD = [(dict(C=0), b"C ="), (dict(C=5), b"C ="), (dict(Cm=9, P=9), b"Cm"), (dict(Cm=0, P=0), b"Cm"), (dict(P=2), b"P ="),
       (dict(mk=_lib.PATCH_MASK_I32, P=0), b"P ="), (dict(mk=_lib.PATCH_MASK_I32, P=9), b"P ="), (dict(mk=_lib.PATCH_MASK_NONE), b"P ="),
       (dict(mk=3), b"mask_kind"), (dict(ik=2), b"image_kind"), (dict(M=0), b"shape"), (dict(W=-1), b"shape"), (dict(B=0), b"B ="),
       (dict(h=0), b"window"), (dict(h=17), b"larger"), (dict(w=17), b"larger"),
       (dict(pos=1.5), b"pos"), (dict(pos=float("nan")), b"pos"), (dict(jitter=-0.5), b"jitter"), (dict(jitter=float("inf")), b"jitter"),
       (dict(H=1 << 15, W=1 << 15), b"H W"), (dict(M=1 << 20, H=1 << 11, W=8, Cm=8, P=8), b"M P"),
       (dict(B=2048, C=4, H=512, W=512, h=512, w=512), b"B max"), (dict(B=2048, C=1, Cm=4, P=4, H=512, W=512, h=512, w=512), b"B max")]


@pytest.mark.parametrize("kw,word", BAD)
def test_bad_descriptor_is_refused_without_a_gpu(kw, word):
    lib = _lib.load()
    d = _desc(**kw)
    p = 0x100000          # never read: the checks come before any launch
    for rc in (lib.uz_patch_index_bytes(ctypes.byref(d)), lib.uz_patch_cut_grid(ctypes.byref(d), None),
               lib.uz_patch_index(ctypes.byref(d), p, 2 * p, None), lib.uz_patch_draw(ctypes.byref(d), p, None, 2 * p, 3 * p, 4 * p, None),
               lib.uz_patch_cut(ctypes.byref(d), p, 2 * p, 3 * p, None, 4 * p, 5 * p, None)):
        assert rc == -1
        assert word in lib.uz_last_error_string()


def test_null_pointers_mismatches_and_overlaps_are_refused_without_a_gpu():
    lib = _lib.load()
    err = lib.uz_last_error_string
    assert lib.uz_patch_index_bytes(None) == -1 and b"null descriptor" in err()
    assert lib.uz_patch_cut_grid(None, None) == -1 and b"null descriptor" in err()
    assert lib.uz_patch_index(None, None, None, None) == -1 and b"null descriptor" in err()
    assert lib.uz_patch_draw(None, None, None, None, None, None, None) == -1 and b"null descriptor" in err()
    assert lib.uz_patch_cut(None, None, None, None, None, None, None, None) == -1 and b"null descriptor" in err()
    d, r = _desc(), ctypes.byref
    none = _desc(mk=_lib.PATCH_MASK_NONE, Cm=0, P=0)
    img, msk, idx, u, co, oimg, omsk, ind, nrm = (k * 0x100000 for k in range(1, 10))      # never read
    assert lib.uz_patch_index_bytes(r(d)) == 4 * 2 * 1 * 17 and lib.uz_patch_index_bytes(r(none)) == 0
    # index
    assert lib.uz_patch_index(r(d), None, idx, None) == -1 and b"null pointer" in err()
    assert lib.uz_patch_index(r(none), msk, idx, None) == -1 and b"no foreground planes" in err()
    assert lib.uz_patch_index(r(d), msk + 2, idx, None) == -1 and b"aligned" in err()
    assert lib.uz_patch_index(r(d), msk, msk + 4 * 2 * 256 - 4, None) == -1 and b"overlap" in err()
    # draw
    assert lib.uz_patch_draw(r(d), None, None, idx, msk, co, None) == -1 and b"null pointer" in err()
    assert lib.uz_patch_draw(r(d), u, ind, idx, msk, co, None) == -1 and b"use_indices" in err()
    assert lib.uz_patch_draw(r(_desc(ui=1)), u, None, idx, msk, co, None) == -1 and b"use_indices" in err()
    assert lib.uz_patch_draw(r(_desc(ui=2)), u, ind, idx, msk, co, None) == -1 and b"use_indices" in err()
    assert lib.uz_patch_draw(r(d), u, None, None, msk, co, None) == -1 and b"mask_kind" in err()
    assert lib.uz_patch_draw(r(none), u, None, idx, None, co, None) == -1 and b"mask_kind" in err()
    assert lib.uz_patch_draw(r(d), u, None, idx, msk, co + 1, None) == -1 and b"aligned" in err()
    assert lib.uz_patch_draw(r(d), u, None, idx, msk, u + 32, None) == -1 and b"overlap" in err()
    assert lib.uz_patch_draw(r(d), u, None, idx, msk, idx + 4 * 33, None) == -1 and b"overlap" in err()
    # cut
    assert lib.uz_patch_cut(r(d), img, msk, None, None, oimg, omsk, None) == -1 and b"null pointer" in err()
    assert lib.uz_patch_cut(r(d), img, None, co, None, oimg, omsk, None) == -1 and b"mask_kind" in err()
    assert lib.uz_patch_cut(r(none), img, msk, co, None, oimg, None, None) == -1 and b"mask_kind" in err()
    assert lib.uz_patch_cut(r(d), img, msk, co, nrm, oimg, omsk, None) == -1 and b"norm" in err()
    assert lib.uz_patch_cut(r(d), img + 2, msk, co, None, oimg, omsk, None) == -1 and b"aligned" in err()
    nimg = 4 * 2 * 3 * 16 * 16
    for args in ((img, msk, co, None, img + nimg - 4, omsk), (img, msk, co, None, oimg, msk), (img, msk, co, None, co, omsk),
                 (img, msk, co, None, oimg, oimg + 4)):
        assert lib.uz_patch_cut(r(d), *args, None) == -1 and b"overlap" in err()
    u8 = _desc(ik=_lib.PATCH_IMAGE_U8)
    assert lib.uz_patch_cut(r(u8), img, msk, co, nrm, nrm + 4, omsk, None) == -1 and b"overlap" in err()
    assert lib.uz_patch_cut(r(u8), img, msk, co, nrm + 2, oimg, omsk, None) == -1 and b"aligned" in err()


def test_launch_plan_caps_the_grid():
    lib = _lib.load()
    units = ctypes.c_int(0)
    assert lib.uz_patch_cut_grid(ctypes.byref(_desc(B=16, H=1024, W=1024, h=256, w=256)), ctypes.byref(units)) == 1024 and units.value == 1024
    assert lib.uz_patch_cut_grid(ctypes.byref(_desc(B=2, H=37, W=41, h=11, w=13)), ctypes.byref(units)) == 2 and units.value == 2
    # the walk case of tests/test_patch_sampler_gpu.py: 17 rows x 16 runs = 272 runs, two units per patch, the second nearly empty
    walk = _desc(M=2, C=1, B=1025, H=40, W=70, h=17, w=61, mk=_lib.PATCH_MASK_I32, Cm=0, P=3)
    grid = lib.uz_patch_cut_grid(ctypes.byref(walk), ctypes.byref(units))
    assert units.value == 2050 and grid == 2048
