"""CPU: GpuAugment's surface and the checker of its GPU tests.

tests/augment_ref.py (float64 numpy) is pinned against torch: its picture against F.grid_sample, its displacement field against
F.interpolate, its flips and whole-pixel shifts against torch.flip and slices.  Also here: the argument checks of GpuAugment,
the refusals of the three ABI entries (the library loads without a GPU), the export, and the cap on the share of mask pixels
the GPU tests may leave out of the mask comparison."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_ref as R  # tests/augment_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from unet_zoo_amd import _lib
from unet_zoo_amd.augment import GpuAugment

SHAPES = [(37, 41), (64, 48), (200, 264)]


def _sets_params(H, W):
    return R.params_from_draws(R.draws_for_sets(H, W), H, W, **R.RANGES)


def test_export():
    assert unet_zoo_amd.GpuAugment is GpuAugment and "GpuAugment" in unet_zoo_amd.__all__
    for name in ("uz_augment_params", "uz_augment_grid", "uz_augment_apply"):
        assert name in _lib.EXPORTS


def test_draws_reproduce_the_parameter_sets():
    H, W = 37, 41
    p = _sets_params(H, W)
    for n, (theta, s, hf, vf, tx, ty) in enumerate(R.SETS):
        fx, fy = (-1.0 if hf else 1.0), (-1.0 if vf else 1.0)
        want = [np.cos(theta) * fx / s, np.sin(theta) * fy / s, W / 2 + tx - 0.5, -np.sin(theta) * fx / s, np.cos(theta) * fy / s,
                H / 2 + ty - 0.5, 1.0, 0.0]
        np.testing.assert_allclose(p[n, :8], want, rtol=0, atol=2e-6)      # the draws are float32
    assert (p[:, 8:] == 0).all()


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("fill", [0.0, 0.75])
def test_picture_equals_grid_sample(H, W, fill):
    g = torch.Generator().manual_seed(H * 1000 + W)
    img = torch.randn(4, 3, H, W, generator=g, dtype=torch.float64)
    disp = torch.randn(4, 2, 5, 5, generator=g, dtype=torch.float64) * 2.0
    p = _sets_params(H, W)
    for d in (None, disp.numpy()):
        got, _, _ = R.apply(img.numpy(), None, p, d, image_fill=fill)
        grid = []
        for n in range(4):
            sx, sy = R.source_coords(p[n], H, W, None if d is None else d[n])
            grid.append(np.stack([(2 * sx + 1) / W - 1, (2 * sy + 1) / H - 1], -1))
        grid = torch.from_numpy(np.stack(grid))
        want = F.grid_sample(img - fill, grid, mode="bilinear", padding_mode="zeros", align_corners=False) + fill
        err = (torch.from_numpy(got) - want).abs().max().item()
        assert err <= 1e-10, err


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("G", [2, 4, 16])
def test_displacement_equals_interpolate(H, W, G):
    disp = torch.randn(2, G, G, generator=torch.Generator().manual_seed(G), dtype=torch.float64) * 3.0
    want = F.interpolate(disp[None], size=(H, W), mode="bilinear", align_corners=True)[0]
    assert (torch.from_numpy(R.displacement(disp.numpy(), H, W)) - want).abs().max().item() <= 1e-10


@pytest.mark.parametrize("hflip,vflip", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("tx,ty", [(0, 0), (3, -2)])
def test_flips_and_whole_pixel_shifts_are_exact(hflip, vflip, tx, ty):
    H, W = 64, 48          # translate = 0.125: (2 * 0.75 - 1) * 0.125 * 48 = 3, (2 * 0.375 - 1) * 0.125 * 64 = -2, exactly
    g = torch.Generator().manual_seed(5)
    img = torch.randn(1, 2, H, W, generator=g, dtype=torch.float64)
    lab = torch.randint(0, 5, (1, H, W), generator=g, dtype=torch.int32)
    u = np.array([[0.25 if hflip else 0.75, 0.25 if vflip else 0.75, 0.5, 0.5, 0.75 if tx else 0.5, 0.375 if ty else 0.5, 0.5, 0.5]])
    p = R.params_from_draws(u, H, W, hflip=0.5, vflip=0.5, translate=0.125)
    got, mgot, band = R.apply(img.numpy(), lab.numpy(), p, image_fill=0.5, label_fill=-100)
    assert torch.equal(torch.from_numpy(got), R.flipped_shifted(img, hflip, vflip, tx, ty, 0.5))
    assert torch.equal(torch.from_numpy(mgot), R.flipped_shifted(lab, hflip, vflip, tx, ty, -100))
    assert not band.any()


@pytest.mark.parametrize("H,W", SHAPES + [(33, 34)])
def test_tie_band_of_the_parameter_sets_stays_under_the_cap(H, W):
    p = _sets_params(H, W)
    for n in range(4):
        share = R.tie_band(*R.source_coords(p[n], H, W)).mean()
        assert share <= R.TIE_CAP, (n, share)


@pytest.mark.parametrize("kw,word", [
    (dict(hflip=1.5), "hflip"), (dict(vflip=-0.1), "vflip"), (dict(rotate=-1.0), "rotate"), (dict(translate=-0.1), "translate"),
    (dict(brightness=-0.1), "brightness"), (dict(contrast=float("nan")), "contrast"), (dict(scale=(0.0, 1.0)), "scale"),
    (dict(scale=(1.2, 1.1)), "scale"), (dict(scale=1.0), "scale"), (dict(grid_distort=(1, 2.0)), "G"),
    (dict(grid_distort=(17, 2.0)), "G"), (dict(grid_distort=(4, -1.0)), "sigma_px"), (dict(grid_distort=4), "grid_distort"),
    (dict(label_fill=2 ** 31), "label_fill"), (dict(label_fill=1.5), "label_fill"), (dict(image_fill=float("inf")), "image_fill")])
def test_constructor_refuses_bad_arguments_by_name(kw, word):
    with pytest.raises(ValueError, match=word):
        GpuAugment(**kw)


def test_call_refuses_bad_tensors_before_any_kernel():
    aug = GpuAugment(grid_distort=(4, 2.0))
    x = torch.zeros(2, 3, 16, 16)
    with pytest.raises(ValueError, match="images"):
        aug(torch.zeros(2, 3, 16, 16, dtype=torch.float64))
    with pytest.raises(ValueError, match="images"):
        aug(torch.zeros(3, 16, 16))
    with pytest.raises(ValueError, match="C = 5"):
        aug.bind(torch.zeros(2, 5, 16, 16))
    with pytest.raises(ValueError, match="masks"):
        aug.bind(x, torch.zeros(2, 1, 16, 16, dtype=torch.float16))
    with pytest.raises(ValueError, match="masks"):
        aug.bind(x, torch.zeros(2, 1, 16, 16, dtype=torch.bool))
    with pytest.raises(ValueError, match="masks"):
        aug.bind(x, torch.zeros(2, 1, 16, 8))
    with pytest.raises(ValueError, match="masks"):
        aug.bind(x, torch.zeros(2, 9, 16, 16))
    with pytest.raises(ValueError, match="masks"):
        aug.bind(x, torch.zeros(2, 1, 16, 16, dtype=torch.int32))         # class indices are (N, H, W)
    with pytest.raises(ValueError, match="masks"):
        aug(x, torch.zeros(3, 16, 16, dtype=torch.int64))
    with pytest.raises(ValueError, match="u takes"):
        aug.force_draws(u=torch.zeros(2, 7))
    with pytest.raises(ValueError, match="disp takes"):
        aug.force_draws(disp=torch.zeros(2, 2, 5, 5))
    with pytest.raises(ValueError, match="disp takes"):
        GpuAugment().force_draws(disp=torch.zeros(2, 2, 4, 4))
    with pytest.raises(_lib.HipLibraryError):                              # good arguments on the CPU: no fallback
        aug(x, torch.zeros(2, 1, 16, 16))
    with pytest.raises(TypeError, match="GpuAugment"):
        unet_zoo_amd.GraphedStep(unet_zoo_amd.create_model("unet"), augment=object())


def _desc(N=2, C=3, H=16, W=16, kind=_lib.AUGMENT_MASK_F32, Cm=1, G=0, ph=0.5, pv=0.0, rot=15.0, smin=0.9, smax=1.1, tr=0.05,
          br=0.1, co=0.1, ifill=0.0, mfill=0.0, lfill=-100):
    return _lib.AugmentDesc(N, C, H, W, kind, Cm, G, ph, pv, rot, smin, smax, tr, br, co, ifill, mfill, lfill)


@pytest.mark.parametrize("kw,word", [(dict(C=0), b"C ="), (dict(C=5), b"C ="), (dict(Cm=9), b"Cm"), (dict(Cm=0), b"Cm"),
                                     (dict(kind=3), b"mask_kind"), (dict(G=1), b"G ="), (dict(G=17), b"G ="),
                                     (dict(G=4, H=1), b"H, W >= 2"), (dict(N=0), b"shape"), (dict(W=-1), b"shape"),
                                     (dict(N=2048, C=4, H=512, W=512), b"too large"),
                                     (dict(N=2048, C=1, Cm=4, H=512, W=512), b"too large"),
                                     (dict(ifill=float("nan")), b"fill")])
def test_apply_descriptor_check_refuses_without_a_gpu(kw, word):
    lib = _lib.load()
    assert lib.uz_augment_grid(ctypes.byref(_desc(**kw)), None) == -1
    assert word in lib.uz_last_error_string()
    # the launch entry point makes the same check before it touches a pointer
    assert lib.uz_augment_apply(ctypes.byref(_desc(**kw)), None, None, None, None, None, None, None) == -1
    assert word in lib.uz_last_error_string()


@pytest.mark.parametrize("kw,word", [(dict(ph=1.5), b"probability"), (dict(pv=-0.5), b"probability"), (dict(smin=0.0), b"scale"),
                                     (dict(smin=1.2), b"scale"), (dict(rot=-1.0), b"range"), (dict(tr=-0.1), b"range"),
                                     (dict(br=-0.1), b"range"), (dict(co=float("inf")), b"range"), (dict(N=0), b"shape")])
def test_params_descriptor_check_refuses_without_a_gpu(kw, word):
    lib = _lib.load()
    p = 0x1000          # never read: the checks come before any launch
    assert lib.uz_augment_params(ctypes.byref(_desc(**kw)), p, p + 0x1000, None) == -1
    assert word in lib.uz_last_error_string()


def test_null_pointers_mismatches_and_overlaps_are_refused_without_a_gpu():
    lib = _lib.load()
    assert lib.uz_augment_params(None, None, None, None) == -1 and b"null descriptor" in lib.uz_last_error_string()
    assert lib.uz_augment_apply(None, None, None, None, None, None, None, None) == -1 and b"null descriptor" in lib.uz_last_error_string()
    assert lib.uz_augment_grid(None, None) == -1 and b"null descriptor" in lib.uz_last_error_string()
    d = _desc()
    img, msk, par, oimg, omsk = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000      # never read
    assert lib.uz_augment_params(ctypes.byref(d), None, par, None) == -1 and b"null pointer" in lib.uz_last_error_string()
    assert lib.uz_augment_params(ctypes.byref(d), par, par + 32, None) == -1 and b"overlap" in lib.uz_last_error_string()
    assert lib.uz_augment_apply(ctypes.byref(d), img, msk, None, None, oimg, omsk, None) == -1
    assert b"null pointer" in lib.uz_last_error_string()
    assert lib.uz_augment_apply(ctypes.byref(d), img, None, par, None, oimg, omsk, None) == -1
    assert b"mask_kind" in lib.uz_last_error_string()
    assert lib.uz_augment_apply(ctypes.byref(_desc(kind=0)), img, msk, par, None, oimg, None, None) == -1
    assert b"mask_kind" in lib.uz_last_error_string()
    assert lib.uz_augment_apply(ctypes.byref(_desc(G=4)), img, msk, par, None, oimg, omsk, None) == -1
    assert b"displacement" in lib.uz_last_error_string()
    assert lib.uz_augment_apply(ctypes.byref(d), img, msk, par, 0x600000, oimg, omsk, None) == -1
    assert b"displacement" in lib.uz_last_error_string()
    nimg = 4 * 2 * 3 * 16 * 16
    for args in ((img, msk, par, None, img, omsk), (img, msk, par, None, img + nimg - 4, omsk), (img, msk, par, None, oimg, msk),
                 (img, msk, par, None, oimg, img), (img, msk, par, None, par, omsk), (img, msk, par, None, oimg, oimg + 4)):
        assert lib.uz_augment_apply(ctypes.byref(d), *args, None) == -1
        assert b"overlap" in lib.uz_last_error_string()
    assert lib.uz_augment_apply(ctypes.byref(d), img + 2, msk, par, None, oimg, omsk, None) == -1
    assert b"aligned" in lib.uz_last_error_string()


def test_launch_plan_caps_the_grid():
    lib = _lib.load()
    units = ctypes.c_int(0)
    assert lib.uz_augment_grid(ctypes.byref(_desc(N=16, H=256, W=256)), ctypes.byref(units)) == 1024 and units.value == 1024
    assert lib.uz_augment_grid(ctypes.byref(_desc(N=2, H=37, W=41)), ctypes.byref(units)) == 4 and units.value == 4
    grid = lib.uz_augment_grid(ctypes.byref(_desc(N=3, C=1, H=768, W=1024, kind=_lib.AUGMENT_MASK_I32)), ctypes.byref(units))
    assert units.value == 3 * 768 and 0 < grid < units.value       # the walk case of tests/test_augment_gpu.py
