"""GPU: GpuAugment (uz_augment.hip) against the float64 restatement tests/augment_ref.py (pinned to torch by
tests/test_augment.py), eagerly and inside GraphedStep's graphs.

Bounds.  Picture: 2 D eps + 8 * 2^-23 max|picture| (augment_ref.image_bound) -- D the input's largest neighbouring-pixel
difference, eps = 4 ulp of 2 max(H, W) the float32 error of a source coordinate (plus 4 ulp of the largest displacement with a
grid): a bilinear surface's Lipschitz bound times the coordinate error, plus the rounding of the interpolation.  With a jitter
the same bound holds for the jittered picture (D scales by the contrast).  Mask: exact, except where sx + 0.5 or sy + 0.5 lies
within 1e-3 of an integer (float64); that band may hold at most 1 % of a case's pixels (asserted here and in test_augment.py).
The oracle takes the (N, 16) parameters the GPU formed; uz_augment_params itself is held to the restatement separately."""
import numpy as np
import pytest
import torch

import augment_ref as R  # tests/augment_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from unet_zoo_amd import _lib, ops
from unet_zoo_amd.augment import GpuAugment
from unet_zoo_amd.loss import MulticlassLoss

pytestmark = pytest.mark.gpu
DEV = "cuda"
ZERO = dict(hflip=0.0, vflip=0.0, rotate=0.0, scale=(1.0, 1.0), translate=0.0, brightness=0.0, contrast=0.0)


def _batch(shape, mask, seed=0):
    """pictures (N, C, H, W) fp32 and a mask: "f1" / "f2" / "f3" fp32 0/1 maps with that many channels, "i" int32 labels"""
    N, _, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    if mask == "i":
        t = torch.randint(0, 5, (N, H, W), generator=g, dtype=torch.int32)
    elif mask is None:
        t = None
    else:
        t = (torch.rand((N, int(mask[1]), H, W), generator=g) > 0.5).float()
    return x, t


def _run(aug, x, t):
    xa, ta = aug(x.to(DEV), None if t is None else t.to(DEV))
    torch.cuda.synchronize()
    return xa.cpu(), None if ta is None else ta.cpu(), aug.last_params.double().cpu().numpy()


def _check(aug, x, t, got_x, got_t, params, disp=None, extra_eps=0.0):
    """picture within the bound, mask exact outside the tie band, the band under its cap; returns (error, bound)"""
    H, W = x.shape[-2:]
    want_x, want_t, band = R.apply(x.numpy(), None if t is None else t.numpy(), params, disp, aug.image_fill, aug.mask_fill, aug.label_fill)
    gain = float(np.abs(params[:, 6]).max())
    bound = R.image_bound(x.numpy(), H, W, extra_eps, gain=gain, top=float(np.abs(want_x).max()))
    err = float(np.abs(got_x.double().numpy() - want_x).max())
    print(f"{tuple(x.shape)}: picture error {err:.3e}, bound {bound:.3e}; tie band {band.mean():.4%}")
    assert err <= bound, (err, bound)
    if t is not None:
        assert band.mean() <= R.TIE_CAP, band.mean()
        keep = ~band if got_t.dim() == 3 else ~band[:, None].repeat(got_t.shape[1], 1)
        assert np.array_equal(got_t.numpy()[keep], want_t[keep])
    return err, bound


# ---- 1. identity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 37, 41), (2, 4, 16, 32)])
@pytest.mark.parametrize("mask", ["f1", "f3", "i"])
def test_identity_is_bit_exact(shape, mask):
    x, t = _batch(shape, mask)
    got_x, got_t, p = _run(GpuAugment(**ZERO), x, t)
    assert torch.equal(got_x, x) and torch.equal(got_t, t) and got_t.dtype == t.dtype
    H, W = shape[-2:]
    assert np.array_equal(p[:, :8], np.tile([1, 0, W / 2 - 0.5, 0, 1, H / 2 - 0.5, 1, 0], (shape[0], 1))) and not p[:, 8:].any()


# ---- 2. flips and a whole-pixel translation ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["f2", "i"])
def test_flips_and_integer_translation_are_bit_exact(mask):
    shape = (4, 3, 64, 48)          # translate = 0.125: (2 * 0.75 - 1) * 0.125 * 48 = 3, (2 * 0.375 - 1) * 0.125 * 64 = -2, exactly
    x, t = _batch(shape, mask)
    flips = [(False, False), (True, False), (False, True), (True, True)]
    u = torch.tensor([[0.25 if h else 0.75, 0.25 if v else 0.75, 0.5, 0.5, 0.75, 0.375, 0.5, 0.5] for h, v in flips])
    aug = GpuAugment(**{**ZERO, "hflip": 0.5, "vflip": 0.5, "translate": 0.125}, image_fill=0.5, mask_fill=0.25, label_fill=-100)
    aug.force_draws(u=u)
    got_x, got_t, _ = _run(aug, x, t)
    for n, (h, v) in enumerate(flips):
        assert torch.equal(got_x[n], R.flipped_shifted(x[n], h, v, 3, -2, 0.5)), n
        assert torch.equal(got_t[n], R.flipped_shifted(t[n], h, v, 3, -2, -100 if mask == "i" else 0.25)), n
    if mask == "i":
        assert (got_t == -100).any()


# ---- 3. general warp -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,mask", [((4, 3, 37, 41), "f2"), ((4, 1, 64, 48), "i"), ((4, 4, 33, 34), "f1")])
def test_general_warp(shape, mask):
    H, W = shape[-2:]
    x, t = _batch(shape, mask, seed=3)
    aug = GpuAugment(**{**ZERO, **R.RANGES}, image_fill=0.25, mask_fill=0.5, label_fill=-100)
    u = R.draws_for_sets(H, W)
    aug.force_draws(u=torch.from_numpy(u))
    got_x, got_t, p = _run(aug, x, t)
    # uz_augment_params: flips and signs exact, the six map entries within 1e-6 relative of the restatement
    want = R.params_from_draws(u, H, W, **R.RANGES)
    assert np.array_equal(np.sign(p[:, :6]), np.sign(want[:, :6]))
    for n, (_, _, hf, vf, _, _) in enumerate(R.SETS):
        assert (p[n, 0] * p[n, 4] - p[n, 1] * p[n, 3] < 0) == (hf != vf)
    rel = np.abs(p[:, :6] - want[:, :6]) / np.abs(want[:, :6])
    print("uz_augment_params: largest relative error of a map entry", rel.max())
    assert rel.max() <= 1e-6 and np.array_equal(p[:, 6:], want[:, 6:])
    _check(aug, x, t, got_x, got_t, p)


# ---- 4. displacement grid --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,sigma", [(4, 3.0), (16, 1.0)])
def test_displacement_grid(G, sigma):
    shape = (2, 3, 37, 41)
    x, t = _batch(shape, "i", seed=4)
    disp = torch.randn((2, 2, G, G), generator=torch.Generator().manual_seed(G)) * sigma
    aug = GpuAugment(**{**ZERO, **R.RANGES}, grid_distort=(G, sigma), label_fill=-1)
    aug.force_draws(u=torch.from_numpy(R.draws_for_sets(37, 41)[1:3]), disp=disp)
    got_x, got_t, p = _run(aug, x, t)
    _check(aug, x, t, got_x, got_t, p, disp.double().numpy(), extra_eps=4.0 * R.ulp32(float(disp.abs().max())))


# ---- 5. jitter ---------------------------------------------------------------------------------------------------------------------
def test_jitter_on_a_warp_and_alone():
    shape = (4, 3, 37, 41)
    x, t = _batch(shape, "f1", seed=5)
    # brightness = (2 * 0.25 - 1) * 0.4 = -0.2, contrast = 1 + (2 * 0.75 - 1) * 0.6 = 1.3
    aug = GpuAugment(**{**ZERO, **R.RANGES, "brightness": 0.4, "contrast": 0.6}, image_fill=0.25)
    aug.force_draws(u=torch.from_numpy(R.draws_for_sets(37, 41, u_brightness=0.25, u_contrast=0.75)))
    got_x, got_t, p = _run(aug, x, t)
    assert np.allclose(p[:, 6], 1.3, rtol=1e-6, atol=0) and np.allclose(p[:, 7], -0.2, rtol=1e-6, atol=0)
    _check(aug, x, t, got_x, got_t, p)
    alone = GpuAugment(**{**ZERO, "brightness": 0.4, "contrast": 0.6})
    u = torch.full((4, 8), 0.5)
    u[:, 6], u[:, 7] = 0.25, 0.75
    alone.force_draws(u=u)
    got_x, got_t, p = _run(alone, x, t)
    assert torch.equal(got_t, t)
    c, b = p[0, 6], p[0, 7]
    # c * x + b to 1 ulp -- of the larger of the product and the offset: the multiply-add may be fused or not, and the two
    # forms differ by a rounding of c * x, which a cancelling sum does not shrink
    tol = np.spacing((np.abs(c * x.double().numpy()) + abs(b)).astype(np.float32)).astype(np.float64)
    assert (np.abs(got_x.double().numpy() - (c * x.double().numpy() + b)) <= tol).all()


# ---- 6. walk -----------------------------------------------------------------------------------------------------------------------
def test_workgroups_walk_several_units():
    shape = (3, 1, 768, 1024)
    H, W = shape[-2:]
    desc = _lib.AugmentDesc(3, 1, H, W, _lib.AUGMENT_MASK_I32, 0, 0, 0.5, 0.5, 45.0, 0.75, 1.3, 0.25, 0.0, 0.0, 0.0, 0.0, -100)
    grid, units = ops.augment_grid(desc)
    if units <= grid:
        pytest.skip(f"the launch plan does not cap the grid at this shape ({grid} workgroups for {units} units)")
    assert units == 3 * 768 and units > grid          # some workgroups take two units, the rest one
    x, t = _batch(shape, "i", seed=6)
    aug = GpuAugment(**{**ZERO, **R.RANGES})
    aug.force_draws(u=torch.from_numpy(R.draws_for_sets(H, W)[:3]))
    got_x, got_t, p = _run(aug, x, t)
    _check(aug, x, t, got_x, got_t, p)


# ---- 7. own draws ------------------------------------------------------------------------------------------------------------------
def test_own_draws_follow_the_seed_and_stay_in_range():
    shape = (8, 3, 40, 56)
    H, W = shape[-2:]
    x, t = _batch(shape, "f1", seed=7)
    kw = dict(hflip=0.5, vflip=0.5, rotate=20.0, scale=(0.8, 1.2), translate=0.1, brightness=0.2, contrast=0.3, grid_distort=(4, 2.0))
    aug = GpuAugment(**kw)
    torch.manual_seed(11)
    a_x, a_t, a_p = _run(aug, x, t)
    b_x, b_t, b_p = _run(aug, x, t)                  # the next draws
    torch.manual_seed(11)
    c_x, c_t, c_p = _run(GpuAugment(**kw), x, t)
    assert torch.equal(a_x, c_x) and torch.equal(a_t, c_t) and np.array_equal(a_p, c_p)
    assert not torch.equal(a_x, b_x) and not np.array_equal(a_p, b_p)
    tol = 1e-5
    for p in (a_p, b_p):
        a, b, ox, c, d, oy, con, bri = (p[:, k] for k in range(8))
        assert (np.abs(ox - (W / 2 - 0.5)) <= 0.1 * W + tol).all() and (np.abs(oy - (H / 2 - 0.5)) <= 0.1 * H + tol).all()
        assert (np.abs(con - 1.0) <= 0.3 + tol).all() and (np.abs(bri) <= 0.2 + tol).all()
        s = 1.0 / np.sqrt(np.abs(a * d - b * c))
        assert ((s >= 0.8 - tol) & (s <= 1.2 + tol)).all()
        fx = np.sign(a)                             # |theta| <= 20 degrees: the cosine keeps the flip's sign
        theta = np.degrees(np.arctan2(-c * fx, a * fx))
        assert (np.abs(theta) <= 20.0 + 1e-3).all()
        assert np.allclose(np.abs(a), np.abs(d), rtol=1e-6) and np.allclose(np.abs(b), np.abs(c), rtol=1e-6, atol=1e-9)
        assert not p[:, 8:].any()
    assert len({float(v) for v in np.sign(a_p[:, 0])} | {float(v) for v in np.sign(b_p[:, 0])}) == 2      # 16 draws at p = 0.5


# ---- 8. in the step ----------------------------------------------------------------------------------------------------------------
def _model(classes):
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=classes)
    m.run_dtype = torch.float32
    return m.cuda().train()


def _step_case(multiclass):
    g = torch.Generator().manual_seed(8)
    x = torch.randn((2, 3, 64, 64), generator=g)
    if multiclass:
        return x, torch.randint(0, 3, (2, 64, 64), generator=g), 3, (lambda: MulticlassLoss.ce_dice(ignore_index=-100))
    return x, (torch.rand((2, 1, 64, 64), generator=g) > 0.5).float(), 1, (lambda: "bce_dice")


@pytest.mark.parametrize("multiclass", [False, True])
def test_step_with_augment_equals_step_fed_with_augmented_batches(multiclass):
    x, t, classes, crit = _step_case(multiclass)
    kw = dict(hflip=0.5, vflip=0.5, rotate=25.0, scale=(0.8, 1.2), translate=0.1, brightness=0.2, contrast=0.2, grid_distort=(4, 2.0),
              label_fill=-100)
    gd = torch.Generator().manual_seed(9)
    u, disp = torch.rand((2, 8), generator=gd), torch.randn((2, 2, 4, 4), generator=gd) * 2.0
    aug = GpuAugment(**kw)
    aug.force_draws(u=u.to(DEV), disp=disp.to(DEV), sticky=True)
    xa, ta = (v.clone() for v in aug(x.to(DEV), t.to(DEV)))
    assert ta.dtype == (torch.int32 if multiclass else torch.float32)
    if multiclass:
        assert (ta == -100).any()                    # the rotation brings the outside in: those pixels are ignored
    plain = unet_zoo_amd.GraphedStep(_model(classes), crit(), lr=1e-3)
    fused = unet_zoo_amd.GraphedStep(_model(classes), crit(), lr=1e-3, augment=aug)
    assert plain.augmented is None
    for k in range(3):
        l0 = plain(xa, ta).clone()
        g0 = plain.flat_grad.clone()
        l1 = fused(x, t).clone()
        g1 = fused.flat_grad.clone()
        assert torch.equal(l0, l1) and torch.equal(g0, g1), k
        assert torch.equal(fused.augmented[0], xa) and torch.equal(fused.augmented[1], ta)
    assert torch.equal(plain.dice, fused.dice)


def test_step_draws_afresh_in_every_replay_and_follows_the_seed():
    x, t, classes, crit = _step_case(False)
    kw = dict(hflip=0.5, vflip=0.5, rotate=25.0, scale=(0.8, 1.2), translate=0.1, brightness=0.2, contrast=0.2, grid_distort=(4, 2.0))
    runs = []
    for _ in range(2):
        torch.manual_seed(21)
        step = unet_zoo_amd.GraphedStep(_model(classes), crit(), lr=1e-3, augment=GpuAugment(**kw))
        torch.manual_seed(22)
        losses, seen = [], []
        for _ in range(3):
            losses.append(step(x, t).clone())
            seen.append(step.augmented[0].clone())
        assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
        runs.append(torch.stack(losses))
    assert torch.equal(runs[0], runs[1])


def test_step_with_an_eager_criterion_augments_in_the_forward_graph():
    x, t, classes, _ = _step_case(False)
    aug = GpuAugment(hflip=0.5, rotate=25.0)
    u = torch.rand((2, 8), generator=torch.Generator().manual_seed(10))
    aug.force_draws(u=u.to(DEV), sticky=True)
    xa, ta = (v.clone() for v in aug(x.to(DEV), t.to(DEV)))

    def bce(out, tt):
        return torch.nn.functional.binary_cross_entropy_with_logits(out, tt)
    plain = unet_zoo_amd.GraphedStep(_model(classes), bce, lr=1e-3)
    fused = unet_zoo_amd.GraphedStep(_model(classes), bce, lr=1e-3, augment=aug)
    for k in range(2):
        l0, l1 = plain(xa, ta).clone(), fused(x, t).clone()
        assert torch.equal(l0, l1) and torch.equal(plain.flat_grad, fused.flat_grad), k
