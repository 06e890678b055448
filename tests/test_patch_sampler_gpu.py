"""GPU: PatchSampler (uz_patch.hip) against the numpy restatement tests/patch_ref.py (held to a brute force by
tests/test_patch_sampler.py), eagerly and inside GraphedStep's graphs.

Index, coordinates, fp32 pictures and both mask kinds are compared for EQUALITY: the integer picks are one float64 product on
both sides and the cut is a copy.  uint8 pictures are held to 1 ulp (float32) of the restatement's float64 v * scale + shift:
the kernel's fused multiply-add rounds that value once."""
import numpy as np
import pytest
import torch

import patch_ref as R  # tests/patch_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from unet_zoo_amd import _lib, ops
from unet_zoo_amd.augment import GpuAugment
from unet_zoo_amd.loss import MulticlassLoss
from unet_zoo_amd.patches import PatchSampler

pytestmark = pytest.mark.gpu
DEV = "cuda"
BELOW_HALF = float(np.nextafter(np.float32(0.5), np.float32(0)))


def _mask(kind, M, H, W, seed=0):
    """"f1" / "f3": fp32 masks with that many channels; "i": labels for num_classes = 4.  Picture 0 is empty; with M = 3 picture 1
    holds a full plane and the last plane / class is present in the last picture only."""
    g = np.random.default_rng(seed)
    if kind == "i":
        lab = (g.integers(1, 4, (M, H, W)) * (g.random((M, H, W)) < 0.3)).astype(np.int32)
        lab[g.random((M, H, W)) < 0.03] = -100
        lab[g.random((M, H, W)) < 0.03] = 7
        lab[0][lab[0] > 0] = 0
        if M == 3:
            lab[1] = 1
        lab[:-1][lab[:-1] == 3] = 0
        return lab, 4
    Cm = int(kind[1])
    mask = (g.random((M, Cm, H, W)) < 0.3).astype(np.float32)
    mask[0] = 0.0
    if M == 3:
        mask[1, 0] = 1.0
    if Cm > 1:
        mask[:-1, -1] = 0.0
    mask[mask == 0] = np.where(g.random(mask.shape) < 0.5, 0.5, 0.0)[mask == 0]      # 0.5 itself is background
    return mask, None


def _sampler(mask, nc, window, batch, C=1, images=None, **kw):
    M, H, W = mask.shape[0], mask.shape[-2], mask.shape[-1]
    if images is None:
        images = torch.zeros((M, C, H, W))
    return PatchSampler(images, torch.from_numpy(mask), window=window, batch=batch, num_classes=nc, **kw)


# ---- 1. index ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,H,W", [(3, 37, 41), (2, 16, 130)])
@pytest.mark.parametrize("kind", ["f1", "f3", "i"])
def test_index_equals_the_restatement(kind, M, H, W):
    mask, nc = _mask(kind, M, H, W)
    pool = _sampler(mask, nc, (8, 8), 2)
    torch.cuda.synchronize()
    want = R.index(mask, nc)
    assert want[0, :, H].sum() == 0 and (want[-1, -1, H] > 0 or kind == "f1")
    if M == 3:
        assert want[1, 0, H] == H * W
        assert kind == "f1" or (want[:-1, -1, H] == 0).all()
    got = pool.index.cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want)


# ---- 2. draw ----------------------------------------------------------------------------------------------------------------------
PIXELS = [(0, 0), (5, 63), (5, 64), (5, 65), (5, 129), (15, 129)]      # row-major order; 130 columns: chunk edges and the tail chunk


def _edge_pool():
    mask = np.zeros((2, 1, 16, 130), dtype=np.float32)
    for y, x in PIXELS:
        mask[0, 0, y, x] = 1.0
    mask[1, 0] = (np.random.default_rng(1).random((16, 130)) < 0.2).astype(np.float32)
    return mask


def _edge_draws():
    g = np.random.default_rng(2)
    rows = []
    for k in range(len(PIXELS)):          # rank 0 .. count - 1 of picture 0, each at two places of the window
        for u4, u5 in ((0.0, 0.999), (float(g.random()), float(g.random()))):
            rows.append([0.0, 0.1, 0.3, (k + 0.5) / len(PIXELS), u4, u5, 0.0, 0.0])
    rows.append([0.0, BELOW_HALF, 0.3, 0.0, 0.7, 0.2, 0.0, 0.0])          # u1 just below pos: foreground mode
    rows.append([0.0, 0.5, 0.3, 0.0, 0.7, 0.2, 0.0, 0.0])                 # u1 at pos: random mode
    for _ in range(6):                                                    # picture 1, either mode
        rows.append([0.75] + [float(v) for v in g.random(7)])
    return np.array(rows, dtype=np.float32)


@pytest.mark.parametrize("window", [(7, 12), (16, 130), (5, 65)])      # h odd; the picture itself; one chunk and a pixel wide
@pytest.mark.parametrize("jitter", [0.0, 1.0])
def test_draw_equals_the_restatement_at_the_edges(window, jitter):
    mask, u = _edge_pool(), _edge_draws()
    h, w = window
    pool = _sampler(mask, None, window, len(u), pos=0.5, jitter=jitter)
    pool.force_draws(torch.from_numpy(u))
    pool()
    torch.cuda.synchronize()
    got = pool.last_coords.cpu().numpy()
    want = R.draw(u, R.index(mask), R.planes(mask), 2, 16, 130, h, w, 0.5, jitter)
    assert np.array_equal(got, want), (got, want)
    n = 2 * len(PIXELS)
    assert (want[:n, 0] == 0).all() and (want[:n, 3] == 0).all() and want[n, 3] == 0 and want[n + 1, 3] == -1
    for r in range(n):          # the restatement is right about these: the pixel of that rank lies in the window
        py, px = PIXELS[r // 2]
        assert want[r, 1] <= py < want[r, 1] + h and want[r, 2] <= px < want[r, 2] + w
        if jitter == 0.0:
            assert want[r, 1] == min(max(py - h // 2, 0), 16 - h) and want[r, 2] == min(max(px - w // 2, 0), 130 - w)


@pytest.mark.parametrize("kind,M,H,W", [("i", 3, 37, 41), ("f3", 3, 37, 41), ("i", 2, 16, 130)])
def test_draw_equals_the_restatement_on_random_draws(kind, M, H, W):
    mask, nc = _mask(kind, M, H, W, seed=3)
    u = np.random.default_rng(4).random((96, 8), dtype=np.float32)
    pool = _sampler(mask, nc, (11, 13), 96, pos=0.7, jitter=0.37)
    pool.force_draws(torch.from_numpy(u))
    pool()
    torch.cuda.synchronize()
    want = R.draw(u, R.index(mask, nc), R.planes(mask, nc), M, H, W, 11, 13, 0.7, 0.37)
    assert np.array_equal(pool.last_coords.cpu().numpy(), want)
    assert (want[:, 3] >= 0).sum() > 10 and (want[:, 3] == -1).sum() > 10 and len(set(want[:, 3])) >= 3      # both modes, several planes


# ---- 3. cut -----------------------------------------------------------------------------------------------------------------------
def _coords(M, H, W, h, w):
    return np.array([[0, 0, 0, -1], [M - 1, H - h, W - w, 0], [-1, 0, 0, -1], [1, 5, 3, 0], [1, 7, 9, -1], [0, H - h, 1, -1],
                     [M - 1, 2, W - w, -1]], dtype=np.int32)


@pytest.mark.parametrize("C,dtype,kind,window", [(1, "f", "f3", (11, 13)), (4, "f", "i", (12, 16)), (3, "u", "f1", (11, 13)),
                                                 (4, "u", "i", (12, 16)), (1, "u", None, (9, 18)), (2, "f", None, (12, 16))])
def test_cut_equals_slicing(C, dtype, kind, window):
    M, H, W = 3, 37, 41
    h, w = window
    g = np.random.default_rng(C)
    image = g.integers(0, 256, (M, C, H, W)).astype(np.uint8) if dtype == "u" else g.standard_normal((M, C, H, W)).astype(np.float32)
    mask, nc = _mask(kind, M, H, W, seed=5) if kind else (None, None)
    norm = R.norm_of([0.485, 0.456, 0.406, 0.5][:C], [0.229, 0.224, 0.225, 0.25][:C]) if dtype == "u" and C > 1 else None
    coords = _coords(M, H, W, h, w)
    B = len(coords)
    mk = _lib.PATCH_MASK_NONE if kind is None else _lib.PATCH_MASK_I32 if kind == "i" else _lib.PATCH_MASK_F32
    Cm = mask.shape[1] if mk == _lib.PATCH_MASK_F32 else 0
    desc = _lib.PatchDesc(M, C, H, W, _lib.PATCH_IMAGE_U8 if dtype == "u" else _lib.PATCH_IMAGE_F32, mk, Cm,
                          0 if kind is None else 3 if kind == "i" else Cm, B, h, w, 0, 0.5, 1.0)
    d_mask = None if mask is None else torch.from_numpy(mask).to(DEV)
    out = torch.full((B, C, h, w), float("nan"), device=DEV)
    mout = None if mask is None else torch.full((B,) + mask.shape[1:-2] + (h, w), -7, dtype=d_mask.dtype, device=DEV)
    ops.patch_cut(desc, torch.from_numpy(image).to(DEV), d_mask, torch.from_numpy(coords).to(DEV),
                  None if norm is None else torch.from_numpy(norm).to(DEV), out, mout)
    torch.cuda.synchronize()
    want, mwant = R.cut(image, mask, coords, h, w, norm)
    got = out.cpu().numpy()
    assert not got[2].any()                                               # m = -1: zeros
    if dtype == "u" and norm is not None:
        err = np.abs(got.astype(np.float64) - want)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        print(f"uint8 C = {C}: largest error {float((err / ulp).max()):.3f} ulp")
        assert (err <= ulp).all()
    else:
        assert np.array_equal(got.astype(np.float64), want)               # fp32 copies; uint8 without norm: the integers
    if mask is not None:
        assert mout.cpu().numpy().dtype == mask.dtype and np.array_equal(mout.cpu().numpy(), mwant)


# ---- 4. walk ----------------------------------------------------------------------------------------------------------------------
def test_workgroups_walk_several_units():
    M, H, W, h, w, B = 2, 40, 70, 17, 61, 1025
    lab, nc = _mask("i", M, H, W, seed=6)
    lab[0] = lab[1][::-1]                                                # both pictures hold foreground
    image = torch.randn((M, 1, H, W), generator=torch.Generator().manual_seed(6))
    pool = _sampler(lab, nc, (h, w), B, images=image, pos=0.5)
    grid, units = ops.patch_cut_grid(pool.desc)
    if units <= grid:
        pytest.skip(f"the launch plan does not cap the grid at this shape ({grid} workgroups for {units} units)")
    assert units == 2 * B                                                # some workgroups take two units, the rest one
    torch.manual_seed(6)
    x, t = pool()
    torch.cuda.synchronize()
    coords = pool.last_coords.cpu().numpy()
    assert np.array_equal(coords, R.draw(pool.u.cpu().numpy(), R.index(lab, nc), R.planes(lab, nc), M, H, W, h, w, 0.5, 1.0))
    want, mwant = R.cut(image.numpy(), lab, coords, h, w)
    assert np.array_equal(x.cpu().numpy().astype(np.float64), want) and np.array_equal(t.cpu().numpy(), mwant)


# ---- 5. own draws -----------------------------------------------------------------------------------------------------------------
def test_own_draws_follow_the_seed_and_hold_their_foreground():
    M, H, W, h, w, B = 4, 40, 56, 16, 24, 32
    mask, _ = _mask("f3", M, H, W, seed=7)
    image = torch.randn((M, 3, H, W), generator=torch.Generator().manual_seed(7))
    runs = []
    for seed in (11, None, 11):
        if seed is not None:
            pool = _sampler(mask, None, (h, w), B, images=image, pos=0.6)
            torch.manual_seed(seed)
        x, t = pool()
        torch.cuda.synchronize()
        runs.append((x.cpu(), t.cpu(), pool.last_coords.cpu(), pool.u.cpu()))
    a, b, c = runs
    assert all(torch.equal(p, q) for p, q in zip(a, c))
    assert not torch.equal(a[2], b[2]) and not torch.equal(a[0], b[0])
    for x, t, coords, u in (a, b):
        coords = coords.numpy()
        assert np.array_equal(coords, R.draw(u.numpy(), R.index(mask), R.planes(mask), M, H, W, h, w, 0.6, 1.0))
        m, y0, x0, plane = coords.T
        assert ((m >= 0) & (m < M) & (y0 >= 0) & (y0 <= H - h) & (x0 >= 0) & (x0 <= W - w)).all()
        assert (plane >= 0).any() and (plane == -1).any()
        for k in np.flatnonzero(plane >= 0):
            assert (t[int(k), int(plane[k])] > 0.5).any(), k                       # a foreground patch holds foreground of its plane


# ---- 6. set_indices ---------------------------------------------------------------------------------------------------------------
def test_set_indices_names_the_pictures():
    M, H, W, B = 5, 20, 24, 6
    image = torch.arange(1, M + 1, dtype=torch.float32).view(M, 1, 1, 1).expand(M, 1, H, W).contiguous()
    lab = torch.zeros((M, H, W), dtype=torch.int64)
    lab[:, 3:9, 4:12] = torch.arange(1, M + 1).view(M, 1, 1) % 3          # classes 1, 2, 0, 1, 2
    pool = PatchSampler(image, lab, window=(8, 8), batch=B, pos=0.5, num_classes=3)
    with pytest.raises(ValueError, match="indices"):
        pool.set_indices([0, 1])
    idx = [3, 0, 7, 4, -1, 3]
    pool.set_indices(idx)
    for _ in range(2):                                                    # they hold until they are set again
        x, t = pool()
        torch.cuda.synchronize()
        coords = pool.last_coords.cpu().numpy()
        assert coords[:, 0].tolist() == [3, 0, -1, 4, -1, 3]
        for b, m in enumerate(coords[:, 0]):
            assert (x[b] == float(m + 1 if m >= 0 else 0)).all()
        want, mwant = R.cut(image.numpy(), lab.numpy().astype(np.int32), coords, 8, 8)
        assert np.array_equal(x.cpu().numpy().astype(np.float64), want) and np.array_equal(t.cpu().numpy(), mwant)
        want_c = R.draw(pool.u.cpu().numpy(), R.index(lab.numpy().astype(np.int32), 3), R.planes(lab.numpy().astype(np.int32), 3),
                        M, H, W, 8, 8, 0.5, 1.0, indices=idx)
        assert np.array_equal(coords, want_c)
    pool.set_indices(torch.tensor([1, 1, 1, 2, 2, 2]))
    pool()
    assert pool.last_coords[:, 0].tolist() == [1, 1, 1, 2, 2, 2]
    pool.set_indices(None)                                                # nothing was captured: drawn pictures again
    assert pool.desc.use_indices == 0


# ---- 7. in the step ---------------------------------------------------------------------------------------------------------------
def _model(classes):
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=classes)
    m.run_dtype = torch.float32
    return m.cuda().train()


def _step_pool(multiclass, **kw):
    g = torch.Generator().manual_seed(8)
    x = torch.randn((3, 3, 96, 112), generator=g)
    if multiclass:
        t = torch.randint(0, 3, (3, 96, 112), generator=g) * (torch.rand((3, 96, 112), generator=g) < 0.2)
        t[0, :4] = -100
        pool = PatchSampler(x, t, window=(64, 64), batch=2, pos=0.5, num_classes=3, **kw)
        return pool, 3, (lambda: MulticlassLoss.ce_dice(ignore_index=-100))
    t = (torch.rand((3, 1, 96, 112), generator=g) < 0.2).float()
    return PatchSampler(x, t, window=(64, 64), batch=2, pos=0.5, **kw), 1, (lambda: "bce_dice")


FORCED = torch.tensor([[0.9, 0.1, 0.2, 0.6, 0.3, 0.8, 0.0, 0.0], [0.4, 0.9, 0.5, 0.5, 0.99, 0.01, 0.0, 0.0]])


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("multiclass", [False, True])
def test_step_with_source_equals_step_fed_with_the_patches(multiclass, augment):
    pool, classes, crit = _step_pool(multiclass)
    pool.force_draws(FORCED, sticky=True)
    xs, ts = (v.clone() for v in pool())
    assert ts.dtype == (torch.int32 if multiclass else torch.float32)
    assert pool.last_coords[:, 3].tolist()[1] == -1 and pool.last_coords[0, 3].item() >= 0      # one patch of either mode
    aug = None
    if augment:
        aug = GpuAugment(hflip=0.5, vflip=0.5, rotate=25.0, scale=(0.8, 1.2), translate=0.1, brightness=0.2, contrast=0.2, label_fill=-100)
        aug.force_draws(u=torch.rand((2, 8), generator=torch.Generator().manual_seed(9)).to(DEV), sticky=True)
        xs, ts = (v.clone() for v in aug(xs, ts))
    plain = unet_zoo_amd.GraphedStep(_model(classes), crit(), lr=1e-3)
    fused = unet_zoo_amd.GraphedStep(_model(classes), crit(), lr=1e-3, augment=aug, source=pool)
    assert plain.sampled is None and plain.coords is None
    with pytest.raises(TypeError, match="without arguments"):
        fused(xs, ts)
    for k in range(3):
        l0 = plain(xs, ts).clone()
        g0 = plain.flat_grad.clone()
        l1 = fused().clone()
        g1 = fused.flat_grad.clone()
        assert torch.equal(l0, l1) and torch.equal(g0, g1), k
        assert torch.equal(plain.dice, fused.dice), k
        seen = fused.augmented if augment else fused.sampled
        assert torch.equal(seen[0], xs) and torch.equal(seen[1], ts)
        assert torch.equal(fused.coords, pool.last_coords)
    assert "PatchSampler" in fused.describe()


def test_step_with_an_eager_criterion_samples_in_the_forward_graph():
    pool, classes, _ = _step_pool(False)
    pool.force_draws(FORCED, sticky=True)
    xs, ts = (v.clone() for v in pool())

    def bce(out, tt):
        return torch.nn.functional.binary_cross_entropy_with_logits(out, tt)
    plain = unet_zoo_amd.GraphedStep(_model(classes), bce, lr=1e-3)
    fused = unet_zoo_amd.GraphedStep(_model(classes), bce, lr=1e-3, source=pool)
    for k in range(2):
        l0, l1 = plain(xs, ts).clone(), fused().clone()
        assert torch.equal(l0, l1) and torch.equal(plain.flat_grad, fused.flat_grad), k


def test_step_draws_afresh_in_every_replay_and_follows_the_seed():
    runs = []
    for _ in range(2):
        pool, classes, crit = _step_pool(False)
        step = unet_zoo_amd.GraphedStep(_model(classes), crit(), lr=1e-3, source=pool)
        torch.manual_seed(22)
        losses, seen = [], []
        for _ in range(3):
            losses.append(step().clone())
            seen.append(step.coords.clone())
        assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])      # seen[0]: first replay after the capture
        with pytest.raises(RuntimeError, match="captured"):
            pool.set_indices([0, 1])
        runs.append((torch.stack(losses), torch.stack(seen)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_step_refuses_a_source_whose_masks_do_not_fit_the_criterion():
    pool, classes, _ = _step_pool(True)
    with pytest.raises(ValueError, match="source"):
        unet_zoo_amd.GraphedStep(_model(1), "bce_dice", source=pool)
    nomask = PatchSampler(torch.zeros((2, 3, 96, 112)), window=(64, 64), batch=2)
    with pytest.raises(ValueError, match="no masks"):
        unet_zoo_amd.GraphedStep(_model(1), "bce_dice", source=nomask)
