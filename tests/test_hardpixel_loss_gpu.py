"""GPU: HardPixelLoss (uz_hardpixel_loss) -- the pixel losses, the exact selection, the loss and its gradients against the
definition restated with torch on the CPU in float64 (tests/hardpixel_ref.py), and inside GraphedStep / GraphedEval against
the eager step.

Bounds are those of tests/test_region_loss_gpu.py: |loss - ref| < 2e-6 max(1, |ref|), max |dlogits - ref| <= 2e-6 max |ref grad|,
the Dice metric within 1e-6 of the base's.  torch's own float32 evaluation of the term deviates from float64 by at most 0.070
(value: binary mode, 3 x 1 x 17 x 23 per image, keep 0.1, gamma 2) and 0.36 (gradient: class mode, K = 4, focal gamma 2 over every
pixel) of these bounds on the cases below (tests/test_hardpixel_loss.py prints every share).

The device's exp and log are not the CPU's, so the checks are layered:
 1. `losses` within 2e-6 max(1, f) of the float64 f;
 2. `selection` exactly what the reference's selection yields on the device's OWN losses: m, n_above, n_tie, and tau bit for bit;
 3. loss and gradient against float64 evaluated with that kept set; the loss also against the fully independent reference
    (it is continuous across near-tie swaps)."""
import pytest
import torch

import hardpixel_ref as R  # tests/hardpixel_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from unet_zoo_amd import HardPixelLoss, MulticlassLoss, RegionLoss
from unet_zoo_amd import _lib as L
from unet_zoo_amd.augment import GpuAugment
from unet_zoo_amd.capture import _check_capture
from unet_zoo_amd.optim import FlatClipAdamW

pytestmark = pytest.mark.gpu

DEV = "cuda"


def check_loss(got, ref):
    got, ref = float(got), float(ref)
    print(f"loss {got:.9g} ref {ref:.9g} |diff| {abs(got - ref):.3e} bound {2e-6 * max(1.0, abs(ref)):.3e} "
          f"share {abs(got - ref) / (2e-6 * max(1.0, abs(ref))):.3f}")
    assert abs(got - ref) < 2e-6 * max(1.0, abs(ref))


def check_grad(got, ref):
    err, top = (got.detach().cpu().double() - ref).abs().max().item(), ref.abs().max().item()
    print(f"grad max|diff| {err:.3e} bound {2e-6 * top:.3e} (max |ref grad| {top:.3e}) share {err / (2e-6 * max(top, 1e-300)):.3f}")
    assert err <= 2e-6 * top


BASES = {
    "bce_dice": ("bce_dice", lambda: "bce_dice", {}),
    "region_dice": ("region", lambda: RegionLoss.dice(), R.REGION_KW),
    "focal_tversky": ("region", lambda: RegionLoss(**R.FOCAL_KW), R.FOCAL_KW),
    "multiclass": ("multiclass", lambda: MulticlassLoss(**R.CLASS_KW), R.CLASS_KW),
}


def check_layers(crit, base, x, target, weight, base_scale, loss, grad, **kw):
    """the three layers of the module docstring for one map; returns the device's selection (S, 4) int64"""
    kind, _, base_kw = BASES[base]
    cls = kind == "multiclass"
    losses, sel = crit.losses.cpu(), crit.selection.cpu().long()
    S = x.shape[0] if kw.get("per_image") else 1
    assert losses.dtype == torch.float32 and tuple(losses.shape) == ((x.shape[0],) + tuple(x.shape[2:]) if cls else tuple(x.shape))
    assert crit.selection.dtype == torch.int32 and tuple(sel.shape) == (S, 4)
    # 1. the pixel losses against float64
    ind_loss, _, (ind_term,), (f64,), _ = R.reference(kind, [x], target, [1.0], weight, base_scale, base_kw=base_kw, **kw)
    share = ((losses.double() - f64).abs() / f64.clamp(min=1.0)).max().item() / 2e-6
    print(f"losses max|diff| / max(1, f): {2e-6 * share:.3e} share {share:.3f}")
    assert share <= 1.0
    valid = R.pixel_losses(x, target, cls, ignore_index=base_kw.get("ignore_index", -100))[2]
    assert not losses[~valid].any()
    # 2. the selection on the device's own losses, exactly
    want = R.selection_of(losses, valid, S, kw.get("keep", 0.1), kw.get("min_kept", 0), kw.get("max_prob"))
    assert torch.equal(sel, want), (sel.tolist(), want.tolist())
    # 3. loss and gradient in float64 with the device's kept set; the loss also fully independently
    ref_loss, (ref_grad,), (term,), _, _ = R.reference(kind, [x], target, [1.0], weight, base_scale, base_kw=base_kw, losses=[losses], **kw)
    check_loss(loss.item(), ref_loss.item())
    check_grad(grad, ref_grad)
    assert abs(crit.term.item() - term.item()) < 2e-6 * max(1.0, abs(term.item()))
    check_loss(loss.item(), ind_loss.item())
    return sel


# ------------------------------------------------------------------------------------------- binary mode: select, loss, protocol
@pytest.mark.parametrize("shape,per_image,base,keep,gamma", R.BINARY_CASES,
                         ids=[f"{'x'.join(map(str, s))}-{'image' if p else 'batch'}-{b}-keep{k}-gamma{g:g}" for s, p, b, k, g in R.BINARY_CASES])
def test_binary_mode_matches_the_definition(shape, per_image, base, keep, gamma):
    weight, base_scale = (0.5, 1.0) if base != "focal_tversky" else (0.3, 0.6)
    x, t = R.make_inputs(shape)
    make = BASES[base][1]
    crit = HardPixelLoss(base=make(), weight=weight, base_scale=base_scale, keep=keep, gamma=gamma, per_image=per_image)
    xd, td = x.to(DEV), t.to(DEV)
    loss, dice, (g,) = crit.direct(xd, td)
    torch.cuda.synchronize()
    assert loss.dim() == 0 and dice.dim() == 0 and loss.is_cuda and g.shape == xd.shape and g.dtype == torch.float32
    sel = check_layers(crit, base, x, t, weight, base_scale, loss, g, keep=keep, gamma=gamma, per_image=per_image)
    n = t.numel() // (shape[0] if per_image else 1)
    assert (sel[:, 0] == (n if keep == 1.0 else R.kept_count(n, 0, keep, 0))).all()
    # the Dice metric is the base's
    b = make()
    base_dice = unet_zoo_amd.loss.loss_and_dice(xd, td)[1] if isinstance(b, str) else b.loss_and_dice(xd, td)[1]
    assert abs(dice.item() - base_dice.item()) < 1e-6
    # a second call: the same bits, the selection included
    first_sel, first_losses = crit.selection.clone(), crit.losses.clone()
    loss2, dice2, (g2,) = crit.direct(xd, td)
    assert torch.equal(loss2, loss) and torch.equal(dice2, dice) and torch.equal(g2, g)
    assert torch.equal(crit.selection, first_sel) and torch.equal(crit.losses, first_losses)
    # no gradient asked for: the same loss, and no gradient buffer is handed to the library
    seen = []
    real = L.hardpixel_loss

    def spy(desc, items, *a):
        seen.append([bool(it.dlogits) for it in items])
        return real(desc, items, *a)
    L.hardpixel_loss = spy
    try:
        with torch.no_grad():
            loss3, dice3 = crit.loss_and_dice(xd, td)
    finally:
        L.hardpixel_loss = real
    assert seen == [[False]] and torch.equal(loss3, loss) and torch.equal(dice3, dice) and not loss3.requires_grad
    # through autograd: the same numbers again
    leaf = xd.clone().requires_grad_(True)
    loss4 = crit(leaf, td)
    loss4.backward()
    assert torch.equal(loss4.detach(), loss) and torch.equal(leaf.grad, g)


# ------------------------------------------------------------------------------------------------------------------ class mode
@pytest.mark.parametrize("K,mode,per_image,blank", R.CLASS_CASES,
                         ids=[f"K{K}-{m}-{'image_one_blank' if p else 'batch'}" for K, m, p, _ in R.CLASS_CASES])
def test_class_mode_matches_the_reference(K, mode, per_image, blank):
    x, y = R.class_case_inputs(K, blank)
    keep, min_kept, max_prob = R.CLASS_MODES[mode]
    base = MulticlassLoss(**R.CLASS_KW)
    if mode == "topk":
        crit = HardPixelLoss.topk(base, 0.1, weight=0.5, base_scale=0.8, per_image=per_image)
    else:
        crit = HardPixelLoss.ohem(base, max_prob, min_kept=min_kept, weight=0.5, base_scale=0.8, per_image=per_image)
    assert (crit.keep, crit.min_kept, crit.max_prob) == (keep, min_kept, max_prob)
    loss, dice, (grad,) = crit.direct(x.to(DEV), y.to(DEV))                # labels (N, H, W), int64
    sel = check_layers(crit, "multiclass", x, y, 0.5, 0.8, loss, grad, keep=keep, min_kept=min_kept, max_prob=max_prob, per_image=per_image)
    losses = crit.losses.cpu()
    valid = (y >= 0) & (y < K)
    assert (~valid).sum() > 5 * y.shape[2] and (y >= K).any() and (y == -7).any() == (not blank)
    c = int((losses[valid] > R.threshold(max_prob)).sum())
    n = int(valid.sum())
    if mode == "topk":
        assert sel[0, 0] == R.kept_count(int(valid[0].sum()) if per_image else n, 0, 0.1, 0)
    elif mode == "ohem":
        assert c < 50 and sel[0, 0] == 50                                  # min_kept decides
    else:
        assert c > 5 and sel[0, 0] == c                                    # c > k: max_prob decides
    _, base_dice = base.loss_and_dice(x.to(DEV), y.to(DEV))
    assert abs(dice.item() - base_dice.item()) < 1e-6
    # exactly nothing of the term at a pixel in no segment, on all K logits: the gradient there is the base's, which is zero
    assert not grad.cpu()[(~valid).unsqueeze(1).expand_as(x)].any()
    if blank:                                                              # a segment without a valid pixel adds 0
        assert sel[1].tolist() == [0, 0, 0, 0] and not grad.cpu()[1].any() and not losses[1].any()
        one = HardPixelLoss.topk(MulticlassLoss(**R.CLASS_KW), 0.1, weight=0.5, base_scale=0.8, per_image=True)
        one.direct(x[:1].to(DEV), y[:1].to(DEV))
        assert abs(crit.term.item() - one.term.item()) < 2e-6 * max(1.0, one.term.item())      # the mean over the segments with n > 0
    # int64 labels of shape (N, 1, H, W) and no gradient: the same loss
    with torch.no_grad():
        loss2, _ = crit.loss_and_dice(x.to(DEV), y.unsqueeze(1).to(DEV))
    assert torch.equal(loss2, loss)


@pytest.mark.parametrize("K,keep,gamma,per_image", R.FOCAL_CLASS_CASES,
                         ids=[f"K{K}-keep{k:g}-gamma{g:g}-{'image' if p else 'batch'}" for K, k, g, p in R.FOCAL_CLASS_CASES])
def test_class_mode_with_the_focal_modulation(K, keep, gamma, per_image):
    """(1 - p_t)^gamma CE over every pixel (HardPixelLoss.focal) and as a focal top-k: df/dl in the class-mode gradient, q^gamma
    by multiplication (gamma = 2) and by powf (gamma = 1.5)"""
    x, y = R.make_class_inputs(K, lift=4.0)
    base = MulticlassLoss(**R.CLASS_KW)
    if keep == 1.0:
        crit = HardPixelLoss.focal(base, gamma, weight=0.5, base_scale=0.8, per_image=per_image)
    else:
        crit = HardPixelLoss.topk(base, keep, gamma=gamma, weight=0.5, base_scale=0.8, per_image=per_image)
    loss, _, (grad,) = crit.direct(x.to(DEV), y.to(DEV))
    sel = check_layers(crit, "multiclass", x, y, 0.5, 0.8, loss, grad, keep=keep, gamma=gamma, per_image=per_image)
    valid = (y >= 0) & (y < K)
    n = [int(valid[i].sum()) for i in range(y.shape[0])] if per_image else [int(valid.sum())]
    assert sel[:, 0].tolist() == [R.kept_count(v, 0, keep, 0) for v in n]
    assert not grad.cpu()[(~valid).unsqueeze(1).expand_as(x)].any()
    # the term's own gradient (the base scaled away) against the usual focal formula by float64 autograd
    if keep == 1.0 and not per_image:
        alone = HardPixelLoss.focal(MulticlassLoss(**R.CLASS_KW), gamma, weight=1.0, base_scale=0.0)
        l1, _, (g1,) = alone.direct(x.to(DEV), y.to(DEV))
        leaf = x.double().requires_grad_(True)
        logp = torch.log_softmax(leaf, 1).gather(1, y.clamp(0, K - 1).unsqueeze(1)).squeeze(1)
        want = ((1 - logp.exp()) ** gamma * -logp)[valid].mean()
        check_loss(l1.item(), want.item())
        check_grad(g1, torch.autograd.grad(want, leaf)[0])


# ------------------------------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("per_image", [True, False], ids=["image", "batch"])
def test_ties_share_the_weight_whatever_their_order(per_image):
    """logits snapped to multiples of 0.25: fewer than 200 distinct f, more than 100 of them equal to tau -- the fractional tie
    weight; the same through bf16 (the snapped values are exact)"""
    x, t = R.make_tied_inputs()
    crit = HardPixelLoss(base=RegionLoss.dice(), weight=0.5, keep=R.TIED_KEEP, per_image=per_image)
    loss, _, (g,) = crit.direct(x.to(DEV), t.to(DEV))
    sel = check_layers(crit, "region_dice", x, t, 0.5, 1.0, loss, g, keep=R.TIED_KEEP, per_image=per_image)
    assert crit.losses.unique().numel() < 200
    assert (sel[:, 2] >= 100).all() and ((sel[:, 0] - sel[:, 1] > 0) & (sel[:, 0] - sel[:, 1] < sel[:, 2])).all()
    first = (crit.losses, crit.selection.clone(), loss.clone())
    assert torch.equal(x.bfloat16().float(), x)
    with torch.no_grad():
        loss_b = crit(x.to(DEV).bfloat16(), t.to(DEV))
    assert torch.equal(crit.selection, first[1])
    check_loss(loss_b.item(), first[2].item())
    # the same pixels in another order (the maps flipped): the same selection; the value but for the order of the sums
    loss_f, _, _ = crit.direct(x.flip(2, 3).contiguous().to(DEV), t.flip(2, 3).contiguous().to(DEV))
    assert torch.equal(crit.selection, first[1])
    check_loss(loss_f.item(), first[2].item())


# ------------------------------------------------------------------------------------------------- every round of the select
def test_losses_that_differ_in_the_last_digit_only():
    """every l between 1 and 1 + 256 ulps: three rounds find one full bin each, the last one decides"""
    x, t = R.make_narrow_inputs()
    crit = HardPixelLoss(base=RegionLoss.dice(), weight=0.5, keep=0.25, per_image=True)
    loss, _, (g,) = crit.direct(x.to(DEV), t.to(DEV))
    bits = crit.losses.cpu().view(torch.int32)
    assert ((bits >> 8) == (0x3F800000 >> 8)).all() and (bits & 255).unique().numel() > 50
    check_layers(crit, "region_dice", x, t, 0.5, 1.0, loss, g, keep=0.25, per_image=True)


@pytest.mark.parametrize("mode,big", [("class", 60.0), ("binary", 60.0), ("binary", 200.0)], ids=["class60", "binary60", "binary200"])
def test_a_segment_of_equal_losses_with_everything_kept(mode, big):
    """image 0: logits of +-`big` on the right side, keep = 1: every f of that segment is the same value -- exactly 0 where
    exp(-2 big) (class) or exp(-big) (binary) underflows in fp32, 8.76e-27 in the binary mode at 60 -- so every round sees ONE
    bin and n_tie = n; image 1 is ordinary (and keeps the gradient bound inside fp32's range)"""
    g = torch.Generator().manual_seed(11)
    if mode == "class":
        y = torch.randint(0, 4, (2, 9, 31), generator=g)
        x = 3.0 * torch.randn(2, 4, 9, 31, generator=g)
        x[0] = big * (2.0 * torch.nn.functional.one_hot(y[0], 4).permute(2, 0, 1).float() - 1.0)
        crit = HardPixelLoss(base=MulticlassLoss(**R.CLASS_KW), weight=0.5, keep=1.0, per_image=True)
        base = "multiclass"
    else:
        y = (torch.rand(2, 1, 9, 31, generator=g) > 0.5).float()
        x = 3.0 * torch.randn(2, 1, 9, 31, generator=g)
        x[0] = big * (2.0 * y[0] - 1.0)
        crit = HardPixelLoss(base=RegionLoss.dice(), weight=0.5, keep=1.0, per_image=True)
        base = "region_dice"
    loss, _, (grad,) = crit.direct(x.to(DEV), y.to(DEV))
    sel = check_layers(crit, base, x, y, 0.5, 1.0, loss, grad, keep=1.0, per_image=True)
    f = crit.losses.cpu()[0]
    assert f.unique().numel() == 1 and sel[0, :3].tolist() == [279, 0, 279] and sel[1, 0] == 279
    if mode == "class" or big > 100:
        assert not f.any() and sel[0, 3] == 0
    else:
        assert 0.0 < f.reshape(-1)[0] < 1e-25


@pytest.mark.parametrize("per_image", [False, True], ids=["batch", "image"])
def test_a_segment_with_a_single_valid_pixel(per_image):
    x, _ = R.make_class_inputs(4)
    y = torch.full((2, 33, 47), -100)
    y[1, 20, 30] = 2
    crit = HardPixelLoss.topk(MulticlassLoss(**R.CLASS_KW), 0.1, weight=0.5, per_image=per_image)
    loss, _, (grad,) = crit.direct(x.to(DEV), y.to(DEV))
    sel = check_layers(crit, "multiclass", x, y, 0.5, 1.0, loss, grad, keep=0.1, per_image=per_image)
    assert sel[-1, :3].tolist() == [1, 0, 1] and sel[-1, 3] == int(crit.losses[1, 20, 30].cpu().view(torch.int32))
    assert abs(crit.term.item() - crit.losses[1, 20, 30].item()) < 2e-6 * max(1.0, crit.term.item())
    if per_image:
        assert sel[0].tolist() == [0, 0, 0, 0]
    hit = torch.zeros_like(x, dtype=torch.bool)
    hit[1, :, 20, 30] = True
    assert grad.cpu()[hit].any() and not grad.cpu()[~hit].any()


# ----------------------------------------------------------------------------------------------------------- workgroups walk
def _capped(crit, shape, max_workgroups):
    """a second object whose plan for `shape` was built in the test with max_workgroups set"""
    twin = HardPixelLoss(base=crit.base, weight=crit.weight, base_scale=crit.base_scale, keep=crit.keep, min_kept=crit.min_kept,
                         max_prob=crit.max_prob, gamma=crit.gamma, per_image=crit.per_image)
    dev = torch.device(DEV, torch.cuda.current_device())
    plan = twin._build_plan(1, shape, dev, 0)
    plan[0].max_workgroups = max_workgroups
    grid, units = L.hardpixel_grid(plan[0])
    assert grid == max_workgroups < units, (grid, units)
    twin._plans[(1, tuple(shape), dev.index, 0)] = plan
    return twin


@pytest.mark.parametrize("mode", ["binary", "class"])
def test_workgroups_walk_several_units(mode):
    """(2, 3, 40, 40) is five units of one segment, the class case (3, 4, 50, 60) five as well: with 2 and with 3 workgroups the
    results are the bits of the uncapped call (counts are integers, the float64 sums are per unit)"""
    if mode == "binary":
        x, t = R.make_inputs((2, 3, 40, 40))
        crit = HardPixelLoss(base=RegionLoss.dice(), weight=0.5, keep=0.1, gamma=2.0)
        kw, base = dict(keep=0.1, gamma=2.0), "region_dice"
    else:
        g = torch.Generator().manual_seed(12)
        x, t = 3.0 * torch.randn(3, 4, 50, 60, generator=g), R.make_labels(3, 4, 50, 60, seed=12)
        crit = HardPixelLoss.ohem(MulticlassLoss(**R.CLASS_KW), 0.7, min_kept=50, weight=0.5)
        kw, base = dict(keep=R.MIN_KEEP, min_kept=50, max_prob=0.7), "multiclass"
    xd, td = x.to(DEV), t.to(DEV)
    loss, dice, (grad,) = crit.direct(xd, td)
    check_layers(crit, base, x, t, 0.5, 1.0, loss, grad, **kw)
    desc = crit._plan(1, x.shape, xd.device, 0)[0]
    assert L.hardpixel_grid(desc) == (5, 5)
    for cap in (2, 3):
        twin = _capped(crit, tuple(x.shape), cap)
        loss2, dice2, (grad2,) = twin.direct(xd, td)
        assert twin._plan(1, x.shape, xd.device, 0)[0].max_workgroups == cap
        assert torch.equal(loss2, loss) and torch.equal(dice2, dice) and torch.equal(grad2, grad)
        assert torch.equal(twin.losses, crit.losses) and torch.equal(twin.selection, crit.selection) and torch.equal(twin.term, crit.term)


# ------------------------------------------------------------------------------------------------------------------ protocol
@pytest.mark.parametrize("base", list(BASES))
def test_weight_zero_reproduces_the_base_exactly(base):
    if base == "multiclass":
        x, t = R.make_class_inputs(4)
    else:
        x, t = R.make_inputs((3, 1, 17, 23))
    make = BASES[base][1]
    xd, td = x.to(DEV), t.to(DEV)
    b = make()
    if isinstance(b, str):
        want_l, want_d, want_g = unet_zoo_amd.loss.loss_and_dice_direct(xd, td)
    else:
        want_l, want_d, want_g = b.direct(xd, td)
    want_g = want_g[0].clone()
    loss, dice, (grad,) = HardPixelLoss(base=make(), weight=0.0).direct(xd, td)
    assert torch.equal(loss, want_l) and torch.equal(dice, want_d) and torch.equal(grad, want_g)


def test_three_maps_cost_one_call_dict_and_list():
    g = torch.Generator().manual_seed(7)
    shape = (2, 1, 24, 20)
    maps = {f"d{i}": 2.0 * torch.randn(shape, generator=g) for i in range(3)}
    t = (torch.rand(shape, generator=g) > 0.6).float()
    ow = (1.0, 0.5, 0.25)
    kw = dict(alpha=0.6, beta=0.4, gamma=1.5)
    hp = dict(keep=0.2, gamma=2.0, per_image=True)
    calls = []
    real = L.hardpixel_loss

    def spy(desc, items, *a):
        calls.append((desc.n_items, sum(1 for it in items if it.dlogits)))
        return real(desc, items, *a)
    L.hardpixel_loss = spy
    try:
        crit = HardPixelLoss(base=RegionLoss(output_weights=dict(zip(maps, ow)), **kw), weight=0.7, base_scale=0.9, **hp)
        leaves = {k: v.to(DEV).requires_grad_(True) for k, v in maps.items()}
        loss, dice = crit.loss_and_dice(leaves, t.to(DEV))
        assert calls == [(3, 3)]                                      # ONE uz_hardpixel_loss for the three maps
        loss.backward()
        assert calls == [(3, 3)]                                      # ... and none in backward
    finally:
        L.hardpixel_loss = real
    ref_loss, ref_grads, terms, fs, _ = R.reference("region", list(maps.values()), t, ow, 0.7, 0.9, base_kw=kw, **hp)
    assert ((crit.losses.cpu().double() - fs[0]).abs() / fs[0].clamp(min=1.0)).max() <= 2e-6      # the main map of a dict is its first
    ones = torch.ones_like(t, dtype=torch.bool)
    assert torch.equal(crit.selection.cpu().long(), R.selection_of(crit.losses.cpu(), ones, 2, 0.2))
    check_loss(loss.item(), ref_loss.item())
    for leaf, gr in zip(leaves.values(), ref_grads):                  # every map is mined on its own
        check_grad(leaf.grad, gr)
    assert abs(crit.term.item() - terms[0].item()) < 2e-6 * max(1.0, abs(terms[0].item()))
    _, base_dice = RegionLoss(**kw).loss_and_dice(maps["d0"].to(DEV), t.to(DEV))
    assert abs(dice.item() - base_dice.item()) < 1e-6 and not dice.requires_grad
    # a list with weights by position: the main map is the last
    crit2 = HardPixelLoss(base=RegionLoss(output_weights=list(ow), **kw), weight=0.7, base_scale=0.9, **hp)
    loss2, _, gouts = crit2.direct([v.to(DEV) for v in maps.values()], t.to(DEV))
    assert ((crit2.losses.cpu().double() - fs[2]).abs() / fs[2].clamp(min=1.0)).max() <= 2e-6
    assert torch.equal(crit2.selection.cpu().long(), R.selection_of(crit2.losses.cpu(), ones, 2, 0.2))
    check_loss(loss2.item(), ref_loss.item())
    for got, gr in zip(gouts, ref_grads):
        check_grad(got, gr)
    assert abs(crit2.term.item() - terms[2].item()) < 2e-6 * max(1.0, abs(terms[2].item()))
    # "bce_dice" over a list: unit weights
    ref3, g3, _, _, _ = R.reference("bce_dice", list(maps.values()), t, (1.0, 1.0, 1.0), 0.7, **hp)
    loss3, _, gouts3 = HardPixelLoss(weight=0.7, **hp).direct([v.to(DEV) for v in maps.values()], t.to(DEV))
    check_loss(loss3.item(), ref3.item())
    for got, gr in zip(gouts3, g3):
        check_grad(got, gr)


def test_set_weights_equals_a_fresh_object():
    shape = (3, 1, 17, 23)
    x, t = R.make_inputs(shape)
    xd, td = x.to(DEV), t.to(DEV)
    crit = HardPixelLoss.topk(RegionLoss.dice(), 0.1, weight=0.5)
    crit.direct(xd, td)
    crit.set_weights(weight=0.3, base_scale=0.0)                      # the mined term alone: the base is still launched
    loss, dice, (grad,) = crit.direct(xd, td)
    fresh = HardPixelLoss.topk(RegionLoss.dice(), 0.1, weight=0.3, base_scale=0.0)
    fresh_loss, fresh_dice, (fresh_grad,) = fresh.direct(xd, td)
    assert torch.equal(loss, fresh_loss) and torch.equal(grad, fresh_grad) and torch.equal(dice, fresh_dice)
    check_layers(crit, "region_dice", x, t, 0.3, 0.0, loss, grad, keep=0.1)
    assert abs(loss.item() - 0.3 * crit.term.item()) < 2e-6
    _, base_dice = RegionLoss.dice().loss_and_dice(xd, td)
    assert abs(dice.item() - base_dice.item()) < 1e-6


# ------------------------------------------------------------------------------------------------- inside the graphed runners
def _make(dtype, train=True, num_classes=1):
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=num_classes)
    m.run_dtype = dtype
    m = m.cuda()
    return m.train() if train else m.eval()


def _batch(seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 3, 32, 32, generator=g).cuda(), (torch.rand(2, 1, 32, 32, generator=g) > 0.5).float().cuda()


def _eager_twin(gs, m1, m2):
    n1 = {id(p): n for n, p in m1.named_parameters()}
    p2 = dict(m2.named_parameters())
    opt = FlatClipAdamW([p2[n1[id(p)]] for p in gs.opt.params], lr=1e-3, weight_decay=1e-5, max_norm=1.0)
    m2._pack_cache.repoint()
    m2.grads_in_place = True
    return opt


def _criterion(weight=0.5):
    return HardPixelLoss.topk(RegionLoss(alpha=0.7, beta=0.3, gamma=4 / 3), 0.25, weight=weight, per_image=True)


def test_graphed_step_equals_eager_step_bitwise_and_set_weights_does_not_recapture():
    x, t = _batch()
    m1, m2 = _make(torch.float32), _make(torch.float32)
    crit1, crit2 = _criterion(), _criterion()
    gs = unet_zoo_amd.GraphedStep(m1, crit1, lr=1e-3, weight_decay=1e-5, max_norm=1.0)
    assert gs._fused_loss
    opt = None
    g_res, e_res = [], []
    graphs = None
    for k in range(4):
        if k == 2:                               # less base, more of the mined term; the graphs stay what they are
            graphs = (gs._cur, tuple(gs._cur.phases), gs._g_opt)
            crit1.set_weights(weight=1.0, base_scale=0.25)
            crit2 = _criterion()                 # a fresh object with the new weights: the eager step's
            crit2.set_weights(weight=1.0, base_scale=0.25)
        loss = gs(x, t)
        torch.cuda.synchronize()
        g_res.append((loss.item(), gs.dice.item(), gs.grad_norm.item()))
        if opt is None:
            opt = _eager_twin(gs, m1, m2)
        l2, d2 = crit2.loss_and_dice(m2(x), t)
        l2.backward()
        opt.step()
        torch.cuda.synchronize()
        e_res.append((l2.item(), d2.item(), opt.last_grad_norm().item()))
        assert torch.equal(crit1.selection, crit2.selection) and torch.equal(crit1.losses, crit2.losses)
    cur = gs._cur
    assert cur.fwd is None and len(cur.phases) == 1
    for gk in cur.phases:
        _check_capture(gk, "forward + loss + backward graph")
    assert "eager" not in gs.describe()
    assert graphs[0] is gs._cur and all(a is b for a, b in zip(graphs[1], gs._cur.phases)) and graphs[2] is gs._g_opt
    assert g_res == e_res, (g_res, e_res)
    assert torch.equal(gs.opt.flat_p, opt.flat_p)
    assert all(r[0] == r[0] and 0.0 < r[0] < 40.0 for r in g_res) and len(set(r[0] for r in g_res)) == 4
    # the selection of the step's main map, made inside the graph: the reference's on the step's own losses
    ones = torch.ones(2, 1, 32, 32, dtype=torch.bool)
    assert torch.equal(crit1.selection.cpu().long(), R.selection_of(crit1.losses.cpu(), ones, 2, 0.25))
    assert (crit1.selection[:, 0] == 256).all()


def test_graphed_eval_equals_eager_eval_bitwise_and_follows_set_weights():
    m = _make(torch.float32, train=False)
    crit = _criterion()
    batches = [_batch(seed=s) for s in (1, 2, 3)]

    def eager(weight):
        c, res = _criterion(weight), []
        for x, t in batches:
            with torch.no_grad():
                loss, dice = c.loss_and_dice(m(x), t)
            res.append((loss.clone(), dice.clone(), c.selection.clone()))
        return res
    want, want2 = eager(0.5), eager(1.5)
    ev = unet_zoo_amd.GraphedEval(m, crit)
    assert ev._fused_loss
    for (x, t), (loss, dice, sel) in zip(batches, want):         # the first call captures, the others replay the same graph
        l, d = ev(x, t)
        torch.cuda.synchronize()
        assert torch.equal(l, loss) and torch.equal(d, dice) and l.dim() == 0 and torch.equal(crit.selection, sel)
    graph = next(iter(ev._graphs.values()))
    _check_capture(graph.graph, "evaluation graph")
    crit.set_weights(weight=1.5)
    for (x, t), (loss, dice, sel), (old, _, _) in zip(batches, want2, want):
        l, d = ev(x, t)
        torch.cuda.synchronize()
        assert torch.equal(l, loss) and torch.equal(d, dice) and not torch.equal(l, old) and torch.equal(crit.selection, sel)
    assert len(ev._graphs) == 1 and next(iter(ev._graphs.values())) is graph and ev.captures == 1      # no recapture
    assert "eager" not in ev.describe()


def test_step_with_augment_selects_against_the_augmented_mask():
    x, t = _batch()
    t = torch.zeros_like(t)
    t[:, :, 10:22, 6:20] = 1.0                    # a block that the warp rotates, scales and partly moves out of the picture
    torch.manual_seed(5)
    aug = GpuAugment(hflip=0.5, vflip=0.5, rotate=25.0, scale=(0.8, 1.2), translate=0.1, grid_distort=(4, 2.0))
    crit = HardPixelLoss.topk(RegionLoss.dice(), 0.25, weight=0.5)
    step = unet_zoo_amd.GraphedStep(_make(torch.float32), crit, lr=1e-3, augment=aug)
    seen = []
    for _ in range(2):                            # every replay draws afresh: two different masks, two selections
        step(x, t)
        torch.cuda.synchronize()
        mask = step.augmented[1].cpu()
        assert not torch.equal(mask, t.cpu()) and 0 < int((mask > 0.5).sum()) < mask.numel()
        # the reference's losses for THAT mask, given the step's logits (a static tensor of the graph)
        logits = step.outputs.detach().float().cpu()
        assert logits.shape == mask.shape
        f64 = R.pixel_losses(logits, mask, False)[0]
        assert ((crit.losses.cpu().double() - f64).abs() / f64.clamp(min=1.0)).max() <= 2e-6
        against_old = R.pixel_losses(logits, t.cpu(), False)[0]
        assert ((crit.losses.cpu().double() - against_old).abs() / against_old.clamp(min=1.0)).max() > 1e-3
        want = R.selection_of(crit.losses.cpu(), torch.ones_like(mask, dtype=torch.bool), 1, 0.25)
        assert torch.equal(crit.selection.cpu().long(), want) and want[0, 0] == 512
        seen.append(mask)
    assert not torch.equal(seen[0], seen[1])


def test_multiclass_step_equals_eager_step_bitwise():
    x, _ = _batch()
    g = torch.Generator().manual_seed(9)
    y = torch.randint(0, 4, (2, 32, 32), generator=g)
    y[:, 10, :] = -100
    y = y.cuda()
    m1, m2 = _make(torch.float32, num_classes=4), _make(torch.float32, num_classes=4)
    crit1, crit2 = (HardPixelLoss.ohem(MulticlassLoss.ce_dice(), 0.7, min_kept=200, weight=0.5) for _ in range(2))
    gs = unet_zoo_amd.GraphedStep(m1, crit1, lr=1e-3, weight_decay=1e-5, max_norm=1.0)
    assert gs._fused_loss
    opt = None
    for _ in range(3):
        loss = gs(x, y)
        torch.cuda.synchronize()
        if opt is None:
            opt = _eager_twin(gs, m1, m2)
        l2, d2 = crit2.loss_and_dice(m2(x), y)
        l2.backward()
        opt.step()
        torch.cuda.synchronize()
        assert loss.item() == l2.item() and gs.dice.item() == d2.item() and gs.grad_norm.item() == opt.last_grad_norm().item()
        assert torch.equal(crit1.selection, crit2.selection) and torch.equal(crit1.losses, crit2.losses)
    assert "eager" not in gs.describe() and torch.equal(gs.opt.flat_p, opt.flat_p)
    valid = (y >= 0).cpu()
    want = R.selection_of(crit1.losses.cpu(), valid, 1, R.MIN_KEEP, 200, 0.7)
    assert torch.equal(crit1.selection.cpu().long(), want) and want[0, 0] >= 200 and tuple(crit1.losses.shape) == (2, 32, 32)
