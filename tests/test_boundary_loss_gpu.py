"""GPU: BoundaryLoss (uz_boundary_loss) -- the signed squared distance transform against scipy's, integer for integer, the loss
and its gradients against the definition restated with torch on the CPU in float64 (tests/boundary_ref.py), and inside
GraphedStep / GraphedEval against the eager step.

Bounds are those of tests/test_region_loss_gpu.py: |loss - ref| < 2e-6 max(1, |ref|), max |dlogits - ref| <= 2e-6 max |ref grad|,
the Dice metric within 1e-6 of the base's.  torch's own float32 evaluation of the boundary term deviates from float64 by at
most 0.16 of these bounds on the cases below (the largest share: the gradient at 8 x 1500, where |phi| reaches 1499 and the
loss is 97)."""
import numpy as np
import pytest
import torch

import boundary_ref as R  # tests/boundary_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from unet_zoo_amd import BoundaryLoss, MulticlassLoss, RegionLoss
from unet_zoo_amd import _lib as L
from unet_zoo_amd.augment import GpuAugment
from unet_zoo_amd.capture import _check_capture
from unet_zoo_amd.optim import FlatClipAdamW

pytestmark = pytest.mark.gpu

DEV = "cuda"


def check_loss(got, ref):
    got, ref = float(got), float(ref)
    print(f"loss {got:.9g} ref {ref:.9g} |diff| {abs(got - ref):.3e} bound {2e-6 * max(1.0, abs(ref)):.3e}")
    assert abs(got - ref) < 2e-6 * max(1.0, abs(ref))


def check_grad(got, ref):
    err, top = (got.detach().cpu().double() - ref).abs().max().item(), ref.abs().max().item()
    print(f"grad max|diff| {err:.3e} bound {2e-6 * top:.3e} (max |ref grad| {top:.3e})")
    assert err <= 2e-6 * top


def check_sd2(crit, want):
    got = crit.sd2.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} integers differ"


def make_inputs(shape, seed=0):
    """as tests/test_region_loss_gpu.py: x = 3 randn, t = rand > 0.7; image 1: empty target; image 2 (N > 2): all foreground"""
    g = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(shape, generator=g)
    t = (torch.rand(shape, generator=g) > 0.7).float()
    if shape[0] > 1:
        t[1] = 0.0
    if shape[0] > 2:
        t[2] = 1.0
        x[2] = x[2].abs() + 2.0
    return x, t


def make_labels(N, K, H, W, seed=0):
    """blocky labels 0 .. K-1 with an ignored stripe (-100), out-of-range labels (K + 3, -7) and one image without class 1"""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, K, (N, (H + 3) // 4, (W + 3) // 4), generator=g)
    y = coarse.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :H, :W].contiguous()
    y[:, H // 3, :] = -100
    y[0, 0, 0] = K + 3
    y[-1, H - 1, W // 2] = -7
    y[-1][y[-1] == 1] = 2
    return y


SHAPES = [(1, 1, 4, 4), (3, 1, 17, 23), (5, 1, 64, 48), (2, 3, 33, 20)]
BASES = {
    "bce_dice": ("bce_dice", lambda: "bce_dice", {}),
    "region_dice": ("region", lambda: RegionLoss.dice(), dict(alpha=0.5, beta=0.5, smooth=0.5)),
    "focal_tversky": ("region", lambda: RegionLoss(alpha=0.7, beta=0.3, gamma=4 / 3, smooth=1e-3, pos_weight=2.5),
                      dict(alpha=0.7, beta=0.3, gamma=4 / 3, smooth=1e-3, pos_weight=2.5)),
}

_REFS = {}


def reference(shape, base, weight, base_scale=1.0, spacing=1.0):
    """inputs and the float64 results of one binary case, computed once"""
    key = (shape, base, weight, base_scale, spacing)
    if key not in _REFS:
        x, t = make_inputs(shape)
        kind, _, kw = BASES[base]
        loss, (grad,), (term,), sd2 = R.reference(kind, [x], t, [1.0], weight, base_scale, spacing, base_kw=kw)
        _REFS[key] = (x, t, loss.item(), grad, term.item(), sd2)
    return _REFS[key]


# ------------------------------------------------------------------------------------------------- the transform, bit for bit
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_sd2_equals_scipy_exactly(shape):
    x, t, _, _, _, sd2 = reference(shape, "bce_dice", 0.01)
    crit = BoundaryLoss()
    crit.direct(x.to(DEV), t.to(DEV))
    check_sd2(crit, sd2)
    if shape[0] > 2:
        assert not sd2[1].any() and not sd2[2].any() and sd2[0].any()      # the empty and the full plane inside the batch


def test_one_pixel_in_a_corner_of_8x1500():
    """d2 above 2^20, rows without any foreground, |phi| up to 1499: the transform, the loss and the gradient"""
    g = torch.Generator().manual_seed(2)
    x = 3.0 * torch.randn(1, 1, 8, 1500, generator=g)
    t = torch.zeros(1, 1, 8, 1500)
    t[0, 0, 7, 1499] = 1.0
    ref_loss, (ref_grad,), _, sd2 = R.reference("region", [x], t, [1.0], 0.25, base_kw=dict(alpha=0.5, beta=0.5, smooth=0.5))
    assert sd2.max() == 7 * 7 + 1499 * 1499 > 2 ** 20 and sd2[0, 7, 1499] == -1
    crit = BoundaryLoss(base=RegionLoss.dice(), weight=0.25)
    loss, _, (grad,) = crit.direct(x.to(DEV), t.to(DEV))
    check_sd2(crit, sd2)
    assert ref_loss.item() > 50.0
    check_loss(loss.item(), ref_loss.item())
    check_grad(grad, ref_grad)


def test_empty_full_and_edge_masks():
    H, W = 21, 70
    t = torch.zeros(8, 1, H, W)
    t[1] = 1.0                                   # full
    t[2, 0, :, :5] = 1.0                         # a band on the left edge
    t[3, 0, H - 3:, :] = 1.0                     # ... on the bottom edge
    t[4, 0, 0, 0] = t[4, 0, 0, W - 1] = t[4, 0, H - 1, 0] = t[4, 0, H - 1, W - 1] = 1.0      # the four corners
    t[5] = 1.0
    t[5, 0, 10, 64] = 0.0                        # full but one pixel, at a word boundary of the row
    t[6, 0, :, 63:65] = 1.0                      # a column pair across the 64-pixel word boundary
    t[7, 0, 5, :] = 1.0                          # one full row
    sd2 = R.sd2_planes(R.planes_binary(t.numpy()))
    assert not sd2[0].any() and not sd2[1].any() and sd2[2, 0, 0] == -25 and sd2[5, 10, 64] == 1
    crit = BoundaryLoss(base=RegionLoss.dice())
    crit.direct(torch.zeros(8, 1, H, W, device=DEV), t.to(DEV))
    check_sd2(crit, sd2)
    # the same planes as channels of two images: a plane is an (image, channel)
    crit.direct(torch.zeros(2, 4, H, W, device=DEV), t.reshape(2, 4, H, W).to(DEV))
    check_sd2(crit, sd2)


@pytest.mark.parametrize("include_background", [False, True], ids=["foreground", "with_background"])
@pytest.mark.parametrize("K", [4, 8])
def test_class_mode_matches_the_reference(K, include_background):
    N, H, W = 3, 33, 20
    g = torch.Generator().manual_seed(K)
    x = 2.0 * torch.randn(N, K, H, W, generator=g)
    y = make_labels(N, K, H, W, seed=K)
    kw = dict(w_ce=0.4, w_dice=0.6, smooth=1.0, include_background=True, reduce="image")
    ref_loss, (ref_grad,), (term,), sd2 = R.reference("multiclass", [x], y, [1.0], 0.05, 0.8, 1.5, include_background, base_kw=kw)
    assert sd2.shape[0] == N * (K if include_background else K - 1)
    base = MulticlassLoss(**kw)
    crit = BoundaryLoss(base=base, weight=0.05, base_scale=0.8, spacing=1.5, include_background=include_background)
    loss, dice, (grad,) = crit.direct(x.to(DEV), y.to(DEV))
    check_sd2(crit, sd2)
    check_loss(loss.item(), ref_loss.item())
    check_grad(grad, ref_grad)
    assert abs(crit.term.item() - term.item()) < 2e-6 * max(1.0, abs(term.item()))
    _, base_dice = base.loss_and_dice(x.to(DEV), y.to(DEV))
    assert abs(dice.item() - base_dice.item()) < 1e-6
    ign = ((y == -100) | (y < 0) | (y >= K)).unsqueeze(1).expand_as(x)
    assert ign.any() and not grad.cpu()[ign].any()                     # exactly nothing at an ignored pixel
    # int64 labels of shape (N, 1, H, W) and no gradient: the same loss
    with torch.no_grad():
        loss2, _ = crit.loss_and_dice(x.to(DEV), y.unsqueeze(1).to(DEV))
    assert torch.equal(loss2, loss)


def test_workgroups_walk_several_units():
    """the smallest binary batch whose column pass has more units than workgroups; exact sd2 again"""
    N, H, W = 9, 256, 256
    grid, units = L.boundary_grid(L.BoundaryDesc(L.BOUNDARY_BINARY, 1, N, 1, H, W, 0, -100, 0, 1.0))
    assert units > grid, (units, grid)
    assert L.boundary_grid(L.BoundaryDesc(L.BOUNDARY_BINARY, 1, N - 1, 1, H, W, 0, -100, 0, 1.0))[1] <= grid
    g = torch.Generator().manual_seed(4)
    t = (torch.rand(N, 1, H, W, generator=g) > 0.99).float()
    ii, jj = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    for n in range(N):                            # a disc per image, the last image (the walked units) included
        t[n, 0][(ii - 40 - 20 * n) ** 2 + (jj - 200 + 15 * n) ** 2 <= (10 + 3 * n) ** 2] = 1.0
    t[3] = 0.0
    sd2 = R.sd2_planes(R.planes_binary(t.numpy()))
    x = torch.randn(N, 1, H, W, generator=g)
    crit = BoundaryLoss(base=RegionLoss.dice(), weight=0.02)
    loss, _, (grad,) = crit.direct(x.to(DEV), t.to(DEV))
    check_sd2(crit, sd2)
    ref_loss, (ref_grad,), _, _ = R.reference("region", [x], t, [1.0], 0.02, base_kw=dict(alpha=0.5, beta=0.5, smooth=0.5))
    check_loss(loss.item(), ref_loss.item())
    check_grad(grad, ref_grad)


# ------------------------------------------------------------------------------------------------------ loss and gradients
CASES = [(s, b) for s in SHAPES for b in BASES]


@pytest.mark.parametrize("shape,base", CASES, ids=[f"{'x'.join(map(str, s))}-{b}" for s, b in CASES])
def test_loss_and_gradient_match_the_float64_definition(shape, base):
    weight, base_scale, spacing = (0.05, 1.0, 1.0) if base != "focal_tversky" else (0.3, 0.6, 0.7)
    x, t, ref_loss, ref_grad, ref_term, sd2 = reference(shape, base, weight, base_scale, spacing)
    make = BASES[base][1]
    crit = BoundaryLoss(base=make(), weight=weight, base_scale=base_scale, spacing=spacing)
    xd, td = x.to(DEV), t.to(DEV)
    loss, dice, (g,) = crit.direct(xd, td)
    torch.cuda.synchronize()
    assert loss.dim() == 0 and dice.dim() == 0 and loss.is_cuda and g.shape == xd.shape and g.dtype == torch.float32
    check_sd2(crit, sd2)
    check_loss(loss.item(), ref_loss)
    check_grad(g, ref_grad)
    assert abs(crit.term.item() - ref_term) < 2e-6 * max(1.0, abs(ref_term))
    # the Dice metric is the base's
    b = make()
    base_dice = unet_zoo_amd.loss.loss_and_dice(xd, td)[1] if isinstance(b, str) else b.loss_and_dice(xd, td)[1]
    assert abs(dice.item() - base_dice.item()) < 1e-6
    # a second call: the same bits
    loss2, dice2, (g2,) = crit.direct(xd, td)
    assert torch.equal(loss2, loss) and torch.equal(dice2, dice) and torch.equal(g2, g)
    # no gradient asked for: the same loss, and no gradient buffer is handed to the library
    seen = []
    real = L.boundary_loss

    def spy(desc, items, *a):
        seen.append([bool(it.dlogits) for it in items])
        return real(desc, items, *a)
    L.boundary_loss = spy
    try:
        with torch.no_grad():
            loss3, dice3 = crit.loss_and_dice(xd, td)
    finally:
        L.boundary_loss = real
    assert seen == [[False]] and torch.equal(loss3, loss) and torch.equal(dice3, dice) and not loss3.requires_grad
    # through autograd: the same numbers again, and the gradient arrives in the logits' dtype
    leaf = xd.clone().requires_grad_(True)
    loss4 = crit(leaf, td)
    loss4.backward()
    assert torch.equal(loss4.detach(), loss) and torch.equal(leaf.grad, g)


@pytest.mark.parametrize("base", list(BASES) + ["multiclass"])
def test_weight_zero_reproduces_the_base_exactly(base):
    if base == "multiclass":
        g = torch.Generator().manual_seed(3)
        x, t = 2.0 * torch.randn(2, 4, 33, 20, generator=g), make_labels(2, 4, 33, 20)
        make = lambda: MulticlassLoss.ce_dice()      # noqa: E731
    else:
        x, t = make_inputs((3, 1, 17, 23))
        make = BASES[base][1]
    xd, td = x.to(DEV), t.to(DEV)
    b = make()
    if isinstance(b, str):
        want_l, want_d, want_g = unet_zoo_amd.loss.loss_and_dice_direct(xd, td)
    else:
        want_l, want_d, want_g = b.direct(xd, td)
    want_g = want_g[0].clone()
    loss, dice, (grad,) = BoundaryLoss(base=make(), weight=0.0).direct(xd, td)
    assert torch.equal(loss, want_l) and torch.equal(dice, want_d) and torch.equal(grad, want_g)


def test_three_maps_share_one_transform_dict_and_list():
    g = torch.Generator().manual_seed(7)
    shape = (2, 1, 24, 20)
    maps = {f"d{i}": 2.0 * torch.randn(shape, generator=g) for i in range(3)}
    t = (torch.rand(shape, generator=g) > 0.6).float()
    ow = (1.0, 0.5, 0.25)
    kw = dict(alpha=0.6, beta=0.4, gamma=1.5)
    ref_loss, ref_grads, terms, sd2 = R.reference("region", list(maps.values()), t, ow, 0.1, 0.9, base_kw=kw)
    calls = []
    real = L.boundary_loss

    def spy(desc, items, *a):
        calls.append((desc.n_items, sum(1 for it in items if it.dlogits)))
        return real(desc, items, *a)
    L.boundary_loss = spy
    try:
        crit = BoundaryLoss(base=RegionLoss(output_weights=dict(zip(maps, ow)), **kw), weight=0.1, base_scale=0.9)
        leaves = {k: v.to(DEV).requires_grad_(True) for k, v in maps.items()}
        loss, dice = crit.loss_and_dice(leaves, t.to(DEV))
        assert calls == [(3, 3)]                                      # ONE uz_boundary_loss for the three maps
        loss.backward()
        assert calls == [(3, 3)]                                      # ... and none in backward
    finally:
        L.boundary_loss = real
    check_sd2(crit, sd2)
    check_loss(loss.item(), ref_loss.item())
    for leaf, gr in zip(leaves.values(), ref_grads):
        check_grad(leaf.grad, gr)
    assert abs(crit.term.item() - terms[0].item()) < 2e-6                # the main map of a dict is its first
    _, base_dice = RegionLoss(**kw).loss_and_dice(maps["d0"].to(DEV), t.to(DEV))
    assert abs(dice.item() - base_dice.item()) < 1e-6 and not dice.requires_grad
    # a list with weights by position: the main map is the last
    crit2 = BoundaryLoss(base=RegionLoss(output_weights=list(ow), **kw), weight=0.1, base_scale=0.9)
    loss2, _, gouts = crit2.direct([v.to(DEV) for v in maps.values()], t.to(DEV))
    check_loss(loss2.item(), ref_loss.item())
    for got, gr in zip(gouts, ref_grads):
        check_grad(got, gr)
    assert abs(crit2.term.item() - terms[2].item()) < 2e-6
    # "bce_dice" over a list: unit weights
    ref3, g3, _, _ = R.reference("bce_dice", list(maps.values()), t, (1.0, 1.0, 1.0), 0.1)
    loss3, _, gouts3 = BoundaryLoss(weight=0.1).direct([v.to(DEV) for v in maps.values()], t.to(DEV))
    check_loss(loss3.item(), ref3.item())
    for got, gr in zip(gouts3, g3):
        check_grad(got, gr)


def test_bf16_logits():
    x, t = make_inputs((3, 1, 17, 23))
    xb = x.to(DEV).bfloat16()
    ref_b, (ref_gb,), _, _ = R.reference("region", [xb.float().cpu()], t, [1.0], 0.05, base_kw=dict(alpha=0.5, beta=0.5, smooth=0.5))
    leaf = xb.clone().requires_grad_(True)
    loss = BoundaryLoss(base=RegionLoss.dice(), weight=0.05)(leaf, t.to(DEV))
    loss.backward()
    check_loss(loss.item(), ref_b.item())
    assert leaf.grad.dtype == torch.bfloat16
    assert (leaf.grad.float().cpu().double() - ref_gb).abs().max() <= 2.0 ** -8 * ref_gb.abs().max()    # one bf16 rounding


def test_set_weights_reaches_the_device_scalars():
    x, t = make_inputs((3, 1, 17, 23))
    xd, td = x.to(DEV), t.to(DEV)
    crit = BoundaryLoss(base=RegionLoss.dice(), weight=0.01)
    crit.direct(xd, td)
    crit.rebalance(0.3)
    loss, _, (grad,) = crit.direct(xd, td)
    fresh_loss, _, (fresh_grad,) = BoundaryLoss(base=RegionLoss.dice(), weight=0.3, base_scale=0.7).direct(xd, td)
    assert torch.equal(loss, fresh_loss) and torch.equal(grad, fresh_grad)
    x_, t_, ref_loss, ref_grad, _, _ = reference((3, 1, 17, 23), "region_dice", 0.3, 0.7)
    check_loss(loss.item(), ref_loss)
    check_grad(grad, ref_grad)


# ------------------------------------------------------------------------------------------------- inside the graphed runners
STEP_MODELS = [("unet", {}), ("u2net", {}), ("nested_unet", {"deep_supervision": True})]


def _make(name, kw, dtype, train=True):
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model(name, in_channels=3, num_classes=1, **kw)
    m.run_dtype = dtype
    m = m.cuda()
    return m.train() if train else m.eval()


def _batch(seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 3, 64, 64, generator=g).cuda(), (torch.rand(2, 1, 64, 64, generator=g) > 0.5).float().cuda()


def _criterion(name, weight=0.05):
    u2 = ("main", "side1", "side2", "side3", "side4", "side5", "side6")
    weights = {"u2net": dict(zip(u2, (1.0, 0.5, 0.5, 0.25, 0.25, 0.125, 0.125))),
               "nested_unet": [0.25, 0.5, 0.75, 1.0]}.get(name)
    return BoundaryLoss(base=RegionLoss(alpha=0.7, beta=0.3, gamma=4 / 3, output_weights=weights), weight=weight)


@pytest.mark.parametrize("name,kw", STEP_MODELS, ids=[c[0] for c in STEP_MODELS])
def test_graphed_step_equals_eager_step_bitwise_and_set_weights_does_not_recapture(name, kw):
    x, t = _batch()
    dt = torch.float32
    m1 = _make(name, kw, dt)
    crit1 = _criterion(name)
    gs = unet_zoo_amd.GraphedStep(m1, crit1, lr=1e-3, weight_decay=1e-5, max_norm=1.0)
    assert gs._fused_loss
    m2 = _make(name, kw, dt)
    crit2 = _criterion(name)
    opt = None
    g_losses, e_losses, g_norms, e_norms, g_dice, e_dice = [], [], [], [], [], []
    graphs = None
    for k in range(4):
        if k == 2:                               # a new epoch: heavier boundary term, the graphs stay what they are
            graphs = (gs._cur, tuple(gs._cur.phases), gs._g_opt)
            crit1.set_weights(weight=0.2, base_scale=0.9)
            crit2 = _criterion(name)             # a fresh object built with the new weights: the eager step's
            crit2.set_weights(weight=0.2, base_scale=0.9)
        loss = gs(x, t)
        torch.cuda.synchronize()
        g_losses.append(loss.item())
        g_dice.append(gs.dice.item())
        g_norms.append(gs.grad_norm.item())
        if opt is None:
            n1 = {id(p): n for n, p in m1.named_parameters()}
            p2 = dict(m2.named_parameters())
            opt = FlatClipAdamW([p2[n1[id(p)]] for p in gs.opt.params], lr=1e-3, weight_decay=1e-5, max_norm=1.0)
            m2._pack_cache.repoint()
            m2.grads_in_place = True
        l2, d2 = crit2.loss_and_dice(m2(x), t)
        l2.backward()
        opt.step()
        torch.cuda.synchronize()
        e_losses.append(l2.item())
        e_dice.append(d2.item())
        e_norms.append(opt.last_grad_norm().item())
    cur = gs._cur
    assert cur.fwd is None and len(cur.phases) == 1
    for gk in cur.phases:
        _check_capture(gk, "forward + loss + backward graph")
    assert "eager" not in gs.describe()
    assert graphs[0] is gs._cur and all(a is b for a, b in zip(graphs[1], gs._cur.phases)) and graphs[2] is gs._g_opt
    assert g_losses == e_losses, (g_losses, e_losses)
    assert g_dice == e_dice
    assert g_norms == e_norms, (g_norms, e_norms)
    assert torch.equal(gs.opt.flat_p, opt.flat_p)
    assert all(l == l and 0.0 < l < 40.0 for l in g_losses) and len(set(g_losses)) == 4
    # the transform of the step's target, computed inside the graph
    check_sd2(crit1, R.sd2_planes(R.planes_binary(t.cpu().numpy())))


def test_graphed_eval_equals_eager_eval_bitwise_and_follows_set_weights():
    m = _make("unet", {}, torch.float32, train=False)
    crit = BoundaryLoss(base=RegionLoss.tversky(0.7, 0.3, gamma=4 / 3), weight=0.05)
    batches = [_batch(seed=s) for s in (1, 2, 3)]

    def eager(weight):
        c, res = BoundaryLoss(base=RegionLoss.tversky(0.7, 0.3, gamma=4 / 3), weight=weight), []
        for x, t in batches:
            with torch.no_grad():
                loss, dice = c.loss_and_dice(m(x), t)
            res.append((loss.clone(), dice.clone()))
        return res
    want, want2 = eager(0.05), eager(0.5)
    ev = unet_zoo_amd.GraphedEval(m, crit)
    assert ev._fused_loss
    for (x, t), (loss, dice) in zip(batches, want):       # the first call captures, the others replay the same graph
        l, d = ev(x, t)
        torch.cuda.synchronize()
        assert torch.equal(l, loss) and torch.equal(d, dice) and l.dim() == 0
    graph = next(iter(ev._graphs.values()))
    _check_capture(graph.graph, "evaluation graph")
    crit.set_weights(weight=0.5)
    for (x, t), (loss, dice), (old, _) in zip(batches, want2, want):
        l, d = ev(x, t)
        torch.cuda.synchronize()
        assert torch.equal(l, loss) and torch.equal(d, dice) and not torch.equal(l, old)
        check_sd2(crit, R.sd2_planes(R.planes_binary(t.cpu().numpy())))
    assert len(ev._graphs) == 1 and next(iter(ev._graphs.values())) is graph and ev.captures == 1      # no recapture
    assert "eager" not in ev.describe()


def test_step_with_augment_transforms_the_augmented_mask():
    x, t = _batch()
    t = torch.zeros_like(t)
    t[:, :, 20:44, 12:40] = 1.0                   # a block that the warp rotates, scales and partly moves out of the picture
    torch.manual_seed(5)
    aug = GpuAugment(hflip=0.5, vflip=0.5, rotate=25.0, scale=(0.8, 1.2), translate=0.1, grid_distort=(4, 2.0))
    crit = BoundaryLoss(base=RegionLoss.dice(), weight=0.05)
    step = unet_zoo_amd.GraphedStep(_make("unet", {}, torch.float32), crit, lr=1e-3, augment=aug)
    seen = []
    for _ in range(2):                            # every replay draws afresh: two different masks, two transforms
        step(x, t)
        torch.cuda.synchronize()
        mask = step.augmented[1].cpu().numpy()
        assert not np.array_equal(mask, t.cpu().numpy())
        check_sd2(crit, R.sd2_planes(R.planes_binary(mask)))
        seen.append(mask)
    assert not np.array_equal(seen[0], seen[1])
