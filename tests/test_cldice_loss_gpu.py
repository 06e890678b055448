"""GPU: ClDiceLoss (uz_cldice_loss) -- probabilities, both soft skeletons, the loss and its gradients against the definition
restated with torch on the CPU in float64 (tests/cldice_ref.py), ties included, and inside GraphedStep / GraphedEval against
the eager step.

Bounds are those of tests/test_region_loss_gpu.py: |loss - ref| < 2e-6 max(1, |ref|), max |dlogits - ref| <= 2e-6 max |ref grad|,
the Dice metric within 1e-6 of the base's; probabilities and skeletons (values in [0, 1]) within 2e-6.  torch's own float32
evaluation of the term uses up at most 0.07 (value) and 0.21 (gradient) of these bounds on tie-free inputs
(tests/test_cldice_loss.py prints the shares).

The tie-free inputs keep distinct probabilities of a plane 1e-5 apart, so that fp32 rounding cannot reorder them and every
minimum, maximum and relu chooses what float64 chooses; the tied inputs have equal LOGITS, hence bit-equal probabilities on
both sides.  In the class mode the device's exp is not the CPU's and the background plane 1 - sum may tie anywhere, so with
include_background the checks are layered: the probabilities against the float64 softmax, then loss and gradient against
float64 evaluated from the device's OWN probabilities."""
import pytest
import torch

import cldice_ref as R  # tests/cldice_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from unet_zoo_amd import ClDiceLoss, MulticlassLoss, RegionLoss
from unet_zoo_amd import _lib as L
from unet_zoo_amd.capture import _check_capture
from unet_zoo_amd.optim import FlatClipAdamW

pytestmark = pytest.mark.gpu

DEV = "cuda"
TH, TW = L.CLDICE_TILE_H, L.CLDICE_TILE_W


def check_loss(got, ref):
    got, ref = float(got), float(ref)
    print(f"loss {got:.9g} ref {ref:.9g} |diff| {abs(got - ref):.3e} bound {2e-6 * max(1.0, abs(ref)):.3e} "
          f"share {abs(got - ref) / (2e-6 * max(1.0, abs(ref))):.3f}")
    assert abs(got - ref) < 2e-6 * max(1.0, abs(ref))


def check_grad(got, ref):
    err, top = (got.detach().cpu().double() - ref).abs().max().item(), ref.abs().max().item()
    print(f"grad max|diff| {err:.3e} bound {2e-6 * top:.3e} (max |ref grad| {top:.3e}) share {err / (2e-6 * top):.3f}")
    assert err <= 2e-6 * top


def check_planes(crit, probs, skeleton, target_skeleton, c0=0):
    """.probs, .skeleton, .target_skeleton (fp32, (N, C, H, W)) within 2e-6 of the float64 planes (of the classes c0 ..)"""
    for name, got, ref in (("probs", crit.probs, probs), ("skeleton", crit.skeleton, skeleton),
                           ("target_skeleton", crit.target_skeleton, target_skeleton)):
        got = got.cpu()
        assert got.dtype == torch.float32 and tuple(got[:, c0:].shape) == tuple(ref.shape), name
        err = (got[:, c0:].double() - ref).abs().max().item()
        print(f"{name} max|diff| {err:.3e}")
        assert err <= 2e-6, name


_REFS = {}


def reference(inputs, shape, k, per_image, weight=0.5, base_scale=1.0):
    """inputs and the float64 results of one binary case on RegionLoss.dice(), computed once"""
    key = (inputs.__name__, shape, k, per_image, weight, base_scale)
    if key not in _REFS:
        x, t = inputs(shape)
        loss, (grad,), (term,), (probs,), (skel,), tskel = R.reference("region", [x], t, [1.0], weight, base_scale, k, 1.0, per_image,
                                                                       base_kw=R.REGION_KW)
        _REFS[key] = (x, t, loss.item(), grad, term.item(), probs, skel, tskel)
    return _REFS[key]


# ------------------------------------------------------------------------------------------------------------------ binary mode
SHAPES = [(3, 1, 17, 23),                        # smaller than the halo at k = 10
          (1, 2, TH, TW),                        # exactly one tile
          (2, 1, 2 * TH + 5, 3 * TW + 7),        # bands across every tile border, ragged edges
          (1, 1, 1, 37), (1, 1, 37, 1)]          # clipped windows: v or h is the pixel itself


@pytest.mark.parametrize("per_image", [False, True], ids=["batch", "image"])
@pytest.mark.parametrize("k", [1, 3, 10])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_binary_mode_matches_the_definition(shape, k, per_image):
    x, t, ref_loss, ref_grad, ref_term, probs, skel, tskel = reference(R.make_inputs, shape, k, per_image)
    crit = ClDiceLoss(base=RegionLoss.dice(), weight=0.5, iterations=k, per_image=per_image)
    xd, td = x.to(DEV), t.to(DEV)
    loss, dice, (g,) = crit.direct(xd, td)
    torch.cuda.synchronize()
    assert loss.dim() == 0 and dice.dim() == 0 and loss.is_cuda and g.shape == xd.shape and g.dtype == torch.float32
    check_planes(crit, probs, skel, tskel)
    check_loss(loss.item(), ref_loss)
    check_grad(g, ref_grad)
    assert abs(crit.term.item() - ref_term) < 2e-6 * max(1.0, abs(ref_term))
    _, base_dice = RegionLoss.dice().loss_and_dice(xd, td)
    assert abs(dice.item() - base_dice.item()) < 1e-6
    # a second call: the same bits
    first = [v.clone() for v in (crit.probs, crit.skeleton, crit.target_skeleton, crit.term)]
    loss2, dice2, (g2,) = crit.direct(xd, td)
    assert torch.equal(loss2, loss) and torch.equal(dice2, dice) and torch.equal(g2, g)
    assert all(torch.equal(a, b) for a, b in zip(first, (crit.probs, crit.skeleton, crit.target_skeleton, crit.term)))
    # no gradient asked for: the same loss, and no gradient buffer is handed to the library
    seen = []
    real = L.cldice_loss

    def spy(desc, items, *a):
        seen.append([bool(it.dlogits) for it in items])
        return real(desc, items, *a)
    L.cldice_loss = spy
    try:
        with torch.no_grad():
            loss3, dice3 = crit.loss_and_dice(xd, td)
    finally:
        L.cldice_loss = real
    assert seen == [[False]] and torch.equal(loss3, loss) and torch.equal(dice3, dice) and not loss3.requires_grad
    # through autograd: the same numbers again
    leaf = xd.clone().requires_grad_(True)
    loss4 = crit(leaf, td)
    loss4.backward()
    assert torch.equal(loss4.detach(), loss) and torch.equal(leaf.grad, g)


@pytest.mark.parametrize("per_image", [False, True], ids=["batch", "image"])
@pytest.mark.parametrize("k", [3, 10])
def test_tied_logits_take_torchs_subgradients(k, per_image):
    """logits snapped to multiples of 1/8: equal probabilities in most windows; the same through bf16 (the values are exact)"""
    shape = (2, 1, 40, 40)
    x, t, ref_loss, ref_grad, _, probs, skel, tskel = reference(R.make_tied_inputs, shape, k, per_image)
    crit = ClDiceLoss(base=RegionLoss.dice(), weight=0.5, iterations=k, per_image=per_image)
    loss, _, (g,) = crit.direct(x.to(DEV), t.to(DEV))
    check_planes(crit, probs, skel, tskel)
    check_loss(loss.item(), ref_loss)
    check_grad(g, ref_grad)
    assert torch.equal(x.bfloat16().float(), x)
    with torch.no_grad():
        loss_b = crit(x.to(DEV).bfloat16(), t.to(DEV))
    check_loss(loss_b.item(), ref_loss)


def test_soft_targets_and_other_bases():
    """a target with values inside (0, 1) (multiples of 1/4: ties in skel(t)'s windows), on "bce_dice" and a focal Tversky base"""
    shape = (2, 2, 21, 19)
    x, t = R.make_inputs(shape)
    g = torch.Generator().manual_seed(2)
    t = t * torch.randint(1, 5, shape, generator=g).float() / 4.0
    assert len(t.unique()) == 5
    focal = dict(alpha=0.7, beta=0.3, gamma=4 / 3, smooth=1e-3, pos_weight=2.5)
    for kind, make, kw, w, bs in (("bce_dice", lambda: "bce_dice", {}, 0.5, 1.0), ("region", lambda: RegionLoss(**focal), focal, 0.3, 0.6)):
        ref_loss, (ref_grad,), _, (probs,), (skel,), tskel = R.reference(kind, [x], t, [1.0], w, bs, 2, 0.25, True, base_kw=kw)
        crit = ClDiceLoss(base=make(), weight=w, base_scale=bs, iterations=2, smooth=0.25, per_image=True)
        loss, _, (grad,) = crit.direct(x.to(DEV), t.to(DEV))
        check_planes(crit, probs, skel, tskel)
        check_loss(loss.item(), ref_loss.item())
        check_grad(grad, ref_grad)


def test_workgroups_walk_several_units():
    """the smallest batch of 64 x 64 maps whose tile passes have more (map, plane, tile) units than workgroups; every third
    logit is 0.5, so equal probabilities lie in the windows of every tile and across every tile border"""
    H = W = 64
    N = 1
    while True:
        grid, units = L.cldice_grid(L.ClDiceDesc(L.CLDICE_BINARY, 1, N, 1, H, W, 0, 0, -100, 3, 1.0, 0))
        if units > grid:
            break
        N += 1
    assert 1 < N <= 2048
    grid1, units1 = L.cldice_grid(L.ClDiceDesc(L.CLDICE_BINARY, 1, N - 1, 1, H, W, 0, 0, -100, 3, 1.0, 0))
    assert units1 <= grid1
    x, t = R.make_inputs((2, 1, H, W))
    reps = (N + 1) // 2
    x = torch.cat([x.roll(r, 3) for r in range(reps)])[:N].contiguous()
    t = torch.cat([t.roll(r, 3) for r in range(reps)])[:N].contiguous()
    x.view(-1)[::3] = 0.5
    ref_loss, (ref_grad,), _, (probs,), (skel,), tskel = R.reference("region", [x], t, [1.0], 0.5, base_kw=R.REGION_KW)
    crit = ClDiceLoss(base=RegionLoss.dice(), weight=0.5)
    loss, _, (grad,) = crit.direct(x.to(DEV), t.to(DEV))
    check_planes(crit, probs, skel, tskel)
    check_loss(loss.item(), ref_loss.item())
    check_grad(grad, ref_grad)


# ------------------------------------------------------------------------------------------------------------------ class mode
@pytest.mark.parametrize("per_image", [False, True], ids=["batch", "image"])
@pytest.mark.parametrize("K", [4, 8])
def test_class_mode_matches_the_reference(K, per_image):
    x, y = R.make_class_inputs(K)
    N, _, H, W = x.shape
    kw = R.CLASS_KW
    xd, yd = x.to(DEV), y.to(DEV)
    ign = ((y == -100) | (y < 0) | (y >= K)).unsqueeze(1).expand_as(x)
    assert ign.any()
    # 1. the background excluded: the fully independent reference (the foreground planes are tie-free by construction)
    crit = ClDiceLoss(base=MulticlassLoss(**kw), weight=0.5, base_scale=0.8, iterations=3, per_image=per_image)
    loss, dice, (grad,) = crit.direct(xd, yd)                          # labels (N, H, W), int64
    ref_loss, (ref_grad,), (term,), (probs,), (skel,), tskel = R.reference("multiclass", [x], y, [1.0], 0.5, 0.8, 3, 1.0, per_image,
                                                                           False, base_kw=kw)
    check_planes(crit, probs, skel, tskel, c0=1)
    assert not crit.skeleton[:, 0].any()                               # the excluded plane is never written
    check_loss(loss.item(), ref_loss.item())
    check_grad(grad, ref_grad)
    assert abs(crit.term.item() - term.item()) < 2e-6 * max(1.0, abs(term.item()))
    _, base_dice = MulticlassLoss(**kw).loss_and_dice(xd, yd)
    assert abs(dice.item() - base_dice.item()) < 1e-6
    assert not grad.cpu()[ign].any()                                   # exactly nothing on all K logits of an ignored pixel
    with torch.no_grad():                                              # int64 labels of shape (N, 1, H, W): the same loss
        loss2, _ = crit.loss_and_dice(xd, y.unsqueeze(1).to(DEV))
    assert torch.equal(loss2, loss)
    # 2. the background included, in layers
    crit = ClDiceLoss(base=MulticlassLoss(**kw), weight=1.0, base_scale=0.0, iterations=3, per_image=per_image, include_background=True)
    loss, _, (grad,) = crit.direct(xd, yd)
    valid = ~ign[:, :1]
    p64 = torch.softmax(x.double(), 1) * valid
    got_p = crit.probs.cpu()
    print(f"probs max|diff| {(got_p.double() - p64).abs().max().item():.3e}")
    assert (got_p.double() - p64).abs().max() <= 2e-6 and not got_p[ign].any()
    V, g_ref = R.class_term_from_probs(x, y, got_p, 3, 1.0, per_image, True)
    check_loss(loss.item(), V.item())                                  # base_scale = 0, weight = 1: the term alone
    check_grad(grad, g_ref)
    assert abs(crit.term.item() - V.item()) < 2e-6
    assert not grad.cpu()[ign].any()


# ------------------------------------------------------------------------------------------------------------------ protocol
@pytest.mark.parametrize("base", ["bce_dice", "region_dice", "focal_tversky", "multiclass"])
def test_weight_zero_reproduces_the_base_exactly(base):
    if base == "multiclass":
        x, t = R.make_class_inputs(4)
        make = lambda: MulticlassLoss.ce_dice()      # noqa: E731
    else:
        x, t = R.make_inputs((3, 1, 17, 23))
        make = {"bce_dice": lambda: "bce_dice", "region_dice": RegionLoss.dice,
                "focal_tversky": lambda: RegionLoss(alpha=0.7, beta=0.3, gamma=4 / 3, smooth=1e-3, pos_weight=2.5)}[base]
    xd, td = x.to(DEV), t.to(DEV)
    b = make()
    if isinstance(b, str):
        want_l, want_d, want_g = unet_zoo_amd.loss.loss_and_dice_direct(xd, td)
    else:
        want_l, want_d, want_g = b.direct(xd, td)
    want_g = want_g[0].clone()
    loss, dice, (grad,) = ClDiceLoss(base=make(), weight=0.0).direct(xd, td)
    assert torch.equal(loss, want_l) and torch.equal(dice, want_d) and torch.equal(grad, want_g)


def test_three_maps_cost_one_call_dict_and_list():
    shape = (2, 1, 24, 20)
    maps = {f"d{i}": R.make_inputs(shape, seed=i)[0] for i in range(3)}
    t = R.bands(shape)
    ow = (1.0, 0.5, 0.25)
    kw = dict(alpha=0.6, beta=0.4, gamma=1.5)
    ref_loss, ref_grads, terms, probs, skels, tskel = R.reference("region", list(maps.values()), t, ow, 0.7, 0.9, base_kw=kw)
    calls = []
    real = L.cldice_loss

    def spy(desc, items, *a):
        calls.append((desc.n_items, sum(1 for it in items if it.dlogits)))
        return real(desc, items, *a)
    L.cldice_loss = spy
    try:
        crit = ClDiceLoss(base=RegionLoss(output_weights=dict(zip(maps, ow)), **kw), weight=0.7, base_scale=0.9)
        leaves = {k: v.to(DEV).requires_grad_(True) for k, v in maps.items()}
        loss, dice = crit.loss_and_dice(leaves, t.to(DEV))
        assert calls == [(3, 3)]                                      # ONE uz_cldice_loss for the three maps: skel(t) once
        loss.backward()
        assert calls == [(3, 3)]                                      # ... and none in backward
    finally:
        L.cldice_loss = real
    check_planes(crit, probs[0], skels[0], tskel)                     # the main map of a dict is its first
    check_loss(loss.item(), ref_loss.item())
    for leaf, gr in zip(leaves.values(), ref_grads):
        check_grad(leaf.grad, gr)
    assert abs(crit.term.item() - terms[0].item()) < 2e-6 * max(1.0, abs(terms[0].item()))
    _, base_dice = RegionLoss(**kw).loss_and_dice(maps["d0"].to(DEV), t.to(DEV))
    assert abs(dice.item() - base_dice.item()) < 1e-6 and not dice.requires_grad
    # a list with weights by position: the main map is the last
    crit2 = ClDiceLoss(base=RegionLoss(output_weights=list(ow), **kw), weight=0.7, base_scale=0.9)
    loss2, _, gouts = crit2.direct([v.to(DEV) for v in maps.values()], t.to(DEV))
    check_planes(crit2, probs[2], skels[2], tskel)
    check_loss(loss2.item(), ref_loss.item())
    for got, gr in zip(gouts, ref_grads):
        check_grad(got, gr)
    assert abs(crit2.term.item() - terms[2].item()) < 2e-6 * max(1.0, abs(terms[2].item()))
    # "bce_dice" over a list: unit weights
    ref3, g3, _, _, _, _ = R.reference("bce_dice", list(maps.values()), t, (1.0, 1.0, 1.0), 0.7)
    loss3, _, gouts3 = ClDiceLoss(weight=0.7).direct([v.to(DEV) for v in maps.values()], t.to(DEV))
    check_loss(loss3.item(), ref3.item())
    for got, gr in zip(gouts3, g3):
        check_grad(got, gr)


def test_bf16_logits():
    x, t = R.make_inputs((3, 1, 17, 23))
    xb = x.to(DEV).bfloat16()                                         # bf16 rounding ties many logits: the reference sees the same
    ref_b, (ref_gb,), _, (probs,), (skel,), tskel = R.reference("region", [xb.float().cpu()], t, [1.0], 0.5, base_kw=R.REGION_KW)
    leaf = xb.clone().requires_grad_(True)
    crit = ClDiceLoss(base=RegionLoss.dice(), weight=0.5)
    loss = crit(leaf, t.to(DEV))
    loss.backward()
    check_planes(crit, probs, skel, tskel)
    check_loss(loss.item(), ref_b.item())
    assert leaf.grad.dtype == torch.bfloat16
    assert (leaf.grad.float().cpu().double() - ref_gb).abs().max() <= 2.0 ** -8 * ref_gb.abs().max()    # one bf16 rounding


def test_set_weights_equals_a_fresh_object():
    shape = (3, 1, 17, 23)
    x, t, ref_loss, ref_grad, ref_term, _, _, _ = reference(R.make_inputs, shape, 3, False, 0.3, 0.0)
    xd, td = x.to(DEV), t.to(DEV)
    crit = ClDiceLoss(base=RegionLoss.dice(), weight=0.5)
    crit.direct(xd, td)
    crit.set_weights(weight=0.3, base_scale=0.0)                      # the term alone: the base is still launched
    loss, dice, (grad,) = crit.direct(xd, td)
    fresh_loss, fresh_dice, (fresh_grad,) = ClDiceLoss(base=RegionLoss.dice(), weight=0.3, base_scale=0.0).direct(xd, td)
    assert torch.equal(loss, fresh_loss) and torch.equal(grad, fresh_grad) and torch.equal(dice, fresh_dice)
    check_loss(loss.item(), ref_loss)
    check_grad(grad, ref_grad)
    assert abs(loss.item() - 0.3 * ref_term) < 2e-6 * max(1.0, ref_term)
    _, base_dice = RegionLoss.dice().loss_and_dice(xd, td)
    assert abs(dice.item() - base_dice.item()) < 1e-6


# ------------------------------------------------------------------------------------------------- inside the graphed runners
STEP_MODELS = [("unet", {}), ("u2net", {}), ("nested_unet", {"deep_supervision": True})]


def _make(name, kw, dtype, train=True, num_classes=1):
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model(name, in_channels=3, num_classes=num_classes, **kw)
    m.run_dtype = dtype
    m = m.cuda()
    return m.train() if train else m.eval()


def _batch(seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 3, 64, 64, generator=g).cuda(), R.bands((2, 1, 64, 64)).roll(seed, 3).cuda()


def _criterion(name, weight=0.5):
    u2 = ("main", "side1", "side2", "side3", "side4", "side5", "side6")
    weights = {"u2net": dict(zip(u2, (1.0, 0.5, 0.5, 0.25, 0.25, 0.125, 0.125))),
               "nested_unet": [0.25, 0.5, 0.75, 1.0]}.get(name)
    return ClDiceLoss(base=RegionLoss(alpha=0.7, beta=0.3, gamma=4 / 3, output_weights=weights), weight=weight)


def _eager_twin(gs, m1, m2):
    n1 = {id(p): n for n, p in m1.named_parameters()}
    p2 = dict(m2.named_parameters())
    opt = FlatClipAdamW([p2[n1[id(p)]] for p in gs.opt.params], lr=1e-3, weight_decay=1e-5, max_norm=1.0)
    m2._pack_cache.repoint()
    m2.grads_in_place = True
    return opt


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
        if k == 2:                               # more clDice, less base; the graphs stay what they are
            graphs = (gs._cur, tuple(gs._cur.phases), gs._g_opt)
            crit1.set_weights(weight=1.0, base_scale=0.25)
            crit2 = _criterion(name)             # a fresh object built with the new weights: the eager step's
            crit2.set_weights(weight=1.0, base_scale=0.25)
        loss = gs(x, t)
        torch.cuda.synchronize()
        g_losses.append(loss.item())
        g_dice.append(gs.dice.item())
        g_norms.append(gs.grad_norm.item())
        if opt is None:
            opt = _eager_twin(gs, m1, m2)
        l2, d2 = crit2.loss_and_dice(m2(x), t)
        l2.backward()
        opt.step()
        torch.cuda.synchronize()
        e_losses.append(l2.item())
        e_dice.append(d2.item())
        e_norms.append(opt.last_grad_norm().item())
        assert torch.equal(crit1.skeleton, crit2.skeleton) and torch.equal(crit1.probs, crit2.probs)
        assert torch.equal(crit1.term, crit2.term)
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
    # the target's skeleton, formed inside the graph: the definition's
    assert (crit1.target_skeleton.cpu().double() - R.skel(t.cpu().double(), 3)).abs().max() <= 2e-6


def test_graphed_eval_equals_eager_eval_bitwise_and_follows_set_weights():
    m = _make("unet", {}, torch.float32, train=False)
    crit = ClDiceLoss(base=RegionLoss.tversky(0.7, 0.3, gamma=4 / 3), weight=0.5)
    batches = [_batch(seed=s) for s in (1, 2, 3)]

    def eager(weight):
        c, res = ClDiceLoss(base=RegionLoss.tversky(0.7, 0.3, gamma=4 / 3), weight=weight), []
        for x, t in batches:
            with torch.no_grad():
                loss, dice = c.loss_and_dice(m(x), t)
            res.append((loss.clone(), dice.clone(), c.skeleton.clone()))
        return res
    want, want2 = eager(0.5), eager(1.5)
    ev = unet_zoo_amd.GraphedEval(m, crit)
    assert ev._fused_loss
    for (x, t), (loss, dice, skel) in zip(batches, want):        # the first call captures, the others replay the same graph
        l, d = ev(x, t)
        torch.cuda.synchronize()
        assert torch.equal(l, loss) and torch.equal(d, dice) and l.dim() == 0 and torch.equal(crit.skeleton, skel)
    graph = next(iter(ev._graphs.values()))
    _check_capture(graph.graph, "evaluation graph")
    crit.set_weights(weight=1.5)
    for (x, t), (loss, dice, skel), (old, _, _) in zip(batches, want2, want):
        l, d = ev(x, t)
        torch.cuda.synchronize()
        assert torch.equal(l, loss) and torch.equal(d, dice) and not torch.equal(l, old) and torch.equal(crit.skeleton, skel)
    assert len(ev._graphs) == 1 and next(iter(ev._graphs.values())) is graph and ev.captures == 1      # no recapture
    assert "eager" not in ev.describe()


def test_multiclass_step_equals_eager_step_bitwise():
    x, _ = _batch()
    y = R.make_labels(2, 4, 64, 64).cuda()
    m1, m2 = _make("unet", {}, torch.float32, num_classes=4), _make("unet", {}, torch.float32, num_classes=4)
    crit1, crit2 = (ClDiceLoss(base=MulticlassLoss.ce_dice(), weight=0.5) for _ in range(2))
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
        assert torch.equal(crit1.skeleton, crit2.skeleton)
    assert "eager" not in gs.describe() and torch.equal(gs.opt.flat_p, opt.flat_p)
    assert tuple(crit1.skeleton.shape) == (2, 4, 64, 64)
