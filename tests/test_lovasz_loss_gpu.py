"""GPU: LovaszLoss (uz_lovasz_loss) -- the errors bit for bit and the ranks of the segmented stable sort integer for integer
against the definition restated with torch on the CPU in float64 (tests/lovasz_ref.py), the loss and its gradients against
it, and inside GraphedStep / GraphedEval against the eager step.

Bounds are those of tests/test_region_loss_gpu.py: |loss - ref| < 2e-6 max(1, |ref|), max |dlogits - ref| <= 2e-6 max |ref grad|,
the Dice metric within 1e-6 of the base's.  torch's own float32 evaluation of the term deviates from float64 by at most 0.054
(value) and 0.39 (gradient: class mode, K = 4, per image, present classes) of these bounds on the cases below, with ONE kind
of exception that tests/test_lovasz_loss.py reports: the class mode with per_image=True and classes="all" where an image lacks
a class -- plain float32 autograd lands at 2.2 (K = 4) and 3.0 (K = 8) times the gradient bound there, because
p_k (d_k - sum_c p_c d_c) cancels at the pixel that carries the whole weight of the absent class's segment (p = 0.993).  The
bound is kept; the kernel takes that difference without a cancellation (0.18 of the bound in float32 on the CPU).

In the class mode the device's exp is not the CPU's, so the checks are layered: errors within 2e-6 of the float64 softmax;
ranks equal to the stable argsort of the device's OWN errors, exactly; loss and gradient against float64 evaluated with the
device's permutation; the loss also against the fully independent reference (it is continuous across near-tie swaps)."""
import pytest
import torch

import lovasz_ref as R  # tests/lovasz_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from unet_zoo_amd import LovaszLoss, MulticlassLoss, RegionLoss
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
    print(f"grad max|diff| {err:.3e} bound {2e-6 * top:.3e} (max |ref grad| {top:.3e}) share {err / (2e-6 * top):.3f}")
    assert err <= 2e-6 * top


def check_sort(crit, errors, ranks):
    """errors bit for bit (the reference's value of e IS the fp32 one), ranks integer for integer"""
    got_e, got_r = crit.errors.cpu(), crit.ranks.cpu()
    assert got_e.dtype == torch.float32 and got_r.dtype == torch.int32 and got_e.shape == errors.shape == got_r.shape
    assert torch.equal(got_e, errors.float()), f"{int((got_e != errors.float()).sum())} of {errors.numel()} errors differ"
    assert torch.equal(got_r.long(), ranks), f"{int((got_r.long() != ranks).sum())} of {ranks.numel()} ranks differ"


BASES = {
    "bce_dice": ("bce_dice", lambda: "bce_dice", {}),
    "region_dice": ("region", lambda: RegionLoss.dice(), R.REGION_KW),
    "focal_tversky": ("region", lambda: RegionLoss(**R.FOCAL_KW), R.FOCAL_KW),
}

_REFS = {}


def reference(inputs, shape, base, weight, base_scale, per_image):
    """inputs and the float64 results of one binary case, computed once"""
    key = (inputs.__name__, shape, base, weight, base_scale, per_image)
    if key not in _REFS:
        x, t = inputs(shape)
        kind, _, kw = BASES[base]
        loss, (grad,), (term,), (errors,), (ranks,) = R.reference(kind, [x], t, [1.0], weight, base_scale, per_image, base_kw=kw)
        _REFS[key] = (x, t, loss.item(), grad, term.item(), errors, ranks)
    return _REFS[key]


# ------------------------------------------------------------------------------------------- binary mode: sort, loss, protocol
CASES = [(s, p, "region_dice") for s in R.SHAPES for p in (True, False)] + [((3, 1, 17, 23), True, "bce_dice"),
                                                                            ((3, 1, 17, 23), False, "focal_tversky")]


@pytest.mark.parametrize("shape,per_image,base", CASES,
                         ids=[f"{'x'.join(map(str, s))}-{'image' if p else 'batch'}-{b}" for s, p, b in CASES])
def test_binary_mode_matches_the_definition(shape, per_image, base):
    weight, base_scale = (0.5, 1.0) if base != "focal_tversky" else (0.3, 0.6)
    x, t, ref_loss, ref_grad, ref_term, errors, ranks = reference(R.make_inputs, shape, base, weight, base_scale, per_image)
    make = BASES[base][1]
    crit = LovaszLoss(base=make(), weight=weight, base_scale=base_scale, per_image=per_image)
    xd, td = x.to(DEV), t.to(DEV)
    loss, dice, (g,) = crit.direct(xd, td)
    torch.cuda.synchronize()
    assert loss.dim() == 0 and dice.dim() == 0 and loss.is_cuda and g.shape == xd.shape and g.dtype == torch.float32
    N, C, H, W = shape
    assert tuple(crit.errors.shape) == ((N * C, H * W) if per_image else (C, N * H * W))
    check_sort(crit, errors, ranks)
    if shape[0] > 2 and per_image:                 # image 1 is empty: the hinge of its largest error alone; image 2 is full
        assert (ranks[1] >= 0).any() and (ranks[2] == -1).all()
    check_loss(loss.item(), ref_loss)
    check_grad(g, ref_grad)
    assert abs(crit.term.item() - ref_term) < 2e-6 * max(1.0, abs(ref_term))
    # the Dice metric is the base's
    b = make()
    base_dice = unet_zoo_amd.loss.loss_and_dice(xd, td)[1] if isinstance(b, str) else b.loss_and_dice(xd, td)[1]
    assert abs(dice.item() - base_dice.item()) < 1e-6
    # a second call: the same bits, the ranks included
    first_ranks = crit.ranks.clone()
    loss2, dice2, (g2,) = crit.direct(xd, td)
    assert torch.equal(loss2, loss) and torch.equal(dice2, dice) and torch.equal(g2, g) and torch.equal(crit.ranks, first_ranks)
    # no gradient asked for: the same loss, and no gradient buffer is handed to the library
    seen = []
    real = L.lovasz_loss

    def spy(desc, items, *a):
        seen.append([bool(it.dlogits) for it in items])
        return real(desc, items, *a)
    L.lovasz_loss = spy
    try:
        with torch.no_grad():
            loss3, dice3 = crit.loss_and_dice(xd, td)
    finally:
        L.lovasz_loss = real
    assert seen == [[False]] and torch.equal(loss3, loss) and torch.equal(dice3, dice) and not loss3.requires_grad
    # through autograd: the same numbers again
    leaf = xd.clone().requires_grad_(True)
    loss4 = crit(leaf, td)
    loss4.backward()
    assert torch.equal(loss4.detach(), loss) and torch.equal(leaf.grad, g)


@pytest.mark.parametrize("per_image", [True, False], ids=["image", "batch"])
def test_ties_come_out_in_index_order(per_image):
    """logits snapped to multiples of 0.25: hundreds of equal errors; the same through bf16 (the snapped values are exact)"""
    shape = (2, 1, 40, 40)
    x, t, ref_loss, ref_grad, _, errors, ranks = reference(R.make_tied_inputs, shape, "region_dice", 0.5, 1.0, per_image)
    values, counts = errors[errors > 0].unique(return_counts=True)
    assert counts.max() >= 100 and len(values) < 200
    crit = LovaszLoss(base=RegionLoss.dice(), weight=0.5, per_image=per_image)
    loss, _, (g,) = crit.direct(x.to(DEV), t.to(DEV))
    check_sort(crit, errors, ranks)
    check_loss(loss.item(), ref_loss)
    check_grad(g, ref_grad)
    assert torch.equal(x.bfloat16().float(), x)
    with torch.no_grad():
        loss_b = crit(x.to(DEV).bfloat16(), t.to(DEV))
    check_sort(crit, errors, ranks)
    check_loss(loss_b.item(), ref_loss)


def test_keys_over_the_whole_exponent_range():
    """logits randn * 10 ** uniform(-3, 6): every one of the four digit passes has work"""
    shape = (2, 1, 48, 50)
    x, t, ref_loss, ref_grad, _, errors, ranks = reference(R.make_spread_inputs, shape, "region_dice", 0.5, 1.0, True)
    bits = errors[errors > 0].float().view(torch.int32)
    for shift in (0, 8, 16, 24):
        assert len(((bits >> shift) & 255).unique()) > 8
    crit = LovaszLoss(base=RegionLoss.dice(), weight=0.5)
    loss, _, (g,) = crit.direct(x.to(DEV), t.to(DEV))
    check_sort(crit, errors, ranks)
    check_loss(loss.item(), ref_loss)
    check_grad(g, ref_grad)


@pytest.mark.parametrize("per_image", [True, False], ids=["image", "one_batch_segment"])
def test_workgroups_walk_several_units(per_image):
    """the smallest batch of 64 x 64 maps whose passes have more (segment, tile) units than workgroups -- per image, and as ONE
    segment of 2052 sort tiles; every third logit is 0.5, so equal errors lie across every tile border, in element order and in
    sorted order"""
    N, H, W = 513, 64, 64
    grid, units = L.lovasz_grid(L.LovaszDesc(L.LOVASZ_BINARY, 1, N, 1, H, W, int(per_image), 0, -100, 0))
    assert units > grid, (units, grid)
    assert L.lovasz_grid(L.LovaszDesc(L.LOVASZ_BINARY, 1, N - 1, 1, H, W, int(per_image), 0, -100, 0))[1] <= grid
    g = torch.Generator().manual_seed(8)
    x = 2.0 * torch.randn(N, 1, H, W, generator=g)
    x.view(-1)[::3] = 0.5
    t = (torch.rand(N, 1, H, W, generator=g) > 0.7).float()
    t[3] = 0.0
    ref_loss, (ref_grad,), _, (errors,), (ranks,) = R.reference("region", [x], t, [1.0], 0.5, per_image=per_image, base_kw=R.REGION_KW)
    crit = LovaszLoss(base=RegionLoss.dice(), weight=0.5, per_image=per_image)
    loss, _, (grad,) = crit.direct(x.to(DEV), t.to(DEV))
    check_sort(crit, errors, ranks)
    check_loss(loss.item(), ref_loss.item())
    check_grad(grad, ref_grad)


# ------------------------------------------------------------------------------------------------------------------ class mode
@pytest.mark.parametrize("per_image", [True, False], ids=["image", "batch"])
@pytest.mark.parametrize("classes", ["present", "all"])
@pytest.mark.parametrize("K", [4, 8])
def test_class_mode_matches_the_reference(K, classes, per_image):
    x, y = R.make_class_inputs(K)
    N, _, H, W = x.shape
    assert not (y[-1] == 1).any() and (y[0] == 1).any()                # one image without class 1
    kw = R.CLASS_KW
    base = MulticlassLoss(**kw)
    crit = LovaszLoss(base=base, weight=0.5, base_scale=0.8, per_image=per_image, classes=classes)
    loss, dice, (grad,) = crit.direct(x.to(DEV), y.to(DEV))            # labels (N, H, W), int64
    errors, ranks = crit.errors.cpu(), crit.ranks.cpu().long()
    # 1. the errors against the float64 softmax (the range is [0, 1])
    ind_loss, _, (ind_term,), (ind_errors,), _ = R.reference("multiclass", [x], y, [1.0], 0.5, 0.8, per_image, classes, base_kw=kw)
    assert tuple(errors.shape) == ((N * K, H * W) if per_image else (K, N * H * W))
    print(f"errors max|diff| {(errors.double() - ind_errors).abs().max().item():.3e}")
    assert (errors.double() - ind_errors).abs().max() <= 2e-6
    # 2. the ranks: the stable argsort of the device's own errors, exactly
    assert torch.equal(ranks, R.ranks_of(errors)), f"{int((ranks != R.ranks_of(errors)).sum())} ranks differ"
    # 3. loss and gradient against float64 with the device's permutation
    ref_loss, (ref_grad,), (term,), _, _ = R.reference("multiclass", [x], y, [1.0], 0.5, 0.8, per_image, classes, base_kw=kw, ranks=[ranks])
    check_loss(loss.item(), ref_loss.item())
    check_grad(grad, ref_grad)
    assert abs(crit.term.item() - term.item()) < 2e-6 * max(1.0, abs(term.item()))
    # 4. the loss against the fully independent reference
    check_loss(loss.item(), ind_loss.item())
    _, base_dice = base.loss_and_dice(x.to(DEV), y.to(DEV))
    assert abs(dice.item() - base_dice.item()) < 1e-6
    # exactly nothing at an ignored pixel, on all K logits; rank -1 and no error there
    ign = ((y == -100) | (y < 0) | (y >= K))
    assert ign.any() and not grad.cpu()[ign.unsqueeze(1).expand_as(x)].any()
    ign_seg = ign.unsqueeze(1).expand_as(x)
    ign_seg = ign_seg.reshape(N * K, H * W) if per_image else ign_seg.permute(1, 0, 2, 3).reshape(K, N * H * W)
    assert (ranks[ign_seg] == -1).all() and not errors[ign_seg].any()
    # int64 labels of shape (N, 1, H, W) and no gradient: the same loss
    with torch.no_grad():
        loss2, _ = crit.loss_and_dice(x.to(DEV), y.unsqueeze(1).to(DEV))
    assert torch.equal(loss2, loss)


# ------------------------------------------------------------------------------------------------------------------ protocol
@pytest.mark.parametrize("base", list(BASES) + ["multiclass"])
def test_weight_zero_reproduces_the_base_exactly(base):
    if base == "multiclass":
        g = torch.Generator().manual_seed(3)
        x, t = 2.0 * torch.randn(2, 4, 33, 20, generator=g), R.make_labels(2, 4, 33, 20)
        make = lambda: MulticlassLoss.ce_dice()      # noqa: E731
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
    loss, dice, (grad,) = LovaszLoss(base=make(), weight=0.0).direct(xd, td)
    assert torch.equal(loss, want_l) and torch.equal(dice, want_d) and torch.equal(grad, want_g)


def test_three_maps_cost_one_call_dict_and_list():
    g = torch.Generator().manual_seed(7)
    shape = (2, 1, 24, 20)
    maps = {f"d{i}": 2.0 * torch.randn(shape, generator=g) for i in range(3)}
    t = (torch.rand(shape, generator=g) > 0.6).float()
    ow = (1.0, 0.5, 0.25)
    kw = dict(alpha=0.6, beta=0.4, gamma=1.5)
    ref_loss, ref_grads, terms, errors, ranks = R.reference("region", list(maps.values()), t, ow, 0.7, 0.9, base_kw=kw)
    calls = []
    real = L.lovasz_loss

    def spy(desc, items, *a):
        calls.append((desc.n_items, sum(1 for it in items if it.dlogits)))
        return real(desc, items, *a)
    L.lovasz_loss = spy
    try:
        crit = LovaszLoss(base=RegionLoss(output_weights=dict(zip(maps, ow)), **kw), weight=0.7, base_scale=0.9)
        leaves = {k: v.to(DEV).requires_grad_(True) for k, v in maps.items()}
        loss, dice = crit.loss_and_dice(leaves, t.to(DEV))
        assert calls == [(3, 3)]                                      # ONE uz_lovasz_loss for the three maps
        loss.backward()
        assert calls == [(3, 3)]                                      # ... and none in backward
    finally:
        L.lovasz_loss = real
    check_sort(crit, errors[0], ranks[0])                             # the main map of a dict is its first
    check_loss(loss.item(), ref_loss.item())
    for leaf, gr in zip(leaves.values(), ref_grads):                  # every map is sorted on its own
        check_grad(leaf.grad, gr)
    assert abs(crit.term.item() - terms[0].item()) < 2e-6 * max(1.0, abs(terms[0].item()))
    _, base_dice = RegionLoss(**kw).loss_and_dice(maps["d0"].to(DEV), t.to(DEV))
    assert abs(dice.item() - base_dice.item()) < 1e-6 and not dice.requires_grad
    # a list with weights by position: the main map is the last
    crit2 = LovaszLoss(base=RegionLoss(output_weights=list(ow), **kw), weight=0.7, base_scale=0.9)
    loss2, _, gouts = crit2.direct([v.to(DEV) for v in maps.values()], t.to(DEV))
    check_sort(crit2, errors[2], ranks[2])
    check_loss(loss2.item(), ref_loss.item())
    for got, gr in zip(gouts, ref_grads):
        check_grad(got, gr)
    assert abs(crit2.term.item() - terms[2].item()) < 2e-6 * max(1.0, abs(terms[2].item()))
    # "bce_dice" over a list: unit weights
    ref3, g3, _, _, _ = R.reference("bce_dice", list(maps.values()), t, (1.0, 1.0, 1.0), 0.7)
    loss3, _, gouts3 = LovaszLoss(weight=0.7).direct([v.to(DEV) for v in maps.values()], t.to(DEV))
    check_loss(loss3.item(), ref3.item())
    for got, gr in zip(gouts3, g3):
        check_grad(got, gr)


def test_bf16_logits():
    x, t = R.make_inputs((3, 1, 17, 23))
    xb = x.to(DEV).bfloat16()
    ref_b, (ref_gb,), _, (errors,), (ranks,) = R.reference("region", [xb.float().cpu()], t, [1.0], 0.5, base_kw=R.REGION_KW)
    leaf = xb.clone().requires_grad_(True)
    crit = LovaszLoss(base=RegionLoss.dice(), weight=0.5)
    loss = crit(leaf, t.to(DEV))
    loss.backward()
    check_sort(crit, errors, ranks)                                   # bf16 logits are widened first: e is the fp32 one
    check_loss(loss.item(), ref_b.item())
    assert leaf.grad.dtype == torch.bfloat16
    assert (leaf.grad.float().cpu().double() - ref_gb).abs().max() <= 2.0 ** -8 * ref_gb.abs().max()    # one bf16 rounding


def test_set_weights_equals_a_fresh_object():
    shape = (3, 1, 17, 23)
    x, t = R.make_inputs(shape)
    xd, td = x.to(DEV), t.to(DEV)
    crit = LovaszLoss(base=RegionLoss.dice(), weight=0.5)
    crit.direct(xd, td)
    crit.set_weights(weight=0.3, base_scale=0.0)                      # the IoU fine-tuning phase: the base is still launched
    loss, dice, (grad,) = crit.direct(xd, td)
    fresh_loss, fresh_dice, (fresh_grad,) = LovaszLoss(base=RegionLoss.dice(), weight=0.3, base_scale=0.0).direct(xd, td)
    assert torch.equal(loss, fresh_loss) and torch.equal(grad, fresh_grad) and torch.equal(dice, fresh_dice)
    _, _, ref_loss, ref_grad, ref_term, _, _ = reference(R.make_inputs, shape, "region_dice", 0.3, 0.0, True)
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
    return torch.randn(2, 3, 64, 64, generator=g).cuda(), (torch.rand(2, 1, 64, 64, generator=g) > 0.5).float().cuda()


def _criterion(name, weight=0.5):
    u2 = ("main", "side1", "side2", "side3", "side4", "side5", "side6")
    weights = {"u2net": dict(zip(u2, (1.0, 0.5, 0.5, 0.25, 0.25, 0.125, 0.125))),
               "nested_unet": [0.25, 0.5, 0.75, 1.0]}.get(name)
    return LovaszLoss(base=RegionLoss(alpha=0.7, beta=0.3, gamma=4 / 3, output_weights=weights), weight=weight)


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
        if k == 2:                               # the fine-tuning phase: less base, more Lovasz; the graphs stay what they are
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
        assert torch.equal(crit1.ranks, crit2.ranks) and torch.equal(crit1.errors, crit2.errors)
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
    # the ranks of the step's main map, sorted inside the graph: the stable argsort of its own errors
    assert torch.equal(crit1.ranks.cpu().long(), R.ranks_of(crit1.errors.cpu()))


def test_graphed_eval_equals_eager_eval_bitwise_and_follows_set_weights():
    m = _make("unet", {}, torch.float32, train=False)
    crit = LovaszLoss(base=RegionLoss.tversky(0.7, 0.3, gamma=4 / 3), weight=0.5)
    batches = [_batch(seed=s) for s in (1, 2, 3)]

    def eager(weight):
        c, res = LovaszLoss(base=RegionLoss.tversky(0.7, 0.3, gamma=4 / 3), weight=weight), []
        for x, t in batches:
            with torch.no_grad():
                loss, dice = c.loss_and_dice(m(x), t)
            res.append((loss.clone(), dice.clone(), c.ranks.clone()))
        return res
    want, want2 = eager(0.5), eager(1.5)
    ev = unet_zoo_amd.GraphedEval(m, crit)
    assert ev._fused_loss
    for (x, t), (loss, dice, ranks) in zip(batches, want):       # the first call captures, the others replay the same graph
        l, d = ev(x, t)
        torch.cuda.synchronize()
        assert torch.equal(l, loss) and torch.equal(d, dice) and l.dim() == 0 and torch.equal(crit.ranks, ranks)
    graph = next(iter(ev._graphs.values()))
    _check_capture(graph.graph, "evaluation graph")
    crit.set_weights(weight=1.5)
    for (x, t), (loss, dice, ranks), (old, _, _) in zip(batches, want2, want):
        l, d = ev(x, t)
        torch.cuda.synchronize()
        assert torch.equal(l, loss) and torch.equal(d, dice) and not torch.equal(l, old) and torch.equal(crit.ranks, ranks)
    assert len(ev._graphs) == 1 and next(iter(ev._graphs.values())) is graph and ev.captures == 1      # no recapture
    assert "eager" not in ev.describe()


def test_step_with_augment_sorts_against_the_augmented_mask():
    x, t = _batch()
    t = torch.zeros_like(t)
    t[:, :, 20:44, 12:40] = 1.0                   # a block that the warp rotates, scales and partly moves out of the picture
    torch.manual_seed(5)
    aug = GpuAugment(hflip=0.5, vflip=0.5, rotate=25.0, scale=(0.8, 1.2), translate=0.1, grid_distort=(4, 2.0))
    crit = LovaszLoss(base=RegionLoss.dice(), weight=0.5)
    step = unet_zoo_amd.GraphedStep(_make("unet", {}, torch.float32), crit, lr=1e-3, augment=aug)
    seen = []
    for _ in range(2):                            # every replay draws afresh: two different masks, two sorts
        step(x, t)
        torch.cuda.synchronize()
        mask = step.augmented[1].cpu()
        assert not torch.equal(mask, t.cpu())
        # the reference's sort for THAT mask, given the step's logits (a static tensor of the graph)
        logits = step.outputs.detach().float().cpu()
        assert logits.shape == mask.shape
        ref_e, ref_b = R.binary_segments(logits, mask, True)
        check_sort(crit, ref_e, R.ranks_of(ref_e))
        G = int((mask > 0.5).sum())
        assert 0 < G < mask.numel() and int((crit.ranks >= 0).sum()) > 0
        seen.append(mask)
    assert not torch.equal(seen[0], seen[1])


def test_multiclass_step_equals_eager_step_bitwise():
    x, _ = _batch()
    g = torch.Generator().manual_seed(9)
    y = torch.randint(0, 4, (2, 64, 64), generator=g)
    y[:, 10, :] = -100
    y = y.cuda()
    m1, m2 = _make("unet", {}, torch.float32, num_classes=4), _make("unet", {}, torch.float32, num_classes=4)
    crit1, crit2 = (LovaszLoss(base=MulticlassLoss.ce_dice(), weight=0.5) for _ in range(2))
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
        assert torch.equal(crit1.ranks, crit2.ranks)
    assert "eager" not in gs.describe() and torch.equal(gs.opt.flat_p, opt.flat_p)
    assert tuple(crit1.ranks.shape) == (2 * 4, 64 * 64)
