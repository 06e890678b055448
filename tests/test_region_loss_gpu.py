"""GPU: RegionLoss (uz_region_loss) -- BCE + soft Dice / Tversky / focal Tversky over one or several output maps --
against the formula restated with torch on the CPU in float64, and inside GraphedStep / GraphedEval against the eager step.

Bounds are those of tests/test_loss_gpu.py: |loss - ref| < 2e-6 max(1, |ref|), max |dlogits - ref| <= 2e-6 max |ref grad|,
Dice within 1e-6.  torch's own float32 evaluation of the formula deviates from float64 by at most 1.6e-7 (loss) and 3.3e-7 of
the largest gradient on these shapes."""
import pytest
import torch
import torch.nn.functional as F

import unet_zoo_amd
from unet_zoo_amd import RegionLoss
from unet_zoo_amd import _lib as L
from unet_zoo_amd.loss import bce_dice_with_logits
from unet_zoo_amd.optim import FlatClipAdamW
from unet_zoo_amd.capture import _check_capture

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ---------------------------------------------------------------------------------------------------------------- the oracle
def oracle_map(x, t, w_bce=1.0, w_region=1.0, alpha=0.5, beta=0.5, smooth=1.0, gamma=1.0, reduce="image", pos_weight=None):
    """the formula of RegionLoss for one map, float64 on the CPU (x may require grad)"""
    x, t = x.double(), t.double()
    pw = 1.0 if pos_weight is None else pos_weight
    p = torch.sigmoid(x)
    bce = (-(pw * t * F.logsigmoid(x) + (1 - t) * F.logsigmoid(-x))).mean()
    groups = {"batch": 1, "image": x.shape[0], "channel": x.shape[0] * x.shape[1]}[reduce]
    pf, tf = p.reshape(groups, -1), t.reshape(groups, -1)
    I, S, T = (pf * tf).sum(1), pf.sum(1), tf.sum(1)
    ti = (I + smooth) / (I + alpha * (S - I) + beta * (T - I) + smooth)
    q = 1 - ti
    region = (q if gamma == 1 else q ** gamma).mean()          # gamma == 1: no 0 ** 0
    return w_bce * bce + w_region * region


def oracle(maps, t, weights, **kw):
    """(loss, [d loss / d map]) of the weighted sum over the maps"""
    leaves = [m.detach().double().requires_grad_(True) for m in maps]
    loss = sum(w * oracle_map(v, t, **kw) for w, v in zip(weights, leaves))
    grads = torch.autograd.grad(loss, leaves)
    return loss.detach(), list(grads)


def dice_reference(prediction, target, epsilon=1e-7):
    """utils/metrics.py:7-24 of the reference, as tests/test_loss_gpu.py restates it"""
    p = (prediction > 0).double().flatten()
    t = target.double().flatten()
    union = p.sum() + t.sum()
    if union == 0:
        return 1.0
    return ((2.0 * (p * t).sum() + epsilon) / (union + epsilon)).item()


def check_loss(got, ref):
    got, ref = float(got), float(ref)
    print(f"loss {got:.9g} ref {ref:.9g} |diff| {abs(got - ref):.3e} bound {2e-6 * max(1.0, abs(ref)):.3e}")
    assert abs(got - ref) < 2e-6 * max(1.0, abs(ref))


def check_grad(got, ref):
    err, top = (got.detach().cpu().double() - ref).abs().max().item(), ref.abs().max().item()
    print(f"grad max|diff| {err:.3e} bound {2e-6 * top:.3e} (max |ref grad| {top:.3e})")
    assert err <= 2e-6 * top


def make_inputs(shape, seed=0):
    """x = 3 randn, t = rand > 0.7; image 1: empty target; image 2 (N > 2): all foreground, labelled and confidently predicted"""
    g = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(shape, generator=g)
    t = (torch.rand(shape, generator=g) > 0.7).float()
    if shape[0] > 1:
        t[1] = 0.0
    if shape[0] > 2:
        t[2] = 1.0
        x[2] = x[2].abs() + 2.0
    return x, t


SHAPES = [(1, 1, 4, 4), (3, 1, 17, 23), (5, 1, 64, 48), (2, 3, 33, 20)]
SETTINGS = {
    "defaults": dict(),
    "focal_tversky": dict(reduce="image", alpha=0.7, beta=0.3, gamma=4 / 3, smooth=1e-3, pos_weight=2.5),
    "region_only_gamma2": dict(w_bce=0.0, gamma=2.0, reduce="image"),
}
CASES = [(s, k) for s in SHAPES for k in SETTINGS] + [((2, 3, 33, 20), "channel"), ((2, 3, 33, 20), "batch")]
SETTINGS["channel"] = dict(reduce="channel")
SETTINGS["batch"] = dict(reduce="batch")

_REFS = {}


def reference(shape, name):
    """inputs and the oracle's results of one case, computed once"""
    key = (shape, name)
    if key not in _REFS:
        x, t = make_inputs(shape)
        loss, (grad,) = oracle([x], t, [1.0], **SETTINGS[name])
        _REFS[key] = (x, t, loss.item(), grad, dice_reference(x, t))
    return _REFS[key]


# ------------------------------------------------------------------------------------------------- the kernel and the oracle
@pytest.mark.parametrize("shape,name", CASES, ids=[f"{'x'.join(map(str, s))}-{k}" for s, k in CASES])
def test_kernel_matches_the_float64_formula(shape, name):
    x, t, ref_loss, ref_grad, ref_dice = reference(shape, name)
    crit = RegionLoss(**SETTINGS[name])
    xd, td = x.to(DEV), t.to(DEV)
    loss, dice, (g,) = crit.direct(xd, td)
    torch.cuda.synchronize()
    assert loss.dim() == 0 and dice.dim() == 0 and loss.is_cuda and g.shape == xd.shape and g.dtype == torch.float32
    check_loss(loss.item(), ref_loss)
    check_grad(g, ref_grad)
    assert abs(dice.item() - ref_dice) < 1e-6
    # a second call: the same bits
    loss2, dice2, (g2,) = crit.direct(xd, td)
    torch.cuda.synchronize()
    assert torch.equal(loss2, loss) and torch.equal(dice2, dice) and torch.equal(g2, g)
    # no gradient asked for (dlogits = NULL, no third launch): the same loss and Dice
    with torch.no_grad():
        loss3, dice3 = crit.loss_and_dice(xd, td)
    torch.cuda.synchronize()
    assert torch.equal(loss3, loss) and torch.equal(dice3, dice) and not loss3.requires_grad
    # through autograd: the same numbers again, and the gradient arrives in the logits' dtype
    leaf = xd.clone().requires_grad_(True)
    loss4 = crit(leaf, td)
    loss4.backward()
    torch.cuda.synchronize()
    assert torch.equal(loss4.detach(), loss) and torch.equal(leaf.grad, g)


def test_unaligned_views_take_the_scalar_path_with_the_same_numbers():
    """a group length that is a multiple of 4 behind a pointer that is not 16-byte aligned"""
    x, t, ref_loss, ref_grad, _ = reference((5, 1, 64, 48), "defaults")
    n = x.numel()
    buf = torch.zeros(n + 1, device=DEV)
    buf[1:] = x.flatten().to(DEV)
    xd = buf[1:].view(x.shape)
    assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
    loss, _, (g,) = RegionLoss().direct(xd, t.to(DEV))
    check_loss(loss.item(), ref_loss)
    check_grad(g, ref_grad)


def test_saturated_logits_give_finite_loss_and_gradient():
    g = torch.Generator().manual_seed(5)
    shape = (2, 1, 16, 16)
    x = torch.where(torch.rand(shape, generator=g) > 0.5, 40.0, -40.0)
    t = (torch.rand(shape, generator=g) > 0.5).float()
    for kw in (dict(), dict(gamma=2.0, alpha=0.3, beta=0.7, pos_weight=3.0)):
        loss, dice, (grad,) = RegionLoss(**kw).direct(x.to(DEV), t.to(DEV))
        assert torch.isfinite(loss).item() and torch.isfinite(grad).all().item()
        ref_loss, (ref_grad,) = oracle([x], t, [1.0], **kw)
        check_loss(loss.item(), ref_loss.item())
        check_grad(grad, ref_grad)
        assert abs(dice.item() - dice_reference(x, t)) < 1e-6


@pytest.mark.parametrize("gamma", [1.0, 2.0])
def test_perfect_prediction_has_the_oracles_region_gradient(gamma):
    """TI = 1 in every image: gamma == 1 keeps the factor 1 (no 0 ** 0, no NaN), gamma > 1 makes the gradient vanish"""
    g = torch.Generator().manual_seed(6)
    shape = (2, 1, 16, 16)
    x = torch.where(torch.rand(shape, generator=g) > 0.5, 40.0, -40.0)
    t = (x > 0).float()
    kw = dict(w_bce=0.0, gamma=gamma)
    loss, _, (grad,) = RegionLoss(**kw).direct(x.to(DEV), t.to(DEV))
    ref_loss, (ref_grad,) = oracle([x], t, [1.0], **kw)
    assert torch.isfinite(loss).item() and torch.isfinite(grad).all().item()
    check_loss(loss.item(), ref_loss.item())
    if gamma == 1.0:
        assert ref_grad.abs().max().item() > 0.0
        check_grad(grad, ref_grad)
    else:
        # (1 - TI) is zero up to the rounding of the sums, and the gradient carries it as a factor
        assert ref_grad.abs().max().item() < 1e-30 and grad.abs().max().item() < 1e-30


def test_without_the_region_term_it_is_the_fused_bce():
    g = torch.Generator().manual_seed(3)
    shape = (3, 1, 37, 53)
    x = (torch.randn(shape, generator=g) * 4).to(DEV)
    t = (torch.rand(shape, generator=g) > 0.6).float().to(DEV)
    a = x.clone().requires_grad_(True)
    b = x.clone().requires_grad_(True)
    la, da = RegionLoss(w_region=0.0).loss_and_dice(a, t)
    lb, db = bce_dice_with_logits(b, t)
    la.backward()
    lb.backward()
    check_loss(la.item(), lb.item())
    check_grad(a.grad, b.grad.cpu().double())
    assert torch.equal(da, db)


# ----------------------------------------------------------------------------------------------------------------- containers
def _spy(monkeypatch):
    calls = []
    real = L.region_loss

    def spy(desc, items, out2, ws):
        calls.append((desc.n_items, sum(1 for it in items if it.dlogits)))
        return real(desc, items, out2, ws)
    monkeypatch.setattr(L, "region_loss", spy)
    return calls


def test_dict_of_three_maps_with_weights_by_key(monkeypatch):
    g = torch.Generator().manual_seed(7)
    shape = (2, 1, 24, 20)
    maps = {f"d{i}": 2.0 * torch.randn(shape, generator=g) for i in range(3)}
    t = (torch.rand(shape, generator=g) > 0.6).float()
    weights = {"d0": 1, "d1": .5, "d2": .25}
    kw = dict(alpha=0.6, beta=0.4, gamma=1.5)
    ref_loss, ref_grads = oracle(list(maps.values()), t, [1.0, 0.5, 0.25], **kw)
    own = [oracle([v], t, [1.0], **kw)[1][0] for v in maps.values()]
    for w, gr, o in zip((1.0, 0.5, 0.25), ref_grads, own):
        assert torch.allclose(gr, w * o, rtol=1e-12, atol=0)          # the oracle itself: a map's gradient is weight x its own
    calls = _spy(monkeypatch)
    leaves = {k: v.to(DEV).requires_grad_(True) for k, v in maps.items()}
    loss, dice = RegionLoss(output_weights=weights, **kw).loss_and_dice(leaves, t.to(DEV))
    assert calls == [(3, 3)]                                          # one uz_region_loss per forward: three launches in all
    loss.backward()
    assert calls == [(3, 3)]                                          # ... and none in backward
    check_loss(loss.item(), ref_loss.item())
    for leaf, gr in zip(leaves.values(), ref_grads):
        check_grad(leaf.grad, gr)
    assert abs(dice.item() - dice_reference(maps["d0"], t)) < 1e-6 and not dice.requires_grad
    # a map that needs no gradient gets none (NULL dlogits), the others are unchanged
    part = {k: v.detach().clone().requires_grad_(k != "d1") for k, v in leaves.items()}
    loss2 = RegionLoss(output_weights=weights, **kw)(part, t.to(DEV))
    loss2.backward()
    assert calls[-1] == (3, 2) and part["d1"].grad is None
    assert torch.equal(loss2.detach(), loss.detach()) and torch.equal(part["d2"].grad, leaves["d2"].grad)


def test_list_of_two_maps_takes_the_dice_of_the_last(monkeypatch):
    g = torch.Generator().manual_seed(8)
    shape = (3, 1, 17, 23)
    maps = [2.0 * torch.randn(shape, generator=g) for _ in range(2)]
    t = (torch.rand(shape, generator=g) > 0.6).float()
    ref_loss, ref_grads = oracle(maps, t, [1.0, 1.0])
    calls = _spy(monkeypatch)
    leaves = [v.to(DEV).requires_grad_(True) for v in maps]
    loss, dice = RegionLoss().loss_and_dice(leaves, t.to(DEV))
    loss.backward()
    assert calls == [(2, 2)]
    check_loss(loss.item(), ref_loss.item())
    for leaf, gr in zip(leaves, ref_grads):
        check_grad(leaf.grad, gr)
    assert abs(dice.item() - dice_reference(maps[-1], t)) < 1e-6
    assert abs(dice_reference(maps[0], t) - dice_reference(maps[-1], t)) > 1e-3      # the two maps do differ
    # weights by position; direct() hands the gradients over in the order of the maps
    loss_w, dice_w, gouts = RegionLoss(output_weights=[0.25, 2.0]).direct([v.detach() for v in leaves], t.to(DEV))
    ref_w, ref_gw = oracle(maps, t, [0.25, 2.0])
    check_loss(loss_w.item(), ref_w.item())
    assert len(gouts) == 2 and torch.equal(dice_w, dice)
    for got, gr in zip(gouts, ref_gw):
        check_grad(got, gr)


def test_bf16_logits_and_refusals_at_call():
    x, t, ref_loss, ref_grad, _ = reference((3, 1, 17, 23), "defaults")
    xb = x.to(DEV).bfloat16()
    ref_b, (ref_gb,) = oracle([xb.float().cpu()], t, [1.0])
    leaf = xb.clone().requires_grad_(True)
    loss = RegionLoss()(leaf, t.to(DEV))
    loss.backward()
    check_loss(loss.item(), ref_b.item())
    assert leaf.grad.dtype == torch.bfloat16
    assert (leaf.grad.float().cpu().double() - ref_gb).abs().max() <= 2.0 ** -8 * ref_gb.abs().max()    # one bf16 rounding
    with pytest.raises(ValueError, match="shape"):
        RegionLoss()(x.to(DEV), t.to(DEV)[:2])
    with pytest.raises(ValueError, match="shape"):
        RegionLoss()([x.to(DEV), x.to(DEV)[:, :, :8]], t.to(DEV))
    with pytest.raises(L.HipLibraryError):
        RegionLoss()(x.to(DEV), t)
    with pytest.raises(ValueError, match="output_weights"):
        RegionLoss(output_weights=[1.0, 2.0])(x.to(DEV), t.to(DEV))


# ------------------------------------------------------------------------------------------------- inside the graphed step
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


def _criterion(name):
    u2 = ("main", "side1", "side2", "side3", "side4", "side5", "side6")
    weights = {"u2net": dict(zip(u2, (1.0, 0.5, 0.5, 0.25, 0.25, 0.125, 0.125))),
               "nested_unet": [0.25, 0.5, 0.75, 1.0]}.get(name)
    return RegionLoss(alpha=0.7, beta=0.3, gamma=4 / 3, output_weights=weights)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name,kw", STEP_MODELS, ids=[c[0] for c in STEP_MODELS])
def test_graphed_step_equals_eager_step_bitwise(name, kw, dt):
    x, t = _batch()
    m1 = _make(name, kw, dt)
    gs = unet_zoo_amd.GraphedStep(m1, _criterion(name), lr=1e-3, weight_decay=1e-5, max_norm=1.0)
    g_losses, g_norms, g_dice = [], [], []
    for _ in range(3):
        loss = gs(x, t)
        torch.cuda.synchronize()
        g_losses.append(loss.item())
        g_dice.append(gs.dice.item())
        g_norms.append(gs.grad_norm.item())
    # fused: no separate forward graph, and no captured graph holds a memset node
    cur = gs._cur
    assert cur.fwd is None and len(cur.phases) == 1
    for gk in cur.phases:
        _check_capture(gk, "forward + loss + backward graph")
    _check_capture(gs._g_opt, "optimizer graph")
    assert "eager" not in gs.describe()
    # eager: the same kernels through the autograd nodes, the same flat optimizer in the same order
    m2 = _make(name, kw, dt)
    crit = _criterion(name)
    n1 = {id(p): n for n, p in m1.named_parameters()}
    p2 = dict(m2.named_parameters())
    opt = FlatClipAdamW([p2[n1[id(p)]] for p in gs.opt.params], lr=1e-3, weight_decay=1e-5, max_norm=1.0)
    m2._pack_cache.repoint()
    m2.grads_in_place = True
    e_losses, e_norms, e_dice = [], [], []
    for _ in range(3):
        loss, dice = crit.loss_and_dice(m2(x), t)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        e_losses.append(loss.item())
        e_dice.append(dice.item())
        e_norms.append(opt.last_grad_norm().item())
    assert g_losses == e_losses, (g_losses, e_losses)
    assert g_dice == e_dice
    assert g_norms == e_norms, (g_norms, e_norms)
    assert torch.equal(gs.opt.flat_p, opt.flat_p)
    assert all(l == l and 0.0 < l < 40.0 for l in g_losses) and len(set(g_losses)) == 3


def test_strings_and_callables_keep_their_routes():
    m = _make("unet", {}, torch.float32)
    with pytest.raises(ValueError, match="unknown built-in criterion"):
        unet_zoo_amd.GraphedStep(m, "region")
    with pytest.raises(ValueError, match="unknown built-in criterion"):
        unet_zoo_amd.GraphedEval(m.eval(), "region")
    crit = RegionLoss()
    assert unet_zoo_amd.GraphedStep(m.train(), crit)._fused_loss
    assert not unet_zoo_amd.GraphedStep(m, lambda out, tt: crit(out, tt))._fused_loss      # a plain callable stays eager
    assert unet_zoo_amd.GraphedEval(m.eval(), crit)._fused_loss


def test_graphed_eval_equals_eager_eval_bitwise():
    m = _make("unet", {}, torch.float32, train=False)
    crit = RegionLoss.tversky(0.7, 0.3, gamma=4 / 3)
    batches = [_batch(seed=s) for s in (1, 2, 3)]
    want = []
    for x, t in batches:
        with torch.no_grad():
            loss, dice = crit.loss_and_dice(m(x), t)
        torch.cuda.synchronize()
        want.append((loss.clone(), dice.clone()))
    ev = unet_zoo_amd.GraphedEval(m, crit)
    for (x, t), (loss, dice) in zip(batches, want):       # the first call captures, the others replay the same graph
        l, d = ev(x, t)
        torch.cuda.synchronize()
        assert torch.equal(l, loss) and torch.equal(d, dice) and l.dim() == 0
    assert len(ev._graphs) == 1
    _check_capture(next(iter(ev._graphs.values())).graph, "evaluation graph")
    ml, md = ev.evaluate([(x.cpu(), t.cpu()) for x, t in batches])
    assert ml == sum(w[0].double() for w in want).item() / 3
    assert md == sum(w[1].double() for w in want).item() / 3
    assert "eager" not in ev.describe()


# ------------------------------------------------------------------------------------------------------- a stock torch model
def test_plain_torch_model_gets_its_gradient_through_the_loss():
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, 20, 24, generator=g)
    t = (torch.rand(2, 1, 20, 24, generator=g) > 0.6).float()
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(3, 1, 1)

    def cpu_grads(dtype):
        c = torch.nn.Conv2d(3, 1, 1).to(dtype)
        c.load_state_dict({k: v.to(dtype) for k, v in conv.state_dict().items()})
        out = c(x.to(dtype))
        if dtype == torch.float64:
            loss = oracle_map(out, t)
        else:      # the same formula in float32
            p = torch.sigmoid(out)
            bce = F.binary_cross_entropy_with_logits(out, t)
            pf, tf = p.reshape(2, -1), t.reshape(2, -1)
            I, S, T = (pf * tf).sum(1), pf.sum(1), tf.sum(1)
            loss = bce + (1 - (I + 1.0) / (I + 0.5 * (S - I) + 0.5 * (T - I) + 1.0)).mean()
        loss.backward()
        return c.weight.grad.double(), c.bias.grad.double()

    ref_w, _ = cpu_grads(torch.float64)
    f32_w, _ = cpu_grads(torch.float32)
    top = ref_w.abs().max().item()
    own = (f32_w - ref_w).abs().max().item() / top          # what float32 torch itself loses on this little graph
    bound = min(max(4.0 * own, 1e-6), 1e-5)
    dev = torch.nn.Conv2d(3, 1, 1)
    dev.load_state_dict(conv.state_dict())
    dev = dev.cuda()
    RegionLoss()(dev(x.cuda()), t.cuda()).backward()
    err = (dev.weight.grad.cpu().double() - ref_w).abs().max().item() / top
    print(f"weight grad rel err {err:.3e}, float32 torch's own {own:.3e}, bound {bound:.3e}")
    assert err <= bound
