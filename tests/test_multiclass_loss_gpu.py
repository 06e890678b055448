"""GPU: MulticlassLoss (uz_class_loss) -- softmax cross-entropy + soft Dice over class-index labels, one or several output
maps -- against the formulas restated with torch on the CPU in float64 (tests/multiclass_ref.py), and inside GraphedStep /
GraphedEval against the eager step.

Bounds are those of tests/test_region_loss_gpu.py: |loss - ref| < 2e-6 max(1, |ref|), max |dlogits - ref| <= 2e-6 max |ref grad|.
The metric and the counts come from an argmax and from counting: they are compared exactly."""
import pytest
import torch

import multiclass_ref as R  # tests/multiclass_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from unet_zoo_amd import MulticlassLoss, RegionLoss
from unet_zoo_amd import _lib as L
from unet_zoo_amd.graph import PhasedStep
from unet_zoo_amd.optim import FlatClipAdamW
from unet_zoo_amd.capture import _check_capture

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


def check_metric(dice, counts, x, y, ignore_index=-100, include_background=True):
    ref_metric, ref_counts = R.metric_and_counts(x, y, ignore_index, include_background)
    assert counts.dtype == torch.int64 and torch.equal(counts.cpu(), ref_counts), (counts.cpu().tolist(), ref_counts.tolist())
    assert dice.item() == torch.tensor(ref_metric, dtype=torch.float64).float().item(), (dice.item(), ref_metric)


def make_inputs(shape, ignore_index, seed=0):
    """x = 3 randn; class K - 1 absent from every image; image 1 entirely ignored; row 1 of image 0 ignored; one pixel of
    image 0 carries the label K, which is out of range"""
    N, K, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(shape, generator=g)
    y = torch.randint(0, K - 1, (N, H, W), generator=g)
    if N > 1:
        y[1] = ignore_index
    y[0, 1, :] = ignore_index
    y[0, H - 1, W - 1] = K
    return x, y


SHAPES = [(1, 2, 4, 4), (3, 3, 17, 23), (5, 4, 64, 48), (2, 9, 33, 20), (2, 32, 16, 16)]


def setting(name, K):
    if name == "defaults":
        return dict()
    if name == "ce_dice":
        return R.ce_dice_settings()
    if name == "weighted":
        return dict(class_weight=[0.5 + 0.75 * (c % 3) for c in range(K)], label_smoothing=0.1, include_background=False,
                    reduce="batch", ignore_index=255)
    if name == "dice_only":
        return dict(w_ce=0.0)
    raise KeyError(name)


def criterion(name, K, **more):
    if name == "ce_dice":
        return MulticlassLoss.ce_dice(**more)
    return MulticlassLoss(**setting(name, K), **more)


CASES = [(s, k) for s in SHAPES for k in ("defaults", "ce_dice", "weighted", "dice_only")]
_REFS = {}


def reference(shape, name):
    """inputs and the float64 results of one case, computed once"""
    key = (shape, name)
    if key not in _REFS:
        kw = R.settings(**setting(name, shape[1]))
        x, y = make_inputs(shape, kw["ignore_index"])
        loss, (grad,) = R.reference([x], y, [1.0], **kw)
        _REFS[key] = (x, y, loss.item(), grad, kw)
    return _REFS[key]


# ------------------------------------------------------------------------------------------------- the kernel and the formulas
@pytest.mark.parametrize("shape,name", CASES, ids=[f"{'x'.join(map(str, s))}-{k}" for s, k in CASES])
def test_kernel_matches_the_float64_formula(shape, name):
    x, y, ref_loss, ref_grad, kw = reference(shape, name)
    crit = criterion(name, shape[1])
    xd, yd = x.to(DEV), y.to(DEV)
    loss, dice, (g,) = crit.direct(xd, yd)
    torch.cuda.synchronize()
    assert loss.dim() == 0 and dice.dim() == 0 and loss.is_cuda and g.shape == xd.shape and g.dtype == torch.float32
    check_loss(loss.item(), ref_loss)
    check_grad(g, ref_grad)
    assert crit.counts.shape == (shape[1] + 1, 3)
    check_metric(dice, crit.counts, x, y, kw["ignore_index"], kw["include_background"])
    valid = R.valid_mask(y, shape[1], kw["ignore_index"])
    assert (g.cpu()[~valid.unsqueeze(1).expand_as(x)] == 0).all()             # exactly 0 at pixels that are not valid
    counts = crit.counts.clone()
    # a second call: the same bits
    loss2, dice2, (g2,) = crit.direct(xd, yd)
    torch.cuda.synchronize()
    assert torch.equal(loss2, loss) and torch.equal(dice2, dice) and torch.equal(g2, g) and torch.equal(crit.counts, counts)
    # no gradient asked for (dlogits = NULL, no third launch): the same loss and metric; (N, 1, H, W) int32 labels
    with torch.no_grad():
        loss3, dice3 = crit.loss_and_dice(xd, yd.unsqueeze(1).int())
    torch.cuda.synchronize()
    assert torch.equal(loss3, loss) and torch.equal(dice3, dice) and not loss3.requires_grad
    assert torch.equal(crit.counts, counts)
    # through autograd: the same numbers again, and the gradient arrives in the logits' dtype
    leaf = xd.clone().requires_grad_(True)
    loss4 = crit(leaf, yd)
    loss4.backward()
    torch.cuda.synchronize()
    assert torch.equal(loss4.detach(), loss) and leaf.grad.dtype == xd.dtype and torch.equal(leaf.grad, g)


@pytest.mark.parametrize("shape,name", [((64, 2, 96, 96), "defaults"), ((64, 2, 96, 96), "weighted"), ((16, 32, 96, 96), "ce_dice")],
                         ids=["64x2x96x96-defaults", "64x2x96x96-weighted", "16x32x96x96-ce_dice"])
def test_lanes_that_walk_several_runs(shape, name):
    """the rows of a map are capped at 512: with 64 images of 2304 runs (16 of 9216 one-pixel runs at K = 32) a workgroup
    row covers its image in two trips, the geometry of the training shapes -- sums and the packed per-lane counters
    across trips"""
    x, y, ref_loss, ref_grad, kw = reference(shape, name)
    crit = criterion(name, shape[1])
    loss, dice, (g,) = crit.direct(x.to(DEV), y.to(DEV))
    torch.cuda.synchronize()
    check_loss(loss.item(), ref_loss)
    check_grad(g, ref_grad)
    check_metric(dice, crit.counts, x, y, kw["ignore_index"], kw["include_background"])
    _REFS.pop((shape, name))            # 20 MB of float64 that no other test uses


def test_unaligned_views_take_the_scalar_path_with_the_same_numbers():
    """HW a multiple of 4 behind a pointer that is not 16-byte aligned: scalar loads of the same runs -- the same bits as the
    16-byte path, and the float64 reference within the bounds"""
    shape = (5, 4, 64, 48)
    x, y, ref_loss, ref_grad, kw = reference(shape, "defaults")
    crit = criterion("defaults", 4)
    loss_a, dice_a, (g_a,) = crit.direct(x.to(DEV), y.to(DEV))
    counts_a = crit.counts.clone()
    wide = torch.zeros(x.shape[:-1] + (x.shape[-1] + 1,), device=DEV)
    wide[..., 1:] = x.to(DEV)
    buf = torch.zeros(x.numel() + 1, device=DEV)
    buf[1:] = wide[..., 1:].reshape(-1)                      # x[..., 1:] made contiguous at an odd offset
    xd = buf[1:].view(x.shape)
    assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
    loss, dice, (g,) = crit.direct(xd, y.to(DEV))
    torch.cuda.synchronize()
    check_loss(loss.item(), ref_loss)
    check_grad(g, ref_grad)
    check_metric(dice, crit.counts, x, y)
    assert torch.equal(loss, loss_a) and torch.equal(dice, dice_a) and torch.equal(g, g_a) and torch.equal(crit.counts, counts_a)


@pytest.mark.parametrize("mag", [80.0, 1e4])
def test_saturated_logits_give_finite_loss_and_gradient(mag):
    g = torch.Generator().manual_seed(5)
    shape = (2, 5, 16, 16)
    x = torch.where(torch.rand(shape, generator=g) > 0.5, mag, -mag)
    y = torch.randint(0, 5, (2, 16, 16), generator=g)
    for crit in (MulticlassLoss(), MulticlassLoss.ce_dice(), MulticlassLoss(label_smoothing=0.2, class_weight=[1, 2, 3, 4, 5])):
        loss, dice, (grad,) = crit.direct(x.to(DEV), y.to(DEV))
        assert torch.isfinite(loss).item() and torch.isfinite(grad).all().item() and torch.isfinite(dice).item()
        check_metric(dice, crit.counts, x, y)


def test_all_ignored_batch():
    """no valid pixel: CE = 0 (torch gives NaN), the Dice term of the empty sums 1 - smooth / smooth = 0, zero gradient, metric 1"""
    g = torch.Generator().manual_seed(6)
    x = 3.0 * torch.randn(2, 4, 12, 10, generator=g)
    y = torch.full((2, 12, 10), -100)
    for crit in (MulticlassLoss(w_dice=0.7), MulticlassLoss.ce_dice(), MulticlassLoss(w_dice=0.7, label_smoothing=0.1)):
        loss, dice, (grad,) = crit.direct(x.to(DEV), y.to(DEV))
        ref = crit.w_dice * R.dice_part(x, y, crit.smooth, -100, True, crit.reduce, crit.square).item()
        assert ref == 0.0 and loss.item() == ref
        assert (grad == 0).all().item() and dice.item() == 1.0
        assert crit.counts.tolist() == [[0, 0, 0]] * 4 + [[0, 240, 0]]


# ----------------------------------------------------------------------------------------------------------------- containers
def _spy(monkeypatch):
    calls = []
    real = L.class_loss

    def spy(desc, items, labels, cw, out2, counts, ws):
        calls.append((desc.n_items, sum(1 for it in items if it.dlogits), desc.metric_item))
        return real(desc, items, labels, cw, out2, counts, ws)
    monkeypatch.setattr(L, "class_loss", spy)
    return calls


def test_dict_of_three_maps_with_weights_by_key(monkeypatch):
    g = torch.Generator().manual_seed(7)
    shape = (2, 3, 24, 20)
    maps = {f"d{i}": 2.0 * torch.randn(shape, generator=g) for i in range(3)}
    y = torch.randint(0, 3, (2, 24, 20), generator=g)
    y[0, :3] = -100
    weights = {"d0": 1, "d1": .5, "d2": .25}
    kw = dict(label_smoothing=0.05, smooth=0.5)
    ref_loss, ref_grads = R.reference(list(maps.values()), y, [1.0, 0.5, 0.25], **kw)
    calls = _spy(monkeypatch)
    leaves = {k: v.to(DEV).requires_grad_(True) for k, v in maps.items()}
    crit = MulticlassLoss(output_weights=weights, **kw)
    loss, dice = crit.loss_and_dice(leaves, y.to(DEV))
    assert calls == [(3, 3, 0)]                                       # one uz_class_loss per forward: three launches in all
    loss.backward()
    assert calls == [(3, 3, 0)]                                       # ... and none in backward
    check_loss(loss.item(), ref_loss.item())
    for leaf, gr in zip(leaves.values(), ref_grads):
        check_grad(leaf.grad, gr)
    check_metric(dice, crit.counts, maps["d0"], y)                    # the main map: the first value of a dict
    assert not dice.requires_grad
    assert R.metric_and_counts(maps["d0"], y)[0] != R.metric_and_counts(maps["d2"], y)[0]
    # a map that needs no gradient gets none (NULL dlogits), the others are unchanged
    part = {k: v.detach().clone().requires_grad_(k != "d1") for k, v in leaves.items()}
    loss2 = MulticlassLoss(output_weights=weights, **kw)(part, y.to(DEV))
    loss2.backward()
    assert calls[-1] == (3, 2, 0) and part["d1"].grad is None
    assert torch.equal(loss2.detach(), loss.detach()) and torch.equal(part["d2"].grad, leaves["d2"].grad)


def test_list_of_two_maps_takes_the_metric_of_the_last(monkeypatch):
    g = torch.Generator().manual_seed(8)
    shape = (3, 4, 17, 23)
    maps = [2.0 * torch.randn(shape, generator=g) for _ in range(2)]
    y = torch.randint(0, 4, (3, 17, 23), generator=g)
    ref_loss, ref_grads = R.reference(maps, y, [1.0, 1.0])
    calls = _spy(monkeypatch)
    leaves = [v.to(DEV).requires_grad_(True) for v in maps]
    crit = MulticlassLoss()
    loss, dice = crit.loss_and_dice(leaves, y.to(DEV))
    loss.backward()
    assert calls == [(2, 2, 1)]
    check_loss(loss.item(), ref_loss.item())
    for leaf, gr in zip(leaves, ref_grads):
        check_grad(leaf.grad, gr)
    check_metric(dice, crit.counts, maps[-1], y)
    assert R.metric_and_counts(maps[0], y)[0] != R.metric_and_counts(maps[-1], y)[0]       # the two maps do differ
    # weights by position; direct() hands the gradients over in the order of the maps
    loss_w, dice_w, gouts = MulticlassLoss(output_weights=[0.25, 2.0]).direct([v.detach() for v in leaves], y.to(DEV))
    ref_w, ref_gw = R.reference(maps, y, [0.25, 2.0])
    check_loss(loss_w.item(), ref_w.item())
    assert len(gouts) == 2 and torch.equal(dice_w, dice) and calls[-1] == (2, 2, 1)
    for got, gr in zip(gouts, ref_gw):
        check_grad(got, gr)


def test_bf16_logits_class_weight_length_and_label_dtypes():
    shape = (3, 3, 17, 23)
    x, y, _, _, kw = reference(shape, "defaults")
    xb = x.to(DEV).bfloat16()
    ref_b, (ref_gb,) = R.reference([xb.float().cpu()], y, [1.0])
    leaf = xb.clone().requires_grad_(True)
    crit = MulticlassLoss()
    loss = crit(leaf, y.to(DEV))
    loss.backward()
    check_loss(loss.item(), ref_b.item())
    assert leaf.grad.dtype == torch.bfloat16
    assert (leaf.grad.float().cpu().double() - ref_gb).abs().max() <= 2.0 ** -8 * ref_gb.abs().max()    # one bf16 rounding
    # any integer dtype gives the same bits (this case's labels -- 0 .. 3 and the ignore_index -100 -- fit int8)
    base = crit.direct(x.to(DEV), y.to(DEV))
    for dt in (torch.int32, torch.int16, torch.int8):
        other = crit.direct(x.to(DEV), y.to(DEV).to(dt))
        assert torch.equal(other[0], base[0]) and torch.equal(other[2][0], base[2][0])
    with pytest.raises(ValueError, match="class_weight"):
        MulticlassLoss(class_weight=[1.0, 2.0])(x.to(DEV), y.to(DEV))
    with pytest.raises(L.HipLibraryError):
        MulticlassLoss()(x.to(DEV), y)


# ------------------------------------------------------------------------------------------------- inside the graphed step
# (create_model hands num_classes to U2NET as out_ch: models/__init__.py)
STEP_MODELS = [("unet", {"num_classes": 3}), ("u2net", {"num_classes": 3}), ("nested_unet", {"num_classes": 3, "deep_supervision": True})]


def _make(name, kw, dtype, train=True):
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model(name, in_channels=3, **kw)
    m.run_dtype = dtype
    m = m.cuda()
    return m.train() if train else m.eval()


def _batch(seed=1):
    """images on the device, int64 labels on the HOST: 0 .. 2, with a band of ignored pixels"""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, 3, (2, 64, 64), generator=g)
    y[0, 5:9] = -100
    return torch.randn(2, 3, 64, 64, generator=g).cuda(), y


def _criterion(name):
    u2 = ("main", "side1", "side2", "side3", "side4", "side5", "side6")
    weights = {"u2net": dict(zip(u2, (1.0, 0.5, 0.5, 0.25, 0.25, 0.125, 0.125))),
               "nested_unet": [0.25, 0.5, 0.75, 1.0]}.get(name)
    return MulticlassLoss.ce_dice(output_weights=weights, label_smoothing=0.05)


class _Direct:
    """the criterion as PhasedStep takes it: direct() hands over (loss, gradients); the metric is kept"""

    def __init__(self, crit):
        self.crit, self.dice = crit, None

    def __call__(self, out, t):
        return self.crit(out, t)

    def direct(self, out, t):
        loss, self.dice, gouts = self.crit.direct(out, t)
        return loss, gouts


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name,kw", STEP_MODELS, ids=[c[0] for c in STEP_MODELS])
def test_graphed_step_equals_eager_step_bitwise(name, kw, dt):
    x, y = _batch()
    assert y.dtype == torch.int64 and not y.is_cuda
    m1 = _make(name, kw, dt)
    gs = unet_zoo_amd.GraphedStep(m1, _criterion(name), lr=1e-3, weight_decay=1e-5, max_norm=1.0)
    g_losses, g_dice = [], []
    for _ in range(2):
        loss = gs(x, y)
        torch.cuda.synchronize()
        g_losses.append(loss.item())
        g_dice.append(gs.dice.item())
    cur = gs._cur
    assert cur.t.dtype == torch.int32 and cur.t.is_cuda          # the static labels
    assert cur.fwd is None and len(cur.phases) == 1              # fused: no separate forward graph ...
    for gk in cur.phases:
        _check_capture(gk, "forward + loss + backward graph")    # ... and no memset node
    assert "eager" not in gs.describe()
    # eager: the same forward, direct(), the same backward, the same flat optimizer in the same order
    m2 = _make(name, kw, dt)
    fn = _Direct(_criterion(name))
    n1 = {id(p): n for n, p in m1.named_parameters()}
    p2 = dict(m2.named_parameters())
    opt = FlatClipAdamW([p2[n1[id(p)]] for p in gs.opt.params], lr=1e-3, weight_decay=1e-5, max_norm=1.0)
    m2._pack_cache.repoint()
    ps = PhasedStep(m2, fn)
    yd = y.cuda()
    e_losses, e_dice = [], []
    for _ in range(2):
        loss = ps.forward(x, yd)
        ps.backward(ps.n_entries, 0, True)
        ps.finish()
        opt.step()
        torch.cuda.synchronize()
        e_losses.append(loss.item())
        e_dice.append(fn.dice.item())
    assert g_losses == e_losses, (g_losses, e_losses)
    assert g_dice == e_dice, (g_dice, e_dice)
    assert torch.equal(gs.opt.flat_p, opt.flat_p)                # every parameter
    n2 = {n: p for n, p in m2.named_parameters()}
    for n, p in m1.named_parameters():
        assert torch.equal(p, n2[n]), n
    assert all(l == l and 0.0 < l < 40.0 for l in g_losses) and len(set(g_losses)) == 2


def test_graphed_eval_equals_eager_eval_bitwise():
    m = _make("unet", {"num_classes": 3}, torch.float32, train=False)
    crit = MulticlassLoss.ce_dice()
    batches = [_batch(seed=s) for s in (1, 2, 3)]
    want = []
    for x, y in batches:
        with torch.no_grad():
            out = m(x)
            loss, dice = crit.loss_and_dice(out, y.cuda())
        torch.cuda.synchronize()
        want.append((loss.clone(), dice.clone(), out.clone()))
    ev = unet_zoo_amd.GraphedEval(m, crit)
    for (x, y), (loss, dice, _) in zip(batches, want):       # the first call captures, the others replay the same graph
        l, d = ev(x, y)
        torch.cuda.synchronize()
        assert torch.equal(l, loss) and torch.equal(d, dice) and l.dim() == 0
    assert len(ev._graphs) == 1
    eg = next(iter(ev._graphs.values()))
    assert eg.t.dtype == torch.int32
    _check_capture(eg.graph, "evaluation graph")
    ml, md = ev.evaluate([(x.cpu(), y) for x, y in batches])
    assert ml == sum(w[0].double() for w in want).item() / 3
    assert md == sum(w[1].double() for w in want).item() / 3
    assert "eager" not in ev.describe()
    # .counts after evaluate's last batch: the counts of that batch, computed with torch
    ref_metric, ref_counts = R.metric_and_counts(want[-1][2].cpu(), batches[-1][1])
    assert torch.equal(crit.counts.cpu(), ref_counts)
    assert ev.dice.item() == torch.tensor(ref_metric, dtype=torch.float64).float().item()


def test_static_target_dtypes_of_the_other_criteria_stay_float32():
    """strings, RegionLoss and callables keep float32 static targets in GraphedStep and GraphedEval; MulticlassLoss asks for
    int32"""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 3, 32, 32, generator=g).cuda()
    t = (torch.rand(1, 1, 32, 32, generator=g) > 0.5).float().cuda()
    y = torch.randint(0, 2, (1, 32, 32), generator=g)
    region = RegionLoss()
    for crit, target, want in (("bce_dice", t, torch.float32), (region, t, torch.float32),
                               (lambda out, tt: region(out, tt), t, torch.float32),
                               ("bce_dice", t.bool(), torch.float32), (MulticlassLoss(), y, torch.int32)):
        classes = 2 if want == torch.int32 else 1
        m = _make("unet", {"num_classes": classes}, torch.float32)
        step = unet_zoo_amd.GraphedStep(m, crit)
        step(x, target)
        torch.cuda.synchronize()
        assert step._cur.t.dtype == want, (crit, step._cur.t.dtype)
        ev = unet_zoo_amd.GraphedEval(m.eval(), crit)
        ev(x, target)
        torch.cuda.synchronize()
        assert next(iter(ev._graphs.values())).t.dtype == want, (crit, want)
    with pytest.raises(ValueError, match="unknown built-in criterion"):
        unet_zoo_amd.GraphedStep(_make("unet", {"num_classes": 2}, torch.float32), "ce_dice")
    assert unet_zoo_amd.GraphedStep(_make("unet", {"num_classes": 2}, torch.float32), MulticlassLoss())._fused_loss
    assert not unet_zoo_amd.GraphedStep(_make("unet", {"num_classes": 2}, torch.float32),
                                        lambda out, tt: MulticlassLoss()(out, tt))._fused_loss      # a plain callable stays eager
