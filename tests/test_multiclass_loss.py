"""MulticlassLoss without a GPU: the constructor's refusals, the published recipe, output weights, the refusals at call time,
the refusals of uz_class_loss / uz_class_loss_workspace_bytes, which come before any launch (the library loads without a
device), and the float64 restatement of the formulas (tests/multiclass_ref.py) pinned against F.cross_entropy, RegionLoss's
documented soft Dice and a hand-computed case."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import multiclass_ref as R  # tests/multiclass_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from unet_zoo_amd import MulticlassLoss, _lib
from unet_zoo_amd.loss import MulticlassLoss as MulticlassLossFromModule


def test_exported_from_the_package():
    assert MulticlassLoss is MulticlassLossFromModule and "MulticlassLoss" in unet_zoo_amd.__all__
    assert MulticlassLoss.target_dtype == torch.int32 and MulticlassLoss().target_dtype == torch.int32


@pytest.mark.parametrize("kw,word", [
    (dict(smooth=0.0), "smooth"), (dict(smooth=-1.0), "smooth"), (dict(smooth=float("nan")), "smooth"),
    (dict(label_smoothing=-0.1), "label_smoothing"), (dict(label_smoothing=1.0), "label_smoothing"),
    (dict(label_smoothing=float("inf")), "label_smoothing"), (dict(w_ce=-1.0), "w_ce"), (dict(w_dice=-0.5), "w_dice"),
    (dict(w_ce=0.0, w_dice=0.0), "both zero"), (dict(reduce="channel"), "reduce"), (dict(reduce=None), "reduce"),
    (dict(ignore_index=1.5), "ignore_index"), (dict(ignore_index=2 ** 31), "ignore_index"), (dict(ignore_index=None), "ignore_index"),
    (dict(class_weight=[1.0, -0.5]), "class_weight"), (dict(class_weight=[1.0]), "class_weight"),
    (dict(class_weight=[1.0] * 33), "class_weight"), (dict(class_weight=[1.0, "x"]), "class_weight"),
    (dict(output_weights=[1.0, -0.5]), "output_weights"), (dict(output_weights={"d0": -1.0}), "output_weights"),
    (dict(w_ce="much"), "w_ce")])
def test_constructor_refuses_and_names_the_argument(kw, word):
    with pytest.raises(ValueError, match=word):
        MulticlassLoss(**kw)


def test_constructor_accepts_the_edges():
    MulticlassLoss(w_ce=0.0)
    MulticlassLoss(w_dice=0.0)
    MulticlassLoss(smooth=1e-6, label_smoothing=0.0)
    assert MulticlassLoss(label_smoothing=0.999).label_smoothing == 0.999
    assert MulticlassLoss(ignore_index=255).ignore_index == 255 and MulticlassLoss(ignore_index=-(2 ** 31)).ignore_index == -2 ** 31
    assert MulticlassLoss(class_weight=[0.0, 2.0]).class_weight == (0.0, 2.0)
    assert MulticlassLoss(class_weight=torch.ones(32)).class_weight == (1.0,) * 32
    for r in ("batch", "image"):
        assert MulticlassLoss(reduce=r).reduce == r
    d = MulticlassLoss()
    assert (d.w_ce, d.w_dice, d.smooth, d.label_smoothing, d.class_weight, d.ignore_index, d.include_background, d.reduce,
            d.square, d.output_weights, d.counts) == (1.0, 1.0, 1.0, 0.0, None, -100, True, "image", False, None, None)


def test_ce_dice_is_the_published_recipe():
    c = MulticlassLoss.ce_dice()
    assert (c.w_ce, c.w_dice, c.square, c.smooth, c.reduce) == (0.4, 0.6, True, 1e-5, "batch")
    assert (c.label_smoothing, c.class_weight, c.ignore_index, c.include_background) == (0.0, None, -100, True)
    c = MulticlassLoss.ce_dice(0.5, 0.5)
    assert (c.w_ce, c.w_dice, c.square, c.smooth, c.reduce) == (0.5, 0.5, True, 1e-5, "batch")
    want = R.ce_dice_settings()
    c = MulticlassLoss.ce_dice()
    assert {k: getattr(c, k) for k in want} == want


def test_output_weights_by_key_and_by_position():
    z = torch.zeros(1)
    dict_out = {"d0": z, "d1": z, "d2": z}
    assert MulticlassLoss().weights_for(dict_out) == (1.0, 1.0, 1.0)
    assert MulticlassLoss().weights_for(z) == (1.0,)
    by_key = MulticlassLoss(output_weights={"d2": 0.25, "d0": 1, "d1": 0.5, "unused": 9.0})
    assert by_key.weights_for(dict_out) == (1.0, 0.5, 0.25)          # the order of the outputs, not of the weights
    by_pos = MulticlassLoss(output_weights=[1, 0.5, 0.25])
    assert by_pos.weights_for(dict_out) == (1.0, 0.5, 0.25) and by_pos.weights_for([z, z, z]) == (1.0, 0.5, 0.25)
    with pytest.raises(ValueError, match="no entry"):
        MulticlassLoss(output_weights={"d0": 1.0}).weights_for(dict_out)
    with pytest.raises(ValueError, match="dict"):
        by_key.weights_for([z, z, z])
    with pytest.raises(ValueError, match="3 output_weights for 2"):
        by_pos.weights_for([z, z])


def test_refusals_at_call_time():
    x, y = torch.zeros(2, 3, 8, 8), torch.zeros(2, 8, 8, dtype=torch.int64)
    with pytest.raises(_lib.HipLibraryError):                    # CPU tensors: there is no CPU path
        MulticlassLoss()(x, y)
    with pytest.raises(_lib.HipLibraryError):
        MulticlassLoss().direct([x], y.view(2, 1, 8, 8).int())
    with pytest.raises(ValueError, match="integer"):             # float targets are masks, not class indices
        MulticlassLoss()(x, y.float())
    with pytest.raises(ValueError, match="integer"):
        MulticlassLoss()(x, y.bool())
    for bad in (y[:1], y[:, :4], y.view(2, 8, 8, 1), torch.zeros(2, 3, 8, 8, dtype=torch.int64)):
        with pytest.raises(ValueError, match="shape"):
            MulticlassLoss()(x, bad)
    with pytest.raises(ValueError, match="shape"):
        MulticlassLoss()([x, x[:, :, :4]], y)
    with pytest.raises(ValueError, match="K = 1"):
        MulticlassLoss()(x[:, :1], y)
    with pytest.raises(ValueError, match="K = 33"):
        MulticlassLoss()(torch.zeros(1, 33, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        MulticlassLoss()(x.double(), y)
    with pytest.raises(ValueError, match="output_weights"):
        MulticlassLoss(output_weights=[1.0, 2.0])(x, y)
    with pytest.raises(ValueError, match="at most 16"):
        MulticlassLoss()([x] * 17, y)


# ------------------------------------------------------------------------------------------------------------- the C entries
def _desc(n_items=1, N=2, K=3, HW=1024, w_ce=1.0, w_dice=1.0, smooth=1.0, label_smoothing=0.0, ignore_index=-100, reduce=1,
          include_background=1, square=0, metric_item=0):
    return _lib.ClassDesc(n_items, N, K, HW, w_ce, w_dice, smooth, label_smoothing, ignore_index, reduce, include_background,
                          square, metric_item)


BAD_DESCS = [(dict(K=1), b"K ="), (dict(K=0), b"K ="), (dict(K=33), b"K ="), (dict(K=-3), b"K ="),
             (dict(n_items=0), b"n_items"), (dict(n_items=_lib.CLASS_MAX_ITEMS + 1), b"n_items"), (dict(n_items=-1), b"n_items"),
             (dict(N=0), b"N ="), (dict(N=-2), b"N ="), (dict(HW=0), b"HW ="), (dict(HW=-16), b"HW ="),
             (dict(smooth=0.0), b"smooth"), (dict(smooth=-1.0), b"smooth"), (dict(smooth=float("nan")), b"smooth"),
             (dict(smooth=float("inf")), b"smooth"), (dict(label_smoothing=-0.01), b"label_smoothing"),
             (dict(label_smoothing=1.0), b"label_smoothing"), (dict(label_smoothing=float("nan")), b"label_smoothing"),
             (dict(w_ce=-1.0), b"w_ce"), (dict(w_dice=-1.0), b"w_dice"), (dict(w_ce=float("nan")), b"w_ce"),
             (dict(w_ce=0.0, w_dice=0.0), b"both zero"), (dict(reduce=2), b"reduce"), (dict(reduce=-1), b"reduce"),
             (dict(metric_item=1), b"metric_item"), (dict(metric_item=-1), b"metric_item"),
             (dict(n_items=3, metric_item=3), b"metric_item")]


def _fake_items(n, weight=1.0, logits=0x1000):
    items = (_lib.ClassItem * n)()
    for it in items:
        it.logits, it.dlogits, it.weight = logits, None, weight
    return items


def _call(lib, d, items, labels=0x2000, cw=None, out=0x3000, counts=None, ws=0x4000):
    return lib.uz_class_loss(ctypes.byref(d) if d is not None else None, items, labels, cw, out, counts, ws, None)


@pytest.mark.parametrize("kw,word", BAD_DESCS)
def test_both_entries_refuse_a_bad_descriptor_before_any_launch(kw, word):
    lib = _lib.load()
    d = _desc(**kw)
    assert lib.uz_class_loss_workspace_bytes(ctypes.byref(d)) == -1
    assert word in lib.uz_last_error_string()
    # the pointers are never followed: the refusal comes first
    n = max(1, min(d.n_items, _lib.CLASS_MAX_ITEMS))
    assert _call(lib, d, _fake_items(n)) == -1
    assert word in lib.uz_last_error_string()
    with pytest.raises(_lib.HipLibraryError):
        _lib.class_loss_workspace_bytes(d)


def test_null_arguments_and_bad_items_are_refused_before_any_launch():
    lib = _lib.load()
    assert lib.uz_class_loss_workspace_bytes(None) == -1 and b"null descriptor" in lib.uz_last_error_string()
    assert _call(lib, None, _fake_items(1)) == -1 and b"null descriptor" in lib.uz_last_error_string()
    d = _desc()
    assert _call(lib, d, None) == -1 and b"null" in lib.uz_last_error_string()
    assert _call(lib, d, _fake_items(1), labels=None) == -1 and b"null" in lib.uz_last_error_string()
    assert _call(lib, d, _fake_items(1), out=None) == -1 and b"null" in lib.uz_last_error_string()
    assert _call(lib, d, _fake_items(1), ws=None) == -1 and b"null" in lib.uz_last_error_string()
    assert _call(lib, d, _fake_items(1), ws=0x4008) == -1 and b"16-byte" in lib.uz_last_error_string()
    assert _call(lib, d, _fake_items(1, logits=None)) == -1 and b"item 0" in lib.uz_last_error_string()
    d2 = _desc(n_items=2)
    items = _fake_items(2)
    items[1].weight = -0.5
    assert _call(lib, d2, items) == -1
    assert b"item 1" in lib.uz_last_error_string() and b"weight" in lib.uz_last_error_string()


@pytest.mark.parametrize("N,HW", [(1, 16), (3, 391), (16, 256 * 256), (8, 512 * 512), (2, 1 << 26), (64, 7)])
def test_workspace_is_positive_and_grows_with_maps_and_classes(N, HW):
    by_items = [_lib.class_loss_workspace_bytes(_desc(n_items=k, N=N, HW=HW)) for k in range(1, _lib.CLASS_MAX_ITEMS + 1)]
    assert by_items[0] > 0 and all(b > a for a, b in zip(by_items, by_items[1:]))
    by_k = [_lib.class_loss_workspace_bytes(_desc(K=k, N=N, HW=HW)) for k in range(2, _lib.CLASS_MAX_K + 1)]
    assert by_k[0] > 0 and all(b > a for a, b in zip(by_k, by_k[1:]))
    assert all(b % 16 == 0 for b in by_items + by_k)


# --------------------------------------------------------------------------------------- the restatement in tests/multiclass_ref.py
def _case(seed=0, N=3, K=5, H=7, W=9):
    g = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(N, K, H, W, generator=g, dtype=torch.float64)
    y = torch.randint(0, K, (N, H, W), generator=g)
    y[0, 1] = -100
    y[1, :, 2] = 255
    return x, y


@pytest.mark.parametrize("weight", [None, [0.5, 2.0, 1.0, 0.0, 3.0]])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("ignore", [-100, 255, 2])
def test_ce_part_and_its_gradient_are_torchs_cross_entropy(weight, eps, ignore):
    x, y = _case()
    y = torch.where(y == 255, torch.full_like(y, ignore), y) if ignore != 255 else y
    y = torch.where(y == -100, torch.full_like(y, ignore), y)
    a = x.clone().requires_grad_(True)
    b = x.clone().requires_grad_(True)
    got = R.ce_part(a, y, weight, ignore, eps)
    w = None if weight is None else torch.tensor(weight, dtype=torch.float64)
    want = F.cross_entropy(b, y, weight=w, ignore_index=ignore, label_smoothing=eps)
    got.backward()
    want.backward()
    assert abs(got.item() - want.item()) < 1e-13 * max(1.0, abs(want.item()))
    assert (a.grad - b.grad).abs().max().item() < 1e-15
    # the closed form the kernel uses: (p_k sum_c a_c - a_k) / W at valid pixels, 0 elsewhere
    K = x.shape[1]
    wv = torch.ones(K, dtype=torch.float64) if w is None else w
    v = R.valid_mask(y, K, ignore)
    onehot = F.one_hot(torch.where(v, y, torch.zeros_like(y)), K).permute(0, 3, 1, 2).double()
    acoef = ((1 - eps) * onehot + eps / K) * wv.view(1, K, 1, 1)
    W = (wv[torch.where(v, y, torch.zeros_like(y))] * v).sum()
    closed = (torch.softmax(x, 1) * acoef.sum(1, keepdim=True) - acoef) / W * v.unsqueeze(1)
    assert (closed - b.grad).abs().max().item() < 1e-15


def test_ce_part_without_a_valid_pixel_is_zero_with_zero_gradient():
    x, y = _case()
    a = x.clone().requires_grad_(True)
    got = R.ce_part(a, torch.full_like(y, -100), None, -100, 0.1)
    got.backward()
    assert got.item() == 0.0 and a.grad.abs().max().item() == 0.0
    assert torch.isnan(F.cross_entropy(x, torch.full_like(y, -100))).item()      # what torch gives instead


@pytest.mark.parametrize("reduce", ["image", "batch"])
def test_two_class_dice_without_background_is_the_soft_dice_of_region_loss(reduce):
    """K = 2, include_background=False, square=False: the Dice part is RegionLoss's documented 1 - (2 I + s) / (S + T + s)
    on p_1 = sigmoid(x_1 - x_0) with the target [y == 1]"""
    g = torch.Generator().manual_seed(4)
    x = 2.0 * torch.randn(3, 2, 6, 5, generator=g, dtype=torch.float64)
    y = torch.randint(0, 2, (3, 6, 5), generator=g)
    s = 0.75
    got = R.dice_part(x, y, smooth=s, include_background=False, reduce=reduce, square=False)
    p = torch.sigmoid(x[:, 1] - x[:, 0])
    t = (y == 1).double()
    groups = 1 if reduce == "batch" else 3
    pf, tf = p.reshape(groups, -1), t.reshape(groups, -1)
    I, S, T = (pf * tf).sum(1), pf.sum(1), tf.sum(1)
    alpha = beta = 0.5                                               # RegionLoss.dice(smooth=s): half the smoothing
    ti = (I + s / 2) / (I + alpha * (S - I) + beta * (T - I) + s / 2)
    want = (1 - ti).mean()
    assert abs(got.item() - want.item()) < 1e-14
    assert abs(want.item() - (1 - (2 * I + s) / (S + T + s)).mean().item()) < 1e-14


def test_metric_and_counts_of_a_hand_computed_case():
    """one 2 x 2 image, K = 3.  logits per pixel -> prediction; labels 0, 1, ignore, 7 (out of range):
         pixel 0: (2, 1, 0) -> 0, label 0: TP of class 0
         pixel 1: (0, 1, 1) -> 1 (tie: the lowest index), label 2: P of class 1, T of class 2
         pixel 2: ignored, pixel 3: out of range -- neither is counted as a prediction"""
    x = torch.tensor([[2.0, 1.0, 0.0], [0.0, 1.0, 1.0], [9.0, 0.0, 0.0], [0.0, 0.0, 9.0]]).t().reshape(1, 3, 2, 2)
    y = torch.tensor([[[0, 2], [-100, 7]]])
    metric, counts = R.metric_and_counts(x, y)
    assert counts.tolist() == [[1, 1, 1], [0, 1, 0], [0, 0, 1], [2, 1, 1]]
    assert metric == (2 * 1 / 2 + 0.0 + 0.0) / 3                       # classes 1 and 2 occur (P or T) and score 0
    metric_fg, counts_fg = R.metric_and_counts(x, y, include_background=False)
    assert metric_fg == 0.0 and torch.equal(counts_fg, counts)
    # a class that occurs neither in the prediction nor in the labels is skipped; nothing left: 1
    y2 = torch.tensor([[[0, -100], [-100, -100]]])
    metric2, counts2 = R.metric_and_counts(x, y2)
    assert metric2 == 1.0 and counts2.tolist() == [[1, 1, 1], [0, 0, 0], [0, 0, 0], [1, 3, 0]]
    assert R.metric_and_counts(x, torch.full_like(y, -100))[0] == 1.0
    assert R.metric_and_counts(x, y2, include_background=False)[0] == 1.0
