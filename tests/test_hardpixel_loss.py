"""CPU: the reference of HardPixelLoss (tests/hardpixel_ref.py) against plain torch (cross-entropy, torch.topk and its autograd
gradient, the usual focal formula, the tie rule); torch's own float32 evaluation of the GPU tests' cases against their
bounds; the library's refusals, workspace and grid without a GPU; the Python class as far as it goes without one."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import hardpixel_ref as R  # tests/hardpixel_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from unet_zoo_amd import BoundaryLoss, HardPixelLoss, LovaszLoss, MulticlassLoss, RegionLoss
from unet_zoo_amd import _lib as L


def _class_inputs(seed=0, N=2, K=5, H=9, W=7):
    g = torch.Generator().manual_seed(seed)
    x = (2.0 * torch.randn(N, K, H, W, generator=g)).double()
    y = torch.randint(0, K, (N, H, W), generator=g)
    y[:, 2, :] = -100
    return x, y


# ----------------------------------------------------------------------------------------------- the reference against plain torch
def test_keep_one_gamma_zero_is_the_mean_cross_entropy():
    x, y = _class_inputs()
    V, _, rows, _ = R.term(x, y, True, keep=1.0)
    assert abs(V.item() - F.cross_entropy(x, y, ignore_index=-100).item()) < 1e-14
    assert rows[0][0] == int((y != -100).sum()) and rows[0][1] + rows[0][2] == rows[0][0]
    g = torch.Generator().manual_seed(1)
    xb = (2.0 * torch.randn(3, 2, 5, 6, generator=g)).double()
    tb = (torch.rand(3, 2, 5, 6, generator=g) > 0.6).double()
    V, _, _, _ = R.term(xb, tb, False, keep=1.0)
    assert abs(V.item() - F.binary_cross_entropy_with_logits(xb, tb).item()) < 1e-14
    # per image: the mean of the images' means; an image without a valid pixel is left out of the mean
    y2 = y.clone()
    y2[1] = -100
    V2, _, rows2, w2 = R.term(x, y2, True, keep=1.0, per_image=True)
    assert abs(V2.item() - F.cross_entropy(x[:1], y[:1], ignore_index=-100).item()) < 1e-14
    assert rows2[1][:3] == (0, 0, 0) and not w2[1].any()


@pytest.mark.parametrize("per_image", [False, True])
def test_keep_below_one_is_torch_topk_and_its_gradient(per_image):
    x, y = _class_inputs(seed=2)
    leaf = x.clone().requires_grad_(True)
    ce = F.cross_entropy(leaf, y, ignore_index=-100, reduction="none")
    valid = y != -100
    if per_image:
        want = sum(torch.topk(ce[n][valid[n]], math.ceil(0.25 * int(valid[n].sum()))).values.mean() for n in range(2)) / 2
    else:
        want = torch.topk(ce[valid], math.ceil(0.25 * int(valid.sum()))).values.mean()
    (want_g,) = torch.autograd.grad(want, leaf)
    leaf2 = x.clone().requires_grad_(True)
    V, f, rows, _ = R.term(leaf2, y, True, keep=0.25, per_image=per_image)
    (g,) = torch.autograd.grad(V, leaf2)
    assert all(r[2] == 1 for r in rows)                        # tie-free
    assert abs(V.item() - want.item()) < 1e-14 and (g - want_g).abs().max() < 1e-15
    assert not g[(~valid).unsqueeze(1).expand_as(g)].any()
    # binary mode, one segment over all C channels of the batch
    gen = torch.Generator().manual_seed(3)
    xb = (2.0 * torch.randn(2, 3, 5, 6, generator=gen)).double().requires_grad_(True)
    tb = (torch.rand(2, 3, 5, 6, generator=gen) > 0.6).double()
    bce = F.binary_cross_entropy_with_logits(xb, tb, reduction="none")
    if per_image:
        want = sum(torch.topk(bce[n].reshape(-1), 9).values.mean() for n in range(2)) / 2       # ceil(0.1 * 90) = 9
    else:
        want = torch.topk(bce.reshape(-1), 18).values.mean()
    V, _, _, _ = R.term(xb, tb, False, keep=0.1, per_image=per_image)
    assert abs(V.item() - want.item()) < 1e-14
    assert (torch.autograd.grad(V, xb)[0] - torch.autograd.grad(want, xb)[0]).abs().max() < 1e-15


def test_focal_is_the_usual_formula():
    x, y = _class_inputs(seed=4)
    valid = y != -100
    logp = F.log_softmax(x, 1).gather(1, y.clamp(min=0).unsqueeze(1)).squeeze(1)
    want = ((1 - logp.exp()) ** 2.0 * -logp)[valid].mean()
    V, _, _, _ = R.term(x, y, True, keep=1.0, gamma=2.0)
    assert abs(V.item() - want.item()) < 1e-14
    g = torch.Generator().manual_seed(5)
    xb = (2.0 * torch.randn(2, 1, 5, 6, generator=g)).double()
    tb = (torch.rand(2, 1, 5, 6, generator=g) > 0.6).double()
    p = torch.sigmoid(xb)
    pt = torch.where(tb > 0.5, p, 1 - p)
    want = ((1 - pt) ** 1.5 * F.binary_cross_entropy_with_logits(xb, tb, reduction="none")).mean()
    V, _, _, _ = R.term(xb, tb, False, keep=1.0, gamma=1.5)
    assert abs(V.item() - want.item()) < 1e-14
    # df/dl of the definition against autograd
    l = torch.linspace(0.01, 6.0, 50, dtype=torch.float64).requires_grad_(True)
    for gamma in (1.0, 2.0, 3.5):
        q = -torch.expm1(-l)
        (d,) = torch.autograd.grad((q ** gamma * l).sum(), l)
        assert (d - (q ** gamma + gamma * q ** (gamma - 1) * torch.exp(-l) * l)).abs().max() < 1e-14


def test_the_tie_rule_weights_sum_to_one_and_ignore_position():
    f = torch.tensor([[0.5, 2.0, 0.5, 0.5, 0.1, 0.5, 3.0, 0.0]], dtype=torch.float64)
    valid = torch.ones_like(f, dtype=torch.bool)
    w, rows = R.weights_of(f, f, valid, 1, keep=0.5)                       # m = 4: 3.0, 2.0 and two of the four 0.5
    assert rows[0][:3] == (4, 2, 4) and rows[0][3].item() == 0.5
    assert w[0].tolist() == [0.125, 0.25, 0.125, 0.125, 0.0, 0.125, 0.25, 0.0] and abs(w.sum().item() - 1.0) < 1e-15
    perm = torch.tensor([7, 3, 1, 6, 0, 2, 5, 4])
    w2, _ = R.weights_of(f[:, perm], f[:, perm], valid, 1, keep=0.5)
    assert torch.equal(w2, w[:, perm])
    V = (w * f).sum()
    assert abs(V.item() - (3.0 + 2.0 + 2 * 0.5) / 4) < 1e-15              # (sum above + (m - n_above) tau) / m
    for x, t in (R.make_tied_inputs(), R.make_inputs((2, 3, 40, 40))):
        for per_image in (False, True):
            _, _, rows, w = R.term(x, t, False, keep=0.1, per_image=per_image)
            assert (w.sum(1) - 1.0).abs().max() < 1e-12 and all(r[1] < r[0] <= r[1] + r[2] for r in rows)


def test_kept_count_and_ohem_threshold():
    assert R.kept_count(1000, 0, 0.1, 0) == 100 and R.kept_count(10, 0, 0.1, 0) == 1       # the fp32 product, one rounding
    assert R.kept_count(1001, 0, 0.1, 0) == 101 and R.kept_count(7, 0, R.MIN_KEEP, 0) == 1
    assert R.kept_count(100, 0, 0.1, 50) == 50 and R.kept_count(30, 0, 0.1, 50) == 30 and R.kept_count(100, 70, 0.1, 50) == 70
    assert R.kept_count(0, 0, 0.5, 10) == 0
    x, y = _class_inputs(seed=6)
    valid = y != -100
    ce = F.cross_entropy(x, y, ignore_index=-100, reduction="none")
    c = int((torch.exp(-ce)[valid] < 0.7).sum())
    assert 20 < c < int(valid.sum())
    _, _, rows, _ = R.term(x, y, True, keep=R.MIN_KEEP, min_kept=5, max_prob=0.7)
    assert rows[0][0] == c
    want = torch.topk(ce[valid], c).values.mean()
    assert abs(R.term(x, y, True, keep=R.MIN_KEEP, min_kept=5, max_prob=0.7)[0].item() - want.item()) < 1e-14
    _, _, rows, _ = R.term(x, y, True, keep=R.MIN_KEEP, min_kept=c + 7, max_prob=0.7)
    assert rows[0][0] == c + 7


def test_selection_from_a_given_fp32_array_is_used_for_value_and_gradient():
    x, t = R.make_inputs((3, 1, 17, 23))
    f64 = R.pixel_losses(x, t, False)[0]
    f32 = f64.float()
    sel = R.selection_of(f32, torch.ones_like(t, dtype=torch.bool), 1, 0.1)
    m = math.ceil(0.1 * t.numel())
    assert sel[0, 0] == m and sel[0, 1] == m - 1 and sel[0, 2] == 1
    assert sel[0, 3] == int(torch.sort(f32.reshape(-1), descending=True).values[m - 1].view(torch.int32))
    a = R.reference("bce_dice", [x], t, [1.0], 0.5, keep=0.1)
    b = R.reference("bce_dice", [x], t, [1.0], 0.5, keep=0.1, losses=[f32])
    assert abs(a[0].item() - b[0].item()) < 1e-12 and (a[1][0] - b[1][0]).abs().max() < 1e-12


# ----------------------------------------------------------------------- float32 against float64 on the cases of the GPU tests
def test_float32_evaluation_of_the_gpu_cases_stays_inside_their_bounds():
    """|V32 - V64| against 2e-6 max(1, |V64|) and max |dV32 - dV64| against 2e-6 max |dV64| for torch's own float32
    evaluation (autograd) of every term of tests/test_hardpixel_loss_gpu.py, with the float64 kept set; the shares are
    printed, the largest are written into that file's docstring"""
    worst_v, worst_g = ("", 0.0), ("", 0.0)
    for name, x, t, cls, kw in R.term_cases():
        leaf = x.double().requires_grad_(True)
        V64, _, _, _ = R.term(leaf, t, cls, **kw)
        (g64,) = torch.autograd.grad(V64, leaf)
        V32, g32 = R.term_float32(x, t, cls, **kw)
        sv = abs(V32.item() - V64.item()) / (2e-6 * max(1.0, abs(V64.item())))
        sg = (g32.double() - g64).abs().max().item() / (2e-6 * g64.abs().max().item())
        print(f"{name}: value {sv:.3f} gradient {sg:.3f}")
        worst_v, worst_g = max(worst_v, (name, sv), key=lambda p: p[1]), max(worst_g, (name, sg), key=lambda p: p[1])
    print(f"largest share of the bound: value {worst_v[1]:.3f} ({worst_v[0]}), gradient {worst_g[1]:.3f} ({worst_g[0]})")
    assert worst_v[1] < 0.5 and worst_g[1] < 0.5


# ---------------------------------------------------------------------------------------------------------- the Python class
def test_package_exports_it():
    assert "HardPixelLoss" in unet_zoo_amd.__all__ and unet_zoo_amd.HardPixelLoss is HardPixelLoss
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in ("uz_hardpixel_workspace_bytes", "uz_hardpixel_grid", "uz_hardpixel_loss"):
        assert name in L.EXPORTS and getattr(raw, name)


def test_constructor_refusals_and_accepted_edges():
    for bad in ("dice", 3, None, lambda o, t: 0, BoundaryLoss(), LovaszLoss(), HardPixelLoss()):      # stacking is out of scope
        with pytest.raises(TypeError, match="HardPixelLoss: base"):
            HardPixelLoss(base=bad)
    with pytest.raises(TypeError, match="LovaszLoss: base"):
        LovaszLoss(base=HardPixelLoss())
    for kw in (dict(weight=-1e-3), dict(base_scale=-1.0), dict(weight=float("nan")), dict(weight=0.0, base_scale=0.0),
               dict(keep=0.0), dict(keep=1.5), dict(keep=-0.1), dict(keep=float("nan")), dict(keep="some"), dict(keep=1e-46),      # 1e-46 is 0 in fp32: what the library would see

               dict(min_kept=-1), dict(min_kept=2.5), dict(min_kept=True), dict(max_prob=0.0), dict(max_prob=1.0),
               dict(max_prob=float("inf")), dict(gamma=0.5), dict(gamma=-1.0), dict(gamma=float("inf")), dict(gamma=0.999)):
        with pytest.raises(ValueError, match="HardPixelLoss:"):
            HardPixelLoss(**kw)
    c = HardPixelLoss()
    assert c.base == "bce_dice" and (c.weight, c.base_scale, c.keep, c.min_kept, c.max_prob, c.gamma) == (1.0, 1.0, 0.1, 0, None, 0.0)
    assert not c.per_image and c.losses is None and c.selection is None and c.term is None and "HardPixelLoss(" in repr(c)
    assert HardPixelLoss(keep=1e-45).keep == 1e-45              # a denormal fp32 is > 0: accepted here as by the library
    assert HardPixelLoss(gamma=1.0).gamma == 1.0 and HardPixelLoss(keep=1.0, per_image=True).per_image
    t = HardPixelLoss.topk(RegionLoss.dice(), k=0.25, weight=0.5)
    assert (t.keep, t.min_kept, t.max_prob, t.gamma, t.weight) == (0.25, 0, None, 0.0, 0.5)
    o = HardPixelLoss.ohem(MulticlassLoss.ce_dice())
    assert (o.keep, o.min_kept, o.max_prob, o.gamma) == (L.HARDPIXEL_MIN_KEEP, 100_000, 0.7, 0.0) and o.class_mode
    assert ctypes.c_float(o.keep).value == o.keep > 0.0                    # the smallest fraction the descriptor takes
    f = HardPixelLoss.focal("bce_dice", per_image=True)
    assert (f.keep, f.gamma, f.per_image) == (1.0, 2.0, True)
    with pytest.raises(ValueError, match="HardPixelLoss: gamma"):
        HardPixelLoss.focal("bce_dice", gamma=0.5)


def test_set_weights_target_dtype_and_weights_follow_the_base():
    c = HardPixelLoss(base=RegionLoss.dice())
    c.set_weights(weight=0.5, base_scale=0.0)
    assert (c.weight, c.base_scale) == (0.5, 0.0)
    with pytest.raises(ValueError, match="HardPixelLoss:"):
        c.set_weights(weight=0.0)
    assert HardPixelLoss().target_dtype == torch.float32 and not HardPixelLoss(base=RegionLoss()).class_mode
    m = HardPixelLoss(base=MulticlassLoss(ignore_index=255))
    assert m.target_dtype == torch.int32 and m.class_mode and m.ignore_index == 255
    maps = {"a": torch.zeros(1), "b": torch.zeros(1)}
    assert HardPixelLoss().weights_for(maps) == (1.0, 1.0)
    assert HardPixelLoss(base=RegionLoss(output_weights={"a": 1, "b": .5})).weights_for(maps) == (1.0, 0.5)


def test_cpu_tensors_and_bad_shapes_are_refused_at_call():
    x, t = torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4)
    for c in (HardPixelLoss(), HardPixelLoss(base=RegionLoss())):
        with pytest.raises(L.HipLibraryError):
            c(x, t)
        with pytest.raises(L.HipLibraryError):
            c.direct(x, t)
    with pytest.raises(ValueError, match="HardPixelLoss: .*shape"):
        HardPixelLoss()(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 5))
    with pytest.raises(ValueError, match="HardPixelLoss: .*integer"):
        HardPixelLoss(base=MulticlassLoss())(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4))


# ------------------------------------------------------------------------------------------------- the library without a GPU
def _desc(mode=L.HARDPIXEL_BINARY, n_items=1, N=2, C=1, H=8, W=8, per_image=0, ignore_index=-100, main=0, keep=0.1, min_kept=0,
          max_prob=0.0, gamma=0.0, max_workgroups=0):
    return L.HardPixelDesc(mode, n_items, N, C, H, W, per_image, ignore_index, main, keep, min_kept, max_prob, gamma, max_workgroups)


def test_bad_descriptors_are_refused_without_a_gpu():
    lib = L.load()
    assert L.hardpixel_workspace_bytes(_desc()) > 0
    bad = [(_desc(mode=2), b"unknown mode"), (_desc(n_items=0), b"n_items"), (_desc(n_items=L.CLASS_MAX_ITEMS + 1), b"n_items"),
           (_desc(N=0), b"non-positive shape"), (_desc(W=0), b"non-positive shape"),
           (_desc(mode=L.HARDPIXEL_CLASS, C=1), b"K = 1"), (_desc(mode=L.HARDPIXEL_CLASS, C=L.CLASS_MAX_K + 1), b"K = 33"),
           (_desc(n_items=2, main=2), b"main_item"), (_desc(main=-1), b"main_item"),
           (_desc(keep=0.0), b"keep"), (_desc(keep=1.0001), b"keep"), (_desc(keep=-0.5), b"keep"), (_desc(keep=float("nan")), b"keep"),
           (_desc(min_kept=-1), b"min_kept"),
           (_desc(max_prob=1.0), b"max_prob"), (_desc(max_prob=-0.1), b"max_prob"), (_desc(max_prob=float("nan")), b"max_prob"),
           (_desc(gamma=0.5), b"gamma"), (_desc(gamma=-1.0), b"gamma"), (_desc(gamma=float("inf")), b"gamma"),
           (_desc(gamma=float("nan")), b"gamma"), (_desc(gamma=0.999), b"gamma"),
           (_desc(max_workgroups=-1), b"max_workgroups"),
           (_desc(n_items=16, N=4097, H=1, W=1, per_image=1), b"segments in the call"),     # 65552 segments
           (_desc(N=17, H=1024, W=1024), b"a segment of"),                                  # 17 * 2^20 in ONE segment
           (_desc(n_items=16, N=65, H=512, W=512, per_image=1), b"elements in 16 maps")]    # above 2^28 elements
    for d, what in bad:
        assert lib.uz_hardpixel_workspace_bytes(ctypes.byref(d)) == -1 and what in lib.uz_last_error_string(), what
        with pytest.raises(L.HipLibraryError, match="uz_hardpixel_grid"):
            L.hardpixel_grid(d)
        assert lib.uz_hardpixel_loss(ctypes.byref(d), None, None, None, None, None, None, None, None, None) < 0
        assert what in lib.uz_last_error_string()                  # the descriptor is refused before any pointer is looked at
    for d in (_desc(keep=1.0), _desc(keep=L.HARDPIXEL_MIN_KEEP), _desc(keep=1e-45), _desc(n_items=16, N=4096, H=1, W=1, per_image=1), _desc(gamma=1.0), _desc(gamma=7.5), _desc(max_prob=0.7),
              _desc(min_kept=10 ** 9), _desc(mode=L.HARDPIXEL_CLASS, C=2), _desc(mode=L.HARDPIXEL_CLASS, C=32),
              _desc(N=16, H=1024, W=1024), _desc(N=17, H=1024, W=1024, per_image=1)):
        assert L.hardpixel_workspace_bytes(d) > 0
    assert lib.uz_hardpixel_workspace_bytes(None) == -1 and b"null descriptor" in lib.uz_last_error_string()
    assert lib.uz_hardpixel_grid(None, None) < 0 and b"null descriptor" in lib.uz_last_error_string()


def _plan(cls, n_items, N, C, H, W, per_image):
    """the workspace formula of DESIGN 3y restated"""
    P = N * H * W if cls else N * C * H * W
    S = N if per_image else 1
    seg = P // S
    chunk = L.HARDPIXEL_TILE * -(-(-(-seg // L.HARDPIXEL_TILE)) // L.HARDPIXEL_MAX_ROWS)
    units = n_items * S * -(-seg // chunk)
    sizes = (4 * P * n_items, 4 * 256 * units, 8 * units, 32 * n_items * S, 8 * units)
    return sum((b + 15) // 16 * 16 for b in sizes), units


def test_workspace_bytes_and_grid_are_pinned():
    cases = [  # (descriptor arguments, bytes, (grid, units))
        (dict(N=3, C=1, H=17, W=23), 5792, (1, 1)),                                                       # small
        (dict(mode=L.HARDPIXEL_CLASS, n_items=3, N=2, C=19, H=33, W=47, per_image=1), 43664, (6, 6)),     # odd
        (dict(N=2, C=3, H=40, W=40), 43648, (5, 5)),                                                     # the walked case of the GPU test
        (dict(N=2049, C=1, H=64, W=64, per_image=1), 37898304, (2048, 4098)),                             # units exceed the grid
        (dict(N=16, C=1, H=1024, W=1024), 2 ** 26 + 256 * 1040 + 32, (256, 256)),                         # 2^24 in one segment: 32 tiles a chunk
    ]
    for kw, want_bytes, want_grid in cases:
        d = _desc(**kw)
        cls = d.mode == L.HARDPIXEL_CLASS
        assert _plan(cls, d.n_items, d.N, d.C, d.H, d.W, d.per_image) == (want_bytes, want_grid[1]), kw
        assert L.hardpixel_workspace_bytes(d) == want_bytes and L.hardpixel_grid(d) == want_grid, kw
    assert L.hardpixel_grid(_desc(N=2, C=3, H=40, W=40, max_workgroups=2)) == (2, 5)
    assert L.hardpixel_grid(_desc(N=2, C=3, H=40, W=40, max_workgroups=9)) == (5, 5)
    assert L.hardpixel_grid(_desc(N=2049, C=1, H=64, W=64, per_image=1, max_workgroups=5)) == (5, 4098)


def test_null_and_overlapping_pointers_are_refused_before_any_launch():
    lib = L.load()
    d = _desc(N=2, C=1, H=8, W=8, per_image=1)                  # maps of 512 bytes, selection of 32
    assert 16 <= L.hardpixel_workspace_bytes(d) < 0x10000
    ok = dict(target=0x30000, scales=0x40000, base_loss=0x40100, out=0x40200, losses=0x50000, selection=0x58000, ws=0x100000)

    def item(logits=0x10000, dlogits=0x20000, weight=1.0):
        its = (L.HardPixelItem * 1)()
        its[0].logits, its[0].dlogits, its[0].weight = logits, dlogits, weight
        return its

    def call(its=None, **kw):
        a = dict(ok)
        a.update(kw)
        return lib.uz_hardpixel_loss(ctypes.byref(d), its or item(), a["target"], a["scales"], a["base_loss"], a["out"], a["losses"],
                                     a["selection"], a["ws"], None)

    for name in ok:
        assert call(**{name: None}) < 0 and b"uz_hardpixel_loss: null pointer" in lib.uz_last_error_string(), name
    assert lib.uz_hardpixel_loss(ctypes.byref(d), None, *ok.values(), None) < 0 and b"null pointer" in lib.uz_last_error_string()
    assert call(its=item(logits=None)) < 0 and b"uz_hardpixel_loss: item 0 has null logits" in lib.uz_last_error_string()
    assert call(its=item(dlogits=None, weight=-1.0)) < 0 and b"item 0 has a negative weight" in lib.uz_last_error_string()
    assert call(ws=0x100008) < 0 and b"uz_hardpixel_loss: the workspace must be 16-byte aligned" in lib.uz_last_error_string()
    for kw in (dict(losses=0x50002), dict(selection=0x58002), dict(out=0x40202), dict(its=item(dlogits=0x20002)), dict(its=item(logits=0x10002))):
        assert call(**kw) < 0 and b"uz_hardpixel_loss: tensors must be 4-byte aligned" in lib.uz_last_error_string(), kw
    for kw in (dict(out=0x40000 + 4), dict(out=0x40100), dict(losses=0x30000 + 256), dict(selection=0x10000), dict(ws=0x30000 - 16),
               dict(its=item(dlogits=0x30000 + 128)),                                        # every output over an input
               dict(out=0x50000), dict(losses=0x58000 + 4), dict(selection=0x100000 + 16), dict(ws=0x20000 - 16),
               dict(its=item(dlogits=0x50000 + 64)), dict(its=item(dlogits=0x58000 - 64)),   # every output over another
               dict(its=item(dlogits=0x10000 + 64))):                                        # dlogits inside logits
        assert call(**kw) < 0 and b"uz_hardpixel_loss: tensors overlap" in lib.uz_last_error_string(), kw
