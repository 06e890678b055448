"""CPU: the reference of ClDiceLoss (tests/cldice_ref.py) -- the two tie facts of torch's subgradients that the definition
names, the soft skeleton on hand-checked planes, the input makers' own assertions; torch's float32 evaluation of the GPU tests'
tie-free cases against their bounds; the Python class and the library's refusals as far as they go without a GPU."""
import pytest
import torch

import cldice_ref as R  # tests/cldice_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from unet_zoo_amd import BoundaryLoss, ClDiceLoss, LovaszLoss, MulticlassLoss, RegionLoss
from unet_zoo_amd import _lib as L
from unet_zoo_amd.capture import resolve_criterion
from unet_zoo_amd.criterion import FusedCriterion


# ------------------------------------------------------------------------------------------------------ the subgradients at ties
def test_erode_of_a_constant_plane_sends_half_up_and_half_left():
    a = torch.full((1, 1, 3, 3), 0.7, dtype=torch.float64, requires_grad=True)
    R.erode(a)[0, 0, 1, 1].backward()
    want = torch.zeros(3, 3, dtype=torch.float64)
    want[0, 1] = 0.5          # v: the first minimum top to bottom is the pixel above the centre
    want[1, 0] = 0.5          # h: the first minimum left to right is the pixel left of it; v == h: half to each
    assert torch.equal(a.grad[0, 0], want)


def test_dilate_of_a_constant_plane_sends_all_to_the_top_left():
    a = torch.full((1, 1, 3, 3), 0.7, dtype=torch.float64, requires_grad=True)
    R.dilate(a)[0, 0, 1, 1].backward()
    want = torch.zeros(3, 3, dtype=torch.float64)
    want[0, 0] = 1.0
    assert torch.equal(a.grad[0, 0], want)


def test_min_routes_to_the_smaller_one_and_relu_has_no_gradient_at_zero():
    a = torch.tensor([[[[0.9, 0.2, 0.9], [0.5, 0.6, 0.8], [0.9, 0.7, 0.9]]]], dtype=torch.float64, requires_grad=True)
    R.erode(a)[0, 0, 1, 1].backward()           # v = 0.2 (up), h = 0.5 (left): all to the pixel above
    want = torch.zeros(3, 3, dtype=torch.float64)
    want[0, 1] = 1.0
    assert torch.equal(a.grad[0, 0], want)
    z = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    torch.relu(z).sum().backward()
    assert not z.grad.any()


# ------------------------------------------------------------------------------------------------------------- the soft skeleton
def test_windows_are_clipped_to_the_picture():
    a = torch.tensor([[[[0.3, 0.9, 0.1, 0.5]]]], dtype=torch.float64)          # one row: v is the pixel itself
    assert torch.equal(R.erode(a), torch.tensor([[[[0.3, 0.1, 0.1, 0.1]]]], dtype=torch.float64))
    assert torch.equal(R.dilate(a), torch.tensor([[[[0.9, 0.9, 0.9, 0.5]]]], dtype=torch.float64))
    assert torch.equal(R.erode(a.transpose(2, 3)), R.erode(a).transpose(2, 3))


def test_skeleton_of_a_bar_is_its_centre_line():
    a = torch.zeros(1, 1, 9, 12, dtype=torch.float64)
    a[0, 0, 3:6, :] = 1.0                                                      # a bar three pixels thick across the picture
    s = R.skel(a, 3)
    want = torch.zeros_like(a)
    want[0, 0, 4, :] = 1.0
    assert torch.equal(s, want)
    thin = torch.zeros(1, 1, 9, 12, dtype=torch.float64)
    thin[0, 0, 4, :] = 1.0                                                     # a line is its own skeleton, at once
    for k in (1, 3, 10):
        assert torch.equal(R.skel(thin, k), thin)


def test_skeleton_depends_on_the_plane_within_k_plus_2():
    g = torch.Generator().manual_seed(0)
    a = torch.rand(1, 1, 41, 41, generator=g, dtype=torch.float64)
    for k in (1, 3):
        Rk = k + 2
        b = a.clone()
        far = torch.ones(41, 41, dtype=torch.bool)
        far[20 - Rk:20 + Rk + 1, 20 - Rk:20 + Rk + 1] = False
        b[0, 0][far] = torch.rand(int(far.sum()), generator=g, dtype=torch.float64)
        assert R.skel(a, k)[0, 0, 20, 20] == R.skel(b, k)[0, 0, 20, 20]


def test_a_perfect_prediction_has_term_zero_and_it_grows_when_a_band_is_cut():
    t = R.bands((1, 1, 40, 40)).double()
    V, _, sp, st = R.term(torch.where(t > 0.5, 40.0, -40.0).double(), t, False, 3, 1.0)
    assert V.item() < 1e-12 and torch.allclose(sp, st, atol=1e-12)
    cut = t.clone()
    cut[0, 0, 18:22, :] = 0.0
    V2, _, _, _ = R.term(torch.where(cut > 0.5, 40.0, -40.0).double(), t, False, 3, 1.0)
    assert V2.item() > 0.05


def test_per_image_and_the_class_planes():
    x, t = R.make_inputs((3, 2, 17, 23))
    Vb, _, _, _ = R.term(x.double(), t, False, 3, 1.0, per_image=False)
    Vi, _, _, _ = R.term(x.double(), t, False, 3, 1.0, per_image=True)
    singles = [R.term(x[n:n + 1, c:c + 1].double(), t[n:n + 1, c:c + 1], False, 3, 1.0)[0] for n in range(3) for c in range(2)]
    assert abs(Vi.item() - sum(s.item() for s in singles) / 6) < 1e-14 and abs(Vb.item() - Vi.item()) > 1e-6
    xc, y = R.make_class_inputs(4)
    p, tc = R.class_planes(xc.double(), y, False, -100)
    assert p.shape[1] == 3 and tc.shape[1] == 3
    bad = ((y == -100) | (y < 0) | (y >= 4)).unsqueeze(1)
    assert not p[bad.expand_as(p)].any() and not tc[bad.expand_as(tc)].any()
    p4, _ = R.class_planes(xc.double(), y, True, -100)
    assert p4.shape[1] == 4 and torch.equal(p4[:, 1:], p)


def test_tied_probabilities_are_bit_equal_and_carry_the_sigmoid_gradient():
    x = torch.tensor([0.5, -1.25, 0.5, 3.0, -1.25, 0.5], dtype=torch.float64, requires_grad=True)
    p = R.sigmoid_tied(x)
    assert p[0] == p[2] == p[5] and p[1] == p[4] and torch.allclose(p, torch.sigmoid(x.detach()), atol=1e-16, rtol=0)
    p.sum().backward()
    s = torch.sigmoid(x.detach())
    assert torch.allclose(x.grad, s * (1 - s), atol=1e-16, rtol=0)


# ------------------------------------------------------------------------------------------------------------ the input makers
GPU_SHAPES = [(3, 1, 17, 23), (1, 2, L.CLDICE_TILE_H, L.CLDICE_TILE_W), (2, 1, 2 * L.CLDICE_TILE_H + 5, 3 * L.CLDICE_TILE_W + 7),
              (1, 1, 1, 37), (1, 1, 37, 1)]


def test_the_makers_hold_what_they_promise():
    for shape in GPU_SHAPES + [(2, 1, 40, 56), (3, 2, 17, 23), (2, 1, 96, 96), (2, 1, 64, 64)]:
        x, t = R.make_inputs(shape)                           # asserts distinct logits and the probability gap itself
        assert x.dtype == torch.float32 and tuple(x.shape) == tuple(t.shape) == shape and set(t.unique().tolist()) <= {0.0, 1.0}
        assert x.min() >= -4.0 and x.max() < 4.0 + 4.0 / (shape[2] * shape[3] - 1)      # a plane's shift: below half a rank step
        if shape[2] > 8 and shape[3] > 8:
            assert 0.2 < t.mean() < 0.6 and not torch.equal(t[0, 0], t[-1, -1])
    x, t = R.make_tied_inputs((2, 1, 40, 40))
    assert len(x.unique()) <= 97
    for K in (4, 8):
        x, y = R.make_class_inputs(K)
        assert x.dtype == torch.float32 and tuple(x.shape) == (2, K, 33, 20) and y.dtype == torch.int64
        p = torch.softmax(x.double(), 1)
        assert p[:, 1:].sum(1).max() < 1.0 and set(range(K)) <= set(y.unique().tolist())


# ---------------------------------------------------------------------------------------- float32 torch against the GPU bounds
def test_float32_torch_stays_inside_half_of_the_gpu_bounds_on_the_tie_free_cases():
    """|V32 - V64| / (2e-6 max(1, |V64|)) and max |g32 - g64| / (2e-6 max |g64|): the share of the bounds of
    tests/test_cldice_loss_gpu.py that torch's own float32 evaluation uses up"""
    worst_v = worst_g = 0.0
    for shape in ((2, 1, 40, 56), (3, 2, 17, 23), (2, 1, 96, 96)):
        x, t = R.make_inputs(shape)
        for k in (1, 3, 10):
            for per_image in (False, True):
                leaf = x.double().requires_grad_(True)
                V64, _, _, _ = R.term(leaf, t, False, k, 1.0, per_image)
                (g64,) = torch.autograd.grad(V64, leaf)
                V32, g32 = R.term_float32(x, t, False, k, 1.0, per_image)
                sv = abs(V32.item() - V64.item()) / (2e-6 * max(1.0, abs(V64.item())))
                sg = (g32.double() - g64).abs().max().item() / (2e-6 * g64.abs().max().item())
                print(f"{shape} k={k} per_image={per_image}: value {sv:.3f} gradient {sg:.3f}")
                worst_v, worst_g = max(worst_v, sv), max(worst_g, sg)
    print(f"largest share of the bound: value {worst_v:.3f}, gradient {worst_g:.3f}")
    assert worst_v <= 0.5 and worst_g <= 0.5


# ---------------------------------------------------------------------------------------------------------- the Python class
def test_package_exports_it_and_it_is_a_fused_criterion():
    assert "ClDiceLoss" in unet_zoo_amd.__all__ and unet_zoo_amd.ClDiceLoss is ClDiceLoss
    c = ClDiceLoss()
    assert isinstance(c, FusedCriterion) and c._NAME == "ClDiceLoss"
    assert set(vars(ClDiceLoss)) & {"_build_plan", "_term"} == {"_build_plan", "_term"}
    assert not set(vars(ClDiceLoss)) & {"set_weights", "loss_and_dice", "direct", "__call__", "forward", "weights_for", "target_dtype", "_launch"}


def test_resolve_criterion_returns_the_fused_pair():
    for c in (ClDiceLoss(), ClDiceLoss(base=RegionLoss.dice()), ClDiceLoss(base=MulticlassLoss())):
        fused, dtype = resolve_criterion(c)
        assert fused == (c.loss_and_dice, c.direct)
        assert dtype == (torch.int32 if c.class_mode else torch.float32)
    assert resolve_criterion(lambda o, t: 0)[0] is None                      # what a Python clDice on max_pool2d gets
    assert ClDiceLoss(base=MulticlassLoss()).target_dtype == torch.int32 and ClDiceLoss().target_dtype == torch.float32


def test_constructor_refusals_and_accepted_edges():
    for bad in ("dice", 3, None, lambda o, t: 0, BoundaryLoss(), ClDiceLoss()):      # stacking is out of scope
        with pytest.raises(TypeError, match="ClDiceLoss: base"):
            ClDiceLoss(base=bad)
    for kw in (dict(weight=-1e-3), dict(base_scale=-1.0), dict(weight=float("nan")), dict(base_scale=float("inf")),
               dict(weight=0.0, base_scale=0.0), dict(weight="much"), dict(iterations=0), dict(iterations=L.CLDICE_MAX_ITERATIONS + 1),
               dict(smooth=0.0), dict(smooth=-1.0), dict(smooth=float("nan")), dict(smooth=float("inf")), dict(smooth=1e300)):
        with pytest.raises(ValueError, match="ClDiceLoss:"):
            ClDiceLoss(**kw)
    for kw in (dict(iterations=3.0), dict(iterations="3"), dict(iterations=True), dict(iterations=None)):
        with pytest.raises(TypeError, match="ClDiceLoss: iterations"):
            ClDiceLoss(**kw)
    c = ClDiceLoss()
    assert c.base == "bce_dice" and c.weight == 0.5 and c.base_scale == 1.0 and c.iterations == 3 and c.smooth == 1.0
    assert not c.per_image and not c.include_background
    assert ClDiceLoss(iterations=1).iterations == 1 and ClDiceLoss(iterations=L.CLDICE_MAX_ITERATIONS).iterations == 10
    assert "ClDiceLoss(" in repr(c) and c.probs is None and c.skeleton is None and c.target_skeleton is None and c.term is None


def test_set_weights_target_dtype_and_weights_follow_the_protocol():
    c = ClDiceLoss(base=RegionLoss.dice())
    c.set_weights(weight=0.25)
    assert (c.weight, c.base_scale) == (0.25, 1.0)
    with pytest.raises(ValueError, match="ClDiceLoss:"):
        c.set_weights(weight=-1.0)
    assert (c.weight, c.base_scale) == (0.25, 1.0)
    m = ClDiceLoss(base=MulticlassLoss(ignore_index=255))
    assert m.class_mode and m.ignore_index == 255
    maps = {"a": torch.zeros(1), "b": torch.zeros(1)}
    assert ClDiceLoss().weights_for(maps) == (1.0, 1.0)
    assert ClDiceLoss(base=RegionLoss(output_weights={"a": 1, "b": .5})).weights_for(maps) == (1.0, 0.5)


def test_cpu_tensors_and_bad_shapes_are_refused_at_call():
    x, t = torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4)
    with pytest.raises(L.HipLibraryError):
        ClDiceLoss()(x, t)
    with pytest.raises(ValueError, match="ClDiceLoss: .*shape"):
        ClDiceLoss()(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 5))
    with pytest.raises(ValueError, match="ClDiceLoss: .*integer"):
        ClDiceLoss(base=MulticlassLoss())(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4))


def _desc(mode=L.CLDICE_BINARY, n_items=1, N=1, C=1, H=8, W=8, per_image=0, bg=0, ignore=-100, k=3, smooth=1.0, main=0):
    return L.ClDiceDesc(mode, n_items, N, C, H, W, per_image, bg, ignore, k, smooth, main)


def test_the_library_refuses_before_any_launch():
    assert L.CLDICE_MAX_ITERATIONS == 10
    for k in range(1, L.CLDICE_MAX_ITERATIONS + 1):
        assert L.cldice_workspace_bytes(_desc(k=k)) > 0
    for bad in (_desc(k=0), _desc(k=L.CLDICE_MAX_ITERATIONS + 1), _desc(smooth=0.0), _desc(smooth=-1.0), _desc(smooth=float("nan")),
                _desc(smooth=float("inf")), _desc(mode=2), _desc(n_items=L.CLASS_MAX_ITEMS + 1), _desc(N=0), _desc(W=0),
                _desc(mode=L.CLDICE_CLASS, C=1), _desc(mode=L.CLDICE_CLASS, C=L.CLASS_MAX_K + 1), _desc(n_items=2, main=2),
                _desc(main=-1), _desc(n_items=16, N=65, H=512, W=512)):
        assert L.load().uz_cldice_workspace_bytes(bad) < 0
        with pytest.raises(L.HipLibraryError, match="uz_cldice_grid"):
            L.cldice_grid(bad)
    # the units: (map, plane, tile); the background plane is no unit unless it is included
    TH, TW = L.CLDICE_TILE_H, L.CLDICE_TILE_W
    assert L.cldice_grid(_desc(n_items=3, N=2, C=2, H=2 * TH + 5, W=3 * TW + 7)) == (3 * 2 * 2 * 3 * 4,) * 2
    assert L.cldice_grid(_desc(mode=L.CLDICE_CLASS, N=2, C=4, H=TH, W=TW))[1] == 2 * 3
    assert L.cldice_grid(_desc(mode=L.CLDICE_CLASS, N=2, C=4, H=TH, W=TW, bg=1))[1] == 2 * 4
    grid, units = L.cldice_grid(_desc(N=16, H=512, W=512))
    assert units == 16 * 256 and grid < units                                   # workgroups walk
    for shape in ((16, 1, 256, 256), (16, 8, 256, 256), (8, 1, 512, 512)):      # the shapes of tools/cldice_bench.py
        assert L.cldice_workspace_bytes(_desc(n_items=7 if shape[0] == 8 else 1, N=shape[0], C=shape[1], H=shape[2], W=shape[3])) > 0


def test_null_and_overlapping_pointers_are_refused_before_any_launch():
    import ctypes
    lib = L.load()
    assert lib.uz_cldice_workspace_bytes(None) == -1 and b"null descriptor" in lib.uz_last_error_string()
    assert lib.uz_cldice_grid(None, None) < 0 and b"null descriptor" in lib.uz_last_error_string()
    d = _desc(N=2)                                                    # 2 x 1 x 8 x 8: maps of 512 bytes
    assert 16 <= L.cldice_workspace_bytes(d) < 0x10000
    items = (L.ClDiceItem * 1)()
    items[0].logits, items[0].dlogits, items[0].weight = 0x10000, 0x20000, 1.0
    # the other pointers at disjoint made-up addresses: nothing is dereferenced before the checks
    ok = dict(target=0x30000, scales=0x40000, base_loss=0x40100, out=0x40200, probs=0x50000, skeleton=0x58000, tskel=0x60000, ws=0x100000)

    def call(its=items, **kw):
        a = dict(ok)
        a.update(kw)
        return lib.uz_cldice_loss(ctypes.byref(d), its, a["target"], a["scales"], a["base_loss"], a["out"], a["probs"], a["skeleton"],
                                  a["tskel"], a["ws"], None)

    def item(logits, dlogits, weight):
        its = (L.ClDiceItem * 1)()
        its[0].logits, its[0].dlogits, its[0].weight = logits, dlogits, weight
        return its

    for name in ok:
        assert call(**{name: None}) < 0 and b"uz_cldice_loss: null pointer" in lib.uz_last_error_string(), name
    assert lib.uz_cldice_loss(ctypes.byref(d), None, *ok.values(), None) < 0 and b"null pointer" in lib.uz_last_error_string()
    assert call(its=item(None, 0x20000, 1.0)) < 0 and b"uz_cldice_loss: item 0 has null logits" in lib.uz_last_error_string()
    assert call(its=item(0x10000, None, -1.0)) < 0 and b"uz_cldice_loss: item 0 has a negative weight" in lib.uz_last_error_string()
    assert call(ws=0x100008) < 0 and b"uz_cldice_loss: the workspace must be 16-byte aligned" in lib.uz_last_error_string()
    for kw in (dict(probs=0x50002), dict(skeleton=0x58002), dict(tskel=0x60002), dict(out=0x40202), dict(its=item(0x10000, 0x20002, 1.0)),
               dict(its=item(0x10002, 0x20000, 1.0))):
        assert call(**kw) < 0 and b"uz_cldice_loss: tensors must be 4-byte aligned" in lib.uz_last_error_string(), kw
    for kw in (dict(out=0x40000 + 4), dict(out=0x40100), dict(probs=0x30000 + 256), dict(skeleton=0x10000), dict(tskel=0x30000 - 64),
               dict(ws=0x30000 - 16), dict(its=item(0x10000, 0x30000 + 128, 1.0)),           # every output over an input
               dict(out=0x50000), dict(probs=0x58000 + 4), dict(skeleton=0x60000 - 4), dict(tskel=0x100000 + 16), dict(ws=0x20000 - 16),
               dict(its=item(0x10000, 0x50000 + 64, 1.0)), dict(its=item(0x10000, 0x60000 + 64, 1.0)),      # every output over another
               dict(its=item(0x10000, 0x10000 + 64, 1.0))):                                  # dlogits inside logits
        assert call(**kw) < 0 and b"uz_cldice_loss: tensors overlap" in lib.uz_last_error_string(), kw
