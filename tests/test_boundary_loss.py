"""CPU: the reference of BoundaryLoss (tests/boundary_ref.py) against a brute force over all pixel pairs, hand-derived cases and
Kervadec's expression; the constructor's and the C ABI's refusals (the library loads without a device)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import boundary_ref as R  # tests/boundary_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from unet_zoo_amd import BoundaryLoss, MulticlassLoss, RegionLoss
from unet_zoo_amd import _lib as L

SHAPES = [(1, 1), (4, 4), (17, 23), (33, 20), (8, 150)]
DENSITIES = [0.02, 0.3, 0.9]


def _mask(shape, density, seed):
    return np.random.default_rng(seed).random(shape) < density


# ------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_sd2_is_the_minimum_over_all_pixel_pairs(shape, density):
    for seed in range(3):
        G = _mask(shape, density, 100 * seed + shape[0])
        got, want = R.sd2_plane(G), R.sd2_brute(G)
        assert got.dtype == np.int64 and np.array_equal(got, want)


def test_hand_derived_cases():
    centre = np.zeros((3, 3), bool)
    centre[1, 1] = True
    assert R.sd2_plane(centre).tolist() == [[2, 1, 2], [1, -1, 1], [2, 1, 2]]
    assert R.phi_of(R.sd2_plane(centre)).tolist() == [[math.sqrt(2), 1, math.sqrt(2)], [1, 0, 1], [math.sqrt(2), 1, math.sqrt(2)]]
    assert not R.sd2_plane(np.zeros((5, 7), bool)).any()         # empty: Kervadec's one_hot2dist
    assert not R.sd2_plane(np.ones((5, 7), bool)).any()          # full: this project's convention
    assert not R.sd2_brute(np.ones((5, 7), bool)).any() and not R.sd2_brute(np.zeros((5, 7), bool)).any()
    # a mask touching the picture's edge: the outside does not exist, so the left column is deep inside
    edge = np.zeros((3, 5), bool)
    edge[:, :3] = True
    assert R.sd2_plane(edge).tolist() == [[-9, -4, -1, 1, 4]] * 3
    assert R.phi_of(R.sd2_plane(edge), spacing=0.5).tolist() == [[-1.0, -0.5, 0.0, 0.5, 1.0]] * 3
    one = np.zeros((1, 1), bool)
    assert R.sd2_plane(one).tolist() == [[0]] and R.sd2_plane(~one).tolist() == [[0]]


@pytest.mark.parametrize("spacing", [1.0, 0.7])
def test_phi_is_kervadecs_expression(spacing):
    for shape in SHAPES:
        for density in DENSITIES:
            G = _mask(shape, density, 7)
            assert np.abs(R.phi_of(R.sd2_plane(G), spacing) - R.phi_kervadec(G, spacing)).max() <= 1e-12
    assert not R.phi_kervadec(np.zeros((4, 4), bool)).any()


def test_class_planes_leave_ignored_and_out_of_range_pixels_out():
    y = np.array([[[0, 1, 2, -100], [7, 1, -1, 2]]])
    p = R.planes_class(y, 3, include_background=False)
    assert p.shape == (2, 2, 4)
    assert p[0].tolist() == [[False, True, False, False], [False, True, False, False]]
    assert p[1].tolist() == [[False, False, True, False], [False, False, False, True]]
    assert R.planes_class(y, 3, include_background=True).shape == (3, 2, 4)
    # ignore_index inside [0, K): the class is empty
    assert not R.planes_class(y, 3, include_background=False, ignore_index=1)[0].any()


def test_reference_gradients_are_the_closed_forms():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 1, 6, 5, generator=g)
    t = (torch.rand(2, 1, 6, 5, generator=g) > 0.6).float()
    phi = torch.from_numpy(R.phi_of(R.sd2_planes(R.planes_binary(t.numpy()))))
    leaf = x.double().requires_grad_(True)
    (grad,) = torch.autograd.grad(R.term_binary(leaf, phi), leaf)
    p = torch.sigmoid(x.double())
    assert torch.allclose(grad, phi.reshape(x.shape) * p * (1 - p) / x.numel(), rtol=1e-12, atol=0)
    K = 4
    xc = torch.randn(2, K, 6, 5, generator=g)
    y = torch.randint(0, K, (2, 6, 5), generator=g)
    y[0, 0] = -100
    y[1, 2, 1] = 9
    phic = torch.from_numpy(R.phi_of(R.sd2_planes(R.planes_class(y.numpy(), K))))
    leaf = xc.double().requires_grad_(True)
    (grad,) = torch.autograd.grad(R.term_class(leaf, y, phic), leaf)
    pc = torch.softmax(xc.double(), dim=1)
    phit = torch.cat([torch.zeros(2, 1, 6, 5, dtype=torch.float64), phic.reshape(2, K - 1, 6, 5)], dim=1)
    valid = ((y >= 0) & (y < K)).double().unsqueeze(1)
    want = pc * (phit - (pc * phit).sum(1, keepdim=True)) * valid / (2 * (K - 1) * 30)
    assert torch.allclose(grad, want, rtol=1e-11, atol=1e-18)
    assert not grad[0, :, 0].any() and not grad[1, :, 2, 1].any()


# ---------------------------------------------------------------------------------------------------------- the Python class
def test_package_exports_it():
    assert "BoundaryLoss" in unet_zoo_amd.__all__ and unet_zoo_amd.BoundaryLoss is BoundaryLoss


def test_constructor_refusals_and_accepted_edges():
    for bad in ("dice", 3, None, lambda o, t: 0):
        with pytest.raises(TypeError, match="base"):
            BoundaryLoss(base=bad)
    for kw in (dict(weight=-1e-3), dict(base_scale=-1.0), dict(weight=float("nan")), dict(base_scale=float("inf")),
               dict(weight=0.0, base_scale=0.0), dict(weight="much"), dict(spacing=0.0), dict(spacing=-1.0),
               dict(spacing=float("inf")), dict(spacing=float("nan"))):
        with pytest.raises(ValueError):
            BoundaryLoss(**kw)
    c = BoundaryLoss()
    assert c.base == "bce_dice" and c.weight == 0.01 and c.base_scale == 1.0 and c.spacing == 1.0 and not c.include_background
    assert BoundaryLoss(weight=0.0).weight == 0.0 and BoundaryLoss(weight=1.0, base_scale=0.0).base_scale == 0.0
    assert BoundaryLoss(base=RegionLoss.dice(), spacing=1e-3, include_background=True).include_background
    assert "BoundaryLoss(" in repr(c)


def test_set_weights_validates_and_rebalance_follows_kervadec():
    c = BoundaryLoss(base=RegionLoss.dice(), weight=0.01)
    c.set_weights(weight=0.02)
    assert (c.weight, c.base_scale) == (0.02, 1.0)
    c.set_weights(base_scale=0.5)
    assert (c.weight, c.base_scale) == (0.02, 0.5)
    for kw in (dict(weight=-1.0), dict(base_scale=float("nan")), dict(weight=0.0, base_scale=0.0), dict(weight=float("inf"))):
        with pytest.raises(ValueError):
            c.set_weights(**kw)
    assert (c.weight, c.base_scale) == (0.02, 0.5)              # a refused call changes nothing
    c.rebalance(0.25)
    assert (c.weight, c.base_scale) == (0.25, 0.75)
    c.rebalance(0.0)
    assert (c.weight, c.base_scale) == (0.0, 1.0)
    c.rebalance(1.0)
    assert (c.weight, c.base_scale) == (1.0, 0.0)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            c.rebalance(bad)


def test_target_dtype_and_ignore_index_follow_the_base():
    assert BoundaryLoss().target_dtype == torch.float32
    assert BoundaryLoss(base=RegionLoss()).target_dtype == torch.float32 and not BoundaryLoss(base=RegionLoss()).class_mode
    c = BoundaryLoss(base=MulticlassLoss(ignore_index=255))
    assert c.target_dtype == torch.int32 and c.class_mode and c.ignore_index == 255


def test_output_weights_are_the_bases():
    maps = {"a": torch.zeros(1), "b": torch.zeros(1)}
    assert BoundaryLoss().weights_for(maps) == (1.0, 1.0)
    assert BoundaryLoss(base=RegionLoss(output_weights={"a": 1, "b": .5})).weights_for(maps) == (1.0, 0.5)
    with pytest.raises(ValueError, match="output_weights"):
        BoundaryLoss(base=MulticlassLoss(output_weights=[1.0])).weights_for(maps)


def test_cpu_tensors_are_refused_at_call():
    x, t = torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4)
    for c in (BoundaryLoss(), BoundaryLoss(base=RegionLoss())):
        with pytest.raises(L.HipLibraryError):
            c(x, t)
        with pytest.raises(L.HipLibraryError):
            c.direct(x, t)
    with pytest.raises(L.HipLibraryError):
        BoundaryLoss(base=MulticlassLoss())(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="shape"):
        BoundaryLoss()(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 5))
    with pytest.raises(ValueError, match="integer"):
        BoundaryLoss(base=MulticlassLoss())(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4))


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def _desc(**kw):
    f = dict(mode=L.BOUNDARY_BINARY, n_items=1, N=2, C=1, H=8, W=8, first_class=0, ignore_index=-100, metric_item=0, spacing=1.0)
    f.update(kw)
    return L.BoundaryDesc(*(f[k] for k in ("mode", "n_items", "N", "C", "H", "W", "first_class", "ignore_index", "metric_item",
                                            "spacing")))


BAD_DESCRIPTORS = [
    (dict(mode=2), b"mode"),
    (dict(n_items=0), b"n_items"),
    (dict(n_items=L.CLASS_MAX_ITEMS + 1), b"n_items"),
    (dict(N=0), b"shape"),
    (dict(C=0), b"shape"),
    (dict(H=0), b"shape"),
    (dict(W=-3), b"shape"),
    (dict(H=4097), b"above 4096"),
    (dict(W=4097), b"above 4096"),
    (dict(mode=L.BOUNDARY_CLASS, C=1), b"K = 1"),
    (dict(mode=L.BOUNDARY_CLASS, C=L.CLASS_MAX_K + 1), b"K = 33"),
    (dict(mode=L.BOUNDARY_CLASS, C=4, first_class=4), b"first_class"),
    (dict(mode=L.BOUNDARY_CLASS, C=4, first_class=-1), b"first_class"),
    (dict(metric_item=1), b"metric_item"),
    (dict(metric_item=-1), b"metric_item"),
    (dict(spacing=0.0), b"spacing"),
    (dict(spacing=-1.0), b"spacing"),
    (dict(spacing=float("inf")), b"spacing"),
    (dict(spacing=float("nan")), b"spacing"),
    (dict(N=2048, C=1, H=1024, W=1024), b"2^31"),
    (dict(N=2 ** 30, C=1, H=1, W=1), b"too many"),
]


@pytest.mark.parametrize("kw,word", BAD_DESCRIPTORS, ids=[f"{i}-{w.decode().split()[0]}" for i, (_, w) in enumerate(BAD_DESCRIPTORS)])
def test_bad_descriptors_are_refused_without_a_gpu(kw, word):
    lib = L.load()
    d = _desc(**kw)
    units = ctypes.c_int(0)
    item = (L.BoundaryItem * 1)()
    for name, call in (("uz_boundary_workspace_bytes", lambda: lib.uz_boundary_workspace_bytes(ctypes.byref(d))),
                       ("uz_boundary_grid", lambda: lib.uz_boundary_grid(ctypes.byref(d), ctypes.byref(units))),
                       ("uz_boundary_loss", lambda: lib.uz_boundary_loss(ctypes.byref(d), item, 16, 16, 16, 16, 16, 16, None))):
        assert call() < 0, name
        msg = lib.uz_last_error_string()
        assert word in msg and name.encode() in msg, msg
    with pytest.raises(L.HipLibraryError):
        L.boundary_workspace_bytes(d)


def test_null_and_overlapping_pointers_are_refused_before_any_launch():
    lib = L.load()
    assert lib.uz_boundary_workspace_bytes(None) == -1 and b"null descriptor" in lib.uz_last_error_string()
    assert lib.uz_boundary_grid(None, None) < 0 and b"null descriptor" in lib.uz_last_error_string()
    d = _desc()                                                       # 2 x 1 x 8 x 8: maps of 512 bytes
    items = (L.BoundaryItem * 1)()
    items[0].logits, items[0].dlogits, items[0].weight = 0x10000, 0x20000, 1.0
    # target, scales, base_loss, out, sd2, workspace at disjoint made-up addresses: nothing is dereferenced before the checks
    ok = dict(target=0x30000, scales=0x40000, base_loss=0x40100, out=0x40200, sd2=0x50000, ws=0x60000)

    def call(its=items, **kw):
        a = dict(ok)
        a.update(kw)
        return lib.uz_boundary_loss(ctypes.byref(d), its, a["target"], a["scales"], a["base_loss"], a["out"], a["sd2"], a["ws"], None)

    for name in ok:
        assert call(**{name: None}) < 0 and b"null pointer" in lib.uz_last_error_string(), name
    assert lib.uz_boundary_loss(ctypes.byref(d), None, *ok.values(), None) < 0 and b"null pointer" in lib.uz_last_error_string()
    none = (L.BoundaryItem * 1)()
    none[0].logits, none[0].dlogits, none[0].weight = None, 0x20000, 1.0
    assert call(its=none) < 0 and b"null logits" in lib.uz_last_error_string()
    neg = (L.BoundaryItem * 1)()
    neg[0].logits, neg[0].dlogits, neg[0].weight = 0x10000, None, -1.0
    assert call(its=neg) < 0 and b"negative weight" in lib.uz_last_error_string()
    assert call(ws=0x60008) < 0 and b"16-byte aligned" in lib.uz_last_error_string()
    assert call(sd2=0x50002) < 0 and b"4-byte aligned" in lib.uz_last_error_string()
    for kw in (dict(sd2=0x30000 + 256), dict(out=0x40000 + 4), dict(out=0x40100), dict(ws=0x50000 + 16), dict(sd2=0x10000),
               dict(target=0x20000 + 128), dict(ws=0x20000 - 16)):
        assert call(**kw) < 0 and b"overlap" in lib.uz_last_error_string(), kw
    same = (L.BoundaryItem * 1)()
    same[0].logits, same[0].dlogits, same[0].weight = 0x10000, 0x10000 + 64, 1.0
    assert call(its=same) < 0 and b"overlap" in lib.uz_last_error_string()


def test_grid_reports_the_column_pass():
    grid, units = L.boundary_grid(_desc(N=2, C=3, H=33, W=20))
    assert (grid, units) == (18, 18)                                   # 6 planes of ceil(660 / 256) units
    grid, units = L.boundary_grid(_desc(N=9, C=1, H=256, W=256))
    assert grid == 2048 and units == 2304                              # eight workgroups per CU; the rest is walked
    grid, units = L.boundary_grid(_desc(mode=L.BOUNDARY_CLASS, N=2, C=4, H=16, W=16, first_class=1))
    assert (grid, units) == (6, 6)
    assert L.boundary_workspace_bytes(_desc()) % 16 == 0
