"""RegionLoss without a GPU: the constructor's refusals, the Dice parametrisation, output weights, and the refusals of
uz_region_loss / uz_region_loss_workspace_bytes, which come before any launch (the library loads without a device)."""
import ctypes

import pytest
import torch

import unet_zoo_amd
from unet_zoo_amd import RegionLoss, _lib
from unet_zoo_amd.loss import RegionLoss as RegionLossFromModule


def test_exported_from_the_package():
    assert RegionLoss is RegionLossFromModule and "RegionLoss" in unet_zoo_amd.__all__


@pytest.mark.parametrize("kw", [dict(smooth=0.0), dict(smooth=-1.0), dict(gamma=0.99), dict(alpha=-0.1), dict(beta=-1e-3),
                                dict(w_bce=-1.0), dict(w_region=-0.5), dict(w_bce=0.0, w_region=0.0), dict(pos_weight=0.0),
                                dict(pos_weight=-2.0), dict(reduce="sample"), dict(reduce=None), dict(output_weights=[1.0, -0.5]),
                                dict(output_weights={"d0": -1.0}), dict(smooth=float("nan")), dict(gamma=float("inf"))])
def test_constructor_refuses(kw):
    with pytest.raises(ValueError):
        RegionLoss(**kw)


def test_constructor_accepts_the_edges():
    RegionLoss(w_bce=0.0)
    RegionLoss(w_region=0.0)
    RegionLoss(alpha=0.0, beta=0.0, gamma=1.0, smooth=1e-6)
    for r in ("batch", "image", "channel"):
        assert RegionLoss(reduce=r).reduce == r
    assert RegionLoss().pos_weight == 1.0 and RegionLoss().reduce == "image"


def test_dice_and_tversky_constructors():
    d = RegionLoss.dice(smooth=1.0)
    assert (d.alpha, d.beta, d.smooth, d.gamma) == (0.5, 0.5, 0.5, 1.0)
    d = RegionLoss.dice(smooth=3.0, w_bce=0.25, reduce="batch")
    assert (d.smooth, d.w_bce, d.reduce) == (1.5, 0.25, "batch")
    # (I + s/2) / (I + (S - I)/2 + (T - I)/2 + s/2) = (2 I + s) / (S + T + s)
    I, S, T, s = 3.25, 7.5, 5.0, 3.0
    ti = (I + d.smooth) / (I + d.alpha * (S - I) + d.beta * (T - I) + d.smooth)
    assert abs(ti - (2 * I + s) / (S + T + s)) < 1e-15
    t = RegionLoss.tversky(0.7, 0.3, gamma=4 / 3)
    assert (t.alpha, t.beta, t.gamma, t.smooth) == (0.7, 0.3, 4 / 3, 1.0)
    with pytest.raises(ValueError):
        RegionLoss.dice(smooth=0.0)


def test_output_weights_by_key_and_by_position():
    z = torch.zeros(1)
    dict_out = {"d0": z, "d1": z, "d2": z}
    assert RegionLoss().weights_for(dict_out) == (1.0, 1.0, 1.0)
    assert RegionLoss().weights_for(z) == (1.0,)
    by_key = RegionLoss(output_weights={"d2": 0.25, "d0": 1, "d1": 0.5, "unused": 9.0})
    assert by_key.weights_for(dict_out) == (1.0, 0.5, 0.25)          # the order of the outputs, not of the weights
    by_pos = RegionLoss(output_weights=[1, 0.5, 0.25])
    assert by_pos.weights_for(dict_out) == (1.0, 0.5, 0.25) and by_pos.weights_for([z, z, z]) == (1.0, 0.5, 0.25)
    with pytest.raises(ValueError, match="no entry"):
        RegionLoss(output_weights={"d0": 1.0}).weights_for(dict_out)
    with pytest.raises(ValueError, match="dict"):
        by_key.weights_for([z, z, z])
    with pytest.raises(ValueError, match="3 output_weights for 2"):
        by_pos.weights_for([z, z])


def test_cpu_tensors_and_shape_mismatch_are_refused_at_call():
    with pytest.raises(_lib.HipLibraryError):
        RegionLoss()(torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, 8, 8))
    with pytest.raises(_lib.HipLibraryError):
        RegionLoss().direct([torch.zeros(2, 1, 8, 8)], torch.zeros(2, 1, 8, 8))


def _desc(n_items=1, n=1024, groups=2, w_bce=1.0, w_region=1.0, alpha=0.5, beta=0.5, smooth=1.0, gamma=1.0, pos_weight=1.0,
          metric_item=0):
    return _lib.RegionDesc(n_items, n, groups, w_bce, w_region, alpha, beta, smooth, gamma, pos_weight, metric_item)


BAD_DESCS = [(dict(n=0), b"n ="), (dict(n=-4), b"n ="), (dict(groups=3), b"divide"), (dict(groups=0), b"divide"),
             (dict(n_items=0), b"n_items"), (dict(n_items=_lib.REGION_MAX_ITEMS + 1), b"n_items"),
             (dict(metric_item=1), b"metric_item"), (dict(metric_item=-1), b"metric_item"),
             (dict(n_items=3, metric_item=3), b"metric_item"), (dict(smooth=0.0), b"smooth"), (dict(smooth=-1.0), b"smooth"),
             (dict(gamma=0.5), b"gamma"), (dict(alpha=-0.1), b"alpha"), (dict(beta=-0.1), b"beta"), (dict(w_bce=-1.0), b"w_bce"),
             (dict(w_region=-1.0), b"w_region"), (dict(w_bce=0.0, w_region=0.0), b"both zero"), (dict(pos_weight=0.0), b"pos_weight"),
             (dict(pos_weight=-1.0), b"pos_weight"), (dict(smooth=float("nan")), b"smooth"), (dict(gamma=float("nan")), b"gamma")]


def _fake_items(n, weight=1.0, logits=0x1000, target=0x2000):
    items = (_lib.RegionItem * n)()
    for it in items:
        it.logits, it.target, it.dlogits, it.weight = logits, target, None, weight
    return items


@pytest.mark.parametrize("kw,word", BAD_DESCS)
def test_both_entries_refuse_a_bad_descriptor_before_any_launch(kw, word):
    lib = _lib.load()
    d = _desc(**kw)
    assert lib.uz_region_loss_workspace_bytes(ctypes.byref(d)) == -1
    assert word in lib.uz_last_error_string()
    # the pointers are never followed: the refusal comes first
    n = max(1, min(d.n_items, _lib.REGION_MAX_ITEMS))
    assert lib.uz_region_loss(ctypes.byref(d), _fake_items(n), 0x3000, 0x4000, None) == -1
    assert word in lib.uz_last_error_string()
    with pytest.raises(_lib.HipLibraryError):
        _lib.region_loss_workspace_bytes(d)


def test_null_arguments_and_bad_items_are_refused_before_any_launch():
    lib = _lib.load()
    assert lib.uz_region_loss_workspace_bytes(None) == -1 and b"null descriptor" in lib.uz_last_error_string()
    assert lib.uz_region_loss(None, _fake_items(1), 0x3000, 0x4000, None) == -1
    assert b"null descriptor" in lib.uz_last_error_string()
    d = _desc()
    assert lib.uz_region_loss(ctypes.byref(d), None, 0x3000, 0x4000, None) == -1 and b"null" in lib.uz_last_error_string()
    assert lib.uz_region_loss(ctypes.byref(d), _fake_items(1), None, 0x4000, None) == -1 and b"null" in lib.uz_last_error_string()
    assert lib.uz_region_loss(ctypes.byref(d), _fake_items(1), 0x3000, None, None) == -1 and b"null" in lib.uz_last_error_string()
    assert lib.uz_region_loss(ctypes.byref(d), _fake_items(1), 0x3000, 0x4008, None) == -1
    assert b"16-byte" in lib.uz_last_error_string()
    assert lib.uz_region_loss(ctypes.byref(d), _fake_items(1, logits=None), 0x3000, 0x4000, None) == -1
    assert b"item 0" in lib.uz_last_error_string()
    assert lib.uz_region_loss(ctypes.byref(d), _fake_items(1, target=None), 0x3000, 0x4000, None) == -1
    assert b"item 0" in lib.uz_last_error_string()
    d2 = _desc(n_items=2)
    items = _fake_items(2)
    items[1].weight = -0.5
    assert lib.uz_region_loss(ctypes.byref(d2), items, 0x3000, 0x4000, None) == -1
    assert b"item 1" in lib.uz_last_error_string() and b"weight" in lib.uz_last_error_string()


@pytest.mark.parametrize("n,groups", [(16, 1), (391 * 3, 3), (16 * 256 * 256, 16), (8 * 512 * 512, 8), (48 * 4096, 48),
                                      (1 << 26, 1), (4096 * 7, 4096)])
def test_workspace_is_positive_and_grows_with_the_number_of_maps(n, groups):
    sizes = [_lib.region_loss_workspace_bytes(_desc(n_items=k, n=n, groups=groups)) for k in range(1, _lib.REGION_MAX_ITEMS + 1)]
    assert sizes[0] > 0
    assert all(b > a for a, b in zip(sizes, sizes[1:]))
    # the rows of one map are capped (as uz_bce_dice's): six doubles per row, one coefficient quad per chunk
    assert sizes[0] <= 1024 * 6 * 8 + groups * (16 + 6 * 8)
