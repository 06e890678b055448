"""GPU: uz_tile_gather / uz_tile_blend against tests/tile_ref.py (float64 torch), and SlidingWindowPredict against the same
composition made by hand with eager forwards and the ops calls.

Acceptance.  The gather is an exact copy.  The blend is bit-reproducible and each value lies within 2K + 6 float32 ulp of the
fp32-rounded float64 result, K the largest number of tiles over one pixel of the case.  The bound is derived, not measured:
numerator and denominator are sums of K non-negative terms (no cancellation); the roundings are one on w, one on the product,
K - 1 additions each and one division, at most about 2K + 2 units; the rest is margin for the comparison's own rounding.  The
decisions on the blended map equal the reference's wherever the reference's margin is at least 1e-5.  A replay of
SlidingWindowPredict equals the by-hand composition bit for bit."""
import numpy as np
import pytest
import torch

import tile_ref as T  # tests/tile_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from oracle import torch_ref
from storage_move import move_two_weights, twin_of  # tests/storage_move.py
from unet_zoo_amd import _lib, ops
from unet_zoo_amd.postprocess import MaskPostprocess
from unet_zoo_amd.predict import GraphedPredict
from unet_zoo_amd.tiled import SlidingWindowPredict

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLIPS = {1: (), 2: (3,), 4: (2,), 8: (2, 3)}       # view bit -> torch.flip dims


def _plan(shape, window, overlap):
    return ops.tile_plan(shape[2], window[0], overlap), ops.tile_plan(shape[3], window[1], overlap)


def _most(shape, window, ys, xs) -> int:
    """K: the largest number of tiles over one pixel of the image"""
    (oy, _), (ox, _) = T.offsets(shape[2], window[0]), T.offsets(shape[3], window[1])
    ky = T.cover(ys, window[0], shape[2])[oy:oy + shape[2]]
    kx = T.cover(xs, window[1], shape[3])[ox:ox + shape[3]]
    return int(ky.max() * kx.max())


# ---- 1. uz_tile_gather -------------------------------------------------------------------------------------------------------------
def _gather_case(shape, window, overlap, pad_mode="constant", seed=0):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    ys, xs = _plan(shape, window, overlap)
    assert ys == T.plan(shape[2], window[0], overlap) and xs == T.plan(shape[3], window[1], overlap)
    want = T.gather(x, ys, xs, window, pad_mode)
    per_image, total = len(ys) * len(xs), shape[0] * len(ys) * len(xs)
    xd = x.to(DEV)
    spans = [(0, total)]
    if shape[0] > 1:
        spans.append((per_image - 3, 7))                          # from image 0 into image 1
    for t0, tn in spans:
        out = torch.full((tn, shape[1]) + tuple(window), float("nan"), device=DEV)
        ops.tile_gather(xd, ys, xs, window, pad_mode, t0, out)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want[t0:t0 + tn]), (shape, window, overlap, pad_mode, t0, tn)
    return ys, xs


@pytest.mark.parametrize("overlap", [0.0, 0.5, 0.75])
def test_gather_is_the_slices_of_the_image(overlap):
    ys, xs = _gather_case((2, 3, 72, 88), (32, 32), overlap)
    if overlap == 0.5:
        assert ys == [0, 16, 32, 40] and xs == [0, 16, 32, 48, 56]      # the last tile is shifted back on both axes


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_gather_pads_an_image_smaller_than_the_window(pad_mode):
    ys, xs = _gather_case((1, 2, 24, 50), (32, 32), 0.5, pad_mode)
    assert ys == [0] and xs == [0, 16, 18]


def test_gather_with_a_window_that_is_not_square():
    _gather_case((2, 3, 72, 88), (32, 48), 0.5)
    _gather_case((2, 3, 72, 88), (48, 32), 0.25, seed=2)


# ---- 2. uz_tile_blend --------------------------------------------------------------------------------------------------------------
def _blend_case(shape, window, overlap, blend, seed=0):
    N, C, H, W = shape
    ys, xs = _plan(shape, window, overlap)
    tiles = torch.rand((N * len(ys) * len(xs), C) + tuple(window), generator=torch.Generator().manual_seed(seed))
    gh, gw = ops.tile_weights(window[0], blend), ops.tile_weights(window[1], blend)
    ref = T.blend(tiles, ys, xs, gh, gw, shape)
    td, ghd, gwd = tiles.to(DEV), gh.to(DEV), gw.to(DEV)
    out = torch.full(shape, float("nan"), device=DEV)
    again = torch.full(shape, float("nan"), device=DEV)
    ops.tile_blend(td, ys, xs, ghd, gwd, out)
    ops.tile_blend(td, ys, xs, ghd, gwd, again)
    torch.cuda.synchronize()
    assert torch.equal(out, again)                                # a fixed sum: bit-reproducible
    K = _most(shape, window, ys, xs)
    dist = T.ulp_distance(out, ref)
    print(f"tile_blend {shape} window {window} overlap {overlap} {blend}: K = {K}, largest distance {dist:.3f} float32 ulp (bound {2 * K + 6})")
    assert dist <= 2 * K + 6, (dist, K)
    return out, ref, K


@pytest.mark.parametrize("blend", ["constant", "gaussian"])
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("overlap", [0.0, 0.5, 0.75])
def test_blend_against_float64_and_its_decisions(overlap, C, blend):
    shape = (2, C, 72, 88)
    out, ref, K = _blend_case(shape, (32, 32), overlap, blend, seed=int(overlap * 100) + C)
    assert K == {0.0: 4, 0.5: 9, 0.75: 16}[overlap]              # overlap 0: the shifted last tile lies over its neighbour
    N, _, H, W = shape
    # the decisions on the blended map against the reference's, except where the reference itself is within 1e-5 of undecided
    if C == 1:
        mask = torch.empty(shape, dtype=torch.uint8, device=DEV)
        ops.mask_decide(out, _lib.POST_BINARY, 0.5, 0, mask, None)
        torch.cuda.synchronize()
        sure = (ref - 0.5).abs() >= 1e-5
        same = mask.cpu().bool() == (ref > 0.5)
    else:
        mask = torch.empty((N, C - 1, H, W), dtype=torch.uint8, device=DEV)
        cmap = torch.empty((N, H, W), dtype=torch.uint8, device=DEV)
        ops.mask_decide(out, _lib.POST_CLASS, 0.5, 1, mask, cmap)
        torch.cuda.synchronize()
        top2 = ref.topk(2, dim=1).values
        sure = (top2[:, 0] - top2[:, 1]) >= 1e-5
        am = ref.argmax(1)
        same = cmap.cpu().long() == am
        onehot = torch.stack([am == c for c in range(1, C)], 1)
        pick = sure[:, None].expand_as(onehot)
        assert torch.equal(mask.cpu().bool()[pick], onehot[pick])
    assert bool(same[sure].all())
    left_out = int((~sure).sum())
    print(f"  decisions: left out {left_out} of {sure.numel()}")
    assert left_out < 0.001 * sure.numel()


@pytest.mark.parametrize("blend", ["constant", "gaussian"])
def test_blend_crops_the_padding(blend):
    out, ref, K = _blend_case((1, 2, 24, 50), (32, 32), 0.5, blend, seed=7)
    assert K == 3 and tuple(out.shape) == (1, 2, 24, 50)


def test_blend_where_workgroups_walk_several_steps():
    shape = (1, 3, 450, 520)
    assert shape[1] * shape[2] * shape[3] > 8 * 256 * 256          # more elements than the grid has threads
    _blend_case(shape, (128, 128), 0.5, "gaussian", seed=11)


def test_constant_weights_without_overlap_lay_the_tiles_side_by_side():
    shape, window = (2, 3, 64, 96), (32, 32)
    ys, xs = _plan(shape, window, 0.0)
    assert ys == [0, 32] and xs == [0, 32, 64]
    tiles = torch.rand((12, 3, 32, 32), generator=torch.Generator().manual_seed(3))
    ones = torch.ones(32, device=DEV)
    out = torch.empty(shape, device=DEV)
    ops.tile_blend(tiles.to(DEV), ys, xs, ones, ones, out)
    torch.cuda.synchronize()
    want = tiles.view(2, 2, 3, 3, 32, 32).permute(0, 3, 1, 4, 2, 5).reshape(shape)       # (n, iy, ix, c, y, x) -> (n, c, iy y, ix x)
    assert torch.equal(out.cpu(), want)


# ---- 3. SlidingWindowPredict ---------------------------------------------------------------------------------------------------------
def _views_of(bits):
    return [b for b in (1, 2, 4, 8) if bits & b]


def _flip(t, bit):
    return torch.flip(t, FLIPS[bit]) if FLIPS[bit] else t


def _make(name, dtype, num_classes=1, in_channels=3, **kw):
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model(name, in_channels=in_channels, num_classes=num_classes, **kw)
    m.run_dtype = dtype
    return m.to(DEV).eval()


def _main(outputs):
    if isinstance(outputs, dict):
        return next(iter(outputs.values()))
    if isinstance(outputs, (list, tuple)):
        return outputs[-1]
    return outputs


def _centre(m, x):
    """move the head's bias so that the logits of x straddle zero: a freshly initialised unet predicts one empty mask"""
    with torch.no_grad():
        med = _main(m(x)).float().median()
        bias = [p for n, p in m.named_parameters() if n.endswith("bias") and p.numel() == 1][-1]
        bias -= med
    return m


def _x(B=2, C=3, H=72, W=88, seed=1):
    return torch_ref.synthetic_batch(B, C, H, W, seed=seed)[0].to(DEV)


def _by_hand(m, x, window, overlap, tile_batch, bits, pp, mode, blend="gaussian", pad_mode="constant"):
    """ops.tile_gather, eager forwards of torch.flip'ped tile batches, ops.tta_merge, ops.tile_blend, then the post-process call
    or ops.mask_decide; returns prob, mask, labels, stats, comps, class_map and the per-tile probabilities"""
    ys, xs = _plan(x.shape, window, overlap)
    total = x.shape[0] * len(ys) * len(xs)
    tiles = None
    for t0 in range(0, total, tile_batch):
        tn = min(tile_batch, total - t0)
        tile = torch.empty((tn, x.shape[1]) + tuple(window), device=DEV)
        ops.tile_gather(x, ys, xs, window, pad_mode, t0, tile)
        with torch.no_grad():
            mains = [_main(m(_flip(tile, b).contiguous())).contiguous() for b in _views_of(bits)]
        if tiles is None:
            tiles = torch.empty((total,) + tuple(mains[0].shape[1:]), dtype=torch.float32, device=DEV)
        ops.tta_merge(mains, bits, mode, tiles[t0:t0 + tn])
    prob = torch.empty((x.shape[0], tiles.shape[1]) + tuple(x.shape[2:]), dtype=torch.float32, device=DEV)
    gh, gw = ops.tile_weights(window[0], blend), ops.tile_weights(window[1], blend)
    ops.tile_blend(tiles, ys, xs, gh.to(DEV), gw.to(DEV), prob)
    labels = stats = comps = cmap = None
    if pp is not None:
        mask = pp(prob, mode="binary" if mode == _lib.POST_BINARY else "class", from_logits=False).clone()
        labels, stats, comps = pp.labels.clone(), pp.stats.clone(), pp.comps.clone()
        cmap = pp.class_map.clone() if pp.class_map is not None else None
    else:
        cls = mode == _lib.POST_CLASS
        N, C, H, W = prob.shape
        mask = torch.empty((N, C - 1 if cls else C, H, W), dtype=torch.uint8, device=DEV)
        cmap = torch.empty((N, H, W), dtype=torch.uint8, device=DEV) if cls else None
        ops.mask_decide(prob, mode, 0.5, 1 if cls else 0, mask, cmap)
    torch.cuda.synchronize()
    return prob, mask, labels, stats, comps, cmap, (tiles, ys, xs, gh, gw)


def _same(pred, mask, want):
    for name, g, w in zip(("prob", "mask", "labels", "stats", "comps", "class_map"),
                          (pred.prob, mask, pred.labels, pred.stats, pred.comps, pred.class_map), want[:6]):
        assert (g is None) == (w is None), name
        assert g is None or torch.equal(g, w), name


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_unet_replay_equals_the_composition_by_hand(dtype):
    x, window = _x(), (32, 32)
    m = _make("unet", dtype)
    _centre(m, T.gather(x.cpu(), *_plan(x.shape, window, 0.5), window).to(DEV))
    kw = dict(fill_holes=True, min_area=4)
    args = (window, 0.5, 16, 3)
    want = _by_hand(m, x, *args, MaskPostprocess(**kw), _lib.POST_BINARY)
    pred = SlidingWindowPredict(m, window=window, overlap=0.5, tile_batch=16, tta=("hflip",), postprocess=MaskPostprocess(**kw))
    for _ in range(2):                                         # the capture's first replay, then a plain replay
        mask = pred(x)
        torch.cuda.synchronize()
        pred.check()
        _same(pred, mask, want)
    assert pred.captures == 1 and pred.class_map is None and "2 x fwd" in pred.describe()
    assert pred.plan["batches"] == [(0, 16), (16, 16), (32, 8)] and pred.plan["forwards"] == 6 and pred.plan["tiles_per_image"] == 20
    assert tuple(mask.shape) == (2, 1, 72, 88) and 0 < int(mask.sum()) < mask.numel()
    tiles, ys, xs, gh, gw = want[6]
    K = _most(x.shape, window, ys, xs)
    dist = T.ulp_distance(pred.prob, T.blend(tiles.cpu(), ys, xs, gh, gw, tuple(pred.prob.shape)))
    print(f"SlidingWindowPredict {dtype}: K = {K}, prob {dist:.3f} float32 ulp from float64 (bound {2 * K + 6})")
    assert dist <= 2 * K + 6
    # a second input shape, the padded one, captures a second graph; the first one is still there
    x2 = _x(B=1, H=24, W=50, seed=3)
    want2 = _by_hand(m, x2, *args, MaskPostprocess(**kw), _lib.POST_BINARY)
    mask2 = pred(x2)
    torch.cuda.synchronize()
    assert pred.captures == 2 and tuple(mask2.shape) == (1, 1, 24, 50) and pred.plan["xs"] == [0, 16, 18]
    _same(pred, mask2, want2)
    pred(x)
    assert pred.captures == 2
    # an optimizer-style in-place change of a parameter is seen by the next call without a new capture
    p = next(m.parameters())
    with torch.no_grad():
        p.add_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(9)).to(DEV))
    want3 = _by_hand(m, x, *args, MaskPostprocess(**kw), _lib.POST_BINARY)
    mask = pred(x)
    torch.cuda.synchronize()
    assert pred.captures == 2 and not torch.equal(want3[0], want[0])
    _same(pred, mask, want3)
    # two parameters moved to new storage, with new values: one new capture, which reads them there (tests/storage_move.py)
    kept = move_two_weights(m)
    before, want3 = want3, _by_hand(twin_of(m, lambda: _make("unet", dtype)), x, *args, MaskPostprocess(**kw), _lib.POST_BINARY)
    mask = pred(x)
    torch.cuda.synchronize()
    assert pred.captures == 3 and len(kept) == 2 and not torch.equal(want3[0], before[0])
    _same(pred, mask, want3)
    _same(pred, mask, _by_hand(m, x, *args, MaskPostprocess(**kw), _lib.POST_BINARY))     # the moved model's own forwards, from now on
    masks = list(pred.predict([x, (x2, None)]))
    assert [tuple(k.shape) for k in masks] == [(2, 1, 72, 88), (1, 1, 24, 50)] and pred.captures == 4 and torch.equal(masks[0], want3[1])


def test_one_window_equal_to_the_image_is_graphed_predict():
    x = _x(B=1, H=64, W=64)
    m = _centre(_make("unet", torch.float32), x)
    plain = GraphedPredict(m)
    mask0 = plain(x)
    pred = SlidingWindowPredict(m, window=(64, 64))
    mask = pred(x)
    torch.cuda.synchronize()
    assert pred.plan["tiles"] == 1 and pred.plan["forwards"] == 1
    ulp = torch.from_numpy(np.spacing(plain.prob.cpu().numpy())).double()
    dist = float(((pred.prob.cpu().double() - plain.prob.cpu().double()).abs() / ulp).max())
    print(f"one window: prob {dist:.3f} float32 ulp from GraphedPredict's (w p / w is not exactly p)")
    assert dist <= 2.0
    sure = (plain.prob - 0.5).abs() >= 1e-6
    assert torch.equal(mask[sure], mask0[sure]) and 0 < int(mask.sum()) < mask.numel()


def test_a_fixed_size_swin_predicts_a_larger_image():
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model("swin_unet_v2", image_size=64, window_size=4, drop_path_rate=0.0)
    m.run_dtype = torch.float32
    m = m.to(DEV).eval()
    x = _x(B=1, H=96, W=128, seed=5)
    with pytest.raises(AssertionError, match="doesn't match model"):       # built for 64 x 64 alone
        GraphedPredict(m)(x)
    want = _by_hand(m, x, (64, 64), 0.5, 4, 1, None, _lib.POST_BINARY)
    pred = SlidingWindowPredict(m, window=(64, 64), overlap=0.5, tile_batch=4)
    mask = pred(x)
    torch.cuda.synchronize()
    assert tuple(mask.shape) == (1, 1, 96, 128) and pred.plan["ys"] == [0, 32] and pred.plan["xs"] == [0, 32, 64]
    assert pred.plan["batches"] == [(0, 4), (4, 2)]
    _same(pred, mask, want)


def test_three_classes_end_to_end():
    x, window = _x(), (32, 32)
    m = _make("unet", torch.float32, num_classes=3)
    want = _by_hand(m, x, window, 0.5, 16, 3, None, _lib.POST_CLASS)
    pred = SlidingWindowPredict(m, window=window, overlap=0.5, tile_batch=16, tta=("hflip",))
    mask = pred(x)
    torch.cuda.synchronize()
    assert tuple(mask.shape) == (2, 2, 72, 88) and tuple(pred.class_map.shape) == (2, 72, 88) and tuple(pred.prob.shape) == (2, 3, 72, 88)
    _same(pred, mask, want)
    am = want[0].argmax(1)
    assert torch.equal(pred.class_map.long(), am) and torch.equal(mask.bool(), torch.stack([am == c for c in (1, 2)], 1))
    off = float((pred.prob.double().sum(1) - 1.0).abs().max()) / float(np.spacing(np.float32(1.0)))
    print(f"three classes: prob sums to 1 within {off:.3f} float32 ulp")
    assert off <= 8.0
