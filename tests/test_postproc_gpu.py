"""GPU: MaskPostprocess (uz_postproc.hip) against tests/postproc_ref.py (numpy + scipy.ndimage, pinned by tests/test_postproc.py),
uz_tta_merge against torch float64, and GraphedPredict against the same composition made by hand.

Acceptance.  Everything uz_postproc writes is an integer and EQUAL to the reference: mask, labels, stats, comps, class_map; the
error word is 0 in every case.  ``prob`` of uz_tta_merge lies within PROB_ULP float32 ulp of the rounded float64 result (the
bound is twice the largest distance measured on an MI355X over these very cases); its decisions equal the
float64 reference's wherever that reference's margin is at least 1e-5."""
import itertools

import numpy as np
import pytest
import torch

import postproc_ref as R  # tests/postproc_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from oracle import torch_ref
from storage_move import move_two_weights, twin_of  # tests/storage_move.py
from unet_zoo_amd import _lib, ops
from unet_zoo_amd.postprocess import MaskPostprocess
from unet_zoo_amd.predict import GraphedPredict

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROB_ULP = 24.0      # 2 x the 12 ulp measured: sigmoid 2 (fp32 inputs) and 3 (bf16), softmax 12 (fp32) and 4 (bf16); 1 to 4 views


def _logits_of(planes: np.ndarray, seed: int = 0) -> torch.Tensor:
    """fp32 logits whose sign is the plane, of varying size"""
    g = torch.Generator().manual_seed(seed)
    mag = 0.25 + torch.rand(planes.shape, generator=g)
    return torch.where(torch.from_numpy(np.ascontiguousarray(planes)), mag, -mag)


def _get(pp: MaskPostprocess):
    torch.cuda.synchronize()
    pp.check()
    return [t.cpu().numpy() if t is not None else None for t in (pp.mask, pp.labels, pp.stats, pp.comps, pp.class_map)]


def _equal(got, want, what=""):
    for name, g, w in zip(("mask", "labels", "stats", "comps", "class_map"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:8].tolist())


def _binary_case(planes: np.ndarray, what="", **kw):
    """planes (N, C, H, W) boolean -> compared in full; returns the kernel's results"""
    x = _logits_of(planes)
    pp = MaskPostprocess(**kw)
    pp(x.to(DEV))
    got = _get(pp)
    assert got[4] is None and not got[2][..., 6:].any()
    _equal(got[:4], R.binary(x.numpy(), 0.0, **kw), what=f"{what} {kw}")
    return got


# ---- 1. seeded blob planes: the whole grid of settings on one input ---------------------------------------------------------------
@pytest.fixture(scope="module")
def blob_logits():
    return torch.from_numpy(R.blobs((2, 3, 37, 150), 3, sigma=1.5))


@pytest.mark.parametrize("fill", [False, True], ids=["nofill", "fill"])
@pytest.mark.parametrize("conn", [1, 2])
def test_blob_planes_every_setting(blob_logits, conn, fill):
    x = blob_logits.to(DEV)
    for min_area, keep in itertools.product((0, 5), (0, 1, 3)):
        kw = dict(connectivity=conn, fill_holes=fill, min_area=min_area, keep_largest=keep)
        pp = MaskPostprocess(**kw)
        pp(x, mode="binary")
        got = _get(pp)
        assert not got[2][..., 6:].any()
        _equal(got[:4], R.binary(blob_logits.numpy(), 0.0, **kw), what=str(kw))
    assert got[2][..., 0].min() > 3                           # the planes hold several components each


def test_probabilities_with_the_half_threshold(blob_logits):
    p = torch.sigmoid(blob_logits.double()).float()
    pp = MaskPostprocess(fill_holes=True, min_area=3)
    pp(p.to(DEV), mode="binary", from_logits=False)
    _equal(_get(pp)[:4], R.binary(p.numpy(), 0.5, fill_holes=True, min_area=3))


# ---- 2. adversarial planes (the planes of tests/postproc_core_main.cpp) -----------------------------------------------------------
@pytest.mark.parametrize("name", list(R.adversarial()))
def test_adversarial_plane(name):
    p = R.adversarial()[name]
    for conn in (1, 2):
        got = _binary_case(p[None, None], what=name, connectivity=conn)
        _binary_case(p[None, None], what=name, connectivity=conn, fill_holes=True, keep_largest=2)
    st = got[2][0, 0]
    HW = p.size
    expect = {"empty": [0, 0, 0, 0, 0, 0], "full": [1, 1, HW, HW, 0, HW], "corners": [4, 4, 4, 4, 0, 1],
              "checkerboard": [1, 1, HW // 2, HW // 2, 0, HW // 2]}.get(name)          # connectivity 2
    if expect is not None:
        assert st[:6].tolist() == expect
    if name in ("serpentine", "spiral", "comb_last_row", "comb_last_column"):
        assert st[0] == 1 and got[3][0, 0, 0, 7] == 0       # one component, rooted at pixel 0
    if name == "checkerboard":
        st1 = _binary_case(p[None, None], what=name, connectivity=1)[2][0, 0]
        assert st1[:6].tolist() == [HW // 2, HW // 2, HW // 2, HW // 2, 0, 1]
    if name == "diagonal_touch":
        assert st[0] == 1 and _binary_case(p[None, None], connectivity=1)[2][0, 0, 0] == 2


# ---- 3. selection ------------------------------------------------------------------------------------------------------------------
def test_equal_areas_the_lowest_roots_win():
    p = R.squares(12, 30, [3] * 5)
    for k in (1, 2):
        got = _binary_case(p[None, None], keep_largest=k)
        assert got[2][0, 0, :2].tolist() == [5, k] and got[3][0, 0, :k, 7].tolist() == [31 + 5 * r for r in range(k)]


def test_min_area_boundary_twelve_components_and_keep_eight():
    p = R.squares(20, 40, [3, 2, 3, 2])                       # areas 9 and 4
    got = _binary_case(p[None, None], min_area=9)
    assert got[2][0, 0, :2].tolist() == [4, 2]                # area == min_area stays
    assert _binary_case(p[None, None], min_area=10)[2][0, 0, :6].tolist() == [4, 0, 26, 0, 0, 0]
    assert _binary_case(p[None, None], min_area=5)[2][0, 0, 1] == 2          # area == min_area - 1 goes
    twelve = R.squares(33, 70, [1, 2, 3, 4, 5, 6, 6, 5, 4, 3, 2, 1])
    got = _binary_case(twelve[None, None])
    assert got[2][0, 0, :2].tolist() == [12, 12] and got[3][0, 0, :, 0].tolist() == [36, 36, 25, 25, 16, 16, 9, 9]
    three = R.squares(20, 40, [2, 4, 3])
    got = _binary_case(three[None, None], keep_largest=8)
    assert got[2][0, 0, :2].tolist() == [3, 3] and got[3][0, 0, :, 0].tolist() == [16, 9, 4, 0, 0, 0, 0, 0]


# ---- 4. holes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.holes()))
def test_holes(name):
    p = R.holes()[name]
    inner = 16 * 35
    filled = {"ring": inner, "ring_in_ring": 27 * 57 - 88, "diagonal_gap": inner, "straight_gap": 0, "u_at_edge": 0, "fill_joins": 9 * 19 - 12}[name]
    for conn in (1, 2):
        got = _binary_case(p[None, None], what=name, connectivity=conn, fill_holes=True)
        assert got[2][0, 0, 4] == filled
    if name == "fill_joins":
        assert got[2][0, 0, 0] == 1 and _binary_case(p[None, None], connectivity=2)[2][0, 0, 0] == 2


# ---- 5. class mode -------------------------------------------------------------------------------------------------------------------
def _class_logits():
    x = R.blobs((2, 4, 21, 70), 9, sigma=1.5)
    x[:, :, 3:6, 10:30] = 0.25                                # ties of all four classes: class 0
    x[0, 1:3, 10:14, 40:60] = 9.0                             # ties of classes 1 and 2: class 1
    x[1, :, 2:19, 5:40] = -1.0                                # a block of class 2 with a core of class 1 that holds class 0
    x[1, 2, 2:19, 5:40] = 2.0
    x[1, 1, 7:13, 15:30] = 4.0
    x[1, 0, 9:11, 20:24] = 6.0
    return x


@pytest.mark.parametrize("background", [False, True], ids=["nobg", "bg"])
def test_class_mode_with_ties_and_class_map(background):
    x = _class_logits()
    for kw in (dict(), dict(fill_holes=True), dict(connectivity=2, fill_holes=True, min_area=100, keep_largest=2)):
        pp = MaskPostprocess(include_background=background, **kw)
        pp(torch.from_numpy(x).to(DEV))
        got = _get(pp)
        want = R.classes(x, include_background=background, **kw)
        _equal(got, want, what=str(kw))
        assert got[0].shape[1] == (4 if background else 3) and not got[2][..., 6:].any()
    first = 0 if background else 1
    cmap = got[4]
    assert cmap[1, 10, 22] == 2 and cmap[1, 8, 16] == 2 and cmap[1, 3, 6] == 2       # class 1's core (area 82) was dropped: a hole of 2
    pp = MaskPostprocess(include_background=background, fill_holes=True)
    pp(torch.from_numpy(x).to(DEV))
    cmap = _get(pp)[4]
    assert cmap[1, 8, 16] == 1 and cmap[1, 10, 22] == (0 if background else 1) and cmap[0, 11, 45] == 1
    assert pp.mask.shape[1] == 4 - first and (not background or cmap[0, 4, 12] == 0)


# ---- 6. limits, walking, reproducibility, capture ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 4096), (4096, 8)])
def test_longest_pictures(shape):
    H, W = shape
    p = np.zeros(shape, dtype=bool)
    if W > H:
        p[3, :] = True
        p[5, 100:4000] = True
    else:
        p[:, 3] = True
        p[100:4000, 5] = True
    got = _binary_case(p[None, None], keep_largest=1)
    assert got[2][0, 0, :6].tolist() == [2, 1, 4096 + 3900, 4096, 0, 4096]
    _binary_case(p[None, None], connectivity=2, fill_holes=True)


def test_workgroups_walk_several_units():
    shape = (4, 4, 130, 261)
    pp = MaskPostprocess(connectivity=2, fill_holes=True, min_area=4, keep_largest=3)
    grid, units = ops.postproc_grid(pp.describe(_lib.POST_BINARY, shape))
    assert units > grid > 0, (grid, units)                    # the smallest (N, C) at this size above the cap of 2048 workgroups
    assert ops.postproc_grid(pp.describe(_lib.POST_BINARY, (4, 3) + shape[2:]))[1] <= grid
    x = torch.from_numpy(R.blobs(shape, 21, sigma=2.0))
    pp(x.to(DEV), mode="binary")
    _equal(_get(pp)[:4], R.binary(x.numpy(), 0.0, connectivity=2, fill_holes=True, min_area=4, keep_largest=3))


def test_two_calls_are_identical_and_a_replay_equals_the_eager_call(blob_logits):
    x = blob_logits.to(DEV)
    pp = MaskPostprocess(connectivity=2, fill_holes=True, min_area=5, keep_largest=3)
    pp(x, mode="binary")
    first = [a.copy() for a in _get(pp)[:4]]
    pp(x, mode="binary")
    _equal(_get(pp)[:4], first, what="second call")
    g = torch.cuda.CUDAGraph()
    for t in (pp.mask, pp.labels, pp.stats, pp.comps):
        t.fill_(77)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            pp(x, mode="binary")
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        g.replay()
    _equal(_get(pp)[:4], first, what="replay")


# ---- 7. uz_tta_merge and uz_flip_views -------------------------------------------------------------------------------------------------
FLIPS = {1: (), 2: (3,), 4: (2,), 8: (2, 3)}       # view bit -> torch.flip dims


def _views_of(bits):
    return [b for b in (1, 2, 4, 8) if bits & b]


def _flip(t, bit):
    return torch.flip(t, FLIPS[bit]) if FLIPS[bit] else t


def test_flip_views_are_torch_flip():
    x = torch.randn(2, 3, 24, 40, generator=torch.Generator().manual_seed(5)).to(DEV)
    for bits in range(1, 16):
        out = [torch.empty_like(x) for _ in _views_of(bits)]
        ops.flip_views(x, bits, out)
        torch.cuda.synchronize()
        for o, b in zip(out, _views_of(bits)):
            assert torch.equal(o, _flip(x, b)), (bits, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mode", [_lib.POST_BINARY, _lib.POST_CLASS], ids=["sigmoid", "softmax"])
def test_tta_merge_against_float64(mode, dtype):
    N, C, H, W = 2, (3 if mode == _lib.POST_BINARY else 5), 24, 40
    worst, left_out, pixels = 0.0, 0, 0
    for bits in range(1, 16):                                  # every subset of views
        vs = _views_of(bits)
        g = torch.Generator().manual_seed(100 + bits)
        logits = [(3.0 * torch.randn(N, C, H, W, generator=g)).to(dtype) for _ in vs]
        prob = torch.empty(N, C, H, W, dtype=torch.float32, device=DEV)
        ops.tta_merge([t.to(DEV) for t in logits], bits, mode, prob)
        again = torch.empty_like(prob)
        ops.tta_merge([t.to(DEV) for t in logits], bits, mode, again)
        torch.cuda.synchronize()
        assert torch.equal(prob, again)                        # a fixed sum: bit-reproducible
        parts = [_flip(torch.sigmoid(t.double()) if mode == _lib.POST_BINARY else torch.softmax(t.double(), 1), b) for t, b in zip(logits, vs)]
        ref = sum(parts) / len(vs)
        r32 = ref.float().double()
        ulp = torch.from_numpy(np.spacing(np.abs(ref.float().numpy()))).double()
        dist = ((prob.cpu().double() - r32).abs() / ulp).max().item()
        worst = max(worst, dist)
        # the decisions on prob against the reference's, except where the reference itself is within 1e-5 of undecided
        if mode == _lib.POST_BINARY:
            mask = torch.empty(N, C, H, W, dtype=torch.uint8, device=DEV)
            ops.mask_decide(prob, mode, 0.5, 0, mask, None)
            sure = (ref - 0.5).abs() >= 1e-5
            same = mask.cpu().bool() == (ref > 0.5)
        else:
            mask = torch.empty(N, C - 1, H, W, dtype=torch.uint8, device=DEV)
            cmap = torch.empty(N, H, W, dtype=torch.uint8, device=DEV)
            ops.mask_decide(prob, mode, 0.5, 1, mask, cmap)
            top2 = ref.topk(2, dim=1).values
            sure = (top2[:, 0] - top2[:, 1]) >= 1e-5
            am = ref.argmax(1)
            same = cmap.cpu().long() == am
            onehot = torch.stack([am == c for c in range(1, C)], 1)
            assert torch.equal(mask.cpu().bool()[sure[:, None].expand_as(onehot)], onehot[sure[:, None].expand_as(onehot)])
        assert bool(same[sure].all()), bits
        left_out += int((~sure).sum())
        pixels += sure.numel()
    print(f"tta_merge {mode=} {dtype}: largest distance {worst:.3f} float32 ulp, left out {left_out} of {pixels}")
    assert left_out < 0.001 * pixels
    assert worst <= PROB_ULP, worst


# ---- 8. GraphedPredict -----------------------------------------------------------------------------------------------------------------
def _make(name, dtype, num_classes=1, in_channels=3, **kw):
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model(name, in_channels=in_channels, num_classes=num_classes, **kw)
    m.run_dtype = dtype
    return m.to(DEV).eval()


def _centre(m, x):
    """move the head's bias so that the logits of x straddle zero: a freshly initialised unet predicts one empty mask"""
    with torch.no_grad():
        med = _main(m(x)).float().median()
        bias = [p for n, p in m.named_parameters() if n.endswith("bias") and p.numel() == 1][-1]
        bias -= med
    return m


def _main(outputs):
    if isinstance(outputs, dict):
        return next(iter(outputs.values()))
    if isinstance(outputs, (list, tuple)):
        return outputs[-1]
    return outputs


def _x(B=2, C=3, H=64, W=64, seed=1):
    return torch_ref.synthetic_batch(B, C, H, W, seed=seed)[0].to(DEV)


def _by_hand(m, x, bits, pp, mode):
    """eager forwards of torch.flip'ped inputs, ops.tta_merge, then the post-process call"""
    with torch.no_grad():
        mains = [_main(m(_flip(x, b).contiguous())).contiguous() for b in _views_of(bits)]
    prob = torch.empty(mains[0].shape, dtype=torch.float32, device=DEV)
    ops.tta_merge(mains, bits, mode, prob)
    mask = pp(prob, mode="binary" if mode == _lib.POST_BINARY else "class", from_logits=False).clone()
    torch.cuda.synchronize()
    return prob, mask, pp.labels.clone(), pp.stats.clone(), pp.comps.clone(), (pp.class_map.clone() if pp.class_map is not None else None)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_unet_replay_equals_the_composition_by_hand(dtype):
    x = _x()
    m = _centre(_make("unet", dtype), x)
    kw = dict(connectivity=2, fill_holes=True, min_area=4, keep_largest=2)
    want = _by_hand(m, x, 7, MaskPostprocess(**kw), _lib.POST_BINARY)
    pred = GraphedPredict(m, tta=("hflip", "vflip"), postprocess=MaskPostprocess(**kw))
    for _ in range(2):                                         # the capture's first replay, then a plain replay
        mask = pred(x)
        torch.cuda.synchronize()
        pred.check()
        for g, w in zip((pred.prob, mask, pred.labels, pred.stats, pred.comps), want):
            assert torch.equal(g, w)
    assert pred.class_map is None and pred.captures == 1 and "3 x fwd" in pred.describe()
    assert torch.equal(_main(pred.outputs), _main(m(x)))
    # no views, no post-process: the mask is GraphedEval's outputs > 0
    plain = GraphedPredict(m)
    mask = plain(x)
    ev = unet_zoo_amd.GraphedEval(m, "bce_dice")
    ev(x, torch.zeros(2, 1, 64, 64, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(mask.bool(), _main(ev.outputs) > 0) and plain.labels is None and plain.stats is None
    assert 0 < int(mask.sum()) < mask.numel()
    # a second input shape captures a second graph; the first one is still there
    x2 = _x(H=32, W=96, seed=3)
    m2 = plain(x2)
    torch.cuda.synchronize()
    assert plain.captures == 2 and tuple(m2.shape) == (2, 1, 32, 96) and torch.equal(m2.bool(), _main(m(x2)) > 0)
    plain(x)
    assert plain.captures == 2
    masks = list(plain.predict([x, (x2, None), x]))
    assert [tuple(k.shape) for k in masks] == [(2, 1, 64, 64), (2, 1, 32, 96), (2, 1, 64, 64)] and torch.equal(masks[0], masks[2])


def test_an_optimizer_step_between_two_calls_is_seen():
    x = _x()
    m = _centre(_make("unet", torch.float32), x)
    t = torch_ref.synthetic_batch(2, 3, 64, 64, seed=1)[1].to(DEV)
    pred = GraphedPredict(m, tta=("hflip",), postprocess=MaskPostprocess(min_area=2))
    pred(x)
    torch.cuda.synchronize()
    prob0 = pred.prob.clone()
    m.train()
    step = unet_zoo_amd.GraphedStep(m, "bce_dice", lr=1e-2)
    step(x, t)
    m.eval()
    want = _by_hand(m, x, 3, MaskPostprocess(min_area=2), _lib.POST_BINARY)
    mask = pred(x)
    torch.cuda.synchronize()
    assert not torch.equal(pred.prob, prob0)
    assert torch.equal(pred.prob, want[0]) and torch.equal(mask, want[1]) and torch.equal(pred.labels, want[2])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_a_parameter_on_new_storage_is_read_there(dtype):
    """storage that moves without GraphedStep: the new capture must read the new addresses (tests/storage_move.py)"""
    x = _x()
    m = _centre(_make("unet", dtype), x)
    pred = GraphedPredict(m, tta=("hflip",), postprocess=MaskPostprocess(min_area=2))
    pred(x)
    torch.cuda.synchronize()
    prob0 = pred.prob.clone()
    kept = move_two_weights(m)
    want = _by_hand(twin_of(m, lambda: _make("unet", dtype)), x, 3, MaskPostprocess(min_area=2), _lib.POST_BINARY)
    mask = pred(x)
    torch.cuda.synchronize()
    assert pred.captures == 2 and len(kept) == 2
    assert torch.equal(pred.prob, want[0]) and torch.equal(mask, want[1]) and torch.equal(pred.labels, want[2])
    assert not torch.equal(pred.prob, prob0)
    # ... and so does the moved model's own eager forward from now on
    again = _by_hand(m, x, 3, MaskPostprocess(min_area=2), _lib.POST_BINARY)
    assert all(torch.equal(a, w) for a, w in zip(again[:3], want[:3]))


@pytest.mark.parametrize("name,kw", [("u2net", {}), ("nested_unet", {"deep_supervision": True})])
def test_the_main_map_of_a_container_is_used(name, kw):
    m = _make(name, torch.float32, **kw)
    x = _x()
    want = _by_hand(m, x, 9, MaskPostprocess(keep_largest=1), _lib.POST_BINARY)
    pred = GraphedPredict(m, tta=("hvflip",), postprocess=MaskPostprocess(keep_largest=1))
    mask = pred(x)
    torch.cuda.synchronize()
    pred.check()
    assert isinstance(pred.outputs, (dict, list, tuple))
    assert torch.equal(pred.prob, want[0]) and torch.equal(mask, want[1]) and torch.equal(pred.comps, want[4])


def test_four_classes_end_to_end():
    m = _make("unet", torch.float32, num_classes=4)
    x = _x()
    kw = dict(fill_holes=True, min_area=3)
    want = _by_hand(m, x, 15, MaskPostprocess(**kw), _lib.POST_CLASS)
    pred = GraphedPredict(m, tta=("hflip", "vflip", "hvflip"), postprocess=MaskPostprocess(**kw))
    mask = pred(x)
    torch.cuda.synchronize()
    pred.check()
    assert tuple(mask.shape) == (2, 3, 64, 64) and tuple(pred.class_map.shape) == (2, 64, 64)
    for g, w in zip((pred.prob, mask, pred.labels, pred.stats, pred.comps, pred.class_map), want):
        assert torch.equal(g, w)
    ref = R.classes(pred.prob.cpu().numpy(), **kw)
    for g, w in zip((mask, pred.labels, pred.stats, pred.comps, pred.class_map), ref):
        assert np.array_equal(g.cpu().numpy(), w)
    plain = GraphedPredict(m)                                  # one view, no post-process: the argmax of the logits
    mk = plain(x)
    torch.cuda.synchronize()
    am = _main(m(x)).argmax(1)
    assert torch.equal(plain.class_map.long(), am) and torch.equal(mk.bool(), torch.stack([am == c for c in (1, 2, 3)], 1))


def test_vnet_runs_and_its_statistics_advance_once_per_view():
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model("vnet", in_channels=1, num_classes=1)
    m.run_dtype = torch.float32
    m = m.to(DEV).eval()
    x = torch_ref.synthetic_batch(2, 1, 32, 32, seed=2)[0].to(DEV)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        a = m(x).clone()
        b = m(torch.flip(x, (3,)).contiguous()).clone()
    twice = {k: v.clone() for k, v in m.state_dict().items()}
    m.load_state_dict(before)
    pred = GraphedPredict(m, tta=("hflip",))
    mask = pred(x)
    torch.cuda.synchronize()
    want = torch.empty_like(pred.prob)
    ops.tta_merge([a, b], 3, _lib.POST_BINARY, want)
    torch.cuda.synchronize()
    assert torch.equal(pred.prob, want) and torch.equal(mask.bool(), want > 0.5)
    after = m.state_dict()
    assert any(k.endswith("running_mean") and not torch.equal(before[k], after[k]) for k in before)
    assert all(torch.equal(after[k], twice[k]) for k in before)          # exactly two forwards' updates
