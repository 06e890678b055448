"""GPU: SurfaceMetrics (uz_surface.hip) against the numpy restatement tests/surface_ref.py (pinned to scipy and
numpy.percentile by tests/test_surface_metrics.py), eagerly and inside GraphedEval's graph.

Acceptance.  The int64 statistics (surface sizes, max d2, the two order statistics, state, mask sizes) are EQUAL to the
reference's.  The float32 values lie within 1 float32 ulp of float32(reference float64) for hd and hdq and within 2 ulp for
assd: the only inexact steps are float64 sqrt / interpolation / sums and one rounding to float32.

Every case is generated from fixed seeds and compared; none is skipped, except test_workgroups_walk_several_units, which
skips when the launch plan does not cap the grid at its shape (then no workgroup walks and the test would show nothing)."""
import numpy as np
import pytest
import torch

import surface_ref as R  # tests/surface_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from unet_zoo_amd import _lib, ops
from unet_zoo_amd.loss import MulticlassLoss
from unet_zoo_amd.surface import SurfaceMetrics

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _logits_of(mask: np.ndarray, seed: int = 0) -> torch.Tensor:
    """fp32 logits whose sign is the mask, of varying size"""
    g = torch.Generator().manual_seed(seed)
    mag = 0.25 + torch.rand(mask.shape, generator=g)
    return torch.where(torch.from_numpy(mask), mag, -mag)


def _run(m: SurfaceMetrics, x: torch.Tensor, t: torch.Tensor):
    out, stats = m(x.to(DEV), t.to(DEV))
    torch.cuda.synchronize()
    return out.cpu().numpy(), stats.cpu().numpy()


def _check(got_out, got_stats, want_out, want_stats, what=""):
    """statistics equal; hd, hdq within 1 float32 ulp and assd within 2 of the rounded reference; the fourth value 0"""
    assert got_stats.shape == want_stats.shape and got_out.shape == want_out.shape[:-1] + (4,)
    assert np.array_equal(got_stats, want_stats), (what, got_stats.tolist(), want_stats.tolist())
    err = np.abs(got_out[..., :3].astype(np.float64) - want_out.astype(np.float32).astype(np.float64)) / R.ulp32(want_out)
    print(f"{what}: errors in float32 ulp: hd {err[..., 0].max():.2f}, hdq {err[..., 1].max():.2f}, assd {err[..., 2].max():.2f}")
    assert err[..., 0].max() <= 1.0 and err[..., 1].max() <= 1.0 and err[..., 2].max() <= 2.0, (what, err.tolist())
    assert not got_out[..., 3].any()


def _binary_case(pred: np.ndarray, targ: np.ndarray, q=95.0, spacing=1.0, what=""):
    x, t = _logits_of(pred), torch.from_numpy(targ).float()
    got = _run(SurfaceMetrics(percentile=q, spacing=spacing), x, t)
    want = R.binary(x.numpy(), t.numpy(), q, spacing)
    _check(*got, *want, what=what)
    return got, want


# ---- 1. binary, odd shape, blobs on the picture's edge, rows without any surface pixel ------------------------------------------
def test_binary_odd_shape_edges_and_empty_rows():
    H, W = 37, 53
    pred, targ = np.zeros((2, 1, H, W), dtype=bool), np.zeros((2, 1, H, W), dtype=bool)
    pred[0, 0] = R.blobs((H, W), 11, count=3)
    targ[0, 0] = R.blobs((H, W), 12, count=3)
    pred[0, 0, :6, :9] = True                 # a corner block: foreground on the picture's edge is surface
    targ[0, 0, -5:, 20:] = True               # ... and a block along the bottom and right edges
    pred[1, 0, 15:19, 30:41] = True           # rows 0 .. 14 and 21 .. 36 hold no surface pixel of either mask
    targ[1, 0, 17:21, 3:9] = True
    (out, stats), _ = _binary_case(pred, targ, what="37 x 53")
    assert (stats[..., 5] == 0).all() and (stats[..., 0] > 0).all()


# ---- 2. binary, prediction and target far apart; a channel of identical masks ---------------------------------------------------
def test_binary_far_apart_and_identical():
    H, W = 96, 160
    yy, xx = np.mgrid[:H, :W]
    pred, targ = np.zeros((1, 2, H, W), dtype=bool), np.zeros((1, 2, H, W), dtype=bool)
    pred[0, 0] = (yy - 20) ** 2 + (xx - 18) ** 2 <= 11 ** 2
    targ[0, 0] = (yy - 70) ** 2 + (xx - 135) ** 2 <= 14 ** 2
    pred[0, 1] = targ[0, 1] = R.blobs((H, W), 5, count=4)
    (out, stats), _ = _binary_case(pred, targ, what="96 x 160")
    assert stats[0, 0, 3] > 2 ** 10 and stats[0, 0, 2] > 2 ** 13          # both histogram levels are used
    assert not out[0, 1].any() and stats[0, 1, 2:6].tolist() == [0, 0, 0, 0] and stats[0, 1, 0] == stats[0, 1, 1] > 0


# ---- 3. a very wide picture: d2 above 2^20 ----------------------------------------------------------------------------------------
def test_very_wide_picture():
    H, W = 8, 1500
    pred, targ = np.zeros((1, 1, H, W), dtype=bool), np.zeros((1, 1, H, W), dtype=bool)
    pred[0, 0, 1:4, 2:7] = True
    targ[0, 0, 3:8, 1489:1497] = True
    pred[0, 0, 6, 40] = True
    (out, stats), _ = _binary_case(pred, targ, what="8 x 1500")
    assert stats[0, 0, 2] > 2 ** 20 and stats[0, 0, 3] > 2 ** 20


# ---- 4. rank edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,q", [("n2", 95.0), ("n2", 100.0), ("n3", 95.0), ("n3", 50.0), ("n3", 100.0), ("n5", 50.0), ("n5", 75.0),
                                     ("n5", 95.0), ("n5", 100.0), ("n5", 0.5)])
def test_rank_edges(case, q):
    H, W = 5, 20
    pred, targ = np.zeros((1, 1, H, W), dtype=bool), np.zeros((1, 1, H, W), dtype=bool)
    if case == "n2":                          # one pixel against one pixel
        pred[0, 0, 1, 2] = targ[0, 0, 4, 6] = True
    elif case == "n3":                        # one pixel against two
        pred[0, 0, 1, 2] = targ[0, 0, 4, 6] = targ[0, 0, 0, 17] = True
    else:                                     # three against two: n = 5, so q = 50 and q = 75 have f = 0
        pred[0, 0, 2, 2:5] = True
        targ[0, 0, 2, 10:12] = True
    (out, stats), _ = _binary_case(pred, targ, q=q, spacing=1.5, what=f"{case} q = {q}")
    assert stats[0, 0, 0] + stats[0, 0, 1] == int(case[1:])
    if case == "n5" and q == 50.0:
        assert stats[0, 0, 3] == 49 and out[0, 0, 1] == np.float32(1.5 * 7.0)


# ---- 5. empty masks: states 1, 2, 3 beside a valid image ---------------------------------------------------------------------------
def test_states():
    H, W = 24, 40
    a, b = R.blobs((H, W), 21), R.blobs((H, W), 22)
    z = np.zeros((H, W), dtype=bool)
    pred, targ = np.stack([z, a, a, z])[:, None], np.stack([b, b, z, z])[:, None]
    (out, stats), _ = _binary_case(pred, targ, what="states")
    assert stats[:, 0, 5].tolist() == [1, 0, 2, 3]
    assert not out[[0, 2, 3]].any() and out[1, 0, 0] > 0
    alone, _ = _binary_case(pred[1:2], targ[1:2], what="the valid image alone")
    assert np.array_equal(alone[0][0], out[1]) and np.array_equal(alone[1][0], stats[1])


# ---- 6. class indices ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("include_background", [False, True])
def test_class_mode(include_background):
    N, K, H, W = 2, 3, 40, 72
    labels = np.zeros((N, H, W), dtype=np.int64)
    shown = np.zeros((N, H, W), dtype=np.int64)       # what the logits favour: the labels' blobs, moved
    for n in range(N):
        for c in (1, 2):
            labels[n][R.blobs((H, W), 30 + 2 * n + c, count=2, rmax=0.2)] = c
            shown[n][R.blobs((H, W), 40 + 2 * n + c, count=2, rmax=0.2)] = c
    g = torch.Generator().manual_seed(9)
    logits = 0.1 * torch.rand(N, K, H, W, generator=g)
    logits += 2.0 * torch.nn.functional.one_hot(torch.from_numpy(shown), K).permute(0, 3, 1, 2)
    logits[:, :, 5:9, 50:60] = 0.5                    # all classes equal: class 0
    logits[:, 1:, 20:24, 30:44] = 3.0                 # classes 1 and 2 equal above class 0: class 1
    labels[:, :, 10:14] = -100                        # an ignored stripe
    labels[0, 3, 3], labels[1, 30, 60], labels[1, 31, 60] = 5, -3, 3
    m = SurfaceMetrics(include_background=include_background)
    got = _run(m, logits, torch.from_numpy(labels))
    want = R.classes(logits.numpy(), labels, first_class=0 if include_background else 1)
    _check(*got, *want, what=f"classes, include_background={include_background}")
    assert got[0].shape == (N, K - (0 if include_background else 1), 4) and (got[1][..., 5] == 0).all()
    # (N, 1, H, W) int32 labels are the same call
    got2 = _run(m, logits, torch.from_numpy(labels)[:, None].int())
    assert np.array_equal(got2[0], got[0]) and np.array_equal(got2[1], got[1])
    assert torch.equal(m.hdq.cpu(), torch.from_numpy(got[0][..., 1])) and torch.equal(m.state.cpu(), torch.from_numpy(got[1][..., 5]))


# ---- 7. workgroups walk several units ---------------------------------------------------------------------------------------------
def test_workgroups_walk_several_units():
    N, C, H, W = 4, 4, 130, 131          # the smallest (pairs, picture) of the plan with more units than the grid's cap
    grid, units = ops.surface_grid(SurfaceMetrics().describe(_lib.SURFACE_BINARY, (N, C, H, W)))
    if units <= grid:
        pytest.skip(f"the launch plan does not cap the grid at this shape ({grid} workgroups for {units} units)")
    assert units == 2 * N * C * 67 and units > grid
    pred = np.stack([R.blobs((H, W), 100 + k, count=2) for k in range(N * C)]).reshape(N, C, H, W)
    targ = np.stack([R.blobs((H, W), 200 + k, count=2) for k in range(N * C)]).reshape(N, C, H, W)
    _binary_case(pred, targ, what="walk")


# ---- 8. determinism and capture ---------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical():
    pred = np.stack([R.blobs((61, 67), 50 + k) for k in range(6)]).reshape(2, 3, 61, 67)
    targ = np.stack([R.blobs((61, 67), 60 + k) for k in range(6)]).reshape(2, 3, 61, 67)
    noise = np.random.RandomState(3).rand(*pred.shape) < 0.2
    x, t = _logits_of(pred ^ noise).to(DEV), torch.from_numpy(targ).float().to(DEV)
    m = SurfaceMetrics()
    o1, s1 = (v.clone() for v in m(x, t))
    o2, s2 = m(x, t)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2) and torch.equal(s1, s2) and (s1[..., 5] == 0).all()


def _unet(dtype, x):
    """a seeded unet in eval mode whose logits at x are of both signs (the head's bias is moved to their median)"""
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=1)
    m.run_dtype = dtype
    m = m.to(DEV).eval()
    with torch.no_grad():
        m.out.conv.bias -= m(x).float().median()
    return m


def _batch(seed, B=2, H=64, W=64, empty=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, H, W, generator=g)
    t = torch.from_numpy(np.stack([R.blobs((H, W), 1000 * seed + k) for k in range(B)])[:, None]).float()
    if empty is not None:
        t[empty] = 0.0
    return x.to(DEV), t.to(DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("criterion", ["bce_dice", "callable"])
def test_graphed_eval_replay_equals_eager(dtype, criterion):
    x, t = _batch(1)
    m = _unet(dtype, x)
    eager = SurfaceMetrics()
    crit = "bce_dice" if criterion == "bce_dice" else (lambda out, tt: torch.nn.functional.binary_cross_entropy_with_logits(out.float(), tt))
    ev = unet_zoo_amd.GraphedEval(m, crit, surface=SurfaceMetrics())
    for seed in (1, 2):                        # the second batch is replayed into the static tensors of the first
        x, t = _batch(seed)
        with torch.no_grad():
            want = [v.clone() for v in eager(m(x), t)]
        ev(x, t)
        torch.cuda.synchronize()
        assert torch.equal(ev.surface[0], want[0]) and torch.equal(ev.surface[1], want[1]), seed
        assert (want[1][..., 5] == 0).any()      # the comparison is of real distances
    assert ev.surface[0].shape == (2, 1, 4) and ev.surface[1].shape == (2, 1, 8)


def test_graphed_eval_with_class_indices():
    torch.manual_seed(0)
    K = 3
    m = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=K)
    m.run_dtype = torch.float32
    m = m.to(DEV).eval()
    x, _ = _batch(4)
    y = torch.from_numpy(np.stack([R.blobs((64, 64), 70 + k) * 1 + R.blobs((64, 64), 80 + k) * 1 for k in range(2)])).to(DEV)
    ev = unet_zoo_amd.GraphedEval(m, MulticlassLoss.ce_dice(), surface=SurfaceMetrics())
    ev(x, y)
    with torch.no_grad():
        want = [v.clone() for v in SurfaceMetrics()(m(x), y)]
    torch.cuda.synchronize()
    assert ev.surface[0].shape == (2, K - 1, 4) and torch.equal(ev.surface[0], want[0]) and torch.equal(ev.surface[1], want[1])


# ---- 9. evaluate ------------------------------------------------------------------------------------------------------------------
def test_evaluate_summary():
    B = 2
    loader = [_batch(5), _batch(6, empty=1), _batch(7)]
    m = _unet(torch.float32, loader[0][0])
    plain = unet_zoo_amd.GraphedEval(m, "bce_dice").evaluate(loader)
    ev = unet_zoo_amd.GraphedEval(m, "bce_dice", surface=SurfaceMetrics(percentile=90.0, spacing=0.5))
    got = ev.evaluate(loader)
    assert got == plain                        # (mean_loss, mean_dice): bit for bit what the pass without surface returns
    s = ev.surface_summary
    vals, states = [], []
    for x, t in loader:
        with torch.no_grad():
            logits = m(x).float().cpu().numpy()
        out, stats = R.binary(logits, t.cpu().numpy(), 90.0, 0.5)
        vals.append(out[:, 0])
        states.append(stats[:, 0, 5])
    vals, states = np.concatenate(vals), np.concatenate(states)
    counts = [int((states == k).sum()) for k in range(4)]
    assert [s["n_valid"], s["n_pred_empty"], s["n_target_empty"], s["n_both_empty"]] == [[c] for c in counts]
    assert sum(counts) == 3 * B * 1 and counts[0] >= 1 and counts[2] + counts[3] == 1 and s["percentile"] == 90.0
    for k, name in enumerate(("hd", "hdq", "assd")):
        want = vals[states == 0, k].mean()
        print(f"{name}: summary {s[name][0]!r}, reference {want!r}")
        assert abs(s[name][0] - want) <= 1e-6 * want, (name, s[name], want)


# ---- 10. multi-output models: the main map ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,extra", [("u2net", {}), ("nested_unet", {"deep_supervision": True})])
def test_multi_output_models(name, extra):
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model(name, in_channels=3, num_classes=1, **extra)
    m.run_dtype = torch.float32
    m = m.to(DEV).eval()
    x, t = _batch(8)
    sm = SurfaceMetrics()
    with torch.no_grad():
        outputs = m(x)
        out, stats = (v.clone() for v in sm(outputs, t))
        main = next(iter(outputs.values())) if isinstance(outputs, dict) else outputs[-1]
        assert isinstance(outputs, (dict, list, tuple)) and len(outputs) > 1
        out1, stats1 = sm(main, t)
    torch.cuda.synchronize()
    assert out.shape == (2, 1, 4) and stats.shape == (2, 1, 8) and out.dtype == torch.float32 and stats.dtype == torch.int64
    assert torch.equal(out, out1) and torch.equal(stats, stats1)
