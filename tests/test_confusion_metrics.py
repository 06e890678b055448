"""CPU: ConfusionMetrics' surface and the checkers of its GPU tests.

The export; the three ABI entries in the header and in the library; every refusal of the ABI without a GPU, with the field
named; every argument check of the class; the edge table; and ``ConfusionMetrics.curves`` (and the plain-loop restatement
tests/confusion_ref.py) pinned against definitions that share no code with either: AUROC against a pairwise count over the binned
scores (and scipy's Mann-Whitney U where scipy is present), AP and the best Dice against a direct loop over thresholds applied to
the scores themselves, and cases derived by hand."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import confusion_ref as R  # tests/confusion_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from unet_zoo_amd import _lib, ops
from unet_zoo_amd.confusion import ConfusionMetrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("uz_confusion_workspace_bytes", "uz_confusion_grid", "uz_confusion_metrics")
BIN, CLS = _lib.CONFUSION_BINARY, _lib.CONFUSION_CLASS


# ---- exports ---------------------------------------------------------------------------------------------------------------------
def test_exports():
    assert unet_zoo_amd.ConfusionMetrics is ConfusionMetrics and "ConfusionMetrics" in unet_zoo_amd.__all__
    header = open(os.path.join(ROOT, "include", "unetzoo_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.EXPORTS and f" {name}(" in header and getattr(raw, name)
    assert "typedef struct uz_confusion_desc" in header and "#define UZ_CONFUSION_BINARY 0" in header and "#define UZ_CONFUSION_CLASS 1" in header
    assert ctypes.sizeof(_lib.ConfusionDesc) == 48
    assert callable(ops.confusion_grid) and callable(ops.confusion_metrics)


# ---- the ABI without a GPU -------------------------------------------------------------------------------------------------------
def _desc(mode=BIN, N=2, C=1, H=16, W=16, first=0, ign=-100, bins=None, maxwg=0):
    return _lib.ConfusionDesc(mode, N, C, H, W, first, ign, (64 if mode == BIN else 0) if bins is None else bins, maxwg)


@pytest.mark.parametrize("kw,word", [
    (dict(mode=2), b"mode"), (dict(mode=-1), b"mode"), (dict(N=0), b"shape"), (dict(C=0), b"shape"), (dict(H=0), b"shape"),
    (dict(W=-3), b"shape"), (dict(H=4097), b"above 4096"), (dict(W=4097), b"above 4096"),
    (dict(mode=CLS, C=1, first=0), b"K ="), (dict(mode=CLS, C=33, first=1), b"K ="), (dict(mode=CLS, C=3, first=3), b"first_class"),
    (dict(mode=CLS, C=3, first=-1), b"first_class"), (dict(mode=CLS, C=3, first=1, bins=64), b"bins"),
    (dict(bins=0), b"bins"), (dict(bins=8), b"bins"), (dict(bins=2048), b"bins"), (dict(bins=48), b"bins"), (dict(bins=-16), b"bins"),
    (dict(maxwg=-1), b"max_workgroups"), (dict(mode=CLS, C=3, first=1, maxwg=-7), b"max_workgroups"),
    (dict(N=128, C=1, H=4096, W=4096), b"too large"), (dict(mode=CLS, N=8, C=16, first=1, H=4096, W=4096), b"too large")])
def test_bad_descriptor_is_rejected_without_a_gpu(kw, word):
    lib = _lib.load()
    d = _desc(**kw)
    assert lib.uz_confusion_workspace_bytes(ctypes.byref(d)) == -1 and word in lib.uz_last_error_string()
    assert lib.uz_confusion_grid(ctypes.byref(d), None) == -1 and word in lib.uz_last_error_string()
    # the launch entry point makes the same check before it touches a pointer
    assert lib.uz_confusion_metrics(ctypes.byref(d), None, None, None, None, None, None, None, None) == -1
    assert word in lib.uz_last_error_string()


# logits, target, edges, counts, hist, out, workspace: never read
GOOD = [0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x10000000]


def test_null_pointers_misalignment_and_overlaps_are_refused_without_a_gpu():
    lib = _lib.load()
    assert lib.uz_confusion_workspace_bytes(None) == -1 and b"null descriptor" in lib.uz_last_error_string()
    assert lib.uz_confusion_grid(None, None) == -1 and b"null descriptor" in lib.uz_last_error_string()
    assert lib.uz_confusion_metrics(None, *([None] * 8)) == -1 and b"null descriptor" in lib.uz_last_error_string()
    d = _desc()
    for k, word in ((0, b"null pointer"), (1, b"null pointer"), (2, b"null edges"), (3, b"null pointer"), (4, b"null hist"),
                    (5, b"null pointer"), (6, b"null pointer")):
        args = list(GOOD)
        args[k] = None
        assert lib.uz_confusion_metrics(ctypes.byref(d), *args, None) == -1 and word in lib.uz_last_error_string(), k
    for k, off, word in ((0, 2, b"4-byte"), (1, 1, b"4-byte"), (2, 2, b"4-byte"), (3, 4, b"8-byte"), (4, 4, b"8-byte"), (5, 2, b"4-byte"),
                         (6, 8, b"16-byte")):
        args = list(GOOD)
        args[k] += off
        assert lib.uz_confusion_metrics(ctypes.byref(d), *args, None) == -1 and word in lib.uz_last_error_string(), k
    nbytes = 4 * 2 * 16 * 16
    ws = lib.uz_confusion_workspace_bytes(ctypes.byref(d))
    hist_bytes = 8 * 2 * 2 * 64
    for a, b, delta in ((1, 0, 0), (1, 0, nbytes - 4), (2, 0, 16), (3, 1, 8), (5, 3, 0), (3, 5, 8), (0, 6, 16), (5, 6, ws - 16),
                        (4, 2, 0), (2, 4, hist_bytes - 8), (3, 4, hist_bytes - 8), (4, 6, ws - 16), (2, 1, nbytes - 4)):
        args = list(GOOD)
        args[a] = GOOD[b] + delta
        assert lib.uz_confusion_metrics(ctypes.byref(d), *args, None) == -1 and b"overlap" in lib.uz_last_error_string(), (a, b)


def test_class_mode_takes_null_edges_and_hist_and_still_checks_the_rest():
    lib = _lib.load()
    d = _desc(mode=CLS, C=3, first=1)
    args = list(GOOD)
    args[2] = args[4] = None
    args[0] = None
    assert lib.uz_confusion_metrics(ctypes.byref(d), *args, None) == -1 and b"null pointer" in lib.uz_last_error_string()
    args[0] = GOOD[3] + 8                              # logits inside counts (2 x 3 x 3 int64)
    assert lib.uz_confusion_metrics(ctypes.byref(d), *args, None) == -1 and b"overlap" in lib.uz_last_error_string()


def test_workspace_and_launch_plan():
    lib = _lib.load()
    last = 0
    for N, C, H, W in ((1, 1, 1, 1), (2, 1, 8, 8), (2, 3, 37, 53), (16, 3, 256, 256)):
        b = lib.uz_confusion_workspace_bytes(ctypes.byref(_desc(N=N, C=C, H=H, W=W)))
        assert b > last and b % 16 == 0, (N, C, H, W, b)
        last = b
    assert lib.uz_confusion_workspace_bytes(ctypes.byref(_desc(bins=1024))) > lib.uz_confusion_workspace_bytes(ctypes.byref(_desc(bins=16)))
    # a unit is 1024 pixels of a plane: 40 x 40 = 1600 pixels are two
    m = ConfusionMetrics(bins=64)
    assert ops.confusion_grid(m.describe(BIN, (2, 2, 40, 40))) == (8, 8)
    assert ops.confusion_grid(m.describe(BIN, (2, 2, 40, 40), max_workgroups=3)) == (3, 8)
    assert ops.confusion_grid(m.describe(BIN, (2, 2, 40, 40), max_workgroups=1)) == (1, 8)
    assert ops.confusion_grid(m.describe(CLS, (3, 5, 19, 23))) == (3, 3)
    grid, units = ops.confusion_grid(m.describe(BIN, (16, 3, 1024, 1024)))
    assert units == 48 * 1024 and 0 < grid < units


# ---- ConfusionMetrics' own checks (no GPU) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,word", [
    (dict(bins=0), "bins"), (dict(bins=8), "bins"), (dict(bins=48), "bins"), (dict(bins=2048), "bins"), (dict(bins=64.0), "bins"),
    (dict(bins=True), "bins"), (dict(bins=64, thresholds=[0.5] * 63), "not both"),
    (dict(thresholds=[0.1, 0.5, 0.9]), "B - 1 values"), (dict(thresholds="abc"), "sequence of numbers"), (dict(thresholds=5), "sequence of numbers"),
    (dict(thresholds=[0.0] + [k / 16 for k in range(2, 16)]), r"in \(0, 1\)"), (dict(thresholds=[k / 16 for k in range(1, 15)] + [1.0]), r"in \(0, 1\)"),
    (dict(thresholds=[k / 16 for k in range(1, 15)] + [float("nan")]), r"in \(0, 1\)"),
    (dict(thresholds=[k / 16 for k in range(15, 0, -1)]), "strictly ascending"), (dict(thresholds=[0.5] * 15), "strictly ascending"),
    (dict(thresholds=[0.9 + k * 1e-12 for k in range(15)]), "rounded to float32"),
    (dict(ignore_index=2 ** 31), "ignore_index"), (dict(ignore_index=1.5), "ignore_index"), (dict(ignore_index=True), "ignore_index")])
def test_constructor_refuses_bad_arguments_by_name(kw, word):
    with pytest.raises(ValueError, match="ConfusionMetrics: .*" + word):
        ConfusionMetrics(**kw)


def test_call_refuses_bad_tensors_before_any_kernel():
    m = ConfusionMetrics()
    x = torch.zeros(2, 3, 16, 16)
    with pytest.raises(ValueError, match="ConfusionMetrics: logits"):
        m(torch.zeros(2, 16, 16), torch.zeros(2, 16, 16))
    with pytest.raises(ValueError, match="ConfusionMetrics: logits"):
        m(x.double(), torch.zeros(2, 3, 16, 16))
    with pytest.raises(ValueError, match="ConfusionMetrics: outputs and target"):
        m(x, None)
    with pytest.raises(ValueError, match="ConfusionMetrics: empty"):
        m(torch.zeros(0, 3, 16, 16), torch.zeros(0, 3, 16, 16))
    with pytest.raises(ValueError, match="target of shape"):
        m(x, torch.zeros(2, 1, 16, 16))
    with pytest.raises(ValueError, match="target of shape"):
        m(x, torch.zeros(2, 16, 8, dtype=torch.int64))
    with pytest.raises(ValueError, match="K = 1"):
        m(torch.zeros(2, 1, 16, 16), torch.zeros(2, 16, 16, dtype=torch.int64))
    with pytest.raises(ValueError, match="K = 33"):
        m(torch.zeros(1, 33, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="target must be"):
        m(x, torch.zeros(2, 3, 16, 16, dtype=torch.bool))
    with pytest.raises(ValueError, match="at most 4096"):
        m(torch.zeros(1, 1, 1, 4097), torch.zeros(1, 1, 1, 4097))
    with pytest.raises(ValueError, match="max_workgroups"):
        m.describe(BIN, (2, 3, 16, 16), max_workgroups=-1)
    for name in ("dice", "iou", "precision", "recall", "specificity", "state"):
        with pytest.raises(RuntimeError, match="no call yet"):
            getattr(m, name)
    with pytest.raises(_lib.HipLibraryError):                              # good arguments on the CPU: no fallback
        m({"d0": x, "d1": x}, torch.zeros(2, 3, 16, 16))
    with pytest.raises(TypeError, match="ConfusionMetrics"):
        unet_zoo_amd.GraphedEval(unet_zoo_amd.create_model("unet"), confusion=object())
    assert "+confusion" in unet_zoo_amd.GraphedEval(unet_zoo_amd.create_model("unet"), confusion=m).describe()
    assert "confusion" not in unet_zoo_amd.GraphedEval(unet_zoo_amd.create_model("unet")).describe()


def test_descriptor_of_a_shape():
    m = ConfusionMetrics(bins=128, include_background=True, ignore_index=7)
    d = m.describe(BIN, (2, 3, 37, 53))
    assert (d.mode, d.N, d.C, d.H, d.W, d.first_class, d.bins, d.max_workgroups) == (BIN, 2, 3, 37, 53, 0, 128, 0)
    d = m.describe(CLS, (2, 5, 8, 9), max_workgroups=4)
    assert (d.mode, d.C, d.first_class, d.ignore_index, d.bins, d.max_workgroups) == (CLS, 5, 0, 7, 0, 4)
    assert ConfusionMetrics().describe(CLS, (2, 5, 8, 9)).first_class == 1 and ConfusionMetrics().bins == 256


# ---- the edge table --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [16, 1024])
def test_uniform_edges_are_ascending_symmetric_and_zero_in_the_middle(B):
    m = ConfusionMetrics(bins=B)
    e = m.edges.numpy()
    assert e.dtype == np.float32 and e.shape == (B - 1,) and m.edges.device.type == "cpu"
    assert (np.diff(e) > 0).all() and np.isfinite(e).all()
    assert np.array_equal(e, -e[::-1])                   # e_k = -e_{B-k}
    assert e[B // 2 - 1] == 0.0                          # e_{B/2}
    want = np.array([np.float32(math.log(k / (B - k))) for k in range(1, B)], dtype=np.float32)
    assert np.array_equal(e, want) and np.array_equal(e, R.edges_uniform(B))
    assert np.array_equal(m.thresholds.numpy(), np.arange(1, B) / B)


def test_explicit_thresholds_are_mapped_the_same_way():
    p = [0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.98, 0.99]
    m = ConfusionMetrics(thresholds=p)
    assert m.bins == 16 and np.array_equal(m.thresholds.numpy(), np.array(p))
    want = np.array([np.float32(math.log(v / (1.0 - v))) for v in p])
    assert np.abs(m.edges.numpy().astype(np.float64) - want.astype(np.float64)).max() <= np.spacing(np.float32(5.0))
    assert np.array_equal(m.edges.numpy(), R.edges_of(p)) and m.edges[7] == 0.0


def test_reference_bins_are_searchsorted_with_nan_in_bin_zero():
    e = R.edges_uniform(16)
    x = np.array([-np.inf, e[0], np.nextafter(e[0], np.float32(-np.inf)), 0.0, np.nextafter(np.float32(0), np.float32(-1)), e[-1], np.inf,
                  np.nan], dtype=np.float32)
    assert R.bins_of(x, e).tolist() == [0, 1, 0, 8, 7, 15, 15, 0]


# ---- curves against definitions that share no code with them ---------------------------------------------------------------------
def _scores(seed, n=1500, B=32, shift=1.0):
    """binned scores of n pixels and their labels: positives sit `shift` higher in logit space"""
    rng = np.random.RandomState(seed)
    y = rng.rand(n) < 0.3
    x = (rng.randn(n) * 1.5 + np.where(y, shift, -shift)).astype(np.float32)
    e = R.edges_uniform(B)
    b = R.bins_of(x, e)
    hist = np.stack((np.bincount(b[~y], minlength=B), np.bincount(b[y], minlength=B)))
    return b, y, hist, np.arange(1, B) / B


def _both(hist, th):
    """the package's curves and the reference's of one pair, after checking that they agree"""
    got, ref = ConfusionMetrics.curves(hist, th), R.curves(hist, th)
    for k in ("auroc", "ap", "best_dice"):
        assert (math.isnan(got[k]) and math.isnan(ref[k])) or abs(got[k] - ref[k]) <= 1e-12, (k, got[k], ref[k])
    assert got["best_threshold"] == ref["best_threshold"]
    assert np.allclose(got["roc"], ref["roc"], rtol=0, atol=1e-15, equal_nan=True) and np.array_equal(got["reliability"], ref["reliability"])
    return got


@pytest.mark.parametrize("seed,shift", [(0, 1.0), (1, 0.2), (2, 3.0), (3, -0.5)])
def test_auroc_is_the_pairwise_count_on_the_binned_scores(seed, shift):
    b, y, hist, th = _scores(seed, shift=shift)
    got = _both(hist, th)
    bp, bn = b[y][:, None], b[~y][None, :]
    brute = ((bp > bn).sum() + 0.5 * (bp == bn).sum()) / (y.sum() * (~y).sum())
    assert abs(got["auroc"] - brute) <= 1e-12, (got["auroc"], brute)
    try:
        from scipy.stats import mannwhitneyu
    except ImportError:
        return
    u = mannwhitneyu(b[y], b[~y], alternative="two-sided").statistic
    assert abs(got["auroc"] - u / (y.sum() * (~y).sum())) <= 1e-12


@pytest.mark.parametrize("seed,shift", [(4, 1.0), (5, 0.1), (6, 2.5)])
def test_ap_and_best_dice_are_a_direct_loop_over_thresholds(seed, shift):
    B = 32
    b, y, hist, th = _scores(seed, B=B, shift=shift)
    got = _both(hist, th)
    n_pos = int(y.sum())
    ap, prev_recall, best, best_j = 0.0, 0.0, -1.0, None
    for j in range(B - 1, -1, -1):                     # predict positive from bin j on: descending thresholds, recall grows
        pred = b >= j
        tp, fp = int((pred & y).sum()), int((pred & ~y).sum())
        recall = tp / n_pos
        ap += (recall - prev_recall) * (tp / (tp + fp) if tp + fp else 0.0)
        prev_recall = recall
    for j in range(1, B):
        pred = b >= j
        tp, fp, fn = int((pred & y).sum()), int((pred & ~y).sum()), int((~pred & y).sum())
        d = 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0
        if d > best or (d == best and (abs(j - B // 2), j) < (abs(best_j - B // 2), best_j)):
            best, best_j = d, j
    assert abs(got["ap"] - ap) <= 1e-12 and abs(got["best_dice"] - best) <= 1e-15 and got["best_threshold"] == th[best_j - 1]
    assert np.array_equal(got["reliability"][:, 0], np.bincount(b[y], minlength=B))
    assert np.array_equal(got["reliability"][:, 1], np.bincount(b, minlength=B))


def test_hand_derived_curves():
    B = 16
    th = np.arange(1, B) / B
    # a perfect separator: negatives in bins 0 .. 3, positives in bins 12 .. 15
    h = np.zeros((2, B), dtype=np.int64)
    h[0, :4] = [5, 1, 1, 3]
    h[1, 12:] = [2, 2, 2, 4]
    got = _both(h, th)
    assert got["auroc"] == 1.0 and got["ap"] == 1.0 and got["best_dice"] == 1.0
    assert got["best_threshold"] == 0.5                 # every j in 4 .. 12 separates: the one nearest B / 2 = 8 is 8
    assert got["roc"][0].tolist() == [0.0, 0.0] and got["roc"][-1].tolist() == [1.0, 1.0] and got["roc"].shape == (B + 1, 2)
    # the inverted separator
    got = _both(h[::-1].copy(), th)
    assert got["auroc"] == 0.0
    # from the top: bins 15 .. 12 bring the ten negatives, then bins 3, 2, 1, 0 bring 3, 1, 1, 5 positives
    assert got["ap"] == pytest.approx(0.3 * 3 / 13 + 0.1 * 4 / 14 + 0.1 * 5 / 15 + 0.5 * 10 / 20, abs=1e-15)
    assert got["best_dice"] == pytest.approx(2 * 5 / (2 * 5 + 10 + 5))      # j = 1: TP = 5 (bins 1 .. 3), FP = 10, FN = 5
    assert got["best_threshold"] == th[0]
    # all positives: no negatives, auroc is nan, ap = 1
    h = np.zeros((2, B), dtype=np.int64)
    h[1, 3], h[1, 9] = 4, 6
    got = _both(h, th)
    assert math.isnan(got["auroc"]) and got["ap"] == 1.0 and np.isnan(got["roc"][:, 0]).all() and got["roc"][-1, 1] == 1.0
    assert got["best_dice"] == 1.0 and got["best_threshold"] == th[2]       # j = 1, 2, 3 take every positive; 3 is nearest 8
    # all negatives: no positives, auroc and ap are nan, best dice 0 at the middle
    got = _both(h[::-1].copy(), th)
    assert math.isnan(got["auroc"]) and math.isnan(got["ap"]) and got["best_dice"] == 0.0 and got["best_threshold"] == 0.5
    # one occupied bin: every pair is a tie
    h = np.zeros((2, B), dtype=np.int64)
    h[0, 6], h[1, 6] = 30, 10
    got = _both(h, th)
    assert got["auroc"] == 0.5 and got["ap"] == 0.25 and got["best_dice"] == pytest.approx(2 * 10 / (2 * 10 + 30))
    assert got["best_threshold"] == th[5]               # j = 1 .. 6 all give that Dice: 6 is nearest 8
    assert got["reliability"][6].tolist() == [10, 40] and got["reliability"].sum() == 50
    # several pairs at once are the pairs one by one
    many = np.stack([_scores(s)[2] for s in range(3)])
    th32 = np.arange(1, 32) / 32
    got = ConfusionMetrics.curves(many, th32)
    for p in range(3):
        one = ConfusionMetrics.curves(many[p], th32)
        for k in ("auroc", "ap", "best_dice", "best_threshold"):
            assert got[k][p] == one[k]
        assert np.array_equal(got["roc"][p], one["roc"])
    with pytest.raises(ValueError, match="thresholds"):
        ConfusionMetrics.curves(many, th)
    with pytest.raises(ValueError, match=r"\(P, 2, B\)"):
        ConfusionMetrics.curves(np.zeros((3, B)), th)


def test_scores_follow_the_kernel_rules():
    s = ConfusionMetrics.scores([3, 0, 0, 0], [1, 2, 0, 0], [2, 0, 5, 0], [10, 4, 1, 0])
    assert s["dice"].tolist() == [6 / 9, 0.0, 0.0, 1.0] and s["iou"].tolist() == [0.5, 0.0, 0.0, 1.0]
    assert s["precision"].tolist() == [0.75, 0.0, 0.0, 0.0] and s["recall"].tolist() == [0.6, 0.0, 0.0, 0.0]
    assert s["specificity"].tolist() == [10 / 11, 4 / 6, 1.0, 0.0]
    for row, want_state in (((3, 1, 2, 10), 0), ((0, 0, 5, 1), 1), ((0, 2, 0, 4), 2), ((0, 0, 0, 0), 3)):
        vals, state = R.score_row(*row)
        assert state == want_state
        got = ConfusionMetrics.scores(*[[v] for v in row])
        assert [got[k][0] for k in ("dice", "iou", "precision", "recall", "specificity")] == list(vals)


def test_reference_counts_on_a_case_counted_by_hand():
    e = R.edges_uniform(16)
    x = np.array([[[[-5.0, -0.1, 0.0, 0.1], [5.0, np.nan, np.inf, -np.inf]]]], dtype=np.float32)
    t = np.array([[[[0.0, 1.0, 0.5, 0.7], [1.0, 1.0, 0.0, 0.0]]]], dtype=np.float32)
    counts, hist, out, state = R.binary(x, t, e)
    # predictions: 0 0 0 1 | 1 0 1 0;  targets: 0 1 0 1 | 1 1 0 0
    assert counts[0, 0].tolist() == [2, 1, 2, 3] and state[0, 0] == 0
    assert hist.sum() == 8 and hist[0, 0, 0].tolist()[0] == 2 and hist[0, 0, 1, 0] == 1      # -5 and -inf; the NaN under a positive
    assert hist[0, 0, 0, 8] == 1 and hist[0, 0, 0, 15] == 1 and hist[0, 0, 1, 15] == 1 and hist[0, 0, 1, 7] == 1 and hist[0, 0, 1, 8] == 1
    assert out[0, 0].tolist() == [4 / 7, 2 / 5, 2 / 3, 0.5, 0.75]
    logits = np.zeros((1, 3, 2, 3), dtype=np.float32)
    logits[0, 2, 0] = 1.0                               # row 0 predicts class 2, row 1 is a tie: class 0
    labels = np.array([[[2, 1, -100], [0, 3, 1]]])
    counts, out, state = R.classes(logits, labels)
    assert counts[0].tolist() == [[1, 0, 0], [1, 0, 1], [0, 0, 1]] and state[0].tolist() == [1, 0]
    assert out[0, 1].tolist() == [2 / 3, 0.5, 0.5, 1.0, 2 / 3] and out[0, 0].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0]
