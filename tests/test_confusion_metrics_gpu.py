"""GPU: ConfusionMetrics (uz_confusion.hip) against the numpy restatement tests/confusion_ref.py (integer counts from
searchsorted / bincount, float64 scores; its curves pinned by tests/test_confusion_metrics.py), eagerly and inside GraphedEval's
graph.

Acceptance for every case: ``counts`` and ``hist`` are EQUAL to the reference's; the five scores of ``out`` lie within 1 float32
ulp of float32(reference float64) -- the only inexact steps are one float64 division and one rounding to float32; the state is
equal; the two spare values are 0.  Every case is generated from fixed seeds and compared; none is skipped."""
import numpy as np
import pytest
import torch

import confusion_ref as R  # tests/confusion_ref.py (pytest puts this directory on sys.path)
import surface_ref
import unet_zoo_amd
from unet_zoo_amd import _lib, ops
from unet_zoo_amd.confusion import ConfusionMetrics
from unet_zoo_amd.loss import MulticlassLoss
from unet_zoo_amd.surface import SurfaceMetrics

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIN, CLS = _lib.CONFUSION_BINARY, _lib.CONFUSION_CLASS


def _np(res):
    torch.cuda.synchronize()
    return tuple(None if v is None else v.cpu().numpy() for v in res)


def _check_scores(out, want_out, want_state, what):
    assert out.dtype == np.float32 and out.shape == want_out.shape[:-1] + (8,), (what, out.shape)
    err = np.abs(out[..., :5].astype(np.float64) - want_out.astype(np.float32).astype(np.float64)) / R.ulp32(want_out)
    print(f"{what}: largest score error {err.max():.2f} float32 ulp; states {np.bincount(want_state.reshape(-1), minlength=4).tolist()}")
    assert err.max() <= 1.0, (what, err.tolist())
    assert np.array_equal(out[..., 5], want_state.astype(np.float32)), (what, out[..., 5].tolist(), want_state.tolist())
    assert not out[..., 6:].any()


def _check_binary(got, x, t, edges, what=""):
    counts, hist, out = got
    wc, wh, wo, ws = R.binary(x, t, edges)
    assert counts.dtype == np.int64 and hist.dtype == np.int64
    assert counts.shape == wc.shape and np.array_equal(counts, wc), (what, counts.tolist(), wc.tolist())
    assert hist.shape == wh.shape and np.array_equal(hist, wh), (what, np.argwhere(hist != wh).tolist()[:8])
    assert (hist.sum((2, 3)) == x.shape[2] * x.shape[3]).all() and (counts.sum(2) == x.shape[2] * x.shape[3]).all()
    _check_scores(out, wo, ws, what)
    return wc, wh, wo, ws


def _check_class(got, x, y, first, ignore_index=-100, what=""):
    counts, hist, out = got
    wc, wo, ws = R.classes(x, y, first, ignore_index)
    assert hist is None and counts.dtype == np.int64
    assert counts.shape == wc.shape and np.array_equal(counts, wc), (what, np.argwhere(counts != wc).tolist()[:8])
    _check_scores(out, wo, ws, what)
    return wc, wo, ws


def _planted(shape, edges, seed, scale=4.0):
    """seeded normal logits times `scale` with, in every plane at seeded places: every edge, its float32 predecessor, 0.0, the
    two infinities, a NaN and +-30; float targets of 0, 1, exactly 0.5 and 0.7"""
    rng = np.random.RandomState(seed)
    x = (rng.randn(*shape) * scale).astype(np.float32)
    plant = np.concatenate([edges, np.nextafter(edges, np.float32(-np.inf)), np.array([0.0, np.inf, -np.inf, np.nan, 30.0, -30.0], dtype=np.float32)])
    planes = x.reshape(-1, shape[2] * shape[3])
    assert len(plant) <= planes.shape[1]
    for p in planes:
        p[rng.permutation(planes.shape[1])[:len(plant)]] = plant
    t = rng.choice(np.array([0.0, 1.0, 0.5, 0.7], dtype=np.float32), size=shape)
    return x, t


def _call(m, x, t):
    return _np(m(torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)))


# ---- 1. binary, odd plane: the 4-byte path, planes that start off a 16-byte boundary ----------------------------------------------
def test_binary_odd_plane_with_planted_values():
    m = ConfusionMetrics(bins=64)
    edges = m.edges.numpy()
    x, t = _planted((2, 3, 37, 53), edges, 1)
    got = _call(m, x, t)
    wc, wh, _, ws = _check_binary(got, x, t, edges, "37 x 53, B = 64")
    assert (wh[..., 0] > 0).all() and (wh[..., -1] > 0).all() and (wh > 0).sum() > 2 * 3 * 2 * 40      # end bins and the middle
    assert (ws == 0).all() and (wc > 0).all()
    assert torch.equal(m.dice, m.out[..., 0]) and torch.equal(m.specificity, m.out[..., 4]) and m.iou.shape == (2, 3)
    assert torch.equal(m.state.cpu(), torch.from_numpy(ws.astype(np.float32)))


# ---- 2. binary, the 16-byte path, the smallest and the largest table, uneven thresholds -------------------------------------------
@pytest.mark.parametrize("kw", [dict(bins=16), dict(bins=1024),
                                dict(thresholds=[0.001, 0.01, 0.05, 0.1, 0.2, 0.3, 0.45, 0.5, 0.52, 0.6, 0.75, 0.9, 0.97, 0.99, 0.9999])],
                         ids=["B16", "B1024", "uneven"])
def test_binary_vector_path_and_table_sizes(kw):
    m = ConfusionMetrics(**kw)
    edges = m.edges.numpy()
    assert np.array_equal(edges, R.edges_uniform(m.bins) if "bins" in kw else R.edges_of(kw["thresholds"]))
    x, t = _planted((1, 2, 64, 64), edges, 2 + m.bins, scale=3.0)
    got = _call(m, x, t)
    _, wh, _, _ = _check_binary(got, x, t, edges, f"64 x 64, B = {m.bins}")
    assert got[1].shape == (1, 2, 2, m.bins) and (wh.sum(2) > 0).all()      # every bin of every plane is occupied


# ---- 3. one bin takes everything: 16 384 counts through the wave sums, not one LDS address ----------------------------------------
@pytest.mark.parametrize("logit,target,state", [(30.0, 1.0, 0), (30.0, 0.0, 2), (-30.0, 0.0, 3), (-30.0, 1.0, 1)])
def test_one_bin_takes_everything(logit, target, state):
    m = ConfusionMetrics(bins=256)
    x, t = np.full((1, 1, 128, 128), logit, dtype=np.float32), np.full((1, 1, 128, 128), target, dtype=np.float32)
    got = _call(m, x, t)
    _, wh, wo, ws = _check_binary(got, x, t, m.edges.numpy(), f"all {logit} against all {target}")
    assert ws[0, 0] == state and wh[0, 0, int(target), 255 if logit > 0 else 0] == 16384 and (wh > 0).sum() == 1
    if state == 3:
        assert got[2][0, 0, :2].tolist() == [1.0, 1.0] and got[2][0, 0, 2:4].tolist() == [0.0, 0.0] and got[2][0, 0, 4] == 1.0
    if state == 0:
        assert got[2][0, 0, :4].tolist() == [1.0, 1.0, 1.0, 1.0] and got[0][0, 0].tolist() == [16384, 0, 0, 0]


# ---- 4. workgroups that walk, and planes that change inside a walk ----------------------------------------------------------------
def test_capped_grid_walks_and_changes_planes():
    m = ConfusionMetrics(bins=64)
    edges = m.edges.numpy()
    x, t = _planted((2, 2, 40, 40), edges, 4)
    xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    free = _np(m(xd, td))
    _check_binary(free, x, t, edges, "40 x 40, the plan's own grid")
    rng = np.random.RandomState(44)
    xc, y = rng.randn(2, 2, 40, 40).astype(np.float32), rng.randint(0, 2, size=(2, 40, 40)).astype(np.int32)
    xcd, yd = torch.from_numpy(xc).to(DEV), torch.from_numpy(y).to(DEV)
    free_cls = _np(m(xcd, yd))
    _check_class(free_cls, xc, y, 1, what="40 x 40 class, the plan's own grid")
    for cap in (3, 1):
        desc, ws, e, counts, hist, out = m._plan(BIN, x.shape, xd.device, max_workgroups=cap)
        grid, units = ops.confusion_grid(desc)
        assert grid == cap and units == 8 and units > grid
        ops.confusion_metrics(desc, xd, td, e, counts, hist, out, ws)
        got = _np((counts, hist, out))
        assert all(np.array_equal(a, b) for a, b in zip(got, free)), cap
        desc, ws, e, counts, hist, out = m._plan(CLS, x.shape, xd.device, max_workgroups=cap)
        grid, units = ops.confusion_grid(desc)
        assert grid == cap and units == 4 and units > grid
        ops.confusion_metrics(desc, xcd, yd, None, counts, None, out, ws)
        got = _np((counts, None, out))
        assert np.array_equal(got[0], free_cls[0]) and np.array_equal(got[2], free_cls[2]), cap


# ---- 5. class mode ----------------------------------------------------------------------------------------------------------------
def _class_case(K, seed, shape=(3, 19, 23), ignore_index=-100):
    rng = np.random.RandomState(seed)
    N, H, W = shape
    x = rng.randn(N, K, H, W).astype(np.float32)
    x[0, :, :5] = 0.25                                   # a region where every class ties: class 0 wins
    x[1, K // 2:, 4:9] = 7.0                             # the upper classes tie above the rest: class K // 2 wins
    x[1, K - 1, 10:14] = x[1, 0, 10:14] = 9.0            # the first and the last tie: class 0 wins
    y = rng.randint(0, K, size=shape).astype(np.int64)
    y[rng.rand(*shape) < 0.1] = ignore_index
    y[rng.rand(*shape) < 0.05] = -1
    y[rng.rand(*shape) < 0.05] = K
    return x, y


@pytest.mark.parametrize("background", [False, True], ids=["fg", "bg"])
@pytest.mark.parametrize("K", [2, 5, 32])
def test_class_mode(K, background):
    ign = -100 if K != 5 else 3                          # K = 5: a label inside [0, K) is the ignored one
    x, y = _class_case(K, 50 + K, ignore_index=ign)
    m = ConfusionMetrics(include_background=background, ignore_index=ign)
    got = _np(m(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)))
    first = 0 if background else 1
    wc, _, _ = _check_class(got, x, y, first, ign, f"K = {K}, first_class = {first}")
    assert got[2].shape == (3, K - first, 8) and got[0].shape == (3, K, K)
    assert wc[0, :, 0].sum() >= 5 * 23 * 0.5 and wc.sum() < 3 * 19 * 23      # the tied region went to class 0; pixels were left out
    if ign == 3:
        assert wc[:, 3].sum() == 0
    # (N, 1, H, W) int32 labels are the same call
    again = _np(m(torch.from_numpy(x).to(DEV), torch.from_numpy(y[:, None].astype(np.int32)).to(DEV)))
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[2], got[2])


def test_class_mode_every_pixel_ignored_and_one_cell_takes_everything():
    K = 5
    x, _ = _class_case(K, 77)
    m = ConfusionMetrics(include_background=True)
    y = np.full((3, 19, 23), -100, dtype=np.int64)
    got = _np(m(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)))
    _check_class(got, x, y, 0, what="every pixel ignored")
    assert not got[0].any() and (got[2][..., 5] == 3).all() and (got[2][..., :2] == 1).all() and not got[2][..., 2:5].any()
    # 64 x 64, label 1 and prediction 3 everywhere: 4096 counts in one cell
    x = np.zeros((1, K, 64, 64), dtype=np.float32)
    x[:, 3] = 1.0
    y = np.ones((1, 64, 64), dtype=np.int64)
    got = _np(m(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)))
    _check_class(got, x, y, 0, what="one cell")
    assert got[0][0, 1, 3] == 4096 and got[0].sum() == 4096 and got[2][0, :, 5].tolist() == [3.0, 1.0, 3.0, 2.0, 3.0]


# ---- 6. the workspace is cleared by the call --------------------------------------------------------------------------------------
def test_alternating_inputs_through_one_object():
    m = ConfusionMetrics(bins=64)
    edges = m.edges.numpy()
    a, b = _planted((2, 2, 33, 31), edges, 60), _planted((2, 2, 33, 31), edges, 61, scale=0.5)
    fresh = [_call(ConfusionMetrics(bins=64), *a), _call(ConfusionMetrics(bins=64), *b)]
    _check_binary(fresh[0], *a, edges, "first input")
    _check_binary(fresh[1], *b, edges, "second input")
    assert not np.array_equal(fresh[0][1], fresh[1][1])
    for k in (0, 1, 0, 0, 1):
        got = _call(m, *(a, b)[k])
        assert all(np.array_equal(g, f) for g, f in zip(got, fresh[k])), k
    xa, ya = _class_case(4, 62)
    xb, yb = _class_case(4, 63)
    fresh = [_np(ConfusionMetrics()(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))) for x, y in ((xa, ya), (xb, yb))]
    for k in (0, 1, 1, 0):
        x, y = ((xa, ya), (xb, yb))[k]
        got = _np(m(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)))
        assert np.array_equal(got[0], fresh[k][0]) and np.array_equal(got[2], fresh[k][2]), k


# ---- 7. containers and dtypes ------------------------------------------------------------------------------------------------------
def test_containers_and_bf16():
    m = ConfusionMetrics(bins=32)
    edges = m.edges.numpy()
    x, t = _planted((2, 1, 24, 40), edges, 70)
    xb = torch.from_numpy(x).to(DEV).bfloat16()
    td = torch.from_numpy(t).to(DEV)
    other = torch.zeros_like(xb)
    want = _np(m(xb.float(), td))
    _check_binary(want, xb.float().cpu().numpy(), t, edges, "bf16 logits")
    for outputs in (xb, {"d0": xb, "d1": other}, [other, other, xb], (other, xb)):
        got = _np(m(outputs, td))
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), type(outputs).__name__
    got = _np(m(xb, td.double()))                       # float64 and bf16 targets go through float32
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


# ---- 8. inside the evaluation graph -------------------------------------------------------------------------------------------------
def _unet(dtype, x, classes=1):
    """a seeded unet in eval mode whose logits at x are of both signs (the head's bias is moved to their median)"""
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=classes)
    m.run_dtype = dtype
    m = m.to(DEV).eval()
    if classes == 1:
        with torch.no_grad():
            m.out.conv.bias -= m(x).float().median()
    return m


def _batch(seed, B=2, H=64, W=64, empty=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, H, W, generator=g)
    t = torch.from_numpy(np.stack([surface_ref.blobs((H, W), 1000 * seed + k) for k in range(B)])[:, None]).float()
    if empty is not None:
        t[empty] = 0.0
    return x.to(DEV), t.to(DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_graphed_eval_replay_equals_eager(dtype):
    x, t = _batch(1)
    m = _unet(dtype, x)
    eager = ConfusionMetrics(bins=64)
    ev = unet_zoo_amd.GraphedEval(m, "bce_dice", confusion=ConfusionMetrics(bins=64))
    assert "+confusion" in ev.describe()
    for seed in (1, 2):                        # the second batch is replayed into the static tensors of the first
        x, t = _batch(seed)
        with torch.no_grad():
            want = [v.clone() for v in eager(m(x), t)]
        ev(x, t)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(ev.confusion, want)), seed
        assert (want[0] > 0).all()             # the comparison is of real counts: all four kinds occur
    assert ev.confusion[0].shape == (2, 1, 4) and ev.confusion[1].shape == (2, 1, 2, 64) and ev.confusion[2].shape == (2, 1, 8)


def _count_reads(monkeypatch):
    """counts the device-to-host copies torch makes through Tensor.cpu / tolist / item / numpy of a device tensor"""
    seen = []
    for name in ("cpu", "tolist", "item", "numpy"):
        orig = getattr(torch.Tensor, name)

        def wrapped(self, *a, _orig=orig, _name=name, **kw):
            if self.is_cuda:
                seen.append(_name)
            return _orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, wrapped)
    return seen


def test_evaluate_summary(monkeypatch):
    loader = [_batch(5), _batch(6, empty=1), _batch(7)]
    m = _unet(torch.float32, loader[0][0])
    plain = unet_zoo_amd.GraphedEval(m, "bce_dice").evaluate(loader)
    cm = ConfusionMetrics(bins=64)
    ev = unet_zoo_amd.GraphedEval(m, "bce_dice", confusion=cm)
    ev.evaluate(loader)                        # captures
    seen = _count_reads(monkeypatch)
    got = ev.evaluate(loader)
    monkeypatch.undo()
    assert seen == ["cpu"], seen               # ONE device-to-host copy for the whole pass
    assert got == plain                        # (mean_loss, mean_dice): bit for bit what the pass without confusion returns
    with torch.no_grad():
        logits = np.concatenate([m(x).float().cpu().numpy() for x, _ in loader])
    target = np.concatenate([t.cpu().numpy() for _, t in loader])
    wc, wh, wo, ws = R.binary(logits, target, cm.edges.numpy())
    s = ev.confusion_summary
    tot = wc.sum(0)                            # (P, 4)
    assert [s["tp"], s["fp"], s["fn"], s["tn"]] == [[int(tot[0, k])] for k in range(4)]
    assert np.array_equal(s["hist"], wh.sum(0)) and s["hist"].sum() == 6 * 64 * 64
    micro, _ = R.score_row(*tot[0])
    for k, name in enumerate(("dice", "iou", "precision", "recall", "specificity")):
        assert s[name] == [micro[k]], (name, s[name], micro[k])
    assert s["miou"] == micro[1]
    states = [int((ws == k).sum()) for k in range(4)]
    assert [s["n_valid"], s["n_pred_empty"], s["n_target_empty"], s["n_both_empty"]] == [[c] for c in states]
    assert sum(states) == 6 and states[0] >= 1 and states[2] + states[3] == 1 and s["n_scored"] == [6 - states[3]]
    scored = ws[:, 0] != 3
    for k, name in ((0, "macro_dice"), (1, "macro_iou")):
        want = wo[scored, 0, k].astype(np.float32).astype(np.float64).mean()      # the per-image scores are float32
        assert abs(s[name][0] - want) <= 1e-6 * want, (name, s[name], want)
    ref = R.curves(wh.sum(0)[0], cm.thresholds.numpy())
    own = ConfusionMetrics.curves(wh.sum(0), cm.thresholds)
    for name in ("auroc", "ap", "best_dice", "best_threshold"):
        assert s["curves"][name][0] == own[name][0] and abs(own[name][0] - ref[name]) <= 1e-12, name
    assert np.array_equal(s["curves"]["roc"], own["roc"]) and np.array_equal(s["curves"]["reliability"][0], ref["reliability"])
    assert 0.0 < s["curves"]["auroc"][0] < 1.0

    # together with surface=: both summaries, still one copy
    sm = SurfaceMetrics(percentile=90.0, spacing=0.5)
    alone = unet_zoo_amd.GraphedEval(m, "bce_dice", surface=SurfaceMetrics(percentile=90.0, spacing=0.5))
    assert alone.evaluate(loader) == plain
    both = unet_zoo_amd.GraphedEval(m, "bce_dice", surface=sm, confusion=ConfusionMetrics(bins=64))
    assert "+surface+confusion" in both.describe()
    both.evaluate(loader)
    seen = _count_reads(monkeypatch)
    assert both.evaluate(loader) == plain
    monkeypatch.undo()
    assert seen == ["cpu"], seen
    assert both.surface_summary == alone.surface_summary and both.surface_summary["n_valid"][0] >= 1
    for k, v in s.items():
        if k not in ("hist", "curves"):
            assert both.confusion_summary[k] == v, k
    assert np.array_equal(both.confusion_summary["hist"], s["hist"])
    # a change of the number of bins during a pass raises
    with pytest.raises(ValueError, match="changed during the pass"):
        changing = unet_zoo_amd.GraphedEval(m, "bce_dice", confusion=cm)

        def batches():
            yield loader[0]
            changing._confusion = ConfusionMetrics(bins=32)
            changing._graphs.clear()
            yield loader[1]
        changing.evaluate(batches())


def test_evaluate_with_class_indices_gives_the_matrix():
    K = 4
    x, _ = _batch(4)
    m = _unet(torch.float32, x, classes=K)
    loader = []
    for seed in (8, 9, 10):
        xs, _ = _batch(seed)
        y = np.stack([surface_ref.blobs((64, 64), 70 + seed + k) * 1 + surface_ref.blobs((64, 64), 80 + seed + k) * 2 for k in range(2)])
        y[:, :3] = -100
        loader.append((xs, torch.from_numpy(y).to(DEV)))
    ev = unet_zoo_amd.GraphedEval(m, MulticlassLoss.ce_dice(), confusion=ConfusionMetrics())
    plain = unet_zoo_amd.GraphedEval(m, MulticlassLoss.ce_dice()).evaluate(loader)
    assert ev.evaluate(loader) == plain
    with torch.no_grad():
        logits = np.concatenate([m(xs).float().cpu().numpy() for xs, _ in loader])
    labels = np.concatenate([y.cpu().numpy() for _, y in loader])
    wc, wo, ws = R.classes(logits, labels, 1)
    s = ev.confusion_summary
    assert np.array_equal(s["matrix"], wc.sum(0)) and s["matrix"].sum() == 6 * 61 * 64 and "curves" not in s
    assert ev.confusion[1] is None and ev.confusion[0].shape == (2, K, K) and ev.confusion[2].shape == (2, K - 1, 8)
    # the micro scores are those of the summed matrix
    total = wc.sum(0)
    for j in range(K - 1):
        c = 1 + j
        tp = int(total[c, c])
        fp, fn = int(total[:, c].sum()) - tp, int(total[c].sum()) - tp
        vals, _ = R.score_row(tp, fp, fn, int(total.sum()) - tp - fp - fn)
        assert [s[k][j] for k in ("dice", "iou", "precision", "recall", "specificity")] == list(vals), j
    assert s["miou"] == pytest.approx(sum(s["iou"]) / (K - 1), abs=1e-15)
    assert [sum(v) for v in zip(s["n_valid"], s["n_pred_empty"], s["n_target_empty"], s["n_both_empty"])] == [6] * (K - 1)
    assert s["n_valid"] == [int((ws[:, j] == 0).sum()) for j in range(K - 1)]
