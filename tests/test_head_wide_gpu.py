"""GPU: the wide 1x1 head (uz_head_wide_*, 9..32 classes on the fp32-input MFMA) -- its three products against float64
(tests/head_wide_ref.py), against the narrow head at K = 8, where workgroups walk several tiles, call to call, and through
Engine.out_conv in whole models, eagerly and inside the step / evaluation graphs.

The bounds are derived, not tuned (u = 2^-23, one fp32 rounding per addend of an fmaf chain, with room for the order):
  forward   |out - ref| <= (C + 8) u sum_c |w| |x|                                   per element
  dx        |dx - ref|  <= (K + 8) u sum_k |g| |w|  (+ 2^-8 |ref| for the bf16 store)
  dw, db    |d - ref|   <= n u sum_p |g| |x|  resp.  n u sum_p |g|,  n = P addends"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_wide_ref as R  # tests/head_wide_ref.py (pytest puts this directory on sys.path)
import unet_zoo_amd
from oracle import torch_ref
from unet_zoo_amd import ConfusionMetrics, MulticlassLoss, ops
from unet_zoo_amd import _lib as L
from unet_zoo_amd.graph import PhasedStep
from unet_zoo_amd.optim import FlatClipAdamW

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -23


def _inputs(dtype, N, HW, C, K, ld, seed=0):
    """x as a channel window [off, off + C) of a (P, ld) buffer whose other columns hold NaN: nothing outside the window may
    be read into a result"""
    g = torch.Generator().manual_seed(seed)
    P = N * HW
    off = 8 if ld > C else 0
    buf = torch.full((P, ld), float("nan"), dtype=dtype)
    buf[:, off:off + C] = torch.randn(P, C, generator=g).to(dtype)
    buf = buf.to(DEV)
    x = ops.Act(buf, off, C, N, 1, HW)
    w = (torch.randn(K, C, generator=g) / C ** 0.5).to(DEV)
    b = (0.1 * torch.randn(K, generator=g)).to(DEV)
    gl = torch.randn(N, K, 1, HW, generator=g).to(DEV)
    return x, w, b, gl


def _xwin(x):
    return x.buf[:, x.off:x.off + x.C]


def _check(name, got, ref, bound, where=None):
    err = (got.detach().cpu().double() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{name}: max |diff| {err.max().item():.3e}, max |diff| / bound {ratio:.3e}")
    bad = err > bound
    assert not bad.any(), f"{name}: {int(bad.sum())} elements over the bound (worst ratio {ratio:.3f})" + (where(bad) if where else "")


def _check_products(x, w, b, gl, out, dx, dw, db, where_px=None):
    N, K, HW, C, P = x.N, w.shape[0], x.H * x.W, x.C, x.P
    xw = _xwin(x)
    if out is not None:
        ref, mag = R.forward(xw, w, b, N, HW)
        _check("forward", out.reshape(N, K, HW), ref, (C + 8) * U * mag, where_px)
    if dx is not None:
        ref, mag = R.input_grad(gl.reshape(N, K, HW), w)
        bound = (K + 8) * U * mag + (2.0 ** -8 * ref.abs() if x.dtype == torch.bfloat16 else 0.0)
        _check("dx", _xwin(dx), ref, bound)
    rw, rb, mw, mb = R.weight_grads(gl.reshape(N, K, HW), xw)
    _check("dw", dw, rw, P * U * mw)
    _check("db", db, rb, P * U * mb)


@pytest.mark.parametrize("ldpad", [0, 16], ids=["dense", "window"])
@pytest.mark.parametrize("C", [8, 32, 64, 96])
@pytest.mark.parametrize("K", [9, 16, 17, 32])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_products_against_float64(dtype, K, C, ldpad):
    """N = 3, H x W = 5 x 7: HW = 35, tiles straddle images, plane starts are not 16-byte aligned, P = 105 is ragged"""
    N, HW = 3, 35
    x, w, b, gl = _inputs(dtype, N, HW, C, K, C + ldpad)
    assert ops.head_wide_supported(x, K)
    out = ops.head_wide_fwd(x, w, b)
    dxbuf = torch.full((x.P, C + ldpad), float("nan"), dtype=dtype, device=DEV)
    dx = ops.Act(dxbuf, x.off, C, N, 1, HW)
    dw, db = ops.head_wide_bwd(x, w, gl, dx)
    torch.cuda.synchronize()
    _check_products(x, w, b, gl, out, dx, dw, db)
    if ldpad:       # nothing was stored outside the window
        assert torch.isnan(dxbuf[:, :x.off]).all() and torch.isnan(dxbuf[:, x.off + C:]).all()
    # dx = NULL (the first layer, no-grad inputs): dw and db bit for bit those of the run with dx
    dw2, db2 = ops.head_wide_bwd(x, w, gl, None)
    torch.cuda.synchronize()
    assert torch.equal(dw2, dw) and torch.equal(db2, db)


@pytest.mark.parametrize("C", [8, 32, 64, 96])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_against_the_narrow_kernel_at_8_classes(dtype, C):
    """same inputs, K = 8: both heads under the same bounds, so they differ by at most twice the bound"""
    N, HW, K = 3, 35, 8
    x, w, b, gl = _inputs(dtype, N, HW, C, K, C, seed=3)
    out_w = ops.head_wide_fwd(x, w, b)
    dx_w = ops.new_act(N, 1, HW, C, dtype, DEV)
    dw_w, db_w = ops.head_wide_bwd(x, w, gl, dx_w)
    out_n = ops.outconv_fwd(x, w, b)
    dx_n = ops.new_act(N, 1, HW, C, dtype, DEV)
    dw_n, db_n = ops.outconv_bwd(x, w, gl, dx_n)
    torch.cuda.synchronize()
    print("wide head:")
    _check_products(x, w, b, gl, out_w, dx_w, dw_w, db_w)
    print("narrow head:")
    _check_products(x, w, b, gl, out_n, dx_n, dw_n, db_n)


def test_walk_of_several_tiles_per_workgroup():
    """every workgroup makes two trips, half of them three, the last tile is ragged, the second image starts inside a tile"""
    lib = L.load()
    C, K, dtype = 32, 19, torch.bfloat16
    code = L.dtype_code(dtype)
    G = lib.uz_head_wide_grid(code, 1, (1 << 31) - 1, C, K)          # the persistent grid at its largest
    tile = 256
    assert G >= 1 and lib.uz_head_wide_grid(code, 1, G * tile, C, K) == G and lib.uz_head_wide_grid(code, 1, G * tile - tile, C, K) == G - 1
    tiles = 2 * G + G // 2
    P = tiles * tile - 100
    N, HW = 2, P // 2
    assert N * HW == P and HW % tile != 0
    assert lib.uz_head_wide_grid(code, N, HW, C, K) == G
    rows = lib.uz_head_wide_bwd_workspace_bytes(code, N, HW, C, K) // (4 * K * (C + 1))
    assert rows == G                                               # the backward walks the same tiles at this shape
    x, w, b, gl = _inputs(dtype, N, HW, C, K, C, seed=5)
    out = ops.head_wide_fwd(x, w, b)
    dx = ops.new_act(N, 1, HW, C, dtype, DEV)
    dw, db = ops.head_wide_bwd(x, w, gl, dx)
    torch.cuda.synchronize()

    def where(bad):                                                # bad: (N, K, HW)
        px = bad.any(1).reshape(-1).nonzero().flatten()
        t = torch.unique(px // tile)
        return (f"\n  tiles {t[:16].tolist()} of {tiles} (grid {G}); trips {torch.unique(t // G).tolist()}; "
                f"workgroups {torch.unique(t % G)[:16].tolist()}")

    _check_products(x, w, b, gl, out, None, dw, db, where)
    ref, mag = R.input_grad(gl.reshape(N, K, HW), w)
    err = (_xwin(dx).cpu().double() - ref).abs()
    bad = (err > (K + 8) * U * mag + 2.0 ** -8 * ref.abs()).any(1)
    if bad.any():
        t = torch.unique(bad.nonzero().flatten() // tile)
        raise AssertionError(f"dx: tiles {t[:16].tolist()} of {tiles} (grid {G}); trips {torch.unique(t // G).tolist()}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_backward_is_deterministic(dtype):
    N, HW, C, K = 4, 3001, 64, 19                                  # several workgroups, several partial rows
    x, w, b, gl = _inputs(dtype, N, HW, C, K, C, seed=7)
    res = []
    for _ in range(2):
        dx = ops.new_act(N, 1, HW, C, dtype, DEV)
        dw, db = ops.head_wide_bwd(x, w, gl, dx)
        torch.cuda.synchronize()
        res.append((dw.clone(), db.clone(), dx.buf.clone()))
    for a, c in zip(*res):
        assert torch.equal(a, c)
    _check_products(x, w, b, gl, None, ops.Act(res[0][2], 0, C, N, 1, HW), res[0][0], res[0][1])


# ---------------------------------------------------------------------------------------------- whole models
@pytest.mark.parametrize("K", [9, 19])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_unet_against_oracle(dtype, K):
    """tests/test_unet_gpu.py::test_against_oracle_on_other_shape_and_classes with 9 and 19 classes, its own tolerances"""
    torch.manual_seed(11)
    m = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=K)
    m.run_dtype = dtype
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.to(DEV).train()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 64, 96, generator=g)
    t = (torch.rand(2, K, 64, 96, generator=g) > 0.5).float()
    logits = m(x.to(DEV))
    assert logits.shape == (2, K, 64, 96)
    F.binary_cross_entropy_with_logits(logits, t.to(DEV)).backward()
    st = torch_ref.clone_state(sd, requires_grad=True)
    torch_ref.set_storage_rounding(None if dtype == torch.float32 else torch.bfloat16)
    try:
        ref = torch_ref.unet_forward(st, x, True)
        F.binary_cross_entropy_with_logits(ref, t).backward()
    finally:
        torch_ref.set_storage_rounding(None)
    rel = 1e-3 if dtype == torch.float32 else 2e-2
    err = (logits.detach().cpu() - ref.detach()).abs().max()
    print(f"logits max |diff| {err.item():.3e} bound {rel * ref.detach().abs().max().item():.3e}")
    assert err <= rel * ref.detach().abs().max()
    dots = []
    total = torch.sqrt(sum((v.grad.double() ** 2).sum() for v in st.values() if v.grad is not None))
    for name, p in m.named_parameters():
        rg = st[name].grad
        if rg.abs().max() < 1e-6:
            continue
        e = (p.grad.cpu() - rg).norm() / rg.norm()
        if dtype == torch.float32:
            assert e <= 2e-2, (name, e.item())
        else:
            cos = F.cosine_similarity(p.grad.cpu().flatten(), rg.flatten(), dim=0)
            if rg.norm() > 2e-3 * total:
                assert cos >= 0.9, (name, cos.item())
        dots.append((p.grad.cpu().flatten(), rg.flatten()))
    a, c = torch.cat([d[0] for d in dots]), torch.cat([d[1] for d in dots])
    cos = F.cosine_similarity(a, c, dim=0)
    print(f"overall cosine {cos.item():.6f}")
    assert cos >= (0.9999 if dtype == torch.float32 else 0.99)


def _run_once(name, kw, x):
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model(name, in_channels=3, num_classes=9, **kw)
    m.run_dtype = torch.bfloat16
    m = m.to(DEV).train()
    out = m(x)
    outs = list(out) if isinstance(out, (list, tuple)) else [out]
    sum(o.float().square().mean() for o in outs).backward()
    torch.cuda.synchronize()
    return [o.detach().clone() for o in outs], {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("name,kw,heads", [("nested_unet", {"deep_supervision": True}, 4),
                                           ("swin_unet_v2", {"image_size": 64, "window_size": 4, "drop_path_rate": 0.0}, 1)],
                         ids=["nested_unet", "swin_unet_v2"])
def test_other_models_at_9_classes_are_finite_and_repeatable(name, kw, heads):
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(2)).to(DEV)
    o1, g1 = _run_once(name, kw, x)
    o2, g2 = _run_once(name, kw, x)
    assert len(o1) == heads and all(o.shape == (2, 9, 64, 64) for o in o1)
    assert all(torch.isfinite(o).all() for o in o1) and all(torch.isfinite(v).all() for v in g1.values())
    assert len(g1) > 0 and any(v.abs().max() > 0 for v in g1.values())
    assert all(torch.equal(a, c) for a, c in zip(o1, o2))
    assert g1.keys() == g2.keys() and all(torch.equal(g1[n], g2[n]) for n in g1)


@pytest.mark.parametrize("K,wide", [(8, False), (9, True)])
def test_routing_by_class_count(monkeypatch, K, wide):
    calls = {}
    for fn in ("head_wide_fwd", "head_wide_bwd", "outconv_fwd", "outconv_bwd"):
        def wrap(*a, _f=getattr(ops, fn), _n=fn, **k):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, fn, wrap)
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=K)
    m.run_dtype = torch.bfloat16
    m = m.to(DEV).train()
    m(torch.randn(2, 3, 32, 32, device=DEV)).float().square().mean().backward()
    torch.cuda.synchronize()
    if wide:
        assert calls == {"head_wide_fwd": 1, "head_wide_bwd": 1}, calls
    else:
        assert calls == {"outconv_fwd": 1, "outconv_bwd": 1}, calls


# ---------------------------------------------------------------------------------------------- inside the graphs
def _make9(dtype, train=True):
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=9)
    m.run_dtype = dtype
    m = m.cuda()
    return m.train() if train else m.eval()


def _batch9(seed=1):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, 9, (2, 32, 32), generator=g)
    return torch.randn(2, 3, 32, 32, generator=g).cuda(), y


class _Direct:
    """the criterion as PhasedStep takes it (tests/test_multiclass_loss_gpu.py)"""

    def __init__(self, crit):
        self.crit, self.dice = crit, None

    def __call__(self, out, t):
        return self.crit(out, t)

    def direct(self, out, t):
        loss, self.dice, gouts = self.crit.direct(out, t)
        return loss, gouts


def test_graphed_step_at_9_classes_equals_eager_step_bitwise():
    x, y = _batch9()
    m1 = _make9(torch.bfloat16)
    gs = unet_zoo_amd.GraphedStep(m1, MulticlassLoss.ce_dice(), lr=1e-3, weight_decay=1e-5, max_norm=1.0)
    g_losses, g_dice = [], []
    for _ in range(3):
        loss = gs(x, y)
        torch.cuda.synchronize()
        g_losses.append(loss.item())
        g_dice.append(gs.dice.item())
    assert "eager" not in gs.describe()
    m2 = _make9(torch.bfloat16)
    fn = _Direct(MulticlassLoss.ce_dice())
    n1 = {id(p): n for n, p in m1.named_parameters()}
    p2 = dict(m2.named_parameters())
    opt = FlatClipAdamW([p2[n1[id(p)]] for p in gs.opt.params], lr=1e-3, weight_decay=1e-5, max_norm=1.0)
    m2._pack_cache.repoint()
    ps = PhasedStep(m2, fn)
    yd = y.cuda()
    e_losses, e_dice = [], []
    for _ in range(3):
        loss = ps.forward(x, yd)
        ps.backward(ps.n_entries, 0, True)
        ps.finish()
        opt.step()
        torch.cuda.synchronize()
        e_losses.append(loss.item())
        e_dice.append(fn.dice.item())
    assert g_losses == e_losses, (g_losses, e_losses)
    assert g_dice == e_dice, (g_dice, e_dice)
    assert torch.equal(gs.opt.flat_p, opt.flat_p)
    assert all(l == l and 0.0 < l < 40.0 for l in g_losses) and len(set(g_losses)) == 3


def test_graphed_eval_at_9_classes_returns_a_9x9_confusion_matrix():
    m = _make9(torch.bfloat16, train=False)
    loader = [(x.cpu(), y) for x, y in (_batch9(seed=s) for s in (1, 2))]
    ev = unet_zoo_amd.GraphedEval(m, MulticlassLoss.ce_dice(), confusion=ConfusionMetrics())
    ev.evaluate(loader)
    s = ev.confusion_summary
    mat = np.asarray(s["matrix"])
    assert mat.shape == (9, 9) and mat.sum() == 2 * 2 * 32 * 32
