"""GPU: the k = 5 convolution family and the BatchNorm + ELU passes of uz_conv5x5.hip against float64 on the CPU.

Bounds come from the number formats, not from what the kernels give:
  * fp32 results (every fp32-mode tensor, and the weight gradient in both modes) from operands the oracle shares exactly:
    only the summation order differs; a sum of K <= 6400 terms in fp32 is off by about eps * sqrt(K) ~ 5e-6 of its size, the
    bound is 1e-4 of the result's norm;
  * bf16-stored results: round-to-nearest is off by at most 2^-9 of each element, so by at most 2^-9 of the norm, plus the
    fp32 summation above: the bound is 2^-8 of the norm; the BatchNorm + ELU passes chain up to three such roundings (the
    stored act1 value before the residual sum, the stored result that ELU' is taken from, the stored output): 2^-7.
dgamma / dbeta are per-channel SUMS over the pixels of terms that carry those roundings and cancel: their error is bounded
against the sum of the terms' magnitudes (sum |dbn * xhat|, sum |dbn|), not against the sum itself.
bf16 operands are rounded BEFORE the oracle sees them (as tests/test_bf16_rounded_oracle_gpu.py does)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from unet_zoo_amd import _lib as L
from unet_zoo_amd import ops
from unet_zoo_amd.ops import Act, act_from_nchw

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
SHAPES = [(1, 6, 10), (2, 24, 40)]      # 60 pixels: less than one 128-pixel tile; 24 x 40: H != W, 15 tiles


def _tol(dt, stored=True, chain=False):
    if dt == torch.float32 or not stored:
        return 1e-4
    return 2.0 ** -7 if chain else 2.0 ** -8


def _close(got, ref, tol):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err, nrm = (got - ref).norm().item(), ref.norm().item()
    print(f"    rel err {err / (nrm + 1e-300):.3e} (bound {tol:.3e})")
    assert err <= tol * nrm + 1e-30, (err, nrm, tol)


def _close_sum(got, ref, scale, tol):
    """a sum of rounded terms: |got - ref| <= tol * sum |term|, per element"""
    got, ref, scale = got.double().cpu(), ref.double().cpu(), scale.double().cpu()
    worst = ((got - ref).abs() / (scale + 1e-300)).max().item()
    print(f"    err / sum|terms| {worst:.3e} (bound {tol:.3e})")
    assert worst <= tol, (worst, tol)


def _rnd(t, dt):
    return t.to(dt).double()


def _nchw(a: Act):
    return a.buf[:, a.off:a.off + a.C].double().cpu().reshape(a.N, a.H, a.W, a.C).permute(0, 3, 1, 2)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [32, 64, 128, 256])
@pytest.mark.parametrize("N,H,W", SHAPES)
def test_conv5x5_forward_input_gradient_weight_gradient(N, H, W, C, dt):
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(C, C, 5, 5, generator=g) / (5.0 * C ** 0.5)
    b = torch.randn(C, generator=g)
    dy = torch.randn(N, C, H, W, generator=g)
    xr, wr, dyr = _rnd(x, dt), _rnd(w, dt), _rnd(dy, dt)
    xa, dya = act_from_nchw(x.to(DEV), dt), act_from_nchw(dy.to(DEV), dt)
    wf = ops.pack_weights(w.to(DEV), L.PACK_CONV_FWD, dt)
    wd = ops.pack_weights(w.to(DEV), L.PACK_CONV_DGRAD, dt)
    outs = []
    for _ in range(2):
        y = ops.new_act(N, H, W, C, dt, DEV)
        stats = ops.conv5x5(xa, wf, b.to(DEV), y, want_stats=True)
        dx = ops.new_act(N, H, W, C, dt, DEV)
        ops.conv5x5(dya, wd, None, dx)
        dw = ops.wgrad5x5(dya, xa, (C, C, 5, 5))
        torch.cuda.synchronize()
        outs.append((y.buf.clone(), stats.clone(), dx.buf.clone(), dw.clone()))
    for a, bb in zip(*outs):
        assert torch.equal(a, bb)                       # two runs bit-identical
    yb, stats, dxb, dw = outs[0]
    _close(_nchw(y), F.conv2d(xr, wr, b.double(), padding=2), _tol(dt))
    _close(_nchw(dx), F.conv_transpose2d(dyr, wr, padding=2), _tol(dt))
    ref_dw = torch.nn.grad.conv2d_weight(xr, (C, C, 5, 5), dyr, padding=2)
    _close(dw, ref_dw, _tol(dt, stored=False))
    # the BatchNorm partial sums are those of the kernel's own stored output
    yv = yb.double().cpu()
    s = stats.double().sum(0).cpu()
    assert torch.allclose(s[0], yv.sum(0), rtol=1e-4, atol=1e-4 * yv.abs().sum(0).max().item())
    assert torch.allclose(s[1], (yv * yv).sum(0), rtol=1e-4)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("K", [1, 3])
def test_thin_output_layer_32_to_num_classes(K, dt):
    """32 -> num_classes: the result and its gradient live in zero-padded 8-column buffers"""
    N, H, W, C = 2, 24, 40, 32
    g = torch.Generator().manual_seed(K)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, 5, 5, generator=g) / 28.0
    b = torch.randn(K, generator=g)
    dy = torch.randn(N, K, H, W, generator=g)
    xr, wr, dyr = _rnd(x, dt), _rnd(w, dt), _rnd(dy, dt)
    xa = act_from_nchw(x.to(DEV), dt)
    y = Act(torch.zeros((N * H * W, 8), dtype=dt, device=DEV), 0, K, N, H, W)
    stats = ops.conv5x5(xa, ops.pack_weights(w.to(DEV), L.PACK_CONV_FWD, dt), b.to(DEV), y, want_stats=True)
    assert stats.shape[1:] == (2, K)
    _close(_nchw(y), F.conv2d(xr, wr, b.double(), padding=2), _tol(dt))
    assert (y.buf[:, K:] == 0).all()
    gb = torch.zeros((N * H * W, 8), dtype=dt, device=DEV)
    gb[:, :K] = dy.permute(0, 2, 3, 1).reshape(-1, K).to(DEV)
    ga = Act(gb, 0, 8, N, H, W)
    dw = ops.wgrad5x5(ga, xa, (K, C, 5, 5))
    _close(dw, torch.nn.grad.conv2d_weight(xr, (K, C, 5, 5), dyr, padding=2), _tol(dt, stored=False))
    wd = torch.zeros((C, 25, 8))
    wd[:, :, :K] = w.flip(2, 3).reshape(K, C, 25).permute(1, 2, 0)
    dx = ops.new_act(N, H, W, C, dt, DEV)
    ops.conv5x5(ga, wd.reshape(C, 200).to(DEV).to(dt), None, dx)
    _close(_nchw(dx), F.conv_transpose2d(dyr, wr, padding=2), _tol(dt))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_pointwise_adapter_3_to_16(dt):
    """k = 1 on the zero-padded 8-channel image: the per-forward 1x1 convolution of VNet's input stage"""
    N, H, W = 2, 16, 48
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, 3, H, W, generator=g)
    w = torch.randn(16, 3, generator=g)
    b = torch.randn(16, generator=g)
    xp = torch.zeros(N, 8, H, W)
    xp[:, :3] = x
    wp = torch.zeros(16, 8)
    wp[:, :3] = w
    y = ops.new_act(N, H, W, 16, dt, DEV)
    ops.conv5x5(act_from_nchw(xp.to(DEV), dt), wp.to(DEV).to(dt), b.to(DEV), y, ksize=1)
    _close(_nchw(y), F.conv2d(_rnd(x, dt), _rnd(w, dt).reshape(16, 3, 1, 1), b.double()), _tol(dt))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("Cin", [1, 3, 16])
@pytest.mark.parametrize("N,H,W", SHAPES)
def test_thin_input_layer_in_channels_to_16(N, H, W, Cin, dt):
    """in_channels -> 16, 5x5: Engine.conv_input (im2col k5 s1 p2 + the one-tap GEMM), its weight gradient un-permuted to
    (16, Cin, 5, 5), and its bias gradient"""
    import torch.nn as nn
    from unet_zoo_amd.engine import Engine
    g = torch.Generator().manual_seed(Cin * 10 + H)
    x = torch.randn(N, Cin, H, W, generator=g)
    dy = torch.randn(N, 16, H, W, generator=g)
    conv = nn.Conv2d(Cin, 16, 5, padding=2)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(16, Cin, 5, 5, generator=g) / (5.0 * Cin ** 0.5))
        conv.bias.copy_(torch.randn(16, generator=g))
    conv = conv.to(DEV)
    xr, wr, dyr = _rnd(x, dt), _rnd(conv.weight.detach().cpu(), dt), _rnd(dy, dt)
    runs = []
    for _ in range(2):
        eng = Engine(dt, torch.device(DEV), True, True)
        y = eng.conv_input(x.to(DEV), conv)
        y.add_grad(act_from_nchw(dy.to(DEV), dt))
        grads = eng.backward(())
        torch.cuda.synchronize()
        runs.append((y.buf.clone(), grads[conv.weight].clone(), grads[conv.bias].clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert (y.N, y.H, y.W, y.C) == (N, H, W, 16)
    _close(_nchw(y), F.conv2d(xr, wr, conv.bias.detach().double().cpu(), padding=2), _tol(dt))
    yb, dw, db = runs[0]
    assert tuple(dw.shape) == (16, Cin, 5, 5)
    _close(dw, torch.nn.grad.conv2d_weight(xr, (16, Cin, 5, 5), dyr, padding=2), _tol(dt, stored=False))
    _close_sum(db, dyr.sum((0, 2, 3)), dyr.abs().sum((0, 2, 3)), _tol(dt, stored=False))


# (act1, act2, res, out2): every combination the model uses
COMBOS = [(False, True, True, True),     # input stage: ELU(bn + x16), dropped skip copy
          (True, False, False, False),   # LUConv
          (True, False, False, True),    # down convolution with Dropout2d behind it
          (True, True, True, True),      # last LUConv of a stage + residual, dropped skip copy
          (True, True, True, False)]     # the same without a reader of the dropped copy


def _elu_ref(t, on):
    return F.elu(t) if on else t


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("combo", COMBOS, ids=["in", "lu", "down_do", "res_do", "res"])
@pytest.mark.parametrize("C,ld", [(32, 32), (1, 8)], ids=["c32", "thin1"])
def test_bn_elu_forward_and_backward(C, ld, combo, dt):
    act1, act2, has_res, has_out2 = combo
    N, H, W = 2, 12, 20
    P = N * H * W
    g = torch.Generator().manual_seed(C * 7 + sum(combo))
    mk = lambda: torch.randn(P, C, generator=g)   # noqa: E731

    def as_act(t):
        buf = torch.zeros((P, ld), dtype=dt, device=DEV)
        buf[:, :C] = t.to(DEV)
        return Act(buf, 0, C, N, H, W)

    x, res, g0, g1, g2 = mk() * 1.5 + 0.3, mk(), mk(), mk(), mk()
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    mask = (torch.rand(N, C, generator=g) >= 0.5).float() * 2.0
    xa = as_act(x)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    if C % 8 == 0:
        stats = ops.colstats(xa)
    else:   # the thin layer's statistics come from its convolution; here from torch
        xs = xa.buf[:, :C].float()
        stats = torch.stack([xs.sum(0), (xs * xs).sum(0)]).reshape(1, 2, C).contiguous()
    vec = ops.bn_finalize(stats, P, gamma.to(DEV), beta.to(DEV), 1e-5, 0.1, rm, rv)
    ra = as_act(res) if has_res else None
    out, out2 = as_act(torch.zeros(P, C)), (as_act(torch.zeros(P, C)) if has_out2 else None)
    mdev = mask.to(DEV) if has_out2 else None
    ops.bn_elu_apply(xa, vec[0], vec[1], out, act1=act1, act2=act2, res=ra, out2=out2, mask2=mdev)

    # float64 oracle on the (rounded) operands, gradients by autograd THROUGH the batch statistics
    xr = _rnd(x, dt).requires_grad_(True)
    rr = _rnd(res, dt).requires_grad_(True)
    gm, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    mean, var = xr.mean(0), xr.var(0, unbiased=False)
    xhat = (xr - mean) / torch.sqrt(var + 1e-5)
    bnout = xhat * gm + bt
    bnout.retain_grad()
    o = _elu_ref(_elu_ref(bnout, act1) + (rr if has_res else 0.0), act2)
    mfull = mask.double().repeat_interleave(H * W, dim=0)
    tol = _tol(dt, chain=True)
    _close(out.buf[:, :C], o.detach(), tol)
    if has_out2:
        _close(out2.buf[:, :C], (o * mfull).detach(), tol)
    G = _rnd(g0, dt) + _rnd(g1, dt) + (_rnd(g2, dt) * mfull if has_out2 else 0.0)
    o.backward(G)
    dx, gres = as_act(torch.zeros(P, C)), (as_act(torch.zeros(P, C)) if has_res else None)
    sums = torch.empty((2, C), dtype=torch.float64, device=DEV)
    dgamma, dbeta = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    runs = []
    for _ in range(2):
        ops.bn_elu_bwd(xa, vec, out, as_act(g0), as_act(g1), as_act(g2) if has_out2 else None, mdev, sums, dx, gres,
                       dgamma, dbeta, act1=act1, act2=act2)
        torch.cuda.synchronize()
        runs.append((dx.buf.clone(), dgamma.clone(), dbeta.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    _close(dx.buf[:, :C], xr.grad, tol)
    _close_sum(dgamma, gm.grad, (bnout.grad * xhat.detach()).abs().sum(0), tol)
    _close_sum(dbeta, bt.grad, bnout.grad.abs().sum(0), tol)
    if has_res:
        _close(gres.buf[:, :C], rr.grad, tol)
