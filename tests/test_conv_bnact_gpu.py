"""GPU: the convolutions whose epilogue forms the eval-mode BatchNorm [+ ReLU] behind them (uz_conv_igemm_bnact,
uz_conv3x3_first_fwd_bnact) through the C ABI, against the two launches they replace (uz_conv_igemm / uz_conv3x3_first_fwd
followed by uz_bn_relu_apply) and a float64 reference on the rounded operands (reference: Conv2d -> BatchNorm2d -> ReLU in
eval mode, unet_zoo/models/common_layers.py:28-33, evaluated by utils/training_loop.py:147-180).

Shapes: the smallest at which tiles, ragged edges, the strided store and the upsampled read can go wrong; every case with
and without the ReLU.  Scales of random sign with |scale| in [0.5, 2]; shifts placed so that about half of the outputs
are clipped.  fp32: bit-identical to the two launches (both apply the same fmaf to the same fp32 value).  bf16: within
the tolerance tests/test_conv_pp_gpu.py applies to the plain kernel's output, and an RMS error not above the two-launch
route's (one rounding against two).  y is NaN before the launch: everything inside [0, Nout) of a pixel must be finite,
everything outside must still be NaN."""
from ctypes import byref

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from unet_zoo_amd import _lib as L
from unet_zoo_amd import ops
from unet_zoo_amd.ops import Act, act_from_nchw

DEV = "cuda"


def relerr(a, b):      # the expression of tests/test_conv_pp_gpu.py
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30)).item()


def rms(a, b):
    return ((a.double() - b.double()) ** 2).mean().sqrt().item()


def desc(dt, N, H, W, Cin, ldx, Cout, ldy, up=False, ntaps=9, taps=None, store=L.STORE_PLAIN, co=0):
    taps = (L.TAPS_CONV_UP2 if up else L.TAPS_CONV) if taps is None else taps
    return L.ConvDesc(L.dtype_code(dt), N, H, W, H // 2 if up else H, W // 2 if up else W, Cin, ldx, Cout, ldy, ntaps, taps, 1,
                      store, co, 0, 0)


def scale_shift(g, Cout, pre):
    """random sign, |scale| in [0.5, 2]; the shift puts the channel's median output at zero: about half are clipped"""
    scale = (0.5 + 1.5 * torch.rand(Cout, generator=g)) * (torch.randint(0, 2, (Cout,), generator=g) * 2 - 1).float()
    med = pre.permute(1, 0, 2, 3).reshape(Cout, -1).median(dim=1).values.float()
    return scale, -med * scale


CASES = [
    # dtype, N, H, W, Cin, Cout, ldy, channel offset, upsampled, kernel family the plan must pick
    (torch.bfloat16, 2, 32, 32, 64, 64, 64, 0, False, "conv3x3_direct_bf16_bn64_resident"),
    (torch.bfloat16, 1, 24, 40, 64, 128, 128, 0, False, "conv3x3_pp128w16_bf16"),          # ragged 8 x 16 tiles
    (torch.bfloat16, 1, 16, 16, 128, 64, 128, 64, False, "conv3x3_direct_bf16_bn64"),      # the upper half of a concat buffer
    (torch.bfloat16, 1, 16, 16, 64, 64, 64, 0, True, "conv3x3_direct_bf16_bn64_resident_up2"),
    (torch.float32, 1, 16, 16, 32, 32, 32, 0, False, "conv3x3_direct_f32_bn64_resident"),
    (torch.float32, 1, 12, 20, 32, 64, 64, 0, False, "conv3x3_direct_f32_bn64_resident"),  # ragged 16 x 16 tiles
    # the generic kernel (igemm_*): a row stride that is no multiple of 16 bytes, which the direct kernels and the LDS-DMA GEMM
    # refuse; a ragged 128-pixel M tile; both N tiles (64 and 128 channels, the second with a channel tail), both dtypes
    (torch.bfloat16, 1, 12, 20, 32, 40, 42, 0, False, "igemm_bf16_128x64"),
    (torch.bfloat16, 2, 24, 24, 32, 136, 138, 0, False, "igemm_bf16_128x128"),
    (torch.float32, 1, 12, 20, 32, 40, 42, 0, False, "igemm_f32_128x64"),
    (torch.float32, 2, 24, 24, 32, 136, 138, 0, False, "igemm_f32_128x128"),
]


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("dt,N,H,W,Cin,Cout,ldy,off,up,kernel", CASES)
def test_conv_bnact_against_two_launches(dt, N, H, W, Cin, Cout, ldy, off, up, kernel, relu):
    g = torch.Generator().manual_seed(31)
    Hi, Wi = (H // 2, W // 2) if up else (H, W)
    x = torch.randn(N, Cin, Hi, Wi, generator=g).to(dt).float()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05).to(dt).float()
    b = torch.randn(Cout, generator=g)
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    pre = F.conv2d(xin.double(), w.double(), b.double(), padding=1)
    scale, shift = scale_shift(g, Cout, pre)
    ref = pre * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    if relu:
        ref = ref.clamp_min(0.0)
        assert 0.3 < (ref == 0).double().mean() < 0.7
    xa = act_from_nchw(x.to(DEV), dt)
    wp = ops.pack_weights(w.to(DEV), L.PACK_CONV_FWD, dt)
    bd, sc, sh = b.to(DEV), scale.to(DEV), shift.to(DEV)
    ybuf = torch.full((N * H * W, ldy), float("nan"), dtype=dt, device=DEV)
    y = Act(ybuf, off, Cout, N, H, W)
    d = desc(dt, N, H, W, Cin, xa.ld, Cout, y.ld, up)
    assert ops.conv_kernel_name(d) == kernel
    lib = L.load()
    assert lib.uz_conv_igemm_bnact_supported(byref(d)) == 1
    L.check(lib.uz_conv_igemm_bnact(byref(d), xa.ptr(), wp.data_ptr(), bd.data_ptr(), sc.data_ptr(), sh.data_ptr(), relu,
                                    y.ptr(), L.stream_ptr()), "uz_conv_igemm_bnact")
    got = y.dense().float().cpu()
    # stores: all of [0, Nout) written, nothing else touched
    assert torch.isfinite(got).all()
    other = torch.ones(ldy, dtype=torch.bool)
    other[off:off + Cout] = False
    if other.any():
        assert torch.isnan(ybuf[:, other.to(DEV)]).all()
    # the two launches it replaces, on the same inputs
    # (the plain convolution on the SAME descriptor, hence the same kernel family; its output window is then copied to a dense
    # tensor, because the element pass takes row strides in multiples of 16 bytes only)
    rawbuf = torch.full((N * H * W, ldy), float("nan"), dtype=dt, device=DEV)
    rawwin = Act(rawbuf, off, Cout, N, H, W)
    L.check(lib.uz_conv_igemm(byref(d), xa.ptr(), wp.data_ptr(), bd.data_ptr(), rawwin.ptr(), None, L.stream_ptr()), "uz_conv_igemm")
    raw = ops.new_act(N, H, W, Cout, dt, DEV)
    raw.buf.copy_(rawbuf[:, off:off + Cout])
    two = ops.new_act(N, H, W, Cout, dt, DEV)
    ops.bn_relu_apply(raw, sc, sh, two, relu=bool(relu))       # uz_bn_relu_apply's kernel (its flag word carries relu = 0)
    two = two.dense().float().cpu()
    e1, e2 = rms(got, ref), rms(two, ref)
    print(f"{kernel} relu={relu}: rel err folded {relerr(got, ref):.3e} two-launch {relerr(two, ref):.3e}; rms {e1:.4e} vs {e2:.4e}")
    if dt == torch.float32:
        assert torch.equal(got, two)
        assert relerr(got, ref) < 1e-5
    else:
        assert relerr(got, ref) < 2e-2
        assert e1 <= e2
    # bitwise repeatable
    ybuf2 = torch.full((N * H * W, ldy), float("nan"), dtype=dt, device=DEV)
    y2 = Act(ybuf2, off, Cout, N, H, W)
    L.check(lib.uz_conv_igemm_bnact(byref(d), xa.ptr(), wp.data_ptr(), bd.data_ptr(), sc.data_ptr(), sh.data_ptr(), relu,
                                    y2.ptr(), L.stream_ptr()), "uz_conv_igemm_bnact")
    assert torch.equal(y.dense(), y2.dense())


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("N,H,W", [(2, 32, 32), (1, 24, 40)])
def test_first_layer_bnact_against_two_launches(N, H, W, relu):
    dt = torch.bfloat16
    Cout = 64
    g = torch.Generator().manual_seed(32)
    x = torch.randn(N, 3, H, W, generator=g)
    w = torch.randn(Cout, 3, 3, 3, generator=g) * 0.2
    b = torch.randn(Cout, generator=g)
    pre = F.conv2d(x.to(dt).double(), w.to(dt).double(), b.double(), padding=1)     # the kernels round x and w to bf16
    scale, shift = scale_shift(g, Cout, pre)
    ref = pre * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    if relu:
        ref = ref.clamp_min(0.0)
        assert 0.3 < (ref == 0).double().mean() < 0.7
    xd, wd, bd, sc, sh = x.to(DEV), w.to(DEV), b.to(DEV), scale.to(DEV), shift.to(DEV)
    ybuf = torch.full((N * H * W, 2 * Cout), float("nan"), dtype=dt, device=DEV)
    y = Act(ybuf, Cout, Cout, N, H, W)               # the upper half of a wider buffer
    lib = L.load()
    L.check(lib.uz_conv3x3_first_fwd_bnact(L.dtype_code(dt), xd.data_ptr(), N, 3, H, W, wd.data_ptr(), bd.data_ptr(), Cout,
                                           sc.data_ptr(), sh.data_ptr(), relu, y.ptr(), y.ld, L.stream_ptr()),
            "uz_conv3x3_first_fwd_bnact")
    got = y.dense().float().cpu()
    assert torch.isfinite(got).all() and torch.isnan(ybuf[:, :Cout]).all()
    raw = ops.new_act(N, H, W, Cout, dt, DEV)
    ops.conv_first_fwd(xd, wd, bd, raw, False)
    two = ops.new_act(N, H, W, Cout, dt, DEV)
    ops.bn_relu_apply(raw, sc, sh, two, relu=bool(relu))       # uz_bn_relu_apply's kernel (its flag word carries relu = 0)
    two = two.dense().float().cpu()
    e1, e2 = rms(got, ref), rms(two, ref)
    print(f"first layer {N}x{H}x{W} relu={relu}: rel err folded {relerr(got, ref):.3e} two-launch {relerr(two, ref):.3e}; "
          f"rms {e1:.4e} vs {e2:.4e}")
    assert relerr(got, ref) < 2e-2
    assert e1 <= e2


def test_unsupported_descriptors_are_refused_without_a_launch():
    dt = torch.bfloat16
    lib = L.load()
    N, H, W, Cin, Co = 1, 8, 8, 64, 32
    code = L.dtype_code(dt)
    cases = {
        # (descriptor, input pixels, output pixels)
        # ConvTranspose2d k2 s2 forward: 1x1 taps, sub-pixel shuffle store
        "shuffle store": (L.ConvDesc(code, N, H, W, H, W, Cin, Cin, 4 * Co, Co, 1, L.TAPS_CONV, 1, L.STORE_SHUFFLE2X2, Co, 0, 0),
                          N * H * W, N * 4 * H * W),
        # its input gradient: 2 x 2 gather
        "gather": (L.ConvDesc(code, N, H, W, 2 * H, 2 * W, Cin, Cin, 4 * Co, 4 * Co, 4, L.TAPS_GATHER2X2, 1, L.STORE_PLAIN, 0, 0, 0),
                   N * 4 * H * W, N * H * W),
        # a 1x1 convolution on the LDS-DMA GEMM
        "1x1 on gemm_dma": (desc(dt, N, H, W, Cin, Cin, 4 * Co, 4 * Co, ntaps=1), N * H * W, N * H * W),
        # unet's 1024 -> 512 at 16 x 16, B = 16: a split-K plan of the ping-pong kernel
        "split-K": (desc(dt, 16, 16, 16, 1024, 1024, 512, 512), 16 * 256, 16 * 256),
    }
    assert ops.conv_kernel_name(cases["1x1 on gemm_dma"][0]).startswith("gemm_dma")
    assert ops.conv_kernel_name(cases["split-K"][0], with_workspace=True).endswith("_splitk")
    for what, (d, pin, pout) in cases.items():
        assert lib.uz_conv_igemm_bnact_supported(byref(d)) == 0, what
        # operands of the full size the descriptor states: a launch, were there one, would stay inside them and show in y
        x = torch.zeros(pin, d.ldx, dtype=dt, device=DEV)
        wp = torch.zeros(d.Nout, d.ntaps * d.Cin, dtype=dt, device=DEV)
        sc = torch.ones(d.Nout, device=DEV)
        y = torch.full((pout, d.ldy), float("nan"), dtype=dt, device=DEV)
        rc = lib.uz_conv_igemm_bnact(byref(d), x.data_ptr(), wp.data_ptr(), None, sc.data_ptr(), sc.data_ptr(), 1,
                                     y.data_ptr(), L.stream_ptr())
        assert rc == -2, (what, rc)          # UZ_ENOTIMPL
        torch.cuda.synchronize()
        assert torch.isnan(y).all(), what    # nothing was launched
