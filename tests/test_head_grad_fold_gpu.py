"""GPU: the 1x1 head's rank-K input gradient is not written down (Engine.fold_head_grad): uz_outconv_bwd_bnred with
dx = NULL + uz_bn_relu_bwd_apply_head against the two launches that store and re-read it (uz_outconv_bwd_bnred +
uz_bn_relu_bwd_apply, unchanged by this work) -- bit for bit -- and against the plain-C restatement (tests/ref/)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import c_ref
import fold_ref  # tests/fold_ref.py (pytest puts this directory on sys.path)
from unet_zoo_amd import ops
from unet_zoo_amd.ops import Act

DEV = "cuda"


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("C", [32, 64, 72])
@pytest.mark.parametrize("H,W", [(5, 7), (16, 16), (33, 9)])
def test_apply_pass_forms_the_head_gradient_bitwise(H, W, C, K):
    N = 2
    P = N * H * W
    g = torch.Generator().manual_seed(1000 * K + 10 * C + H)
    y, vec = fold_ref.bn_case(P, C, g)
    w = torch.randn(K, C, generator=g) * 0.3
    gl = torch.randn(N, K, H, W, generator=g)
    gl[0, :, H // 2] = 0.0          # exact zeros: a row of pixels without a logit gradient
    gl[:, K - 1, :, 0] = 0.0
    ya = Act(y.to(DEV), 0, C, N, H, W)
    xa = Act(ya.buf, 0, C, N, H, W)          # the lazy activation: only a shape for the head's backward
    vd, wd, gd = vec.to(DEV), w.to(DEV), gl.to(DEV)
    for reverse in (False, True):
        # the two launches: dx stored by the head, read back by the apply pass
        dx = ops.new_act(N, H, W, C, torch.bfloat16, DEV)
        dw0, db0 = ops.outconv_bwd(xa, wd, gd, dx, bnred=(ya, vd), lazy=True)
        dy0 = ops.new_act(N, H, W, C, torch.bfloat16, DEV)
        s0 = torch.empty(2, C, dtype=torch.float64, device=DEV)
        dg0, dbt0 = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        ops.bn_relu_bwd(ya, vd, dx, None, None, s0, dy0, dg0, dbt0, partials=dx.bn_partials, reverse=reverse)
        # nothing stored
        dw1, db1, part = ops.outconv_bwd(xa, wd, gd, None, bnred=(ya, vd), lazy=True, store_dx=False)
        dy1 = ops.new_act(N, H, W, C, torch.bfloat16, DEV)
        s1 = torch.empty(2, C, dtype=torch.float64, device=DEV)
        dg1, dbt1 = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        ops.bn_relu_bwd_head(ya, vd, ops.HeadGrad(gd, wd, part), s1, dy1, dg1, dbt1, reverse=reverse)
        assert torch.equal(part, dx.bn_partials) and torch.equal(s0, s1)
        assert torch.equal(fold_ref.bits(dy0.buf), fold_ref.bits(dy1.buf))
        assert torch.equal(fold_ref.bits(dg0), fold_ref.bits(dg1)) and torch.equal(fold_ref.bits(dbt0), fold_ref.bits(dbt1))
        assert torch.equal(fold_ref.bits(dw0), fold_ref.bits(dw1)) and torch.equal(fold_ref.bits(db0), fold_ref.bits(db1))
    # channel 0 (mask all zero) has a zero gradient; the others, negative gamma included, do not
    assert dy1.buf[:, 0].float().abs().max() == 0 and (dy1.buf[:, 1:3].float().abs().amax(0) > 0).all()
    assert torch.isfinite(dy1.buf.float()).all()
    # the restatement on the same bytes
    lib = fold_ref.load()
    yh, vh, wh, gh, sh = c_ref.host(y), c_ref.host(vec), c_ref.host(w), c_ref.host(gl), s1.cpu().numpy().copy()
    ref = np.zeros(P * C, np.uint16)
    assert lib.uz_bn_relu_bwd_apply_head_ref(N, H, W, C, C, C, c_ref.ptr(yh), vh[0].ctypes.data, vh[1].ctypes.data, vh[2].ctypes.data,
                                             vh[3].ctypes.data, c_ref.ptr(gh), c_ref.ptr(wh), K, c_ref.ptr(sh), float(P),
                                             c_ref.ptr(ref)) == 0
    fold_ref.agree_bf16(dy1.buf, c_ref.tensor(ref, torch.bfloat16).reshape(P, C), f"head apply {H}x{W} C={C} K={K}")


def test_unsupported_shapes_are_refused():
    y = ops.new_act(1, 4, 4, 64, torch.bfloat16, DEV)
    assert ops.bn_bwd_head_supported(y, 8) and not ops.bn_bwd_head_supported(y, 9)
    assert not ops.bn_bwd_head_supported(ops.new_act(1, 4, 4, 64, torch.float32, DEV), 1)
