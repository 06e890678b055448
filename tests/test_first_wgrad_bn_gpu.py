"""GPU: the first layer's weight gradient reads the activation's gradient through the BatchNorm + ReLU backward
(uz_conv3x3_first_wgrad_bn, Engine.fold_first_bn_bwd) against the two launches that write and re-read dy
(uz_bn_relu_bwd_apply + uz_conv3x3_first_wgrad, unchanged by this work) -- bit for bit -- and against the plain-C
restatement (tests/ref/)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import c_ref
import fold_ref  # tests/fold_ref.py (pytest puts this directory on sys.path)
from unet_zoo_amd import ops
from unet_zoo_amd.ops import Act

DEV = "cuda"


@pytest.mark.parametrize("Cout", [32, 64])
@pytest.mark.parametrize("Cin", [1, 3])
@pytest.mark.parametrize("H,W", [(8, 32), (9, 33), (20, 40)])   # one tile; tails both ways; several tiles per workgroup
def test_weight_gradient_through_the_batchnorm_backward_bitwise(H, W, Cin, Cout):
    N = 2
    P = N * H * W
    g = torch.Generator().manual_seed(100 * H + 10 * Cin + Cout)
    y, vec = fold_ref.bn_case(P, Cout, g)
    x = torch.randn(N, Cin, H, W, generator=g)
    gr = torch.randn(P, Cout, generator=g).to(torch.bfloat16)
    gr[::7] = 0.0                      # exact zeros
    gr[:, 5] = 0.0
    ya, ga, xd, vd = Act(y.to(DEV), 0, Cout, N, H, W), Act(gr.to(DEV), 0, Cout, N, H, W), x.to(DEV), vec.to(DEV)
    # the two launches
    dy = ops.new_act(N, H, W, Cout, torch.bfloat16, DEV)
    s0 = torch.empty(2, Cout, dtype=torch.float64, device=DEV)
    dg0, db0 = torch.empty(Cout, device=DEV), torch.empty(Cout, device=DEV)
    ops.bn_relu_bwd(ya, vd, ga, None, None, s0, dy, dg0, db0)
    dw0 = ops.conv_first_wgrad(xd, dy)
    # no dy
    s1 = torch.empty(2, Cout, dtype=torch.float64, device=DEV)
    dg1, db1 = torch.empty(Cout, device=DEV), torch.empty(Cout, device=DEV)
    ops.bn_relu_bwd(ya, vd, ga, None, None, s1, None, dg1, db1)
    dw1 = ops.conv_first_wgrad_bn(xd, ga, ya, vd, s1)
    assert torch.equal(s0, s1) and torch.equal(fold_ref.bits(dg0), fold_ref.bits(dg1)) and torch.equal(fold_ref.bits(db0), fold_ref.bits(db1))
    assert torch.equal(fold_ref.bits(dw0), fold_ref.bits(dw1))
    assert torch.isfinite(dw1).all() and dw1.abs().max() > 0
    # the restatement on the same bytes (the criterion of the first convolution's weight gradient in tests/test_c_ref_gpu.py)
    lib = fold_ref.load()
    xh, yh, gh, vh, sh = c_ref.host(x), c_ref.host(y), c_ref.host(gr), c_ref.host(vec), s1.cpu().numpy().copy()
    ref = np.zeros(Cout * Cin * 9, np.float32)
    assert lib.uz_conv3x3_first_wgrad_bn_ref(c_ref.ptr(xh), N, Cin, H, W, c_ref.ptr(gh), Cout, c_ref.ptr(yh), Cout, vh[0].ctypes.data,
                                             vh[1].ctypes.data, vh[2].ctypes.data, vh[3].ctypes.data, c_ref.ptr(sh), float(P), Cout,
                                             c_ref.ptr(ref)) == 0
    r = torch.from_numpy(ref).reshape(Cout, Cin, 3, 3).double()
    assert ((dw1.cpu().double() - r).abs().max() / r.abs().max()).item() < 1e-5
