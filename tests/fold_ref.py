"""TEST INFRASTRUCTURE.  Loader for tests/ref/uz_fold_ref.c, the plain-C restatement of uz_bn_relu_bwd_apply_head and
uz_conv3x3_first_wgrad_bn (host pointers), and the inputs the two GPU test files share."""
import ctypes
import os
import subprocess
import tempfile

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def load():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="uz_fold_ref_"), "libuz_fold_ref.so")
        subprocess.run(["cc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-o", out,
                        os.path.join(_HERE, "ref", "uz_fold_ref.c"), "-lm"], check=True)
        lib = ctypes.CDLL(out)
        ip, vp, dbl = ctypes.c_int, ctypes.c_void_p, ctypes.c_double
        lib.uz_bn_relu_bwd_apply_head_ref.argtypes = [ip, ip, ip, ip, ip, ip, vp, vp, vp, vp, vp, vp, vp, ip, vp, dbl, vp]
        lib.uz_conv3x3_first_wgrad_bn_ref.argtypes = [vp, ip, ip, ip, ip, vp, ip, vp, ip, vp, vp, vp, vp, vp, dbl, ip, vp]
        _lib = lib
    return _lib


def bn_case(P, C, g):
    """raw convolution output y (P, C) bf16 and vec = (scale, shift, mean, invstd) of a BatchNorm over it, with the hard
    channels: 0 -- pre-activation <= 0 everywhere (all-zero mask); 1 -- negative gamma; the rest ordinary"""
    y = torch.randn(P, C, generator=g).to(torch.bfloat16)
    yf = y.float()
    mean, var = yf.mean(0), yf.var(0, unbiased=False)
    invstd = (var + 1e-5).rsqrt()
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    gamma[1] = -gamma[1]
    beta[0] = -50.0
    scale = gamma * invstd
    shift = beta - mean * scale
    assert (torch.addcmul(shift[0], yf[:, 0], scale[0]) <= 0).all()
    return y, torch.stack([scale, shift, mean, invstd]).contiguous()


def bits(t):
    """the tensor's bit patterns (bf16 / fp32): -0.0 and 0.0 differ, NaN equals itself"""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def agree_bf16(got, ref, what):
    """the bf16 criterion of tests/test_c_ref_gpu.py::agree"""
    got, ref = got.detach().cpu().double(), ref.double()
    den = ref.abs() + 1e-2 * ref.abs().max() + 1e-30
    err = ((got - ref).abs() / den).max().item()
    assert err <= 2.0 ** -7, (what, err)
    same = (got == ref).double().mean().item()
    assert same > 0.97, (what, same)
