"""The three products of the 1x1 head restated with torch in float64 (the checker of tests/test_head_wide_gpu.py).

Inputs are taken exactly as the kernels see them: x is (P, C) in the run dtype (bf16 values are widened, which is exact),
w (K, C), b (K) and g (N, K, HW) are fp32.  Besides each product the functions return the sum of the absolute values of its
addends, which the error bounds of the tests are stated in."""
import torch


def _x64(x):
    return x.detach().cpu().to(torch.float64)   # bf16 -> float64 is exact


def forward(x, w, b, N, HW):
    """out (N, K, HW) = b + x w^T, and sum_c |w| |x| in the same shape"""
    x, w, b = _x64(x), _x64(w), _x64(b)
    K = w.shape[0]
    out = (x @ w.t() + b).reshape(N, HW, K).permute(0, 2, 1).contiguous()
    mag = (x.abs() @ w.abs().t()).reshape(N, HW, K).permute(0, 2, 1).contiguous()
    return out, mag


def _g_pk(g):
    N, K, HW = g.shape
    return _x64(g).permute(0, 2, 1).reshape(N * HW, K)


def input_grad(g, w):
    """dx (P, C) = g w, and sum_k |g| |w|"""
    gp, w = _g_pk(g), _x64(w)
    return gp @ w, gp.abs() @ w.abs()


def weight_grads(g, x):
    """dw (K, C) = sum_p g x, db (K) = sum_p g, and the sums of |g| |x| and |g|"""
    gp, x = _g_pk(g), _x64(x)
    return gp.t() @ x, gp.sum(0), gp.abs().t() @ x.abs(), gp.abs().sum(0)
