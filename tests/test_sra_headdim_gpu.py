"""GPU: spatial-reduction attention (uz_sra_fwd / uz_sra_bwd) for head sizes other than 64 -- the multiples of 8 from
8 to 128 that UNeXt needs (128 / 80 / 64, UNeXt-S 64 / 64 / 40) -- in both run modes, against torch autograd and
against the C restatement uz_sra_fwd_ref / uz_sra_bwd_ref.  Query counts that are not a multiple of 128, key counts
that are not a multiple of 32, one and four key segments."""
from ctypes import byref

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import c_ref
from unet_zoo_amd import _lib as L
from unet_zoo_amd import ops
from unet_zoo_amd.ops import Act, act_from_nchw

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
HEAD_DIMS = [8, 40, 64, 80, 128]


def rnd(dt, t):
    return t.to(dt).float() if dt == torch.bfloat16 else t


def relerr(a, b):
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30)).item()


def tokens(t, dt):
    """(B, N, C) fp32 CPU -> Act with N = B, H = 1, W = N"""
    B, N, C = t.shape
    return act_from_nchw(t.permute(0, 2, 1).reshape(B, C, 1, N).contiguous().to(DEV), dt)


def untokens(a):
    return a.dense().cpu().reshape(a.N, a.C, a.H * a.W).permute(0, 2, 1)


def _sra_reference(q, kv, heads, scale):
    B, N, C = q.shape
    d = C // heads
    qh = q.reshape(B, N, heads, d).permute(0, 2, 1, 3)
    kvh = kv.reshape(B, -1, 2, heads, d).permute(2, 0, 3, 1, 4)
    attn = ((qh @ kvh[0].transpose(-2, -1)) * scale).softmax(dim=-1)
    return (attn @ kvh[1]).transpose(1, 2).reshape(B, N, C)


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", HEAD_DIMS)
@pytest.mark.parametrize("heads", [1, 2, 4])
@pytest.mark.parametrize("B,N,NK,nseg", [(2, 200, 49, 1), (1, 340, 100, 4)])
def test_sra_head_dim_against_autograd(dt, D, heads, B, N, NK, nseg):
    g = torch.Generator().manual_seed(31 + D)
    C = heads * D
    q = rnd(dt, torch.randn(B, N, C, generator=g)).requires_grad_(True)
    kv = rnd(dt, torch.randn(B, NK, 2 * C, generator=g)).requires_grad_(True)
    go = rnd(dt, torch.randn(B, N, C, generator=g))
    scale = D ** -0.5
    ref = _sra_reference(q, kv, heads, scale)
    ref.backward(go)
    kps = NK // nseg
    kv_dev = kv.detach().reshape(B, nseg, kps, 2 * C).permute(1, 0, 2, 3).reshape(1, nseg * B * kps, 2 * C)
    qa, kva, goa = tokens(q.detach(), dt), tokens(kv_dev, dt), tokens(go, dt)
    out, dq, dkv = ops.new_act(B, 1, N, C, dt, DEV), ops.new_act(B, 1, N, C, dt, DEV), ops.new_act(1, 1, B * NK, 2 * C, dt, DEV)
    lse = ops.sra_fwd(qa, kva, out, B, heads, kps, scale)
    ops.sra_bwd(qa, kva, out, lse, goa, dq, dkv, B, heads, kps, scale)
    tol = 2e-5 if dt == torch.float32 else 2e-2
    assert relerr(untokens(out), ref.detach()) < tol
    assert relerr(untokens(dq), q.grad) < tol
    dkv_ref = kv.grad.reshape(B, nseg, kps, 2 * C).permute(1, 0, 2, 3).reshape(1, nseg * B * kps, 2 * C)
    assert relerr(untokens(dkv), dkv_ref) < tol


def _npdt(dt):
    return np.float32 if dt == torch.float32 else np.uint16


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", HEAD_DIMS)
@pytest.mark.parametrize("B,Nq,heads,kps,blocks", [(2, 150, 2, 19, 1), (1, 77, 1, 9, 4)])
def test_sra_head_dim_against_the_c_restatement(dt, D, B, Nq, heads, kps, blocks):
    ref = c_ref.load()
    g = torch.Generator().manual_seed(77 + D)
    NK, HD = kps * blocks, heads * D
    scale = D ** -0.5
    q, kv, go = (rnd(dt, torch.randn(s, generator=g)) for s in ((B * Nq, HD), (B * NK, 2 * HD), (B * Nq, HD)))
    dev = lambda t: t.to(dt).to(DEV).contiguous()
    qa, kva, goa = Act(dev(q), 0, HD, B, 1, Nq), Act(dev(kv), 0, 2 * HD, B, 1, NK), Act(dev(go), 0, HD, B, 1, Nq)
    out = ops.new_act(B, 1, Nq, HD, dt, DEV)
    lse = ops.sra_fwd(qa, kva, out, B, heads, kps, scale)
    d = L.SraDesc(L.dtype_code(dt), B, Nq, NK, heads, D, kps, HD, 2 * HD, 2 * HD, HD, scale)
    h = c_ref.host
    qh, kvh = h(q.to(dt)), h(kv.to(dt))
    orf, lr = np.zeros(B * Nq * HD, _npdt(dt)), np.zeros(B * heads * Nq, np.float32)
    vptr = kvh.ctypes.data + HD * kvh.itemsize
    assert ref.uz_sra_fwd_ref(byref(d), c_ref.ptr(qh), c_ref.ptr(kvh), vptr, c_ref.ptr(orf), c_ref.ptr(lr), None) == 0
    want = c_ref.tensor(orf, dt).reshape(-1, HD)
    assert relerr(out.buf.float().cpu(), want.float()) < (1e-4 if dt == torch.float32 else 1e-2)
    assert np.allclose(lse.cpu().numpy(), lr, rtol=1e-3, atol=1e-3)
    dq, dkv = ops.new_act(B, 1, Nq, HD, dt, DEV), ops.new_act(B, 1, NK, 2 * HD, dt, DEV)
    ops.sra_bwd(qa, kva, out, lse, goa, dq, dkv, B, heads, kps, scale)
    oh, goh = h(out.buf), h(go.to(dt))
    lk = lse.cpu().numpy().copy()
    dqr, dkvr = np.zeros(B * Nq * HD, _npdt(dt)), np.zeros(B * NK * 2 * HD, _npdt(dt))
    assert ref.uz_sra_bwd_ref(byref(d), c_ref.ptr(qh), c_ref.ptr(kvh), vptr, c_ref.ptr(oh), c_ref.ptr(lk), c_ref.ptr(goh),
                              HD, c_ref.ptr(dqr), HD, c_ref.ptr(dkvr), 2 * HD, None, None) == 0
    for got, want, what in ((dq.buf, dqr, "dq"), (dkv.buf, dkvr, "dkv")):
        want = c_ref.tensor(want, dt).reshape(got.shape)
        assert relerr(got.float().cpu(), want.float()) < (1e-4 if dt == torch.float32 else 2e-2), what
