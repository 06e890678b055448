"""TEST INFRASTRUCTURE.  What the window-attention GPU tests (test_swin_gpu.py, test_winattn_walk_gpu.py,
test_winattn_wide_gpu.py) share: the restatement of the reference model's attention core, which they run in float64 on the
CPU, and the grid rule of uz_winattn.hip."""
import torch

from oracle import torch_ref

NUM_CU = 256


def attention_core_ref(qkv, tau, bias, heads, ws, shift):
    """the reference's roll -> window_partition -> cosine attention -> window_reverse -> roll back
    (swin_unet_v2.py:127-159, 246-262) on a (B, H, W, 3C) qkv tensor, without the qkv / proj Linears"""
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    d = C // heads
    xs = torch.roll(qkv, shifts=(-shift, -shift), dims=(1, 2)) if shift > 0 else qkv
    xw = xs.view(B, H // ws, ws, W // ws, ws, C3).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C3)
    B_, N, _ = xw.shape
    t = xw.reshape(B_, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    q, k, v = t[0] * d ** -0.5, t[1], t[2]
    attn = torch.einsum("bhqd,bhkd->bhqk", q, k) / torch.maximum(
        q.norm(dim=-1, keepdim=True) * k.norm(dim=-1, keepdim=True).transpose(-2, -1), torch.tensor(1e-6))
    attn = attn / torch.clip(tau.unsqueeze(0)[:, :, :N, :N], min=0.01) + bias.unsqueeze(0)
    if shift > 0:
        mask = torch_ref.swin_attention_mask(H, W, ws, shift)
        nW = mask.shape[0]
        attn = (attn.view(B_ // nW, nW, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, N, N)
    o = (attn.softmax(-1) @ v).transpose(1, 2).reshape(B_, N, C)
    o = o.view(B, H // ws, W // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    return torch.roll(o, shifts=(shift, shift), dims=(1, 2)) if shift > 0 else o


def grid(nwin, heads, slots, num_cu=NUM_CU):
    """attn_grid_x() of uz_winattn.hip: the windows are dealt evenly over at most num_cu * slots / heads workgroups"""
    cap = max(1, num_cu * slots // heads)
    per = -(-nwin // cap)
    return -(-nwin // per)
