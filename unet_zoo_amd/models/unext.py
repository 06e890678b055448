"""UNeXt / UNeXt-S on the HIP engine (reference graph: unet_zoo/models/unext.py — a MiT/PVT-style encoder of three
overlapping patch embeddings with pre-norm transformer blocks, a three-convolution decoder, a x4 bilinear head).

Tokens are NHWC activations, so every `permute / reshape / flatten` between the reference's (B, C, H, W) maps and
(B, N, C) token tensors disappears.  What runs on the GPU:

  * the 7x7 stride-4 embedding of the image as im2col + GEMM, the 3x3 stride-2 embeddings on the LDS-DMA GEMM;
  * LayerNorm; Linear layers with the blocks' residual sums in the GEMM epilogue;
  * spatial-reduction attention: the r x r reduction convolution (space-to-depth + GEMM) and softmax(q k^T * scale) v
    on MFMA for head sizes that are multiples of 8 up to 128 (`uz_sra_*`; UNeXt's are 128 / 80 / 64);
  * the MLP: fc1 -> depthwise 3x3 (`uz_dwconv3x3`) -> GELU -> fc2;
  * the decoder's bilinear align_corners=True resizes and 3x3 convolutions with the `+ skip` in their epilogue;
  * the head `final_conv(final_up(x))` as the 1x1 convolution at quarter resolution followed by the x4 resize of the
    logit planes (Engine.out_conv_resized): no full-resolution embed_dims[0]-channel tensor is ever made.

Module registration order, names and initialisation follow the reference constructor, so `state_dict()` keys and a
seed-0 construction match it tensor for tensor (tests/golden/unext_manifest.json, unext_s_manifest.json).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from ..engine import Engine
from ..graph import HipModule
from ..ops import Act

SRA_HEAD_DIMS = range(8, 129, 8)   # head sizes the attention kernels take


def _head_check(dim: int, num_heads: int) -> None:
    assert dim % num_heads == 0, f"dim {dim} should be divided by num_heads {num_heads}."
    if dim // num_heads not in SRA_HEAD_DIMS:
        raise NotImplementedError(f"UNext on the HIP engine: the attention kernels take head sizes that are multiples "
                                  f"of 8 from 8 to 128, got dim={dim}, num_heads={num_heads} "
                                  f"(head size {dim / num_heads:g})")


class DropPath(nn.Module):
    """unext.py DropPath (registered only for drop_path > 0, which the engine refuses in training)"""

    def __init__(self, drop_prob=None):
        super().__init__()
        self.drop_prob = drop_prob


class DWConv(nn.Module):
    def __init__(self, dim=768):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, 3, 1, 1, bias=True, groups=dim)


class MLP(nn.Module):
    """fc1 -> DWConv -> GELU -> fc2 (dropout p = drop, refused in training when > 0)"""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.dwconv = DWConv(hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)

    def emit(self, eng: Engine, x: Act, residual: Optional[Act] = None) -> Act:
        a = eng.gelu(eng.dwconv_skip(eng.linear(x, self.fc1), self.dwconv.dwconv, skip=False))
        return eng.linear(a, self.fc2, residual=residual)


class Attention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0., sr_ratio=1):
        super().__init__()
        _head_check(dim, num_heads)
        self.dim = dim
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.q = nn.Linear(dim, dim, bias=qkv_bias)
        self.kv = nn.Linear(dim, dim * 2, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.sr_ratio = sr_ratio
        if sr_ratio > 1:
            self.sr = nn.Conv2d(dim, dim, kernel_size=sr_ratio, stride=sr_ratio)
            self.norm = nn.LayerNorm(dim)

    def emit(self, eng: Engine, x: Act, residual: Optional[Act] = None) -> Act:
        q = eng.linear(x, self.q)
        if self.sr_ratio > 1:       # r x r, stride r: a border that r does not divide is dropped, as Conv2d does
            red = eng.layer_norm(eng.patch_conv(x, self.sr), self.norm)
        else:
            red = x
        kv = eng.linear(red, self.kv)
        o = eng.sr_attention(q, kv, x.N, self.num_heads, kv.P // x.N, self.scale)
        return eng.linear(o, self.proj, residual=residual)


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0.,
                 drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm, sr_ratio=1):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale,
                              attn_drop=attn_drop, proj_drop=drop, sr_ratio=sr_ratio)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = MLP(in_features=dim, hidden_features=mlp_hidden_dim, act_layer=act_layer, drop=drop)

    def emit(self, eng: Engine, x: Act) -> Act:
        tx = self.attn.emit(eng, eng.layer_norm(x, self.norm1), residual=x)     # x + attn(norm1(x)): GEMM epilogue
        return self.mlp.emit(eng, eng.layer_norm(tx, self.norm2), residual=tx)  # tx + mlp(norm2(tx))


class OverlapPatchEmbed(nn.Module):
    def __init__(self, img_size=224, patch_size=7, stride=4, in_chans=3, embed_dim=768):
        super().__init__()
        img_size = (img_size, img_size) if isinstance(img_size, int) else img_size
        patch_size = (patch_size, patch_size) if isinstance(patch_size, int) else patch_size
        self.img_size = img_size
        self.patch_size = patch_size
        self.H, self.W = img_size[0] // stride, img_size[1] // stride
        self.num_patches = self.H * self.W
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=stride,
                              padding=(patch_size[0] // 2, patch_size[1] // 2))
        self.norm = nn.LayerNorm(embed_dim)

    def emit(self, eng: Engine, x) -> Act:
        y = eng.conv_input(x, self.proj) if isinstance(x, torch.Tensor) else eng.conv3x3_s2(x, self.proj)
        return eng.layer_norm(y, self.norm)


class UNext(HipModule):
    """Same constructor as the reference's UNext, without its catch-all **kwargs: an argument it does not know raises
    TypeError.  Refused (NotImplementedError): head sizes outside SRA_HEAD_DIMS, a norm_layer other than nn.LayerNorm,
    and dropout / drop-path rates > 0 in a training-mode forward."""

    def __init__(self, input_channels=3, num_classes=1, img_size=224, embed_dims=None,
                 num_heads=None, mlp_ratios=None, qkv_bias=False, qk_scale=None,
                 drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0,
                 norm_layer=nn.LayerNorm, depths=None, sr_ratios=None):
        super().__init__()
        if norm_layer is not nn.LayerNorm:
            raise NotImplementedError(f"UNext on the HIP engine: norm_layer must be nn.LayerNorm, got {norm_layer!r}")
        if embed_dims is None:
            embed_dims = [128, 160, 256]
        if num_heads is None:
            num_heads = [1, 2, 4, 8]
        if mlp_ratios is None:
            mlp_ratios = [4, 4, 4, 4]
        if depths is None:
            depths = [3, 4, 6, 3]
        if sr_ratios is None:
            sr_ratios = [8, 4, 2, 1]
        for i in range(3):
            _head_check(embed_dims[i], num_heads[i])
        self.num_classes = num_classes
        self.depths = depths
        self.sr_ratios = sr_ratios
        self.drop_rates = (drop_rate, attn_drop_rate, drop_path_rate)

        self.patch_embed1 = OverlapPatchEmbed(img_size=img_size, patch_size=7, stride=4,
                                              in_chans=input_channels, embed_dim=embed_dims[0])
        self.patch_embed2 = OverlapPatchEmbed(img_size=img_size // 4, patch_size=3, stride=2,
                                              in_chans=embed_dims[0], embed_dim=embed_dims[1])
        self.patch_embed3 = OverlapPatchEmbed(img_size=img_size // 8, patch_size=3, stride=2,
                                              in_chans=embed_dims[1], embed_dim=embed_dims[2])

        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, sum(depths))]
        cur = 0
        for s in range(3):
            setattr(self, f"block{s + 1}", nn.ModuleList([Block(
                dim=embed_dims[s], num_heads=num_heads[s], mlp_ratio=mlp_ratios[s], qkv_bias=qkv_bias,
                qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate, drop_path=dpr[cur + i],
                norm_layer=norm_layer, sr_ratio=sr_ratios[s])
                for i in range(depths[s])]))
            setattr(self, f"norm{s + 1}", norm_layer(embed_dims[s]))
            cur += depths[s]

        self.decoder_level1 = nn.Conv2d(embed_dims[2], embed_dims[1], 3, padding=1)
        self.decoder_level2 = nn.Conv2d(embed_dims[1], embed_dims[0], 3, padding=1)
        self.decoder_level3 = nn.Conv2d(embed_dims[0], embed_dims[0], 3, padding=1)
        self.final_up = nn.Upsample(scale_factor=4, mode='bilinear', align_corners=True)
        self.final_conv = nn.Conv2d(embed_dims[0], num_classes, 1)

        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)
        elif isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)

    def token_maps(self, H: int, W: int):
        """(h, w) of the three token maps for an H x W input: k7 s4 p3, then k3 s2 p1 twice"""
        h, w = (H - 1) // 4 + 1, (W - 1) // 4 + 1
        maps = [(h, w)]
        for _ in range(2):
            h, w = (h + 1) // 2, (w + 1) // 2
            maps.append((h, w))
        return maps

    def check_input_size(self, H: int, W: int) -> None:
        """Every size runs (odd ones included) as long as each reduction convolution has a full r x r window; the
        reference's Conv2d fails below that too.  Checked before anything is launched."""
        for s, (h, w) in enumerate(self.token_maps(H, W)):
            r = self.sr_ratios[s] if self.depths[s] > 0 else 1
            if r > 1 and (h < r or w < r):
                raise ValueError(f"UNext: a {H}x{W} input gives a {h}x{w} token map at stage {s + 1}, smaller than its "
                                 f"reduction ratio {r}")

    def emit(self, eng: Engine, x: torch.Tensor):
        if self.training and any(p > 0 for p in self.drop_rates):
            raise NotImplementedError("UNext on the HIP engine: drop_rate / attn_drop_rate / drop_path_rate > 0 in "
                                      f"training are not supported (got {self.drop_rates})")
        N, _, H, W = x.shape
        self.check_input_size(H, W)
        t = x
        skips = []
        for s in range(1, 4):
            t = getattr(self, f"patch_embed{s}").emit(eng, t)
            for blk in getattr(self, f"block{s}"):
                t = blk.emit(eng, t)
            t = eng.layer_norm(t, getattr(self, f"norm{s}"))
            skips.append(t)
        x1, x2, x3 = skips
        # F.interpolate(x3, size=x2's, bilinear, align_corners=True) -> decoder_level1 (+ x2 in its epilogue)
        up = eng.resize_bilinear(x3, eng.new_act(N, x2.H, x2.W, x3.C), align_corners=True)
        y = eng.conv_plain(up, self.decoder_level1, residual=x2)
        up = eng.resize_bilinear(y, eng.new_act(N, x1.H, x1.W, y.C), align_corners=True)
        y = eng.conv_plain(up, self.decoder_level2, residual=x1)
        y = eng.conv_plain(y, self.decoder_level3)
        # final_conv(final_up(y)) = resize(final_conv(y)): the 1x1 convolution at quarter resolution
        return (eng.out_conv_resized(y, self.final_conv, 4 * y.H, 4 * y.W, align_corners=True),)


class UNext_S(UNext):
    """UNeXt-S: embed_dims [64, 128, 160], num_heads [1, 2, 4], depths [2, 2, 2]; the five structure arguments are
    dropped from **kwargs, as in the reference."""

    def __init__(self, input_channels=3, num_classes=1, img_size=224, **kwargs):
        for k in ('embed_dims', 'num_heads', 'depths', 'sr_ratios', 'mlp_ratios'):
            kwargs.pop(k, None)
        super().__init__(input_channels=input_channels, num_classes=num_classes, img_size=img_size,
                         embed_dims=[64, 128, 160], num_heads=[1, 2, 4], mlp_ratios=[4, 4, 4], depths=[2, 2, 2],
                         sr_ratios=[8, 4, 2], **kwargs)
