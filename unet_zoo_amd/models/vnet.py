"""VNet (2-D) on the HIP engine (reference graph: unet_zoo/models/vnet.py -- residual stages of 5x5 convolutions, each followed
by an always-batch-statistics BatchNorm and ELU, 2x2 stride-2 convolutions down, 2x2 transposed convolutions up, Dropout2d
on the deep stages and on every skip).

What runs on the GPU:

  * the sixteen 5x5 layers, their input and weight gradients, and the 5x5 output layer on the k = 5 kernels of
    uz_conv5x5.hip (`Engine.conv5x5`); the 5x5 input layer as im2col + GEMM (`Engine.conv_input`);
  * BatchNorm -> ELU, the residual sum with its second ELU and the Dropout2d multiply as ONE element pass per layer
    (`Engine.bn_elu`): the dropped skip goes straight into its half of the decoder's concat buffer while the undropped tensor
    feeds the down path, so neither `torch.cat` nor a dropout pass exists;
  * the k2 s2 convolutions as space-to-depth + GEMM (`Engine.patch_conv`), the transposed ones by `Engine.conv_transpose2x2`.

Kept from the reference, odd as it is:

  * `ContBatchNorm2d` normalises with batch statistics and updates `running_mean` / `running_var` in `eval()` too, and
    `num_batches_tracked` stays 0;
  * with `in_channels` other than 1 or 16 the residual branch of the input stage goes through a 1x1 convolution that is
    created anew, with random weights, inside EVERY forward (train or eval): it is not a parameter, is not saved and gets no
    gradient, and two eval calls on one input differ.  Here its weight and bias are drawn on the device in the forward
    (uniform in +-1/sqrt(in_channels), nn.Conv2d's default for k = 1; a replayed graph draws fresh values): the same
    distribution as the reference, not the same random stream;
  * `nll` is accepted and changes nothing.

Refused: `elu=False` (PReLU) at construction; an input whose height or width is not a multiple of 16 (the reference's
zero-pad path for odd skips); a batch whose coarsest map holds a single value per channel (as torch's batch_norm does).

Module registration order, names and initialisation follow the reference constructor, so `state_dict()` keys and a seed-0
construction match it tensor for tensor (tests/golden/vnet_manifest.json).
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from ..engine import Engine
from ..graph import HipModule
from ..ops import Act
from .. import ops

N_DROPOUT_MASKS = 8
# channel width of the eight Dropout2d draws of one training forward, in call order (vnet.py:83, :102-103)
DROPOUT_WIDTHS = (128, 256, 256, 128, 256, 64, 32, 16)


class ContBatchNorm2d(nn.modules.batchnorm._BatchNorm):
    """BatchNorm2d that ALWAYS uses batch statistics (vnet.py:14-25)"""

    def _check_input_dim(self, input):
        if input.dim() != 4:
            raise ValueError('expected 4D input (got {}D input)'.format(input.dim()))


def _elu(elu: bool) -> nn.Module:
    if not elu:
        raise NotImplementedError("VNet on the HIP engine: elu=False (PReLU activations) is not supported; use elu=True")
    return nn.ELU(inplace=True)


class LUConv(nn.Module):
    def __init__(self, nchan, elu):
        super().__init__()
        self.relu1 = _elu(elu)
        self.conv1 = nn.Conv2d(nchan, nchan, kernel_size=5, padding=2)
        self.bn1 = ContBatchNorm2d(nchan)


def _make_nConv(nchan, depth, elu):
    return nn.Sequential(*[LUConv(nchan, elu) for _ in range(depth)])


def _lu_chain(eng: Engine, x: Act, ops_: nn.Sequential, res: Act, out2: Optional[Act], mask2) -> Act:
    """n x (conv5x5 -> BN -> ELU), then ELU(. + res) in the last layer's pass; out2 = the result times mask2"""
    t = x
    last = len(ops_) - 1
    for i, lu in enumerate(ops_):
        raw, st = eng.conv5x5(t, lu.conv1)
        if i < last:
            t = eng.bn_elu(raw, lu.bn1, st)
        else:
            t = eng.bn_elu(raw, lu.bn1, st, act2=True, res=res, out2=out2, mask2=mask2)
    return t


class InputTransition(nn.Module):
    def __init__(self, in_channels, out_channels_initial=16, elu=True):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels, out_channels_initial, kernel_size=5, padding=2)
        self.bn1 = ContBatchNorm2d(out_channels_initial)
        self.relu1 = _elu(elu)
        self.out_channels_initial = out_channels_initial


class DownTransition(nn.Module):
    def __init__(self, inChans, nConvs, elu, dropout=False):
        super().__init__()
        outChans = 2 * inChans
        self.down_conv = nn.Conv2d(inChans, outChans, kernel_size=2, stride=2)
        self.bn1 = ContBatchNorm2d(outChans)
        self.relu1 = _elu(elu)
        self.relu2 = _elu(elu)
        self.has_dropout = dropout
        if dropout:
            self.do1 = nn.Dropout2d()
        self.ops = _make_nConv(outChans, nConvs, elu)

    def emit(self, eng: Engine, x: Act, do_mask, out2: Optional[Act], mask2) -> Act:
        raw = eng.patch_conv(x, self.down_conv)
        if do_mask is not None:     # `down` stays undropped for the residual sum, the LUConvs read the dropped copy
            dropped = eng.new_act(raw.N, raw.H, raw.W, raw.C)
            down = eng.bn_elu(raw, self.bn1, out2=dropped, mask2=do_mask)
        else:
            down = dropped = eng.bn_elu(raw, self.bn1)
        return _lu_chain(eng, dropped, self.ops, down, out2, mask2)


class UpTransition(nn.Module):
    def __init__(self, inChans, outChans, nConvs, elu, dropout=False):
        super().__init__()
        self.up_conv = nn.ConvTranspose2d(inChans, outChans // 2, kernel_size=2, stride=2)
        self.bn1 = ContBatchNorm2d(outChans // 2)
        self.do2 = nn.Dropout2d()
        self.relu1 = _elu(elu)
        self.relu2 = _elu(elu)
        self.has_dropout = dropout
        if dropout:
            self.do1 = nn.Dropout2d()
        self.ops = _make_nConv(outChans, nConvs, elu)

    def emit(self, eng: Engine, x: Act, cat: Act, slot: Act, out2: Optional[Act], mask2) -> Act:
        """x: the (already dropped) input; cat / slot: the concat buffer, whose second half holds the dropped skip, and its
        first half"""
        raw = eng.new_act(x.N, 2 * x.H, 2 * x.W, self.up_conv.out_channels)
        eng.conv_transpose2x2(x, self.up_conv, raw)
        eng.bn_elu(raw, self.bn1, out=slot)
        return _lu_chain(eng, cat, self.ops, cat, out2, mask2)


class OutputTransition(nn.Module):
    def __init__(self, inChans, num_classes, elu=True):
        super().__init__()
        self.conv1 = nn.Conv2d(inChans, num_classes, kernel_size=5, padding=2)
        self.bn1 = ContBatchNorm2d(num_classes)
        self.relu1 = _elu(elu)


class VNet(HipModule):
    """Same constructor as the reference's VNet (vnet.py:128-143)."""

    def __init__(self, in_channels: int = 1, num_classes: int = 1, elu: bool = True, nll: bool = False):
        super().__init__()
        self.in_channels = in_channels
        self.num_classes = num_classes
        self.in_tr = InputTransition(in_channels, out_channels_initial=16, elu=elu)
        self.down_tr32 = DownTransition(16, 1, elu)
        self.down_tr64 = DownTransition(32, 2, elu)
        self.down_tr128 = DownTransition(64, 3, elu, dropout=True)
        self.down_tr256 = DownTransition(128, 2, elu, dropout=True)
        self.up_tr256 = UpTransition(256, 256, 2, elu, dropout=True)
        self.up_tr128 = UpTransition(256, 128, 2, elu, dropout=True)
        self.up_tr64 = UpTransition(128, 64, 1, elu)
        self.up_tr32 = UpTransition(64, 32, 1, elu)
        self.out_tr = OutputTransition(32, num_classes, elu=elu)
        self._forced: Optional[Tuple[Optional[tuple], Optional[list]]] = None
        self._forced_sticky = False

    # -- test seam --------------------------------------------------------------------------------------------------------
    def force_draws(self, adapter: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                    dropout: Optional[Sequence[torch.Tensor]] = None, sticky: bool = False) -> None:
        """Use these values in place of the NEXT forward's own random draws (golden tests): `adapter` = (weight (16, C) or
        (16, C, 1, 1), bias (16,)) of the per-forward 1x1 convolution, `dropout` = the eight 0/1 keep masks of shape (N, C) in
        the order of DROPOUT_WIDTHS.  Each is cleared by the first forward that USES it (an eval-mode forward draws no masks
        and leaves forced ones for the next training forward) unless sticky=True; force_draws() with no arguments clears
        them."""
        if adapter is None and dropout is None:
            self._forced, self._forced_sticky = None, False
            return
        if dropout is not None:
            dropout = list(dropout)
            if len(dropout) != N_DROPOUT_MASKS or any(m.dim() != 2 or m.shape[1] != c for m, c in zip(dropout, DROPOUT_WIDTHS)):
                raise ValueError(f"force_draws: dropout takes {N_DROPOUT_MASKS} masks of shape (N, C) with C = {DROPOUT_WIDTHS}")
        self._forced, self._forced_sticky = (adapter, dropout), sticky

    def _draws(self, N: int, device, training: bool):
        adapter, masks = self._forced if self._forced is not None else (None, None)
        if training and masks is not None and any(k.shape[0] != N for k in masks):
            raise ValueError(f"force_draws: the masks' batch size {[k.shape[0] for k in masks]} differs from the input's ({N})")
        if self._forced is not None and not self._forced_sticky:     # what this forward uses is consumed
            left = None if training else masks
            self._forced = (None, left) if left is not None else None
        if not training:
            m: List[Optional[torch.Tensor]] = [None] * N_DROPOUT_MASKS      # Dropout2d is the identity
        elif masks is not None:
            m = [(k.to(device=device, dtype=torch.float32) * 2.0).contiguous() for k in masks]
        else:   # keep with probability 0.5, scale by 1 / (1 - p) = 2; torch's generator, as Engine.dropout
            m = [(torch.rand((N, c), device=device) >= 0.5).float() * 2.0 for c in DROPOUT_WIDTHS]
        return adapter, m

    def _x16(self, eng: Engine, x: torch.Tensor, adapter) -> Act:
        """the residual branch of the input stage (vnet.py:56-63) as a (P, 16) activation without gradient"""
        N, C, H, W = x.shape
        P = N * H * W
        if C == 1:
            buf = x.permute(0, 2, 3, 1).reshape(P, 1).expand(P, 16).to(eng.dtype).contiguous()
            return Act(buf, 0, 16, N, H, W, needs_grad=False)
        if C == 16:
            return Act(x.permute(0, 2, 3, 1).reshape(P, 16).to(eng.dtype).contiguous(), 0, 16, N, H, W, needs_grad=False)
        if adapter is not None:
            w, b = adapter
            w = w.to(device=x.device, dtype=torch.float32).reshape(16, C)
            b = b.to(device=x.device, dtype=torch.float32).reshape(16).contiguous()
        else:
            bound = 1.0 / math.sqrt(C)
            w = (torch.rand((16, C), device=x.device) * 2.0 - 1.0) * bound
            b = (torch.rand((16,), device=x.device) * 2.0 - 1.0) * bound
        xin = eng.input_nhwc(x, 8)
        wp = torch.zeros((16, xin.C), dtype=torch.float32, device=x.device)
        wp[:, :C] = w
        y = eng.new_act(N, H, W, 16, needs_grad=False)
        ops.conv5x5(xin, wp.to(eng.dtype), b, y, ksize=1)
        return y

    def check_input_size(self, N: int, H: int, W: int) -> None:
        if H % 16 or W % 16 or H < 16 or W < 16:
            raise ValueError(f"VNet on the HIP engine: input height and width must be multiples of 16, got {H}x{W} "
                             "(the reference's zero padding of odd skip sizes is not implemented)")
        if N * (H // 16) * (W // 16) <= 1:
            raise ValueError("Expected more than 1 value per channel when training, got input size "
                             f"{(N, 256, H // 16, W // 16)} at the coarsest stage (BatchNorm always uses batch statistics)")

    def emit(self, eng: Engine, x: torch.Tensor):
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError(f"VNet: expected a (N, {self.in_channels}, H, W) input, got shape {tuple(x.shape)}")
        N, _, H, W = x.shape
        self.check_input_size(N, H, W)
        x = x.contiguous().float()
        adapter, m = self._draws(N, x.device, eng.training)
        ones = {}

        def skip_mask(i: int) -> torch.Tensor:
            # eval: Dropout2d is the identity, the skip is still copied into its half of the concat buffer
            if m[i] is not None:
                return m[i]
            c = DROPOUT_WIDTHS[i]
            if c not in ones:
                ones[c] = torch.ones((N, c), dtype=torch.float32, device=x.device)
            return ones[c]

        cat32, (up32, skip16) = eng.new_cat(N, H, W, [16, 16])
        cat64, (up64, skip32) = eng.new_cat(N, H // 2, W // 2, [32, 32])
        cat128, (up128, skip64) = eng.new_cat(N, H // 4, W // 4, [64, 64])
        cat256, (up256, skip128) = eng.new_cat(N, H // 8, W // 8, [128, 128])

        it = self.in_tr
        raw = eng.conv_input(x, it.conv1)
        out16 = eng.bn_elu(raw, it.bn1, act1=False, act2=True, res=self._x16(eng, x, adapter), out2=skip16,
                           mask2=skip_mask(7))
        out32 = self.down_tr32.emit(eng, out16, None, skip32, skip_mask(6))
        out64 = self.down_tr64.emit(eng, out32, None, skip64, skip_mask(5))
        out128 = self.down_tr128.emit(eng, out64, m[0], skip128, skip_mask(3))
        if m[2] is not None:    # up_tr256.do1: nothing else reads out256, the dropped copy is what goes on
            d256 = eng.new_act(N, H // 16, W // 16, 256)
            self.down_tr256.emit(eng, out128, m[1], d256, m[2])
        else:
            d256 = self.down_tr256.emit(eng, out128, m[1], None, None)
        if m[4] is not None:    # up_tr128.do1 on up_tr256's output
            u256 = eng.new_act(N, H // 8, W // 8, 256)
            self.up_tr256.emit(eng, d256, cat256, up256, u256, m[4])
        else:
            u256 = self.up_tr256.emit(eng, d256, cat256, up256, None, None)
        u128 = self.up_tr128.emit(eng, u256, cat128, up128, None, None)
        u64 = self.up_tr64.emit(eng, u128, cat64, up64, None, None)
        u32 = self.up_tr32.emit(eng, u64, cat32, up32, None, None)

        ot = self.out_tr
        raw, st = eng.conv5x5(u32, ot.conv1)
        y = eng.bn_elu(raw, ot.bn1, st, pad_grad=self.num_classes % 8 != 0)
        return (eng.logits_from(y),)
