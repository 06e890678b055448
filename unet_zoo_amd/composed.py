"""What the criteria composed on a base loss share (``BoundaryLoss``: boundary.py, ``LovaszLoss``: lovasz.py, ``ClDiceLoss``:
cldice.py, ``HardPixelLoss``: hardpixel.py): ``loss = base_scale * base + weight * term`` with the base's launch first and ONE launch sequence of the term's kernels on the gradients
the base wrote; ``weight`` and ``base_scale`` in two device scalars that the kernels read, so that ``set_weights`` reaches a
captured graph without a new capture.  The three forms are ``FusedCriterion``'s (criterion.py).

A subclass sets ``_NAME`` (the prefix of its messages) and implements ``_build_plan`` and ``_term``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib as L
from .criterion import INT_DTYPES, FusedCriterion, maps_of
from .loss import MulticlassLoss, RegionLoss, bce_dice_direct, bce_dice_with_logits


class ComposedLoss(FusedCriterion):
    """``base_scale * base + weight * term``: the settings and the base's launch of a composed criterion"""

    _NAME = "ComposedLoss"

    def __init__(self, base, weight, base_scale):
        super().__init__()     # _plans: what the term keeps per (number of maps, logits shape, device index, main)
        name = self._NAME
        if isinstance(base, str):
            if base != "bce_dice":
                raise TypeError(f"{name}: base must be 'bce_dice', a RegionLoss or a MulticlassLoss, got {base!r}")
        elif not isinstance(base, (RegionLoss, MulticlassLoss)):
            raise TypeError(f"{name}: base must be 'bce_dice', a RegionLoss or a MulticlassLoss, got {type(base).__name__}")
        self.base = base
        self.class_mode = isinstance(base, MulticlassLoss)
        self.weight, self.base_scale = self._check_weights(weight, base_scale)
        self.ignore_index = base.ignore_index if self.class_mode else -100
        self._scales = {}     # device index -> (weight, base_scale) on the device: what the kernels (and the graphs) read
        self.term: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ the settings
    @classmethod
    def _check_weights(cls, weight, base_scale) -> Tuple[float, float]:
        w, b = cls._num("weight", weight), cls._num("base_scale", base_scale)
        if w < 0 or b < 0:
            raise ValueError(f"{cls._NAME}: weight and base_scale must be >= 0, got {weight!r}, {base_scale!r}")
        if w == 0 and b == 0:
            raise ValueError(f"{cls._NAME}: weight and base_scale are both zero")
        return w, b

    @property
    def target_dtype(self) -> torch.dtype:
        """the static target buffer's dtype in a graphed runner: the base's (int32 labels for a MulticlassLoss)"""
        return getattr(self.base, "target_dtype", torch.float32)

    def set_weights(self, weight: Optional[float] = None, base_scale: Optional[float] = None) -> None:
        """new ``weight`` and / or ``base_scale``: a copy into the device scalars, so captured graphs are NOT captured again
        and use the new values from their next replay on"""
        w, b = self._check_weights(self.weight if weight is None else weight, self.base_scale if base_scale is None else base_scale)
        self.weight, self.base_scale = w, b
        for s in self._scales.values():
            s.copy_(torch.tensor([w, b], dtype=torch.float32))

    def _scales_on(self, device: torch.device) -> torch.Tensor:
        s = self._scales.get(device.index)
        if s is None:
            s = self._scales[device.index] = torch.tensor([self.weight, self.base_scale], dtype=torch.float32, device=device)
        return s

    # ------------------------------------------------------------------ the containers
    def weights_for(self, outputs) -> tuple:
        """the weight of every output map, in the order the model emits them: the base's"""
        if isinstance(self.base, str):
            return (1.0,) * len(maps_of(outputs)[1])
        return self.base.weights_for(outputs)

    # ------------------------------------------------------------------ the launches
    def _base_launch(self, logits, target: torch.Tensor, weights, main: int, need):
        """(base loss, Dice metric, [d(base loss)/d(map) in fp32 or None]) -- the base's own launch"""
        if not isinstance(self.base, str):
            return self.base._launch(logits, target, weights, main, need)
        losses, dices, dl = [], [], []
        for v, g in zip(logits, need):
            if g:
                l, d, grad = bce_dice_direct(v, target)
            else:                                  # dlogits = NULL: no gradient buffer exists
                with torch.no_grad():
                    l, d = bce_dice_with_logits(v.detach(), target)
                grad = None
            losses.append(l)
            dices.append(d)
            dl.append(grad)
        return sum(losses[1:], losses[0]), dices[main], dl

    def _term(self, xs, t: torch.Tensor, shape, dl, weights, main: int, base_loss: torch.Tensor) -> torch.Tensor:
        """the term's launches over all maps (fp32 logits ``xs``, the target as the kernels take it): the combined loss as a
        0-dim device tensor; the gradient buffers ``dl`` are rewritten in place"""
        raise NotImplementedError

    def _launch(self, logits, target: torch.Tensor, weights, main: int, need):
        """the base's launch, then the term's over all maps -> (loss, dice, [d(loss)/d(map) in fp32, or None])"""
        name = self._NAME
        if not logits:
            raise ValueError(f"{name}: no output map")
        shape = tuple(logits[0].shape)
        if len(shape) != 4:
            raise ValueError(f"{name}: output maps must be (N, C, H, W), got shape {shape}")
        for v in logits:
            if tuple(v.shape) != shape:
                raise ValueError(f"{name}: output maps of shape {tuple(v.shape)} and {shape} in one call")
            if v.dtype not in (torch.float32, torch.bfloat16):
                raise ValueError(f"{name}: logits must be float32 or bfloat16, got {v.dtype}")
        if self.class_mode:
            if target.dtype not in INT_DTYPES:
                raise ValueError(f"{name}: the target holds class indices and must have an integer dtype, got {target.dtype}")
            want = (shape[0],) + shape[2:]
            if tuple(target.shape) not in (want, (shape[0], 1) + shape[2:]):
                raise ValueError(f"{name}: logits of shape {shape} against a target of shape {tuple(target.shape)}; "
                                 f"expected {want} or {(shape[0], 1) + shape[2:]}")
        elif tuple(target.shape) != shape:
            raise ValueError(f"{name}: an output map of shape {shape} against a target of shape {tuple(target.shape)}")
        if target.numel() == 0:
            raise ValueError(f"{name}: empty maps")
        L.require_cuda(target, *logits)
        for v in logits:
            if v.device != target.device:
                raise ValueError(f"{name}: an output map on {v.device} against a target on {target.device}")
        base_loss, dice, dl = self._base_launch(logits, target, weights, main, need)
        xs = [v.detach().contiguous().float() for v in logits]      # bf16 logits become fp32, as in the base
        if self.class_mode:
            t = target.detach().reshape((shape[0],) + shape[2:]).contiguous().to(torch.int32)
        else:
            t = target.detach().contiguous().float()
        loss = self._term(xs, t, shape, dl, weights, main, base_loss.detach().reshape(1))
        return loss, dice, dl
