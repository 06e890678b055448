"""Boundary-distance metrics on the device: ``SurfaceMetrics``.

The segmentation papers whose recipes this package carries report two numbers per organ: Dice and HD95, the 95th-percentile
Hausdorff distance.  Dice is formed on the device by the losses; ``SurfaceMetrics`` forms the Hausdorff distance, its
percentile form and the average symmetric surface distance there too (``uz_surface.hip``), exactly as medpy's ``hd``, ``hd95``
and ``assd`` define them in 2D with connectivity 1 (include/unetzoo_hip.h):

    m = unet_zoo_amd.SurfaceMetrics()                       # percentile=95.0, spacing=1.0, background left out
    out, stats = m(model(images), masks)                    # device tensors, STATIC per shape
    m.hd, m.hdq, m.assd, m.state                            # (N, P) views of them
    ev = unet_zoo_amd.GraphedEval(model, "bce_dice", surface=m)      # or inside the evaluation graph

A float target selects the binary mode: prediction ``logits > 0`` (sigmoid > 0.5, what ``loss_and_dice`` thresholds), target
``> 0.5``, every channel its own pair (P = C).  An integer target holds class indices: prediction ``argmax_K`` (ties: the lowest
index), pairs are the classes 1 .. K-1 (0 .. K-1 with ``include_background=True``); a pixel whose label is ``ignore_index`` or
outside ``[0, K)`` belongs to no mask.

``out`` is (N, P, 4) float32: hd, hdq, assd, 0.  ``stats`` is (N, P, 8) int64: |S(A)|, |S(B)|, max d2, D_(k), D_(k+1),
state, |A|, |B| (A the prediction, B the target, S the surface, d2 the squared pixel distances).  ``state`` is 0 when both
masks are non-empty, 1 when the prediction is empty, 2 when the target is, 3 when both are; the three values of such a pair
are 0 and it is for the caller to count or score them (TransUNet's convention, or any other).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

from . import _lib as L
from . import ops
from .criterion import INT_DTYPES, maps_of


class SurfaceMetrics:
    """``percentile``: q of hdq, 0 < q <= 100 (95: HD95).  ``spacing``: one isotropic pixel spacing, positive and finite.
    ``include_background``: class 0 is a pair too (class-index targets only).  ``ignore_index``: the label that belongs to no
    class.

    ``m(outputs, target)`` takes any output container of the zoo and measures its MAIN map (first value of a dict, last
    element of a list), fp32 or bf16 logits (bf16 goes through ``.float()`` as in the losses), against a float target of the
    map's shape or integer class indices of shape (N, H, W) or (N, 1, H, W).  One call is one ``uz_surface_metrics``: seven
    launches, no host read, so it can be captured (``GraphedEval(..., surface=m)``).

    Descriptor, workspace, ``out`` and ``stats`` of a (mode, shape, device) are kept: calls of one object must follow each
    other on one stream or be ordered by the caller, and the results are overwritten by the next call with that shape.  The
    settings are the constructor's; changing an attribute afterwards has no effect on shapes already seen."""

    def __init__(self, percentile: float = 95.0, spacing: float = 1.0, include_background: bool = False, ignore_index: int = -100):
        def num(name, v):
            try:
                f = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"SurfaceMetrics: {name} must be a number, got {v!r}") from None
            if not math.isfinite(f):
                raise ValueError(f"SurfaceMetrics: {name} must be finite, got {v!r}")
            return f
        self.percentile, self.spacing = num("percentile", percentile), num("spacing", spacing)
        if not 0 < self.percentile <= 100:
            raise ValueError(f"SurfaceMetrics: percentile must be in (0, 100], got {percentile!r}")
        if self.spacing <= 0:
            raise ValueError(f"SurfaceMetrics: spacing must be > 0, got {spacing!r}")
        if isinstance(ignore_index, bool) or not isinstance(ignore_index, int) or not -2 ** 31 <= ignore_index < 2 ** 31:
            raise ValueError(f"SurfaceMetrics: ignore_index must be an int32 value, got {ignore_index!r}")
        self.ignore_index = ignore_index
        self.include_background = bool(include_background)
        self._plans: Dict[tuple, tuple] = {}       # (mode, logits shape, device index) -> (descriptor, workspace, out, stats)
        self.out: Optional[torch.Tensor] = None
        self.stats: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ the plan of a shape
    def describe(self, mode: int, shape) -> "L.SurfaceDesc":
        """the descriptor of a call with logits of this (N, C, H, W) shape"""
        N, C, H, W = (int(s) for s in shape)
        first = 0 if self.include_background else 1
        return L.SurfaceDesc(mode, N, C, H, W, first if mode == L.SURFACE_CLASS else 0, self.ignore_index, 0, self.percentile,
                             self.spacing)

    def _plan(self, mode: int, shape, device: torch.device):
        key = (mode, tuple(shape), device.index)
        plan = self._plans.get(key)
        if plan is None:
            desc = self.describe(mode, shape)
            P = desc.C - desc.first_class if mode == L.SURFACE_CLASS else desc.C
            ws = torch.empty((L.surface_workspace_bytes(desc) + 7) // 8, dtype=torch.float64, device=device)
            out = torch.zeros(desc.N, P, 4, dtype=torch.float32, device=device)
            stats = torch.zeros(desc.N, P, 8, dtype=torch.int64, device=device)
            plan = self._plans[key] = (desc, ws, out, stats)
        return plan

    # ------------------------------------------------------------------ one call
    def __call__(self, outputs, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        _, maps, main = maps_of(outputs)
        x = maps[main]
        if not isinstance(x, torch.Tensor) or not isinstance(target, torch.Tensor):
            raise ValueError("SurfaceMetrics: outputs and target must be tensors (or a dict / list of output tensors)")
        shape = tuple(x.shape)
        if len(shape) != 4:
            raise ValueError(f"SurfaceMetrics: logits must be (N, C, H, W), got shape {shape}")
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"SurfaceMetrics: logits must be float32 or bfloat16, got {x.dtype}")
        if x.numel() == 0:
            raise ValueError("SurfaceMetrics: empty maps")
        if shape[2] > L.SURFACE_MAX_HW or shape[3] > L.SURFACE_MAX_HW:
            raise ValueError(f"SurfaceMetrics: maps of {shape[2]} x {shape[3]} pixels, at most {L.SURFACE_MAX_HW} each way")
        if target.dtype in INT_DTYPES:
            mode = L.SURFACE_CLASS
            K = shape[1]
            if not 2 <= K <= L.CLASS_MAX_K:
                raise ValueError(f"SurfaceMetrics: K = {K} classes outside [2, {L.CLASS_MAX_K}]")
            want = (shape[0],) + shape[2:]
            if tuple(target.shape) not in (want, (shape[0], 1) + shape[2:]):
                raise ValueError(f"SurfaceMetrics: logits of shape {shape} against a target of shape {tuple(target.shape)}; "
                                 f"expected {want} or {(shape[0], 1) + shape[2:]}")
        elif target.dtype in (torch.float32, torch.bfloat16, torch.float16, torch.float64):
            mode = L.SURFACE_BINARY
            want = shape
            if tuple(target.shape) != shape:
                raise ValueError(f"SurfaceMetrics: an output map of shape {shape} against a target of shape {tuple(target.shape)}")
        else:
            raise ValueError(f"SurfaceMetrics: the target must be float maps or integer class indices, got {target.dtype}")
        L.require_cuda(x, target)
        if x.device != target.device:
            raise ValueError(f"SurfaceMetrics: an output map on {x.device} against a target on {target.device}")
        xs = x.detach().contiguous().float()
        t = target.detach().reshape(want).contiguous().to(torch.int32 if mode == L.SURFACE_CLASS else torch.float32)
        desc, ws, out, stats = self._plan(mode, shape, xs.device)
        ops.surface_metrics(desc, xs, t, out, stats, ws)
        self.out, self.stats = out, stats
        return out, stats

    # ------------------------------------------------------------------ views of the last call
    def _need(self) -> None:
        if self.out is None:
            raise RuntimeError("SurfaceMetrics: no call yet")

    @property
    def hd(self) -> torch.Tensor:
        self._need()
        return self.out[..., 0]

    @property
    def hdq(self) -> torch.Tensor:
        self._need()
        return self.out[..., 1]

    @property
    def assd(self) -> torch.Tensor:
        self._need()
        return self.out[..., 2]

    @property
    def state(self) -> torch.Tensor:
        self._need()
        return self.stats[..., 5]

    def __repr__(self) -> str:
        return (f"SurfaceMetrics(percentile={self.percentile}, spacing={self.spacing}, "
                f"include_background={self.include_background}, ignore_index={self.ignore_index})")
