"""Boundary loss on the device: Kervadec et al., "Boundary loss for highly unbalanced segmentation" (DESIGN.md 3r).

The mean of ``probability x signed distance map of the target`` is added to a fused region loss; the distance map is the
exact Euclidean distance transform of the target as the step sees it -- after ``GpuAugment`` when there is one -- computed
inside the first graph of ``GraphedStep`` (``uz_boundary_loss.hip``), where host code would need
``scipy.ndimage.distance_transform_edt`` per image and class in the data loader, before the augmentation::

    crit = unet_zoo_amd.BoundaryLoss(base=unet_zoo_amd.RegionLoss.dice(), weight=0.01)
    step = unet_zoo_amd.GraphedStep(model, crit, ...)
    crit.set_weights(weight=0.02)        # per epoch: a copy into two device scalars, no recapture
    crit.rebalance(alpha)                # Kervadec's schedule: base_scale = 1 - alpha, weight = alpha
"""
from __future__ import annotations

from typing import Optional, Union

import torch

from . import _lib as L
from . import ops
from .composed import ComposedLoss
from .loss import MulticlassLoss, RegionLoss

_MAX_HW = L.BOUNDARY_MAX_HW


class BoundaryLoss(ComposedLoss):
    """``base_scale * base + weight * boundary`` on the device, for every output container of the zoo.

    Per plane with target mask ``G`` the signed squared distance ``sd2`` is an integer: ``+min_{g in G} |p - g|^2`` outside
    ``G``, ``-min_{q not in G} |p - q|^2`` inside, and 0 everywhere when ``G`` is empty (Kervadec's ``one_hot2dist``) or the
    whole plane.  Pixels outside the picture do not exist.  The distance map is::

        phi = spacing * sqrt(sd2)             where sd2 > 0
        phi = -spacing * (sqrt(-sd2) - 1)     where sd2 < 0          -- edt(~G) * ~G - (edt(G) - 1) * G with scipy's edt
        phi = 0                               where sd2 = 0

    ``base`` is ``"bce_dice"`` (the reference's criterion), a ``RegionLoss`` or a ``MulticlassLoss``; the last selects the
    class mode and hands over its ``ignore_index`` and ``target_dtype``.

    Binary mode (float target of the maps' shape, ``G = target > 0.5`` per (image, channel) plane, ``p = sigmoid(x)``)::

        B = sum p * phi / (N C H W)

    Class mode (integer labels ``y``, ``p = softmax_K(x)``, ``G_c = (y == c)``, classes ``1 .. K-1`` or, with
    ``include_background=True``, ``0 .. K-1``).  A pixel whose label is ``ignore_index`` or outside ``[0, K)`` is in no
    ``G_c`` (complement for the transform), adds nothing and has zero gradient::

        B = sum over images, classes and valid pixels of p_c * phi_c / (N |classes| H W)

    ``loss = base_scale * base_loss + weight * sum_m ow_m * B_m`` with the base's output weights ``ow`` (ones for
    ``"bce_dice"``); ``phi`` is computed ONCE per call and shared by u2net's seven maps / nested_unet's deep-supervision
    list.  The Dice metric returned beside the loss is the base's, unchanged.  ``.sd2`` is the int32 ``(M, H, W)`` transform
    of the last call (``M = N C`` planes, or ``N |classes|``), ``.term`` the unweighted boundary term of the main map.

    One call is the base's launches plus one ``uz_boundary_loss``: five launches whatever the number of maps, float64 sums
    in a fixed order, no library reduction, no host read -- ``GraphedStep(model, BoundaryLoss(...))`` and ``GraphedEval``
    keep it INSIDE their graphs.  ``weight`` and ``base_scale`` live in two device scalars that the kernels read:
    ``set_weights`` / ``rebalance`` copy into them, and a captured graph sees the new values at its next replay.

    Descriptor, workspace and ``sd2`` of a (number of maps, shape, device, main) are kept, the scalars per device: calls of
    one object must follow each other on one stream or be ordered by the caller, and ``.sd2`` is overwritten by the next
    call of that shape.  ``spacing`` and ``include_background`` are the constructor's for shapes already seen -- build a
    new object to change them.  ``GraphedStep`` / ``GraphedEval`` warm the criterion up outside the capture for the first
    shape; a further input shape allocates its workspace during its own capture (from the graph's pool), as
    ``MulticlassLoss`` does.
    """

    _NAME = "BoundaryLoss"

    def __init__(self, base: Union[str, RegionLoss, MulticlassLoss] = "bce_dice", weight: float = 0.01, base_scale: float = 1.0,
                 include_background: bool = False, spacing: float = 1.0):
        super().__init__(base, weight, base_scale)
        self.spacing = self._num("spacing", spacing)
        if self.spacing <= 0:
            raise ValueError(f"BoundaryLoss: spacing must be > 0, got {spacing!r}")
        self.include_background = bool(include_background)
        self.sd2: Optional[torch.Tensor] = None      # _plans holds (descriptor, item table, workspace, sd2) per key

    # ------------------------------------------------------------------ the settings (set_weights: ComposedLoss)
    def rebalance(self, alpha: float) -> None:
        """Kervadec's schedule: ``base_scale = 1 - alpha``, ``weight = alpha`` for ``alpha`` in [0, 1]"""
        a = self._num("alpha", alpha)
        if not 0.0 <= a <= 1.0:
            raise ValueError(f"BoundaryLoss: alpha must be in [0, 1], got {alpha!r}")
        self.set_weights(weight=a, base_scale=1.0 - a)

    def _build_plan(self, n_items: int, shape, device: torch.device, main: int):
        if n_items > L.CLASS_MAX_ITEMS:
            raise ValueError(f"BoundaryLoss: {n_items} output maps, at most {L.CLASS_MAX_ITEMS} per call")
        N, C, H, W = (int(s) for s in shape)
        if self.class_mode and not 2 <= C <= L.CLASS_MAX_K:
            raise ValueError(f"BoundaryLoss: K = {C} classes outside [2, {L.CLASS_MAX_K}]")
        if H > _MAX_HW or W > _MAX_HW:
            raise ValueError(f"BoundaryLoss: maps of {H} x {W} pixels, at most {_MAX_HW} a side")
        first = 0 if (self.include_background or not self.class_mode) else 1
        desc = L.BoundaryDesc(L.BOUNDARY_CLASS if self.class_mode else L.BOUNDARY_BINARY, n_items, N, C, H, W, first,
                              self.ignore_index, main, self.spacing)
        ws = torch.empty((L.boundary_workspace_bytes(desc) + 7) // 8, dtype=torch.float64, device=device)
        sd2 = torch.zeros(N * (C - first), H, W, dtype=torch.int32, device=device)
        return desc, (L.BoundaryItem * n_items)(), ws, sd2

    def _term(self, xs, t: torch.Tensor, shape, dl, weights, main: int, base_loss: torch.Tensor) -> torch.Tensor:
        """one uz_boundary_loss over all maps on the gradients the base wrote"""
        desc, items, ws, sd2 = self._plan(len(xs), shape, t.device, main)
        out = torch.empty(2, dtype=torch.float32, device=t.device)
        self._fill(items, xs, dl, weights)
        ops.boundary_loss(desc, items, t, self._scales_on(t.device), base_loss, out, sd2, ws)
        self.sd2, self.term = sd2, out[1]
        return out[0]

    def __repr__(self) -> str:
        return (f"BoundaryLoss(base={self.base!r}, weight={self.weight}, base_scale={self.base_scale}, "
                f"include_background={self.include_background}, spacing={self.spacing})")
