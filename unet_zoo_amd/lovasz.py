"""Lovasz hinge / Lovasz-softmax on the device: Berman, Triggs, Blaschko, "The Lovasz-Softmax loss: a tractable surrogate for
the optimization of the intersection-over-union measure in neural networks", CVPR 2018.

The Lovasz extension of the Jaccard loss needs a sort of all pixel errors per image (or per batch) and per class and a scan
over the sorted labels.  ``uz_lovasz_loss.hip`` does both -- a segmented stable radix sort -- inside the first graph of
``GraphedStep``, where a Python callable on ``torch.sort`` splits the step into a forward and backward graphs with eager
library calls in between::

    crit = unet_zoo_amd.LovaszLoss(base=unet_zoo_amd.RegionLoss.dice(), weight=1.0)      # Dice + BCE + Lovasz hinge
    step = unet_zoo_amd.GraphedStep(model, crit, ...)
    crit.set_weights(base_scale=0.0)     # an IoU fine-tuning phase: a copy into two device scalars, no recapture
"""
from __future__ import annotations

from typing import Optional, Union

import torch

from . import _lib as L
from . import ops
from .composed import ComposedLoss
from .loss import MulticlassLoss, RegionLoss


class LovaszLoss(ComposedLoss):
    """``base_scale * base + weight * V`` on the device, for every output container of the zoo.

    A *segment* is a list of (error ``e``, membership bit ``b``).  The elements with ``e > 0`` are ranked ``r = 0, 1, ...`` by
    descending ``e``, ties by ascending position (a stable sort); an element with ``e <= 0`` has rank -1, adds nothing and has
    zero gradient.  With ``G`` members in the whole segment, ``c`` members among ranks ``0 .. r`` and ``n = r + 1 - c`` the
    element at rank ``r`` weighs the Jaccard difference ``g = J_r - J_{r-1}``, ``J_r = 1 - (G - c) / (G + n)``, ``J_{-1} = 0``::

        g = 1 / (G + n)                           where b = 1
        g = (G - c) / ((G + n - 1) (G + n))       where b = 0          (1 at rank 0 of a segment with G = 0)

    and the segment's value is ``L = sum e g`` over its ranked elements.

    ``base`` is ``"bce_dice"`` (the reference's criterion), a ``RegionLoss`` or a ``MulticlassLoss``; the last selects the
    class mode and hands over its ``ignore_index`` and ``target_dtype``.

    Binary mode (float target of the maps' shape): ``b = target > 0.5``, ``s = +1`` where ``b`` else ``-1``, ``e = 1 - x s``
    in fp32 (the Lovasz hinge).  ``per_image=True``: every (image, channel) plane is a segment in row-major pixel order;
    ``per_image=False``: every channel over the batch, image-major.  ``V`` is the mean of ``L`` over the segments.

    Class mode (integer labels ``y``, ``p = softmax_K(x)``): for class ``c``, ``b = (y == c)`` and ``e = |b - p_c|``
    (Lovasz-softmax).  A pixel whose label is ``ignore_index`` or outside ``[0, K)`` is in no segment and has zero gradient.
    ``per_image=True``: ``V = (1/N) sum_n (1/|P_n|) sum_{c in P_n} L_{n,c}`` with ``P_n`` the classes present among image
    n's valid pixels (``classes="present"``) or all ``K`` (``classes="all"``); an image with empty ``P_n`` adds 0.
    ``per_image=False``: a segment per class over the batch's valid pixels, the mean over the present (or all) classes.

    ``loss = base_scale * base_loss + weight * sum_m ow_m * V_m`` with the base's output weights ``ow`` (ones for
    ``"bce_dice"``); every output map is sorted on its own (u2net's seven, nested_unet's deep-supervision list).  The Dice
    metric returned beside the loss is the base's, unchanged.  ``.errors`` (fp32) and ``.ranks`` (int32, -1 where unranked or
    ignored) are the ``(segments, segment length)`` arrays of the main map in the last call, ``.term`` its unweighted ``V``.

    One call is the base's launches plus one ``uz_lovasz_loss``: 19 launches whatever the number of maps and whatever the
    data, float64 sums in a fixed order, a scatter that does not depend on arrival order, no library sort or reduction, no
    host read -- ``GraphedStep(model, LovaszLoss(...))`` and ``GraphedEval`` keep it INSIDE their graphs.  ``weight`` and
    ``base_scale`` live in two device scalars that the kernels read: ``set_weights`` copies into them, and a captured graph
    sees the new values at its next replay.  The base is launched even at ``base_scale = 0``: the Dice metric is its.

    Descriptor, workspace, ``errors`` and ``ranks`` of a (number of maps, shape, device, main) are kept, the scalars per
    device: calls of one object must follow each other on one stream or be ordered by the caller, and the outputs are
    overwritten by the next call of that shape.  The workspace grows linearly with the number of maps (about 17 bytes per
    element of every map).  ``GraphedStep`` / ``GraphedEval`` warm the criterion up outside the capture for the first shape;
    a further input shape allocates its workspace during its own capture (from the graph's pool), as ``MulticlassLoss`` does.
    """

    _NAME = "LovaszLoss"

    def __init__(self, base: Union[str, RegionLoss, MulticlassLoss] = "bce_dice", weight: float = 1.0, base_scale: float = 1.0,
                 per_image: bool = True, classes: str = "present"):
        super().__init__(base, weight, base_scale)
        if classes not in ("present", "all"):
            raise ValueError(f"LovaszLoss: classes must be 'present' or 'all', got {classes!r}")
        self.per_image = bool(per_image)
        self.classes = classes
        self.errors: Optional[torch.Tensor] = None   # _plans holds (descriptor, item table, workspace, errors, ranks) per key
        self.ranks: Optional[torch.Tensor] = None

    def _build_plan(self, n_items: int, shape, device: torch.device, main: int):
        if n_items > L.CLASS_MAX_ITEMS:
            raise ValueError(f"LovaszLoss: {n_items} output maps, at most {L.CLASS_MAX_ITEMS} per call")
        N, C, H, W = (int(s) for s in shape)
        if self.class_mode and not 2 <= C <= L.CLASS_MAX_K:
            raise ValueError(f"LovaszLoss: K = {C} classes outside [2, {L.CLASS_MAX_K}]")
        seg = (N * C, H * W) if self.per_image else (C, N * H * W)
        if seg[1] > L.LOVASZ_MAX_SEGMENT:
            raise ValueError(f"LovaszLoss: a segment of {seg[1]} elements, at most {L.LOVASZ_MAX_SEGMENT}")
        if n_items * N * C * H * W > L.LOVASZ_MAX_ELEMENTS:
            raise ValueError(f"LovaszLoss: {n_items * N * C * H * W} elements in {n_items} maps, at most {L.LOVASZ_MAX_ELEMENTS}")
        desc = L.LovaszDesc(L.LOVASZ_CLASS if self.class_mode else L.LOVASZ_BINARY, n_items, N, C, H, W, int(self.per_image),
                            L.LOVASZ_ALL if self.classes == "all" else L.LOVASZ_PRESENT, self.ignore_index, main)
        ws = torch.empty((L.lovasz_workspace_bytes(desc) + 7) // 8, dtype=torch.float64, device=device)
        errors = torch.zeros(seg, dtype=torch.float32, device=device)
        ranks = torch.full(seg, -1, dtype=torch.int32, device=device)
        return desc, (L.LovaszItem * n_items)(), ws, errors, ranks

    def _term(self, xs, t: torch.Tensor, shape, dl, weights, main: int, base_loss: torch.Tensor) -> torch.Tensor:
        """one uz_lovasz_loss over all maps on the gradients the base wrote"""
        desc, items, ws, errors, ranks = self._plan(len(xs), shape, t.device, main)
        out = torch.empty(2, dtype=torch.float32, device=t.device)
        self._fill(items, xs, dl, weights)
        ops.lovasz_loss(desc, items, t, self._scales_on(t.device), base_loss, out, errors, ranks, ws)
        self.errors, self.ranks, self.term = errors, ranks, out[1]
        return out[0]

    def __repr__(self) -> str:
        return (f"LovaszLoss(base={self.base!r}, weight={self.weight}, base_scale={self.base_scale}, "
                f"per_image={self.per_image}, classes={self.classes!r})")
