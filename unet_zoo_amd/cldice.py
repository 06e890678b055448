"""clDice on the device: Shit, Paetzold, Sekuboyina et al., "clDice -- a novel topology-preserving loss function for tubular
structure segmentation", CVPR 2021.

The centreline Dice compares the soft skeleton of the prediction with the target and the soft skeleton of the target with the
prediction; the soft skeleton is ``iterations + 1`` rounds of min-pool, min-pool, min, max-pool, subtract, relu.
``uz_cldice_loss.hip`` runs all rounds of a tile in LDS, forward and backward, inside the first graph of ``GraphedStep``, where
a Python callable on ``max_pool2d`` splits the step into a forward and backward graphs with about a hundred eager launches per
output map in between::

    crit = unet_zoo_amd.ClDiceLoss(base=unet_zoo_amd.RegionLoss.dice(), weight=0.5, iterations=3)      # Dice + BCE + clDice
    step = unet_zoo_amd.GraphedStep(model, crit, ...)
    crit.set_weights(weight=1.0)         # a copy into two device scalars, no recapture
"""
from __future__ import annotations

import math
from typing import Optional, Union

import torch

from . import _lib as L
from . import ops
from .composed import ComposedLoss
from .loss import MulticlassLoss, RegionLoss


class ClDiceLoss(ComposedLoss):
    """``base_scale * base + weight * V`` on the device, for every output container of the zoo.

    For a plane ``a`` of shape (H, W), with every window clipped to the picture:

    - ``erode(a) = min(v, h)``: ``v`` is the minimum of the vertical 3-window (up, centre, down), ``h`` the minimum of the
      horizontal 3-window (left, centre, right);
    - ``dilate(a)`` is the maximum of the 3 x 3 window, ``open(a) = dilate(erode(a))``;
    - ``skel_k(a)``: start with ``S = relu(a - open(a))``, then ``k = iterations`` times ``a <- erode(a)``,
      ``d = relu(a - open(a))``, ``S <- S + relu(d - S d)``.

    ``skel_k(a)`` at a pixel depends on ``a`` within Chebyshev distance ``R = k + 2``.  For one segment, with prediction
    plane(s) ``p``, target plane(s) ``t`` and ``s = smooth > 0``::

        Tprec = (sum skel(p) t + s) / (sum skel(p) + s)
        Tsens = (sum skel(t) p + s) / (sum skel(t) + s)
        cl    = 1 - 2 Tprec Tsens / (Tprec + Tsens)

    ``V`` is the mean of ``cl`` over the segments and ``loss = base_scale * base_loss + weight * sum_m ow_m V_m`` with the
    base's output weights ``ow`` (ones for ``"bce_dice"``); the Dice metric returned beside the loss is the base's.

    ``base`` is ``"bce_dice"`` (the reference's criterion), a ``RegionLoss`` or a ``MulticlassLoss``; the last selects the
    class mode and hands over its ``ignore_index`` and ``target_dtype``.

    Binary mode (float target of the maps' shape): ``p = sigmoid(x)`` in fp32, ``t`` the target as given -- soft values in
    [0, 1] are allowed -- and ``skel(t)`` gets no gradient.  ``per_image=False`` (the paper's form): one segment per channel
    over the batch; ``per_image=True``: one per (image, channel).

    Class mode (integer labels ``y``): ``p = softmax_K(x)``, ``t_c = (y == c)``; the classes are ``1 .. K-1``, or ``0 .. K-1``
    with ``include_background=True``.  A pixel whose label is ``ignore_index`` or outside ``[0, K)`` has ``p_c = t_c = 0`` in
    every plane before the skeleton, whatever gradient reaches it is dropped: its K logits get exactly zero from the term.
    ``dV/dx_k = p_k (g_k - sum_c p_c g_c)`` with ``g_c = dV/dp_c``, 0 for an excluded class.

    The subgradients are torch's, so float64 CPU autograd through ``max_pool2d``, ``torch.min`` and ``relu`` is the reference
    on any input, ties included: ``relu'(0) = 0``; ``dilate`` routes to the first maximum in row-major window order; ``v`` to
    the first minimum top to bottom, ``h`` left to right; ``min(v, h)`` to the smaller one, half to each on ``v == h``.

    After a call ``.term`` is the unweighted ``V`` of the main map, ``.probs`` and ``.skeleton`` its ``p`` and ``skel(p)``
    (N, C, H, W; the plane of an excluded background class stays zero in ``.skeleton``) and ``.target_skeleton`` ``skel(t)``,
    which is computed once per call whatever the number of maps.

    One call is the base's launches plus one ``uz_cldice_loss``: 6 launches (4 without a gradient) whatever the number of maps
    and the data, float64 sums in a fixed order, no float atomics, no host read -- ``GraphedStep(model, ClDiceLoss(...))`` and
    ``GraphedEval`` keep it INSIDE their graphs.  ``weight`` and ``base_scale`` live in two device scalars that the kernels
    read: ``set_weights`` copies into them, and a captured graph sees the new values at its next replay.

    Descriptor, workspace and the three plane outputs of a (number of maps, shape, device, main) are kept: calls of one object
    must follow each other on one stream or be ordered by the caller, and the outputs are overwritten by the next call of that
    shape.  The workspace is 8 bytes per element of every map (plus the target's planes in the class mode).
    """

    _NAME = "ClDiceLoss"

    def __init__(self, base: Union[str, RegionLoss, MulticlassLoss] = "bce_dice", weight: float = 0.5, base_scale: float = 1.0,
                 iterations: int = 3, smooth: float = 1.0, per_image: bool = False, include_background: bool = False):
        super().__init__(base, weight, base_scale)
        if isinstance(iterations, bool) or not isinstance(iterations, int):
            raise TypeError(f"ClDiceLoss: iterations must be an int, got {iterations!r}")
        if not 1 <= iterations <= L.CLDICE_MAX_ITERATIONS:
            raise ValueError(f"ClDiceLoss: iterations must be in [1, {L.CLDICE_MAX_ITERATIONS}], got {iterations}")
        s = self._num("smooth", smooth)
        if not s > 0 or not math.isfinite(float(torch.tensor(s, dtype=torch.float32))):
            raise ValueError(f"ClDiceLoss: smooth must be positive, got {smooth!r}")
        self.iterations = iterations
        self.smooth = s
        self.per_image = bool(per_image)
        self.include_background = bool(include_background)
        self.probs: Optional[torch.Tensor] = None       # _plans holds (descriptor, item table, workspace, the three outputs) per key
        self.skeleton: Optional[torch.Tensor] = None
        self.target_skeleton: Optional[torch.Tensor] = None

    def _build_plan(self, n_items: int, shape, device: torch.device, main: int):
        if n_items > L.CLASS_MAX_ITEMS:
            raise ValueError(f"ClDiceLoss: {n_items} output maps, at most {L.CLASS_MAX_ITEMS} per call")
        N, C, H, W = (int(s) for s in shape)
        if self.class_mode and not 2 <= C <= L.CLASS_MAX_K:
            raise ValueError(f"ClDiceLoss: K = {C} classes outside [2, {L.CLASS_MAX_K}]")
        if n_items * N * C * H * W > L.CLDICE_MAX_ELEMENTS:
            raise ValueError(f"ClDiceLoss: {n_items * N * C * H * W} elements in {n_items} maps, at most {L.CLDICE_MAX_ELEMENTS}")
        desc = L.ClDiceDesc(L.CLDICE_CLASS if self.class_mode else L.CLDICE_BINARY, n_items, N, C, H, W, int(self.per_image),
                            int(self.include_background), self.ignore_index, self.iterations, self.smooth, main)
        ws = torch.empty((L.cldice_workspace_bytes(desc) + 7) // 8, dtype=torch.float64, device=device)
        planes = tuple(torch.zeros((N, C, H, W), dtype=torch.float32, device=device) for _ in range(3))
        return (desc, (L.ClDiceItem * n_items)(), ws) + planes

    def _term(self, xs, t: torch.Tensor, shape, dl, weights, main: int, base_loss: torch.Tensor) -> torch.Tensor:
        """one uz_cldice_loss over all maps on the gradients the base wrote"""
        desc, items, ws, probs, skeleton, target_skeleton = self._plan(len(xs), shape, t.device, main)
        out = torch.empty(2, dtype=torch.float32, device=t.device)
        self._fill(items, xs, dl, weights)
        ops.cldice_loss(desc, items, t, self._scales_on(t.device), base_loss, out, probs, skeleton, target_skeleton, ws)
        self.probs, self.skeleton, self.target_skeleton, self.term = probs, skeleton, target_skeleton, out[1]
        return out[0]

    def __repr__(self) -> str:
        return (f"ClDiceLoss(base={self.base!r}, weight={self.weight}, base_scale={self.base_scale}, iterations={self.iterations}, "
                f"smooth={self.smooth}, per_image={self.per_image}, include_background={self.include_background})")
