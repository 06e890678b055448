"""Hard-pixel mining on the device: top-k cross-entropy (nnU-Net's ``DC_and_topk``: Dice + CE over the hardest
10 % of the pixels), OHEM cross-entropy (the Cityscapes recipe of mmseg's ``OHEMPixelSampler``: keep the pixels whose
true-class probability is below 0.7, and ``min_kept`` at least) and focal loss (Lin et al., "Focal Loss for Dense Object
Detection", ICCV 2017).

Selection needs the k-th largest pixel loss of an image or a batch.  ``uz_hardpixel_loss.hip`` finds it exactly -- an
MSB-first radix select over the bit patterns of the losses, counts only -- inside the first graph of ``GraphedStep``, where a
Python callable on ``torch.topk`` splits the step into a forward and a backward graph with eager library calls in between::

    crit = unet_zoo_amd.HardPixelLoss.topk(unet_zoo_amd.MulticlassLoss.ce_dice(), k=0.1)        # nnU-Net's DC_and_topk
    crit = unet_zoo_amd.HardPixelLoss.ohem(unet_zoo_amd.MulticlassLoss.ce_dice(), thresh=0.7, min_kept=100_000)
    crit = unet_zoo_amd.HardPixelLoss.focal(unet_zoo_amd.RegionLoss.dice(), gamma=2.0)
    step = unet_zoo_amd.GraphedStep(model, crit, ...)
    crit.set_weights(base_scale=0.0)     # the mined term alone: a copy into two device scalars, no recapture
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Union

import torch

from . import _lib as L
from . import ops
from .composed import ComposedLoss
from .loss import MulticlassLoss, RegionLoss


class HardPixelLoss(ComposedLoss):
    """``base_scale * base + weight * V`` on the device, for every output container of the zoo.

    A *segment* is a list of valid pixels.  Each pixel has a plain loss ``l >= 0`` and a true-class probability
    ``p_t = exp(-l)``.

    Class mode (``base`` is a ``MulticlassLoss``, which hands over its ``ignore_index`` and ``target_dtype``): logits
    ``(N, K, H, W)``, labels ``y`` ``(N, H, W)``; ``l = logsumexp_K(x) - x_y`` in fp32 with the maximum subtracted.  A pixel
    with ``y == ignore_index`` or ``y`` outside ``[0, K)`` is in no segment and gets zero gradient on all K logits.  No class
    weights and no label smoothing enter this term: those stay in the base.

    Binary mode (``base`` is ``"bce_dice"`` or a ``RegionLoss``): logits and target ``(N, C, H, W)``; ``b = target > 0.5``,
    ``s = +1`` where ``b`` else ``-1`` (``LovaszLoss``'s convention), ``l = softplus(-s x)``.  Every element is valid.

    Focal modulation: ``f = (1 - p_t)^gamma * l`` with ``gamma = 0`` or ``gamma >= 1``; values in ``(0, 1)`` are refused,
    ``(1 - p_t)^(gamma - 1)`` is unbounded at ``p_t -> 1``.  ``f`` is increasing in ``l``, so selecting on ``f`` and on ``l``
    keep the same pixels.  ``df/dl = (1 - p_t)^gamma + gamma (1 - p_t)^(gamma - 1) p_t l``, exactly 1 at ``gamma = 0``;
    ``dl/dx_c = p_c - [c == y]`` (class), ``dl/dx = -s (1 - p_t)`` (binary).

    Segments: ``per_image=False`` (the default, as in mmseg's OHEM and nnU-Net's top-k): one per output map over the whole
    batch; ``per_image=True``: one per image -- in binary mode it holds all C channels of the image.

    Kept count of a segment with ``n`` valid pixels: ``k = clamp(max(min_kept, ceil(keep * n)), 1, n)``, the product taken in
    fp32 (one rounding: ``keep=0.1`` of 1000 pixels is 100); with ``max_prob`` set, ``c = #{p_t < max_prob}`` counted on the
    plain ``l > -log(max_prob)``, otherwise ``c = 0``; ``m = max(k, c)``.  A segment with ``n = 0`` adds 0 and has zero
    gradient.

    Value: ``tau`` is the m-th largest ``f`` of the segment, ``n_above = #{f > tau}``, ``n_tie = #{f == tau}``,
    ``V_seg = (sum_{f > tau} f + (m - n_above) * tau) / m``, and ``V`` the mean of ``V_seg`` over the segments of the map
    with ``n > 0``.  Gradient: a pixel with ``f > tau`` weighs ``1 / m``, one with ``f == tau`` weighs
    ``(m - n_above) / (n_tie * m)``, every other pixel 0 -- a subgradient of the top-m sum that does not depend on position
    or arrival order; without ties it is ``torch.topk``'s gradient.

    ``loss = base_scale * base_loss + weight * sum_m ow_m * V_m`` with the base's output weights ``ow`` (ones for
    ``"bce_dice"``); every output map is mined on its own.  The Dice metric returned beside the loss is the base's, unchanged.
    ``.losses`` (fp32, the ``f`` of the main map in the map's own layout, 0 where a pixel is in no segment) and
    ``.selection`` (int32 ``(segments, 4)``: ``m``, ``n_above``, ``n_tie``, the bit pattern of ``tau``) are those of the last
    call, ``.term`` its unweighted ``V``.

    One call is the base's launches plus one ``uz_hardpixel_loss``: 10 launches whatever the number of maps and the data,
    integer counts and float64 sums in a fixed order, no library sort or reduction, no host read --
    ``GraphedStep(model, HardPixelLoss(...))`` and ``GraphedEval`` keep it INSIDE their graphs.  ``weight`` and
    ``base_scale`` live in two device scalars that the kernels read: ``set_weights`` copies into them, and a captured graph
    sees the new values at its next replay.  ``keep``, ``min_kept``, ``max_prob``, ``gamma`` and ``per_image`` are part of the
    descriptor: a plan (descriptor, workspace, ``losses``, ``selection``) is fixed at the first call with a (number of maps,
    shape, device, main) and kept, so changing them afterwards has no effect on shapes already seen -- make a new object.
    Calls of one object must follow each other on one stream or be ordered by the caller; the outputs are overwritten by the
    next call of that shape.  The workspace is about 4 bytes per ``f`` value of every map plus 1 KB per 2048 of them.
    """

    _NAME = "HardPixelLoss"

    def __init__(self, base: Union[str, RegionLoss, MulticlassLoss] = "bce_dice", weight: float = 1.0, base_scale: float = 1.0,
                 keep: float = 0.1, min_kept: int = 0, max_prob: Optional[float] = None, gamma: float = 0.0,
                 per_image: bool = False):
        super().__init__(base, weight, base_scale)
        name = self._NAME
        keep = self._num("keep", keep)
        if not 0.0 < ctypes.c_float(keep).value <= 1.0:      # what the descriptor holds: the library's own test
            raise ValueError(f"{name}: keep must be in (0, 1] as an fp32 value, got {keep!r}")
        if isinstance(min_kept, bool) or not isinstance(min_kept, int) or not 0 <= min_kept < 2 ** 31:
            raise ValueError(f"{name}: min_kept must be an integer >= 0, got {min_kept!r}")
        if max_prob is not None:
            max_prob = self._num("max_prob", max_prob)
            if not 0.0 < max_prob < 1.0:
                raise ValueError(f"{name}: max_prob must be None or in (0, 1), got {max_prob!r}")
        gamma = self._num("gamma", gamma)
        if gamma != 0.0 and gamma < 1.0:
            raise ValueError(f"{name}: gamma must be 0 or >= 1, got {gamma!r}: the derivative's factor (1 - p_t)^(gamma - 1) is "
                             "unbounded at p_t -> 1 for a gamma in (0, 1)")
        self.keep, self.min_kept, self.max_prob, self.gamma = keep, min_kept, max_prob, gamma
        self.per_image = bool(per_image)
        self.losses: Optional[torch.Tensor] = None   # _plans holds (descriptor, item table, workspace, losses, selection) per key
        self.selection: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ the published recipes
    @classmethod
    def topk(cls, base, k: float = 0.1, **kw) -> "HardPixelLoss":
        """the mean over the hardest fraction ``k`` of the pixels (nnU-Net's ``TopKLoss``, ``k`` as a fraction, not per cent)"""
        return cls(base, keep=k, **kw)

    @classmethod
    def ohem(cls, base, thresh: float = 0.7, min_kept: int = 100_000, **kw) -> "HardPixelLoss":
        """online hard example mining: the pixels with ``p_t < thresh``, and the ``min_kept`` hardest at least; ``keep`` is
        the smallest normal fp32, so that ``min_kept`` and ``max_prob`` decide"""
        return cls(base, keep=L.HARDPIXEL_MIN_KEEP, min_kept=min_kept, max_prob=thresh, **kw)

    @classmethod
    def focal(cls, base, gamma: float = 2.0, **kw) -> "HardPixelLoss":
        """the focal loss ``(1 - p_t)^gamma * CE`` over every pixel (``keep=1.0``)"""
        return cls(base, keep=1.0, gamma=gamma, **kw)

    # ------------------------------------------------------------------ the launches
    def _build_plan(self, n_items: int, shape, device: torch.device, main: int):
        if n_items > L.CLASS_MAX_ITEMS:
            raise ValueError(f"HardPixelLoss: {n_items} output maps, at most {L.CLASS_MAX_ITEMS} per call")
        N, C, H, W = (int(s) for s in shape)
        if self.class_mode and not 2 <= C <= L.CLASS_MAX_K:
            raise ValueError(f"HardPixelLoss: K = {C} classes outside [2, {L.CLASS_MAX_K}]")
        fshape = (N, H, W) if self.class_mode else (N, C, H, W)
        seg = math.prod(fshape) // (N if self.per_image else 1)
        if seg > L.HARDPIXEL_MAX_SEGMENT:
            raise ValueError(f"HardPixelLoss: a segment of {seg} elements, at most {L.HARDPIXEL_MAX_SEGMENT}")
        if self.per_image and n_items * N > L.HARDPIXEL_MAX_SEGMENTS:
            raise ValueError(f"HardPixelLoss: {n_items * N} segments in {n_items} maps, at most {L.HARDPIXEL_MAX_SEGMENTS}")
        if n_items * N * C * H * W > L.HARDPIXEL_MAX_ELEMENTS:
            raise ValueError(f"HardPixelLoss: {n_items * N * C * H * W} elements in {n_items} maps, at most {L.HARDPIXEL_MAX_ELEMENTS}")
        desc = L.HardPixelDesc(L.HARDPIXEL_CLASS if self.class_mode else L.HARDPIXEL_BINARY, n_items, N, C, H, W,
                               int(self.per_image), self.ignore_index, main, self.keep, self.min_kept,
                               0.0 if self.max_prob is None else self.max_prob, self.gamma, 0)
        ws = torch.empty((L.hardpixel_workspace_bytes(desc) + 7) // 8, dtype=torch.float64, device=device)
        losses = torch.zeros(fshape, dtype=torch.float32, device=device)
        selection = torch.zeros((N if self.per_image else 1, 4), dtype=torch.int32, device=device)
        return desc, (L.HardPixelItem * n_items)(), ws, losses, selection

    def _term(self, xs, t: torch.Tensor, shape, dl, weights, main: int, base_loss: torch.Tensor) -> torch.Tensor:
        """one uz_hardpixel_loss over all maps on the gradients the base wrote"""
        desc, items, ws, losses, selection = self._plan(len(xs), shape, t.device, main)
        out = torch.empty(2, dtype=torch.float32, device=t.device)
        self._fill(items, xs, dl, weights)
        ops.hardpixel_loss(desc, items, t, self._scales_on(t.device), base_loss, out, losses, selection, ws)
        self.losses, self.selection, self.term = losses, selection, out[1]
        return out[0]

    def __repr__(self) -> str:
        return (f"HardPixelLoss(base={self.base!r}, weight={self.weight}, base_scale={self.base_scale}, keep={self.keep}, "
                f"min_kept={self.min_kept}, max_prob={self.max_prob}, gamma={self.gamma}, per_image={self.per_image})")
