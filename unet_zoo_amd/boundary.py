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

import math
from typing import Optional, Tuple, Union

import torch

from . import _lib as L
from . import ops
from .loss import MulticlassLoss, RegionLoss, _INT_DTYPES, _maps_of, bce_dice_direct, bce_dice_with_logits

_MAX_HW = L.BOUNDARY_MAX_HW


class _BoundaryFn(torch.autograd.Function):
    """ONE node for all output maps: forward is the base's launch plus one uz_boundary_loss on the gradients it wrote"""

    @staticmethod
    def forward(ctx, crit: "BoundaryLoss", target: torch.Tensor, weights: tuple, main: int, *logits: torch.Tensor):
        loss, dice, dl = crit._launch(logits, target, weights, main, ctx.needs_input_grad[4:])
        ctx.dl = dl
        ctx.in_dtypes = tuple(v.dtype for v in logits)
        ctx.mark_non_differentiable(dice)
        return loss, dice

    @staticmethod
    def backward(ctx, g_loss, _g_dice):
        return (None, None, None, None) + tuple(None if d is None else (d * g_loss).to(dt)
                                                for d, dt in zip(ctx.dl, ctx.in_dtypes))


class BoundaryLoss:
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

    def __init__(self, base: Union[str, RegionLoss, MulticlassLoss] = "bce_dice", weight: float = 0.01, base_scale: float = 1.0,
                 include_background: bool = False, spacing: float = 1.0):
        if isinstance(base, str):
            if base != "bce_dice":
                raise TypeError(f"BoundaryLoss: base must be 'bce_dice', a RegionLoss or a MulticlassLoss, got {base!r}")
        elif not isinstance(base, (RegionLoss, MulticlassLoss)):
            raise TypeError(f"BoundaryLoss: base must be 'bce_dice', a RegionLoss or a MulticlassLoss, got {type(base).__name__}")
        self.base = base
        self.class_mode = isinstance(base, MulticlassLoss)
        self.weight, self.base_scale = self._check_weights(weight, base_scale)
        self.spacing = self._num("spacing", spacing)
        if self.spacing <= 0:
            raise ValueError(f"BoundaryLoss: spacing must be > 0, got {spacing!r}")
        self.include_background = bool(include_background)
        self.ignore_index = base.ignore_index if self.class_mode else -100
        self._plans = {}       # (number of maps, logits shape, device index, main) -> (descriptor, item table, workspace, sd2)
        self._scales = {}      # device index -> (weight, base_scale) on the device: what the kernels (and the graphs) read
        self.sd2: Optional[torch.Tensor] = None
        self.term: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ the settings
    @staticmethod
    def _num(name, v) -> float:
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"BoundaryLoss: {name} must be a number, got {v!r}") from None
        if not math.isfinite(f):
            raise ValueError(f"BoundaryLoss: {name} must be finite, got {v!r}")
        return f

    @classmethod
    def _check_weights(cls, weight, base_scale) -> Tuple[float, float]:
        w, b = cls._num("weight", weight), cls._num("base_scale", base_scale)
        if w < 0 or b < 0:
            raise ValueError(f"BoundaryLoss: weight and base_scale must be >= 0, got {weight!r}, {base_scale!r}")
        if w == 0 and b == 0:
            raise ValueError("BoundaryLoss: weight and base_scale are both zero")
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

    def rebalance(self, alpha: float) -> None:
        """Kervadec's schedule: ``base_scale = 1 - alpha``, ``weight = alpha`` for ``alpha`` in [0, 1]"""
        a = self._num("alpha", alpha)
        if not 0.0 <= a <= 1.0:
            raise ValueError(f"BoundaryLoss: alpha must be in [0, 1], got {alpha!r}")
        self.set_weights(weight=a, base_scale=1.0 - a)

    # ------------------------------------------------------------------ the containers
    def weights_for(self, outputs) -> tuple:
        """the weight of every output map, in the order the model emits them: the base's"""
        if isinstance(self.base, str):
            return (1.0,) * len(_maps_of(outputs)[1])
        return self.base.weights_for(outputs)

    def _plan(self, n_items: int, shape, device: torch.device, main: int):
        key = (n_items, tuple(shape), device.index, main)
        plan = self._plans.get(key)
        if plan is None:
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
            plan = self._plans[key] = (desc, (L.BoundaryItem * n_items)(), ws, sd2)
        return plan

    def _scales_on(self, device: torch.device) -> torch.Tensor:
        s = self._scales.get(device.index)
        if s is None:
            s = self._scales[device.index] = torch.tensor([self.weight, self.base_scale], dtype=torch.float32, device=device)
        return s

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

    def _launch(self, logits, target: torch.Tensor, weights, main: int, need):
        """the base's launch, then one uz_boundary_loss over all maps -> (loss, dice, [d(loss)/d(map) in fp32, or None])"""
        if not logits:
            raise ValueError("BoundaryLoss: no output map")
        shape = tuple(logits[0].shape)
        if len(shape) != 4:
            raise ValueError(f"BoundaryLoss: output maps must be (N, C, H, W), got shape {shape}")
        for v in logits:
            if tuple(v.shape) != shape:
                raise ValueError(f"BoundaryLoss: output maps of shape {tuple(v.shape)} and {shape} in one call")
            if v.dtype not in (torch.float32, torch.bfloat16):
                raise ValueError(f"BoundaryLoss: logits must be float32 or bfloat16, got {v.dtype}")
        if self.class_mode:
            if target.dtype not in _INT_DTYPES:
                raise ValueError(f"BoundaryLoss: the target holds class indices and must have an integer dtype, got {target.dtype}")
            want = (shape[0],) + shape[2:]
            if tuple(target.shape) not in (want, (shape[0], 1) + shape[2:]):
                raise ValueError(f"BoundaryLoss: logits of shape {shape} against a target of shape {tuple(target.shape)}; "
                                 f"expected {want} or {(shape[0], 1) + shape[2:]}")
        elif tuple(target.shape) != shape:
            raise ValueError(f"BoundaryLoss: an output map of shape {shape} against a target of shape {tuple(target.shape)}")
        if target.numel() == 0:
            raise ValueError("BoundaryLoss: empty maps")
        L.require_cuda(target, *logits)
        for v in logits:
            if v.device != target.device:
                raise ValueError(f"BoundaryLoss: an output map on {v.device} against a target on {target.device}")
        base_loss, dice, dl = self._base_launch(logits, target, weights, main, need)
        xs = [v.detach().contiguous().float() for v in logits]      # bf16 logits become fp32, as in the base
        if self.class_mode:
            t = target.detach().reshape((shape[0],) + shape[2:]).contiguous().to(torch.int32)
        else:
            t = target.detach().contiguous().float()
        desc, items, ws, sd2 = self._plan(len(xs), shape, t.device, main)
        out = torch.empty(2, dtype=torch.float32, device=t.device)
        for it, x, d, w in zip(items, xs, dl, weights):
            it.logits, it.dlogits, it.weight = x.data_ptr(), (d.data_ptr() if d is not None else None), w
        ops.boundary_loss(desc, items, t, self._scales_on(t.device), base_loss.detach().reshape(1), out, sd2, ws)
        self.sd2, self.term = sd2, out[1]
        return out[0], dice, dl

    # ------------------------------------------------------------------ the three forms
    def loss_and_dice(self, outputs, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(loss, the base's Dice metric of the main output) as 0-dim device tensors; the loss is differentiable with respect
        to every output tensor through ONE autograd node; under ``no_grad`` no gradient buffer is touched"""
        _, maps, main = _maps_of(outputs)
        return _BoundaryFn.apply(self, target, self.weights_for(outputs), main, *maps)

    def __call__(self, outputs, target: torch.Tensor) -> torch.Tensor:
        return self.loss_and_dice(outputs, target)[0]

    def direct(self, outputs, target: torch.Tensor):
        """(loss, dice, d(loss)/d(outputs)) without an autograd node -- the graphed step's form: the base's launch, then one
        uz_boundary_loss on the gradients it returned (fp32, in the order the model emits its outputs)"""
        _, maps, main = _maps_of(outputs)
        loss, dice, dl = self._launch(maps, target, self.weights_for(outputs), main, (True,) * len(maps))
        return loss, dice, tuple(dl)

    def __repr__(self) -> str:
        return (f"BoundaryLoss(base={self.base!r}, weight={self.weight}, base_scale={self.base_scale}, "
                f"include_background={self.include_background}, spacing={self.spacing})")
