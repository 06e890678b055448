"""Loss and Dice metric of the reference's training step on the device.

The reference computes ``criterion(outputs, mask)`` with ``nn.BCEWithLogitsLoss()`` (scripts/train.py:135) and
``dice_coefficient(main_pred_logits, mask)`` (utils/metrics.py:7-24) and reads both back with ``.item()`` every step
(utils/training_loop.py:113-124).  Here one kernel pass produces the loss, its gradient and the Dice value as device
scalars; nothing synchronises with the host until the caller asks for the numbers.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib as L
from .criterion import INT_DTYPES, FusedCriterion, maps_of


def _bce_dice_launch(logits: torch.Tensor, target: torch.Tensor, need_grad: bool):
    """one uz_bce_dice pass -> ((loss, dice) as one fp32 tensor of two, d(loss)/d(logits) in fp32 or None)"""
    L.require_cuda(logits, target)
    assert logits.shape == target.shape, (logits.shape, target.shape)
    x = logits.detach().contiguous().float()
    t = target.detach().contiguous().float()
    n = x.numel()
    lib = L.load()
    dlogits = torch.empty_like(x) if need_grad else None
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    ws = torch.empty(L.check_count(lib.uz_bce_dice_workspace_bytes(n), "uz_bce_dice_workspace_bytes") // 8,
                     dtype=torch.float64, device=x.device)
    L.check(lib.uz_bce_dice(x.data_ptr(), t.data_ptr(), n, dlogits.data_ptr() if need_grad else None, out.data_ptr(),
                            ws.data_ptr(), L.stream_ptr()), "uz_bce_dice")
    return out, dlogits


class _BceDice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits: torch.Tensor, target: torch.Tensor):
        out, ctx.dlogits = _bce_dice_launch(logits, target, ctx.needs_input_grad[0])
        ctx.in_dtype = logits.dtype
        dice = out[1]
        ctx.mark_non_differentiable(dice)
        return out[0], dice

    @staticmethod
    def backward(ctx, g_loss, _g_dice):
        return (ctx.dlogits * g_loss).to(ctx.in_dtype), None


def bce_dice_direct(logits: torch.Tensor, target: torch.Tensor):
    """(loss, dice, d(loss)/d(logits)) from ONE kernel pass and nothing else: no autograd node, hence none of the launches
    loss.backward() adds (the ones_like fill, the multiplication by it, a cast) -- the graphed step's form"""
    out, dlogits = _bce_dice_launch(logits, target, True)
    return out[0], out[1], dlogits


def loss_and_dice_direct(outputs, target: torch.Tensor):
    """loss_and_dice() plus the gradients of the loss with respect to every output tensor, in the order the model emits
    them (HipModule.wrap_outputs keeps that order for dicts and lists); the summed losses of u2net's seven maps /
    nested_unet's deep-supervision heads have unit weights (training_loop.py:24-32, 60-64), so each map's gradient is its
    own BCE gradient"""
    if isinstance(outputs, (dict, list, tuple)):
        _, maps, main = maps_of(outputs)
        trip = [bce_dice_direct(v, target) for v in maps]
        return sum(p[0] for p in trip), trip[main][1], tuple(p[2] for p in trip)
    l, d, g = bce_dice_direct(outputs, target)
    return l, d, (g,)


def bce_dice_with_logits(logits: torch.Tensor, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(BCEWithLogitsLoss(logits, target), dice_coefficient(logits, target)) as 0-dim device tensors"""
    return _BceDice.apply(logits, target)


def loss_and_dice(outputs, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The step's loss and main-output Dice for every output container of the zoo: a tensor; u2net's dict
    (sum over d0..d6, Dice of d0; training_loop.py:24-32); nested_unet's deep-supervision list (sum, Dice of the
    last = finest output)."""
    if isinstance(outputs, (dict, list, tuple)):
        _, maps, main = maps_of(outputs)
        pairs = [bce_dice_with_logits(v, target) for v in maps]
        return sum(p[0] for p in pairs), pairs[main][1]
    return bce_dice_with_logits(outputs, target)


# ---------------------------------------------------------------------------------------------------------------------
# BCE + region term (soft Dice / Tversky / focal Tversky): uz_region_loss, three launches for any number of output maps
# ---------------------------------------------------------------------------------------------------------------------
_REDUCES = ("batch", "image", "channel")


class RegionLoss(FusedCriterion):
    """``w_bce * BCEWithLogits + w_region * region`` on the device, for every output container of the zoo.

    Per output map (logits ``x`` and target ``t`` of one shape ``(N, K, H, W)``; ``p = sigmoid(x)``)::

        BCE     = mean_i [ -(pos_weight * t_i * log p_i + (1 - t_i) * log(1 - p_i)) ]
        I_g, S_g, T_g = sum p t, sum p, sum t   over group g of the flattened map
                  reduce="batch": one group; "image": one per image (K*H*W elements); "channel": one per (image, channel)
        TI_g    = (I_g + smooth) / (I_g + alpha (S_g - I_g) + beta (T_g - I_g) + smooth)          (Tversky index)
        region  = mean_g (1 - TI_g) ** gamma                                                      (gamma > 1: focal Tversky)
        loss    = w_bce * BCE + w_region * region

    ``alpha = beta = 0.5`` is the soft Dice loss: with ``smooth = s / 2`` the index is ``(2 I + s) / (S + T + s)``;
    ``RegionLoss.dice(smooth=s)`` builds exactly that.  ``alpha`` weighs false positives, ``beta`` false negatives.

    For a dict (u2net) or a list (nested_unet with deep supervision) the loss is ``sum_m output_weights[m] * loss(map_m)``;
    ``output_weights`` is a sequence in the order the model emits its maps, or a dict by key for dict outputs; the default
    is one for every map, as in ``loss_and_dice``.

    The Dice METRIC returned beside the loss is ``loss_and_dice``'s: thresholded prediction (``x > 0``), epsilon 1e-7, 1 for
    an empty union, over the whole MAIN map (first value of a dict, last element of a list).

    One call is one ``uz_region_loss``: three launches whatever the number of maps (two without gradients), fixed summation
    order, no library reduction -- so ``GraphedStep(model, RegionLoss(...))`` and ``GraphedEval`` keep the loss INSIDE their
    graphs, where a Python criterion runs eagerly between them.  In a data-parallel step every rank evaluates the loss on its
    own shard (as the reference's replicas do): ``reduce="batch"`` is therefore per shard, not per global batch.

    The workspace of a (number of maps, shape, device) is kept: calls of one object must follow each other on one stream or
    be ordered by the caller (``GraphedStep`` / ``GraphedEval`` and plain training loops are).
    """

    _NAME = "RegionLoss"

    def __init__(self, w_bce: float = 1.0, w_region: float = 1.0, alpha: float = 0.5, beta: float = 0.5,
                 smooth: float = 1.0, gamma: float = 1.0, reduce: str = "image", pos_weight=None, output_weights=None):
        super().__init__()       # _plans: (descriptor, item table, workspace) per key
        num = self._num
        self.w_bce, self.w_region = num("w_bce", w_bce), num("w_region", w_region)
        self.alpha, self.beta = num("alpha", alpha), num("beta", beta)
        self.smooth, self.gamma = num("smooth", smooth), num("gamma", gamma)
        self.pos_weight = 1.0 if pos_weight is None else num("pos_weight", pos_weight)
        if self.smooth <= 0:
            raise ValueError(f"RegionLoss: smooth must be > 0, got {smooth!r}")
        if self.gamma < 1:
            raise ValueError(f"RegionLoss: gamma must be >= 1, got {gamma!r}")
        if self.alpha < 0 or self.beta < 0:
            raise ValueError(f"RegionLoss: alpha and beta must be >= 0, got {alpha!r}, {beta!r}")
        if self.w_bce < 0 or self.w_region < 0:
            raise ValueError(f"RegionLoss: w_bce and w_region must be >= 0, got {w_bce!r}, {w_region!r}")
        if self.w_bce == 0 and self.w_region == 0:
            raise ValueError("RegionLoss: w_bce and w_region are both zero")
        if self.pos_weight <= 0:
            raise ValueError(f"RegionLoss: pos_weight must be > 0, got {pos_weight!r}")
        if reduce not in _REDUCES:
            raise ValueError(f"RegionLoss: reduce must be one of {_REDUCES}, got {reduce!r}")
        self.reduce = reduce
        self.output_weights = self._output_weights(output_weights)

    @classmethod
    def dice(cls, smooth: float = 1.0, **kw) -> "RegionLoss":
        """BCE + soft Dice loss ``1 - (2 I + smooth) / (S + T + smooth)``: alpha = beta = 0.5 and half the smoothing"""
        return cls(alpha=0.5, beta=0.5, smooth=float(smooth) / 2.0, **kw)

    @classmethod
    def tversky(cls, alpha: float, beta: float, **kw) -> "RegionLoss":
        """BCE + Tversky loss (``gamma > 1``: focal Tversky); alpha weighs false positives, beta false negatives"""
        return cls(alpha=alpha, beta=beta, **kw)

    def _groups(self, shape) -> int:
        if self.reduce == "batch":
            return 1
        if len(shape) < 2:
            raise ValueError(f"RegionLoss: reduce={self.reduce!r} needs (N, K, ...) maps, got shape {tuple(shape)}")
        return int(shape[0]) if self.reduce == "image" else int(shape[0]) * int(shape[1])

    def _build_plan(self, n_items: int, shape, device: torch.device, main: int):
        if n_items > L.REGION_MAX_ITEMS:
            raise ValueError(f"RegionLoss: {n_items} output maps, at most {L.REGION_MAX_ITEMS} per call")
        n = 1
        for s in shape:
            n *= int(s)
        desc = L.RegionDesc(n_items, n, self._groups(shape), self.w_bce, self.w_region, self.alpha, self.beta,
                            self.smooth, self.gamma, self.pos_weight, main)
        ws = torch.empty((L.region_loss_workspace_bytes(desc) + 7) // 8, dtype=torch.float64, device=device)
        return desc, (L.RegionItem * n_items)(), ws

    def _launch(self, logits, target: torch.Tensor, weights, main: int, need):
        """one uz_region_loss over all maps -> (loss, dice, [d(loss)/d(map) in fp32, or None where need is False])"""
        L.require_cuda(target, *logits)
        for v in logits:
            if v.shape != target.shape:
                raise ValueError(f"RegionLoss: an output map of shape {tuple(v.shape)} against a target of shape "
                                 f"{tuple(target.shape)}")
            if v.dtype not in (torch.float32, torch.bfloat16):
                raise ValueError(f"RegionLoss: logits must be float32 or bfloat16, got {v.dtype}")
            if v.device != target.device:
                raise ValueError(f"RegionLoss: an output map on {v.device} against a target on {target.device}")
        if target.numel() == 0:
            raise ValueError("RegionLoss: empty maps")
        xs = [v.detach().contiguous().float() for v in logits]     # bf16 logits become fp32, as in bce_dice_with_logits
        t = target.detach().contiguous().float()
        desc, items, ws = self._plan(len(xs), t.shape, t.device, main)
        dl = [torch.empty_like(x) if g else None for x, g in zip(xs, need)]
        out = torch.empty(2, dtype=torch.float32, device=t.device)
        self._fill(items, xs, dl, weights)
        for it in items:           # (an item of this kernel names its target too: all maps share one)
            it.target = t.data_ptr()
        L.region_loss(desc, items, out, ws)
        return out[0], out[1], dl

    def __repr__(self) -> str:
        return (f"RegionLoss(w_bce={self.w_bce}, w_region={self.w_region}, alpha={self.alpha}, beta={self.beta}, "
                f"smooth={self.smooth}, gamma={self.gamma}, reduce={self.reduce!r}, pos_weight={self.pos_weight}, "
                f"output_weights={self.output_weights})")


# ---------------------------------------------------------------------------------------------------------------------
# Softmax cross-entropy + soft Dice over class-index labels: uz_class_loss, three launches for any number of output maps
# ---------------------------------------------------------------------------------------------------------------------
_CLASS_REDUCES = {"batch": L.CLASS_REDUCE_BATCH, "image": L.CLASS_REDUCE_IMAGE}


class MulticlassLoss(FusedCriterion):
    """``w_ce * CrossEntropy + w_dice * Dice`` over softmax probabilities on the device, for every output container of the zoo.

    Per output map (logits ``x`` of shape ``(N, K, H, W)``, labels ``y`` of shape ``(N, H, W)`` or ``(N, 1, H, W)`` holding
    class indices of any integer dtype; ``p = softmax_K(x)``, ``w = class_weight`` or ones, ``e = label_smoothing``).  A pixel
    is VALID when ``y != ignore_index`` and ``0 <= y < K``; a label outside ``[0, K)`` that is not ``ignore_index`` is treated
    as ignored and counted in ``.counts`` (no device assert)::

        a_c(i)  = (1 - e) w_c [c == y_i] + (e / K) w_c
        CE      = sum_valid sum_c a_c(i) (-log p_c(i)) / sum_valid w_{y_i}
                  -- F.cross_entropy(x, y, weight=w, ignore_index=..., label_smoothing=e); but 0 with zero gradient, not NaN,
                  when no pixel is valid
        I, S, T = sum p_c [y == c], sum p_c (square=True: sum p_c^2), sum [y == c]     over the valid pixels of group g
                  reduce="batch": one group; "image": one per image
        dice    = mean over g and c in C of (1 - (2 I + smooth) / (S + T + smooth))
                  C: all classes, or 1 .. K-1 with include_background=False
        loss    = w_ce * CE + w_dice * dice

    ``MulticlassLoss.ce_dice()`` is the published Swin-UNet / TransUNet recipe ``0.4 CE + 0.6 Dice`` with ``square=True``,
    ``smooth=1e-5``, ``reduce="batch"``.

    For a dict (u2net) or a list (nested_unet with deep supervision) the loss is ``sum_m output_weights[m] * loss(map_m)``, as
    in ``RegionLoss``.  The Dice METRIC returned beside the loss is computed from the MAIN map (first value of a dict, last
    element of a list): prediction ``argmax_K x`` (ties: the lowest index), per class over the valid pixels of the batch
    ``2 TP_c / (P_c + T_c)``, averaged over the classes of C that occur in prediction or labels; 1 when none does.
    ``.counts`` is the last call's ``(K + 1, 3)`` int64 device tensor of that map: rows ``TP_c, P_c, T_c``, then
    ``(valid, ignored, out of range)`` -- sum it over an epoch for dataset-level Dice / IoU.

    One call is one ``uz_class_loss``: three launches whatever the number of maps (two without gradients), fixed summation
    order, no library reduction -- ``GraphedStep(model, MulticlassLoss(...))`` and ``GraphedEval`` keep it INSIDE their graphs
    and hold the labels in an int32 static buffer (``target_dtype``).  In a data-parallel step every rank evaluates the loss on
    its own shard: ``reduce="batch"`` is per shard.

    Workspace, counts and the class-weight copy of a (number of maps, shape, device) are kept: calls of one object must
    follow each other on one stream or be ordered by the caller, and ``.counts`` is overwritten by the next call.
    The descriptor of such a plan is built at the first call with that (number of maps, shape, device): the settings are the
    constructor's, and changing an attribute of the object afterwards has no effect on shapes already seen -- build a new
    object instead.  ``GraphedStep`` / ``GraphedEval`` warm the criterion up outside the capture for the first shape; a
    further input shape allocates its workspace and counts during its own capture (from the graph's pool), as
    ``RegionLoss`` does.
    """

    _NAME = "MulticlassLoss"
    target_dtype = torch.int32

    def __init__(self, w_ce: float = 1.0, w_dice: float = 1.0, smooth: float = 1.0, label_smoothing: float = 0.0,
                 class_weight=None, ignore_index: int = -100, include_background: bool = True, reduce: str = "image",
                 square: bool = False, output_weights=None):
        super().__init__()       # _plans: (descriptor, item table, workspace, counts) per key
        num = self._num
        self.w_ce, self.w_dice = num("w_ce", w_ce), num("w_dice", w_dice)
        self.smooth, self.label_smoothing = num("smooth", smooth), num("label_smoothing", label_smoothing)
        if self.w_ce < 0 or self.w_dice < 0:
            raise ValueError(f"MulticlassLoss: w_ce and w_dice must be >= 0, got {w_ce!r}, {w_dice!r}")
        if self.w_ce == 0 and self.w_dice == 0:
            raise ValueError("MulticlassLoss: w_ce and w_dice are both zero")
        if self.smooth <= 0:
            raise ValueError(f"MulticlassLoss: smooth must be > 0, got {smooth!r}")
        if not 0 <= self.label_smoothing < 1:
            raise ValueError(f"MulticlassLoss: label_smoothing must be in [0, 1), got {label_smoothing!r}")
        if isinstance(ignore_index, bool) or not isinstance(ignore_index, int) or not -2 ** 31 <= ignore_index < 2 ** 31:
            raise ValueError(f"MulticlassLoss: ignore_index must be an int32 value, got {ignore_index!r}")
        self.ignore_index = ignore_index
        if reduce not in _CLASS_REDUCES:
            raise ValueError(f"MulticlassLoss: reduce must be one of {tuple(_CLASS_REDUCES)}, got {reduce!r}")
        self.reduce = reduce
        self.include_background, self.square = bool(include_background), bool(square)
        if class_weight is None:
            self.class_weight = None
        else:
            cw = class_weight.tolist() if isinstance(class_weight, torch.Tensor) else list(class_weight)
            self.class_weight = tuple(num(f"class_weight[{i}]", v) for i, v in enumerate(cw))
            if not L.CLASS_MAX_K >= len(self.class_weight) >= 2:
                raise ValueError(f"MulticlassLoss: class_weight must have 2 .. {L.CLASS_MAX_K} entries, got {len(self.class_weight)}")
            if any(v < 0 for v in self.class_weight):
                raise ValueError(f"MulticlassLoss: class_weight must be >= 0, got {class_weight!r}")
        self.output_weights = self._output_weights(output_weights)
        self._cw_dev = {}     # device index -> the class weights, uploaded once
        self.counts: Optional[torch.Tensor] = None

    @classmethod
    def ce_dice(cls, w_ce: float = 0.4, w_dice: float = 0.6, **kw) -> "MulticlassLoss":
        """the published Swin-UNet / TransUNet loss: ``w_ce * CE + w_dice * Dice`` with squared probabilities in the
        denominator, ``smooth = 1e-5``, sums over the whole batch"""
        kw.setdefault("square", True)
        kw.setdefault("smooth", 1e-5)
        kw.setdefault("reduce", "batch")
        return cls(w_ce=w_ce, w_dice=w_dice, **kw)

    def _build_plan(self, n_items: int, shape, device: torch.device, main: int):
        N, K = int(shape[0]), int(shape[1])
        hw = 1
        for s in shape[2:]:
            hw *= int(s)
        desc = L.ClassDesc(n_items, N, K, hw, self.w_ce, self.w_dice, self.smooth, self.label_smoothing, self.ignore_index,
                           _CLASS_REDUCES[self.reduce], int(self.include_background), int(self.square), main)
        ws = torch.empty((L.class_loss_workspace_bytes(desc) + 7) // 8, dtype=torch.float64, device=device)
        counts = torch.zeros(K + 1, 3, dtype=torch.int64, device=device)
        return desc, (L.ClassItem * n_items)(), ws, counts

    def _weights_on(self, device: torch.device, K: int):
        if self.class_weight is None:
            return None
        if len(self.class_weight) != K:
            raise ValueError(f"MulticlassLoss: {len(self.class_weight)} class_weight entries for logits of {K} classes")
        cw = self._cw_dev.get(device.index)
        if cw is None:
            cw = self._cw_dev[device.index] = torch.tensor(self.class_weight, dtype=torch.float32, device=device)
        return cw

    def _launch(self, logits, target: torch.Tensor, weights, main: int, need):
        """one uz_class_loss over all maps -> (loss, dice, [d(loss)/d(map) in fp32, or None where need is False])"""
        if not logits:
            raise ValueError("MulticlassLoss: no output map")
        if len(logits) > L.CLASS_MAX_ITEMS:
            raise ValueError(f"MulticlassLoss: {len(logits)} output maps, at most {L.CLASS_MAX_ITEMS} per call")
        if target.dtype not in INT_DTYPES:
            raise ValueError(f"MulticlassLoss: the target holds class indices and must have an integer dtype, got {target.dtype}")
        shape = tuple(logits[0].shape)
        if len(shape) < 3:
            raise ValueError(f"MulticlassLoss: logits must be (N, K, H, W), got shape {shape}")
        K = shape[1]
        if not 2 <= K <= L.CLASS_MAX_K:
            raise ValueError(f"MulticlassLoss: K = {K} classes outside [2, {L.CLASS_MAX_K}]")
        want = (shape[0],) + shape[2:]
        tshape = tuple(target.shape)
        if tshape == (shape[0], 1) + shape[2:]:
            tshape = want
        if tshape != want:
            raise ValueError(f"MulticlassLoss: logits of shape {shape} against a target of shape {tuple(target.shape)}; "
                             f"expected {want} or {(shape[0], 1) + shape[2:]}")
        for v in logits:
            if tuple(v.shape) != shape:
                raise ValueError(f"MulticlassLoss: output maps of shape {tuple(v.shape)} and {shape} in one call")
            if v.dtype not in (torch.float32, torch.bfloat16):
                raise ValueError(f"MulticlassLoss: logits must be float32 or bfloat16, got {v.dtype}")
        if target.numel() == 0:
            raise ValueError("MulticlassLoss: empty maps")
        L.require_cuda(target, *logits)
        for v in logits:
            if v.device != target.device:
                raise ValueError(f"MulticlassLoss: an output map on {v.device} against a target on {target.device}")
        xs = [v.detach().contiguous().float() for v in logits]     # bf16 logits become fp32, as in RegionLoss
        y = target.detach().reshape(want).contiguous().to(torch.int32)
        cw = self._weights_on(y.device, K)
        desc, items, ws, counts = self._plan(len(xs), shape, y.device, main)
        dl = [torch.empty_like(x) if g else None for x, g in zip(xs, need)]
        out = torch.empty(2, dtype=torch.float32, device=y.device)
        self._fill(items, xs, dl, weights)
        L.class_loss(desc, items, y, cw, out, counts, ws)
        self.counts = counts
        return out[0], out[1], dl

    def __repr__(self) -> str:
        return (f"MulticlassLoss(w_ce={self.w_ce}, w_dice={self.w_dice}, smooth={self.smooth}, "
                f"label_smoothing={self.label_smoothing}, class_weight={self.class_weight}, ignore_index={self.ignore_index}, "
                f"include_background={self.include_background}, reduce={self.reduce!r}, square={self.square}, "
                f"output_weights={self.output_weights})")
