"""What a criterion that sits INSIDE the step and evaluation graphs is, once (DESIGN.md 3k'): ``FusedCriterion``.

A subclass sets ``_NAME`` (the prefix of its messages) and implements ``_launch``; the base class gives it the three forms the
graphed runners take (``loss_and_dice`` through ONE autograd node for all output maps, ``__call__``, ``direct``), the weights of
the output maps, number parsing and the cache of what it keeps per input shape.  ``capture.resolve_criterion`` recognises a
criterion by this class alone.  Nothing here touches the GPU: ``require_cuda`` is each ``_launch``'s.
"""
from __future__ import annotations

import math
from typing import Tuple

import torch

INT_DTYPES = (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64)


def maps_of(outputs):
    """(keys or None, the output tensors in the order the model emits them, index of the main output): first value of a
    dict, last element of a list -- as loss_and_dice picks the map of the Dice metric"""
    if isinstance(outputs, dict):
        return tuple(outputs.keys()), tuple(outputs.values()), 0
    if isinstance(outputs, (list, tuple)):
        return None, tuple(outputs), len(outputs) - 1
    return None, (outputs,), 0


class _FusedFn(torch.autograd.Function):
    """ONE node for all output maps: forward is the criterion's one ``_launch``, which also writes every map's gradient"""

    @staticmethod
    def forward(ctx, crit: "FusedCriterion", target: torch.Tensor, weights: tuple, main: int, taping: bool, *logits: torch.Tensor):
        # needs_input_grad is requires_grad whatever the grad mode (which is off in here): under no_grad nothing is needed
        need = ctx.needs_input_grad[5:] if taping else (False,) * len(logits)
        loss, dice, dl = crit._launch(logits, target, weights, main, need)
        ctx.dl = dl
        ctx.in_dtypes = tuple(v.dtype for v in logits)
        ctx.mark_non_differentiable(dice)
        return loss, dice

    @staticmethod
    def backward(ctx, g_loss, _g_dice):
        return (None, None, None, None, None) + tuple(None if d is None else (d * g_loss).to(dt)
                                                for d, dt in zip(ctx.dl, ctx.in_dtypes))


class FusedCriterion:
    """The base of every criterion the graphed runners capture.  A subclass provides

        _launch(logits, target, weights, main, need) -> (loss, dice, [d(loss)/d(map) in fp32, or None where need is False])

    over all output maps at once (``weights``: one per map, ``main``: the map of the Dice metric), and promises a fixed
    number of launches per descriptor, no library reduction, and that what it keeps per input shape (``_plan``) is allocated
    at the first call with that shape."""

    _NAME = "FusedCriterion"
    target_dtype = torch.float32         # the static target buffer's dtype in a graphed runner

    def __init__(self):
        self._plans = {}      # (number of maps, shape, device index, main) -> what _build_plan made for it

    # ------------------------------------------------------------------ the settings
    @classmethod
    def _num(cls, name, v) -> float:
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"{cls._NAME}: {name} must be a number, got {v!r}") from None
        if not math.isfinite(f):
            raise ValueError(f"{cls._NAME}: {name} must be finite, got {v!r}")
        return f

    @classmethod
    def _output_weights(cls, output_weights):
        """``output_weights`` as the constructors take it: None, a sequence in emission order, or a dict by key"""
        if output_weights is None:
            return None
        if isinstance(output_weights, dict):
            ow = {k: cls._num(f"output_weights[{k!r}]", v) for k, v in output_weights.items()}
        else:
            ow = tuple(cls._num(f"output_weights[{i}]", v) for i, v in enumerate(output_weights))
        if any(v < 0 for v in (ow.values() if isinstance(ow, dict) else ow)):
            raise ValueError(f"{cls._NAME}: output_weights must be >= 0, got {output_weights!r}")
        return ow

    # ------------------------------------------------------------------ the containers
    def weights_for(self, outputs) -> tuple:
        """the weight of every output map, in the order the model emits them"""
        keys, maps, _ = maps_of(outputs)
        ow = self.output_weights
        if ow is None:
            return (1.0,) * len(maps)
        if isinstance(ow, dict):
            if keys is None:
                raise ValueError(f"{self._NAME}: output_weights is a dict but the outputs are not")
            missing = [k for k in keys if k not in ow]
            if missing:
                raise ValueError(f"{self._NAME}: output_weights has no entry for the outputs {missing}")
            return tuple(ow[k] for k in keys)
        if len(ow) != len(maps):
            raise ValueError(f"{self._NAME}: {len(ow)} output_weights for {len(maps)} output maps")
        return ow

    # ------------------------------------------------------------------ what is kept per shape
    def _plan(self, n_items: int, shape, device: torch.device, main: int):
        key = (n_items, tuple(shape), device.index, main)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = self._build_plan(n_items, shape, device, main)
        return plan

    def _build_plan(self, n_items: int, shape, device: torch.device, main: int):
        """(descriptor, item table, workspace, ...) of one (number of maps, shape, device, main): built once"""
        raise NotImplementedError

    @staticmethod
    def _fill(items, xs, dl, weights) -> None:
        """the item table of one launch: every map's fp32 logits, its gradient buffer (or NULL) and its weight"""
        for it, x, d, w in zip(items, xs, dl, weights):
            it.logits, it.dlogits, it.weight = x.data_ptr(), (d.data_ptr() if d is not None else None), w

    def _launch(self, logits, target: torch.Tensor, weights, main: int, need):
        raise NotImplementedError

    # ------------------------------------------------------------------ the three forms
    def loss_and_dice(self, outputs, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(loss, Dice metric of the main output) as 0-dim device tensors; the loss is differentiable with respect to every
        output tensor through ONE autograd node (any CUDA fp32 / bf16 logits: a stock torch model's too); under ``no_grad``
        no gradient buffer is touched"""
        _, maps, main = maps_of(outputs)
        return _FusedFn.apply(self, target, self.weights_for(outputs), main, torch.is_grad_enabled(), *maps)

    def __call__(self, outputs, target: torch.Tensor) -> torch.Tensor:
        return self.loss_and_dice(outputs, target)[0]

    def direct(self, outputs, target: torch.Tensor):
        """(loss, dice, d(loss)/d(outputs)) without an autograd node -- the graphed step's form; the gradients (fp32) come in
        the order the model emits its outputs (HipModule.wrap_outputs keeps it), as from loss_and_dice_direct"""
        _, maps, main = maps_of(outputs)
        loss, dice, dl = self._launch(maps, target, self.weights_for(outputs), main, (True,) * len(maps))
        return loss, dice, tuple(dl)
