"""The reference's evaluation pass as hipGraph replays: ``GraphedEval``.

The reference evaluates after every epoch (unet_zoo/utils/training_loop.py:147-180, ``validate_one_epoch``) and once more
at the end (:287-320, ``evaluate_model``): per batch, under ``model.eval()`` and ``torch.no_grad()``,

    outputs = model(img); loss, dice = criterion / dice_coefficient (outputs, mask); running += loss.item(), dice.item()

Launched eagerly that is ~100 kernel launches from Python per batch (host-bound on small batches and maps; at B = 16, 256 x 256
the GPU work is longer, DESIGN.md 3h'').  ``GraphedEval`` is the same forward + loss + Dice captured once per input shape and
replayed:

    ev = unet_zoo_amd.GraphedEval(model, "bce_dice", fold_bn=True)
    loss, dice = ev(images, masks)                 # 0-dim device tensors, no host sync; ev.outputs = the model's outputs
    mean_loss, mean_dice = ev.evaluate(loader)     # validate_one_epoch: per-batch means, ONE read-back at the end

``fold_bn=True`` runs this object's captures on engines with ``fold_bn_eval`` set: a Conv -> BatchNorm -> ReLU layer without pool or
residual becomes one launch whose epilogue forms the activation from the convolution's fp32 result and the running-statistics
(scale, shift) -- the raw output is neither written nor re-read.  fp32 results are bit-identical to the eager forward; bf16
activations are rounded once instead of twice, so they differ from the eager forward within bf16 rounding.  With
``fold_bn=False`` the replay is bit-identical to the eager forward in both run dtypes.

``ev.loss``, ``ev.dice`` and ``ev.outputs`` are STATIC tensors of the captured graph: the next call with the same input
shape overwrites them in place, so read (``.item()``) or ``.clone()`` what must outlive the call.

Parameters are read where they live: the graph holds their addresses and re-packs the kernel-layout weight copies at its
start (the pack cache's batched launch), so an optimizer step between two calls -- ``GraphedStep`` included -- is seen by the
next replay.  When parameter or buffer STORAGE moves (``GraphedStep``'s first call gathers the parameters into one flat
buffer; ``.to()``; ``load_state_dict`` keeps storage) the graphs are captured again.

Module buffers are not modified by a replay, except where the reference's own eval forward modifies them: vnet's
normalisation uses batch statistics and updates its running statistics in eval mode too, once per call here as there.
"""
from __future__ import annotations

from itertools import chain
from typing import Callable, Dict, Optional, Tuple, Union

import torch
import torch.nn as nn

from . import _lib as L
from .engine import Engine
from .loss import MulticlassLoss, RegionLoss, loss_and_dice
from .step import CAPTURE_MODE, _check_capture, _new_graph, _unwrap


class _EvalGraph:
    """everything captured for one (input shape, target shape)"""
    __slots__ = ("x", "t", "graph", "outputs", "loss", "dice", "folded", "unfolded")


class GraphedEval:
    def __init__(self, model: nn.Module, criterion: Union[str, RegionLoss, MulticlassLoss, Callable] = "bce_dice", *, fold_bn: bool = False):
        self.model = _unwrap(model)
        if isinstance(criterion, str):
            if criterion != "bce_dice":
                raise ValueError(f"unknown built-in criterion {criterion!r}; pass 'bce_dice' or a callable")
            self._fused_loss = True
            self._loss_fn = None
            self._fused = loss_and_dice
        elif isinstance(criterion, (RegionLoss, MulticlassLoss)):
            # uz_region_loss / uz_class_loss: deterministic, no library reduction -- inside the graph, where "bce_dice" sits
            # (two launches: no gradient is asked for); with several ranks each evaluates its own shard, so reduce="batch" is
            # per shard
            self._fused_loss = True
            self._loss_fn = None
            self._fused = criterion.loss_and_dice
        else:
            # evaluated EAGERLY on the static outputs after the replay: library reductions must not be captured on this
            # stack, exactly as in GraphedStep
            self._fused_loss = False
            self._loss_fn = criterion
        # the static target buffer: float32 masks, or what the criterion asks for (MulticlassLoss: int32 class indices)
        self._target_dtype = getattr(criterion, "target_dtype", torch.float32)
        self.fold_bn = bool(fold_bn)
        self._graphs: Dict[tuple, _EvalGraph] = {}
        self._sig: Optional[tuple] = None
        self.loss: Optional[torch.Tensor] = None
        self.dice: Optional[torch.Tensor] = None
        self.outputs = None
        self.folded_layers = 0        # Conv -> BN -> ReLU layers of the last captured forward on the one-launch route
        self.unfolded_layers = 0      # ... and on the two-launch route (fold_bn=True only; both 0 otherwise)

    # ------------------------------------------------------------------ checks (no GPU call)
    def _check_model(self) -> torch.device:
        m = self.model
        if m.training:
            raise RuntimeError("GraphedEval is the EVALUATION pass: call model.eval() first (GraphedStep is the training step)")
        p = next(m.parameters(), None)
        if p is None or p.device.type != "cuda":
            raise RuntimeError("GraphedEval needs the model on an MI355X ('cuda'): unet_zoo_amd has no CPU path")
        return p.device

    def _signature(self) -> tuple:
        """what a captured graph holds by address: parameter / buffer storage and the pack cache's pointer tables"""
        m = self.model
        c = m._pack_cache
        tabs = tuple(t.data_ptr() if t is not None else 0 for t in (c._table, c._table3))
        return (m.run_dtype, tabs, tuple(t.data_ptr() for t in chain(m.parameters(), m.buffers())))

    # ------------------------------------------------------------------ the forward, as HipModule.forward runs it without a tape
    def _forward(self, x: torch.Tensor):
        m = self.model
        with torch.no_grad():
            m._pack_cache.refresh(m.run_dtype)
            eng = Engine(m.run_dtype, x.device, False, False, None, m._pack_cache, False, fold_bn_eval=self.fold_bn)
            outs = tuple(m.emit(eng, x))
            eng.finish_forward()
        self._last_counts = (eng.folded_layers, eng.unfolded_layers)
        return m.wrap_outputs(tuple(o.detach() for o in outs))

    def _capture(self, x: torch.Tensor, t: torch.Tensor) -> _EvalGraph:
        m = self.model
        g = _EvalGraph()
        g.x, g.t = x, t
        # one eager forward that changes nothing: creates the kernel-layout weight copies and the pack cache's pointer tables
        # (host-to-device copies, which a capture must not contain)
        saved = [b.detach().clone() for b in m.buffers()]
        rng = torch.cuda.get_rng_state(x.device)
        side = torch.cuda.Stream(device=x.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            warm = self._forward(x)
            if self._fused_loss and self._fused is not loss_and_dice:
                with torch.no_grad():      # a RegionLoss / MulticlassLoss keeps its workspace (counts, class weights) per shape:
                    # allocated here, outside the capture
                    self._fused(warm, t)
            del warm
            # weight copies registered by that forward leave the pack cache without its pointer tables: build them now
            # (GraphedStep._setup does the same after its dry run), the captured refresh must find them in place
            m._pack_cache.refresh(m.run_dtype)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize(x.device)
        for b, s in zip(m.buffers(), saved):
            b.copy_(s)
        torch.cuda.set_rng_state(rng, x.device)
        torch.cuda.synchronize(x.device)
        g.graph = _new_graph()
        g.loss = g.dice = None
        with torch.cuda.graph(g.graph, capture_error_mode=CAPTURE_MODE):
            g.outputs = self._forward(g.x)
            if self._fused_loss:
                with torch.no_grad():      # no gradient: uz_bce_dice / uz_region_loss / uz_class_loss run with dlogits = NULL
                    g.loss, g.dice = self._fused(g.outputs, g.t)
        _check_capture(g.graph, "evaluation graph")
        g.folded, g.unfolded = self._last_counts
        return g

    # ------------------------------------------------------------------ one batch
    def __call__(self, x: torch.Tensor, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(loss, dice) of one batch as 0-dim device tensors; `outputs` holds the model's output container"""
        dev = self._check_model()
        L.load()
        sig = self._signature()
        if sig != self._sig:
            self._graphs.clear()
        key = (tuple(x.shape), tuple(target.shape))
        g = self._graphs.get(key)
        if g is None:
            # static input buffers of this shape (fp32 on the model's device, what `.float().to(device)` of
            # training_loop.py:166-167 produces; the target in the criterion's target_dtype where it names one); later calls
            # copy into them -- host tensors included
            sx = x.detach().to(device=dev, dtype=torch.float32, copy=True)
            st = target.detach().to(device=dev, dtype=self._target_dtype, copy=True)
            g = self._graphs[key] = self._capture(sx, st)
            self._sig = self._signature()      # (the warm-up forward may have built the pack cache's tables)
        else:                                  # (a fresh capture's static buffers were created from this very batch)
            if x.data_ptr() != g.x.data_ptr():
                g.x.copy_(x)
            if target.data_ptr() != g.t.data_ptr():
                g.t.copy_(target)
        g.graph.replay()
        self.outputs = g.outputs
        self.folded_layers, self.unfolded_layers = g.folded, g.unfolded
        if self._fused_loss:
            self.loss, self.dice = g.loss, g.dice
        else:
            with torch.no_grad():
                self.loss = self._loss_fn(g.outputs, g.t)
                self.dice = loss_and_dice(g.outputs, g.t)[1]
        return self.loss, self.dice

    # ------------------------------------------------------------------ one pass over a loader
    def evaluate(self, loader) -> Tuple[float, float]:
        """validate_one_epoch (training_loop.py:147-180): the means over the loader's batches of the per-batch loss and Dice.
        Batches are (image, mask, ...) sequences; the sums stay on the device (float64) and are read back once."""
        dev = self._check_model()
        tot = torch.zeros(2, dtype=torch.float64, device=dev)
        n = 0
        for batch in loader:
            loss, dice = self(batch[0], batch[1])
            tot += torch.stack((loss.detach().double().reshape(()), dice.detach().double().reshape(())))
            n += 1
        if n == 0:
            raise ValueError("GraphedEval.evaluate: the loader yielded no batch")
        mean = (tot / n).tolist()
        return mean[0], mean[1]

    def describe(self) -> str:
        crit = "" if self._fused_loss else " + eager criterion"
        fold = ", eval BatchNorm folded into the convolution epilogues" if self.fold_bn else ""
        return f"hipGraph(fwd{'+loss+dice' if self._fused_loss else ''}) per input shape{crit}{fold}"
