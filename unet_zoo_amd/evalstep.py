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

``surface=SurfaceMetrics(...)`` adds the boundary distances of the main output map (Hausdorff, HD95, ASSD: surface.py) to the
captured graph, after the loss: ``ev.surface`` is its static ``(out, stats)`` after each call, and ``evaluate`` sums the three
values over the valid (image, pair) occurrences and counts the four states on the device, read back with the two means in the
same single read-back: ``ev.surface_summary``.  Without ``surface`` the graph and every result are unchanged.

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
from .surface import SurfaceMetrics


class _EvalGraph:
    """everything captured for one (input shape, target shape)"""
    __slots__ = ("x", "t", "graph", "outputs", "loss", "dice", "folded", "unfolded", "surface")


class GraphedEval:
    def __init__(self, model: nn.Module, criterion: Union[str, RegionLoss, MulticlassLoss, Callable] = "bce_dice", *, fold_bn: bool = False,
                 surface: Optional[SurfaceMetrics] = None):
        self.model = _unwrap(model)
        if surface is not None and not isinstance(surface, SurfaceMetrics):
            raise TypeError(f"GraphedEval: surface must be a SurfaceMetrics object or None, got {type(surface).__name__}")
        self._surface = surface
        self.surface: Optional[Tuple[torch.Tensor, torch.Tensor]] = None      # the static (out, stats) of the last call
        self.surface_summary: Optional[dict] = None                             # of the last evaluate()
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
            if self._surface is not None:      # its workspace, out and stats of this shape: allocated outside the capture too
                self._surface(warm, t)
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
            g.surface = self._surface(g.outputs, g.t) if self._surface is not None else None
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
        self.surface = g.surface
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
        Batches are (image, mask, ...) sequences; the sums stay on the device (float64) and are read back once.
        With ``surface`` the same read-back carries, per pair column, the sums of hd / hdq / assd over the pairs of state 0
        (float64) and the counts of the four states (int64): ``surface_summary`` holds their means over the valid (image, pair)
        occurrences of the pass (nan for a column with none) and the counts."""
        dev = self._check_model()
        tot = torch.zeros(2, dtype=torch.float64, device=dev)
        ssum = scnt = None
        n = 0
        for batch in loader:
            loss, dice = self(batch[0], batch[1])
            tot += torch.stack((loss.detach().double().reshape(()), dice.detach().double().reshape(())))
            if self.surface is not None:
                out, stats = self.surface
                state = stats[..., 5]                                     # (N, P)
                if ssum is None:
                    ssum = torch.zeros(3, out.shape[1], dtype=torch.float64, device=dev)
                    scnt = torch.zeros(4, out.shape[1], dtype=torch.int64, device=dev)
                elif ssum.shape[1] != out.shape[1]:
                    raise ValueError("GraphedEval.evaluate: the number of surface pairs per image changed during the pass")
                # the values of a pair whose state is not 0 are 0: the plain sum over the images is the sum over the valid ones
                ssum += out[..., :3].double().sum(0).t()
                scnt += torch.stack([(state == s).sum(0) for s in range(4)])
            n += 1
        if n == 0:
            raise ValueError("GraphedEval.evaluate: the loader yielded no batch")
        if ssum is None:
            mean = (tot / n).tolist()
            return mean[0], mean[1]
        P = ssum.shape[1]
        # ONE read-back: the float64 means and sums travel as their bit patterns in front of the int64 counts
        host = torch.cat(((tot / n).view(torch.int64), ssum.reshape(-1).view(torch.int64), scnt.reshape(-1))).cpu()
        mean = host[:2].view(torch.float64).tolist()
        sums = host[2:2 + 3 * P].view(torch.float64).reshape(3, P)
        cnts = host[2 + 3 * P:].reshape(4, P)
        valid = cnts[0].double()
        means = torch.where(valid > 0, sums / valid.clamp(min=1.0), torch.full_like(sums, float("nan")))
        self.surface_summary = {"hd": means[0].tolist(), "hdq": means[1].tolist(), "assd": means[2].tolist(),
                                "n_valid": cnts[0].tolist(), "n_pred_empty": cnts[1].tolist(), "n_target_empty": cnts[2].tolist(),
                                "n_both_empty": cnts[3].tolist(), "percentile": self._surface.percentile}
        return mean[0], mean[1]

    def describe(self) -> str:
        crit = "" if self._fused_loss else " + eager criterion"
        fold = ", eval BatchNorm folded into the convolution epilogues" if self.fold_bn else ""
        surf = "+surface" if self._surface is not None else ""
        return f"hipGraph(fwd{'+loss+dice' if self._fused_loss else ''}{surf}) per input shape{crit}{fold}"
