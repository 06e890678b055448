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

``confusion=ConfusionMetrics(...)`` adds the confusion counts, score histograms and overlap scores of the main output map
(confusion.py) to the captured graph, after the loss and after ``surface``: ``ev.confusion`` is its static ``(counts, hist, out)``
after each call, and ``evaluate`` sums the counts and histograms over images and batches (int64, on the device; for class indices
that sum is the pass's K x K matrix), the per-image dice and iou over the pairs whose state is not 3, and counts the four states;
all of it travels in the same single read-back: ``ev.confusion_summary``.  Without ``confusion`` nothing changes either.

``fold_bn=True`` runs this object's captures on engines with ``fold_bn_eval`` set: a Conv -> BatchNorm -> ReLU layer without pool or
residual becomes one launch whose epilogue forms the activation from the convolution's fp32 result and the running-statistics
(scale, shift) -- the raw output is neither written nor re-read.  fp32 results are bit-identical to the eager forward; bf16
activations are rounded once instead of twice, so they differ from the eager forward within bf16 rounding.  With
``fold_bn=False`` the replay is bit-identical to the eager forward in both run dtypes.

``ev.loss``, ``ev.dice`` and ``ev.outputs`` are STATIC tensors of the captured graph: the next call with the same input
shape overwrites them in place, so read (``.item()``) or ``.clone()`` what must outlive the call.

Parameters are read where they live: the graph holds their addresses and re-packs the kernel-layout weight copies at its
start (the pack cache's batched launch), so an optimizer step between two calls -- ``GraphedStep`` included -- is seen by the
next replay; when their storage moves the graphs are captured again.  The capture protocol is ``capture.py``'s.

Module buffers are not modified by a replay, except where the reference's own eval forward modifies them: vnet's
normalisation uses batch statistics and updates its running statistics in eval mode too, once per call here as there.
"""
from __future__ import annotations

import math
from typing import Callable, Optional, Tuple, Union

import torch
import torch.nn as nn

from .capture import GraphedRunner, resolve_criterion, static_copy
from .criterion import FusedCriterion
from .loss import loss_and_dice
from .confusion import ConfusionMetrics
from .surface import SurfaceMetrics


class _EvalGraph:
    """everything captured for one (input shape, target shape)"""
    __slots__ = ("x", "t", "graph", "outputs", "loss", "dice", "folded", "unfolded", "surface", "confusion")


class GraphedEval(GraphedRunner):
    PASS = "the EVALUATION pass"

    def __init__(self, model: nn.Module, criterion: Union[str, FusedCriterion, Callable] = "bce_dice", *, fold_bn: bool = False,
                 surface: Optional[SurfaceMetrics] = None, confusion: Optional[ConfusionMetrics] = None):
        super().__init__(model, fold_bn)
        if confusion is not None and not isinstance(confusion, ConfusionMetrics):
            raise TypeError(f"GraphedEval: confusion must be a ConfusionMetrics object or None, got {type(confusion).__name__}")
        self._confusion = confusion
        self.confusion: Optional[tuple] = None                                  # the static (counts, hist, out) of the last call
        self.confusion_summary: Optional[dict] = None                           # of the last evaluate()
        if surface is not None and not isinstance(surface, SurfaceMetrics):
            raise TypeError(f"GraphedEval: surface must be a SurfaceMetrics object or None, got {type(surface).__name__}")
        self._surface = surface
        self.surface: Optional[Tuple[torch.Tensor, torch.Tensor]] = None      # the static (out, stats) of the last call
        self.surface_summary: Optional[dict] = None                             # of the last evaluate()
        # a fused criterion sits inside the graph, where "bce_dice" sits (two launches: no gradient is asked for, so its
        # autograd form alone is used); with several ranks each evaluates its own shard, so reduce="batch" is per shard.  Any
        # other callable is evaluated EAGERLY on the static outputs after the replay, exactly as in GraphedStep
        fused, self._target_dtype = resolve_criterion(criterion)
        self._fused_loss = fused is not None
        self._fused = fused[0] if self._fused_loss else None
        self._per_shape_state = isinstance(criterion, FusedCriterion)
        self._loss_fn = None if self._fused_loss else criterion
        self.loss: Optional[torch.Tensor] = None
        self.dice: Optional[torch.Tensor] = None
        self.outputs = None
        self.folded_layers = 0        # Conv -> BN -> ReLU layers of the last captured forward on the one-launch route
        self.unfolded_layers = 0      # ... and on the two-launch route (fold_bn=True only; both 0 otherwise)

    def _capture(self, x: torch.Tensor, t: torch.Tensor) -> _EvalGraph:
        g = _EvalGraph()
        g.x, g.t = x, t
        g.loss = g.dice = None

        def warm():
            out = self._forward(x)
            if self._per_shape_state:
                with torch.no_grad():      # a FusedCriterion keeps its workspace (counts, class weights) per shape:
                    # allocated here, outside the capture
                    self._fused(out, t)
            if self._surface is not None:      # its workspace, out and stats of this shape: allocated outside the capture too
                self._surface(out, t)
            if self._confusion is not None:    # likewise
                self._confusion(out, t)

        def pipeline():
            g.outputs = self._forward(g.x)
            if self._fused_loss:
                with torch.no_grad():      # no gradient: the criterion's kernels run with dlogits = NULL
                    g.loss, g.dice = self._fused(g.outputs, g.t)
            g.surface = self._surface(g.outputs, g.t) if self._surface is not None else None
            g.confusion = self._confusion(g.outputs, g.t) if self._confusion is not None else None

        g.graph = self._capture_graph(pipeline, "evaluation graph", x.device, warm)
        g.folded, g.unfolded = self._last_counts
        return g

    # ------------------------------------------------------------------ one batch
    def __call__(self, x: torch.Tensor, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(loss, dice) of one batch as 0-dim device tensors; `outputs` holds the model's output container"""
        dev = self._check_model()
        key = (tuple(x.shape), tuple(target.shape))
        g = self._lookup(key)
        if g is None:
            # static input buffers of this shape (training_loop.py:166-167)
            g = self._graphs[key] = self._capture(static_copy(x, dev), static_copy(target, dev, self._target_dtype))
        else:                                  # (a fresh capture's static buffers were created from this very batch)
            if x.data_ptr() != g.x.data_ptr():
                g.x.copy_(x)
            if target.data_ptr() != g.t.data_ptr():
                g.t.copy_(target)
        g.graph.replay()
        self.outputs = g.outputs
        self.surface = g.surface
        self.confusion = g.confusion
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
        occurrences of the pass (nan for a column with none) and the counts.
        With ``confusion`` it carries the int64 sums of ``counts`` and ``hist`` too: ``confusion_summary`` holds, per pair, the micro
        dice / iou / precision / recall / specificity of the summed counts (tp, fp, fn, tn), ``miou`` (their mean iou),
        ``macro_dice`` / ``macro_iou`` (means of the per-image scores over the ``n_scored`` occurrences whose state is not 3) and
        the counts of the four states; for class indices ``matrix``, the K x K confusion matrix of the pass; for float targets
        ``hist`` and ``curves`` = ``ConfusionMetrics.curves`` of the summed histograms."""
        dev = self._check_model()
        tot = torch.zeros(2, dtype=torch.float64, device=dev)
        ssum = scnt = None
        ccnt = chist = cmac = cst = None
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
            if self.confusion is not None:
                counts, hist, out = self.confusion
                state = out[..., 5]                                       # (N, P), 0 .. 3 as floats
                if ccnt is None:
                    ccnt = torch.zeros(counts.shape[1:], dtype=torch.int64, device=dev)
                    chist = torch.zeros(hist.shape[1:], dtype=torch.int64, device=dev) if hist is not None else None
                    cmac = torch.zeros(2, out.shape[1], dtype=torch.float64, device=dev)
                    cst = torch.zeros(4, out.shape[1], dtype=torch.int64, device=dev)
                elif (ccnt.shape != counts.shape[1:] or cmac.shape[1] != out.shape[1] or (chist is None) != (hist is None)
                      or (hist is not None and chist.shape != hist.shape[1:])):
                    raise ValueError("GraphedEval.evaluate: the number of confusion pairs per image or of bins changed during the pass")
                ccnt += counts.sum(0)
                if hist is not None:
                    chist += hist.sum(0)
                scored = (state != 3).double()                            # dice = iou = 1 of an empty pair is a convention, left out
                cmac += torch.stack(((out[..., 0].double() * scored).sum(0), (out[..., 1].double() * scored).sum(0)))
                cst += torch.stack([(state == s).sum(0) for s in range(4)])
            n += 1
        if n == 0:
            raise ValueError("GraphedEval.evaluate: the loader yielded no batch")
        if ssum is None and ccnt is None:
            mean = (tot / n).tolist()
            return mean[0], mean[1]
        # ONE read-back: the float64 means and sums travel as their bit patterns beside the int64 counts
        pieces = [(tot / n).view(torch.int64)]
        if ssum is not None:
            pieces += [ssum.reshape(-1).view(torch.int64), scnt.reshape(-1)]
        if ccnt is not None:
            pieces += [ccnt.reshape(-1), cmac.reshape(-1).view(torch.int64), cst.reshape(-1)]
            if chist is not None:
                pieces.append(chist.reshape(-1))
        host = torch.cat(pieces).cpu()
        at = 0

        def take(shape, dtype=torch.int64):
            nonlocal at
            k = math.prod(shape)
            piece = host[at:at + k]
            at += k
            return (piece.view(dtype) if dtype != torch.int64 else piece).reshape(shape)

        mean = take((2,), torch.float64).tolist()
        if ssum is not None:
            P = ssum.shape[1]
            sums = take((3, P), torch.float64)
            cnts = take((4, P))
            valid = cnts[0].double()
            means = torch.where(valid > 0, sums / valid.clamp(min=1.0), torch.full_like(sums, float("nan")))
            self.surface_summary = {"hd": means[0].tolist(), "hdq": means[1].tolist(), "assd": means[2].tolist(),
                                    "n_valid": cnts[0].tolist(), "n_pred_empty": cnts[1].tolist(), "n_target_empty": cnts[2].tolist(),
                                    "n_both_empty": cnts[3].tolist(), "percentile": self._surface.percentile}
        if ccnt is not None:
            P = cmac.shape[1]
            total = take(tuple(ccnt.shape)).numpy()
            macro = take((2, P), torch.float64).numpy()
            states = take((4, P)).numpy()
            hsum = take(tuple(chist.shape)).numpy() if chist is not None else None
            if hsum is not None:                        # binary: (P, 4) = TP, FP, FN, TN
                tp, fp, fn, tn = (total[:, k] for k in range(4))
            else:                                       # class: the K x K matrix of the pass, the pairs are its last P classes
                first = total.shape[0] - P
                diag = total.diagonal()
                tp, fp, fn = diag[first:], (total.sum(0) - diag)[first:], (total.sum(1) - diag)[first:]
                tn = total.sum() - tp - fp - fn
            summary = {k: v.tolist() for k, v in ConfusionMetrics.scores(tp, fp, fn, tn).items()}
            summary["miou"] = float(sum(summary["iou"]) / P)
            scored = (states[0] + states[1] + states[2]).astype("float64")      # the (image, pair) occurrences of state != 3
            with_nan = [(macro[k] / scored.clip(min=1.0)).tolist() for k in range(2)]
            summary["macro_dice"] = [v if c > 0 else float("nan") for v, c in zip(with_nan[0], scored)]
            summary["macro_iou"] = [v if c > 0 else float("nan") for v, c in zip(with_nan[1], scored)]
            summary.update({"n_scored": scored.astype("int64").tolist(), "n_valid": states[0].tolist(), "n_pred_empty": states[1].tolist(),
                            "n_target_empty": states[2].tolist(), "n_both_empty": states[3].tolist(),
                            "tp": tp.tolist(), "fp": fp.tolist(), "fn": fn.tolist(), "tn": tn.tolist()})
            if hsum is not None:
                summary["hist"] = hsum
                summary["curves"] = ConfusionMetrics.curves(hsum, self._confusion.thresholds)
            else:
                summary["matrix"] = total
            self.confusion_summary = summary
        return mean[0], mean[1]

    def describe(self) -> str:
        crit = "" if self._fused_loss else " + eager criterion"
        fold = ", eval BatchNorm folded into the convolution epilogues" if self.fold_bn else ""
        surf = ("+surface" if self._surface is not None else "") + ("+confusion" if self._confusion is not None else "")
        return f"hipGraph(fwd{'+loss+dice' if self._fused_loss else ''}{surf}) per input shape{crit}{fold}"
