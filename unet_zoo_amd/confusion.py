"""Confusion counts, overlap scores and threshold-free curves on the device: ``ConfusionMetrics``.

The papers whose recipes this package carries report per-class Dice and mIoU tables, and next to a Dice at the fixed 0.5
threshold (the reference's ``dice_coefficient``, unet_zoo/utils/metrics.py:7-24) users expect the best threshold on the validation
set, a ROC or a PR curve.  All of these are functions of integer counts, and ``ConfusionMetrics`` forms the counts on the device
(``uz_confusion.hip``, DESIGN.md 3v, include/unetzoo_hip.h): exact, independent of order, summable over a whole pass.

    m = unet_zoo_amd.ConfusionMetrics(bins=256)             # background left out, ignore_index=-100; or thresholds=[...]
    counts, hist, out = m(model(images), masks)             # device tensors, STATIC per shape; hist is None for class indices
    m.dice, m.iou, m.precision, m.recall, m.specificity, m.state        # (N, P) views of out
    m.edges, m.thresholds                                   # the float32 logit-space table in use (B - 1,), the probabilities
    ConfusionMetrics.curves(hist_sum, m.thresholds)         # host, float64, from SUMMED histograms (P, 2, B)
    ev = unet_zoo_amd.GraphedEval(model, "bce_dice", confusion=m)       # or inside the evaluation graph

A float target selects the binary mode: prediction ``logits > 0`` (sigmoid > 0.5, what ``loss_and_dice`` thresholds), target
``> 0.5``, every channel its own pair (P = C).  ``counts`` is (N, P, 4) int64 = TP, FP, FN, TN and ``hist`` (N, P, 2, B) int64:
the histogram of the logits of the target's negatives (``[..., 0, :]``) and positives (``[..., 1, :]``) over B bins whose B - 1
edges are a float32 table IN LOGIT SPACE: ``bin(x) = searchsorted(edges, x, side="right")``, a NaN in bin 0.  The kernel
compares floats against the table and evaluates no sigmoid, so the histogram is reproducible exactly.

An integer target holds class indices: prediction ``argmax_K`` (ties: the lowest index); a pixel whose label is
``ignore_index`` or outside ``[0, K)`` is counted nowhere.  ``counts`` is the (N, K, K) int64 confusion matrix per image, label
as row and prediction as column; pairs are the classes 1 .. K-1 (0 .. K-1 with ``include_background=True``).

``out`` is (N, P, 8) float32: dice, iou, precision, recall, specificity, state, 0, 0.  ``state`` is 0 when both masks are
non-empty, 1 when the prediction is empty, 2 when the target is, 3 when both are.  A score with a zero denominator is 0, except
that dice = iou = 1 in state 3 (the reference's ``union == 0 -> 1.0``).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import ops
from .criterion import INT_DTYPES, maps_of


def _power_of_two_bins(B: int) -> bool:
    return L.CONFUSION_MIN_BINS <= B <= L.CONFUSION_MAX_BINS and B & (B - 1) == 0


class ConfusionMetrics:
    """``bins``: B, a power of two in [16, 1024]: the thresholds are the probabilities k / B, k = 1 .. B - 1.  ``thresholds``
    (instead of ``bins``): B - 1 strictly ascending probabilities in (0, 1), B a power of two in [16, 1024].  Either way the
    edges are ``float32(log(p / (1 - p)))``, formed in float64 on the host once, and must be strictly ascending as float32.
    ``include_background``: class 0 is a pair too (class-index targets only).  ``ignore_index``: the label that belongs to no
    class.

    ``m(outputs, target)`` takes any output container of the zoo and measures its MAIN map (first value of a dict, last
    element of a list), fp32 or bf16 logits (bf16 goes through ``.float()`` as in the losses), against a float target of the
    map's shape or integer class indices of shape (N, H, W) or (N, 1, H, W).  One call is one ``uz_confusion_metrics``: three
    launches, no host read, so it can be captured (``GraphedEval(..., confusion=m)``).

    Descriptor, workspace, ``counts``, ``hist``, ``out`` and the edges of a (mode, shape, device) are kept: calls of one object
    must follow each other on one stream or be ordered by the caller, and the results are overwritten by the next call with
    that shape.  The settings are the constructor's; changing an attribute afterwards has no effect on shapes already seen."""

    def __init__(self, bins: Optional[int] = None, thresholds: Optional[Sequence[float]] = None, include_background: bool = False,
                 ignore_index: int = -100):
        if bins is not None and thresholds is not None:
            raise ValueError("ConfusionMetrics: give bins or thresholds, not both")
        if thresholds is None:
            bins = 256 if bins is None else bins
            if isinstance(bins, bool) or not isinstance(bins, int) or not _power_of_two_bins(bins):
                raise ValueError(f"ConfusionMetrics: bins must be a power of two in [{L.CONFUSION_MIN_BINS}, {L.CONFUSION_MAX_BINS}], "
                                 f"got {bins!r}")
            k = np.arange(1, bins, dtype=np.float64)
            edges64 = np.log(k / (bins - k))            # log(p / (1 - p)) of p = k / B without forming p
            probs = k / bins
        else:
            try:
                probs = np.asarray([float(v) for v in thresholds], dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"ConfusionMetrics: thresholds must be a sequence of numbers, got {thresholds!r}") from None
            if probs.ndim != 1 or not _power_of_two_bins(probs.size + 1):
                raise ValueError(f"ConfusionMetrics: thresholds must be B - 1 values with B a power of two in "
                                 f"[{L.CONFUSION_MIN_BINS}, {L.CONFUSION_MAX_BINS}], got {probs.size}")
            if not (np.isfinite(probs).all() and (probs > 0).all() and (probs < 1).all()):
                raise ValueError("ConfusionMetrics: thresholds must be probabilities in (0, 1)")
            if not (np.diff(probs) > 0).all():
                raise ValueError("ConfusionMetrics: thresholds must be strictly ascending")
            edges64 = np.log(probs) - np.log1p(-probs)
            bins = probs.size + 1
        edges = edges64.astype(np.float32)
        if not (np.isfinite(edges).all() and (np.diff(edges) > 0).all()):
            raise ValueError("ConfusionMetrics: thresholds are not strictly ascending once their logits are rounded to float32")
        if isinstance(ignore_index, bool) or not isinstance(ignore_index, int) or not -2 ** 31 <= ignore_index < 2 ** 31:
            raise ValueError(f"ConfusionMetrics: ignore_index must be an int32 value, got {ignore_index!r}")
        self.bins = int(bins)
        self.thresholds = torch.from_numpy(probs.copy())           # float64 (B - 1,), host
        self.edges = torch.from_numpy(edges.copy())                # float32 (B - 1,), host; the device copies live in the plans
        self.ignore_index = ignore_index
        self.include_background = bool(include_background)
        # (mode, logits shape, device index, max_workgroups) -> (descriptor, workspace, edges on the device, counts, hist, out)
        self._plans: Dict[tuple, tuple] = {}
        self.counts: Optional[torch.Tensor] = None
        self.hist: Optional[torch.Tensor] = None
        self.out: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ the plan of a shape
    def describe(self, mode: int, shape, max_workgroups: int = 0) -> "L.ConfusionDesc":
        """the descriptor of a call with logits of this (N, C, H, W) shape"""
        N, C, H, W = (int(s) for s in shape)
        if isinstance(max_workgroups, bool) or not isinstance(max_workgroups, int) or max_workgroups < 0:
            raise ValueError(f"ConfusionMetrics: max_workgroups must be an int >= 0, got {max_workgroups!r}")
        cls = mode == L.CONFUSION_CLASS
        first = 0 if self.include_background else 1
        return L.ConfusionDesc(mode, N, C, H, W, first if cls else 0, self.ignore_index, 0 if cls else self.bins, max_workgroups)

    def _plan(self, mode: int, shape, device: torch.device, max_workgroups: int = 0):
        key = (mode, tuple(shape), device.index, max_workgroups)
        plan = self._plans.get(key)
        if plan is None:
            desc = self.describe(mode, shape, max_workgroups)
            cls = mode == L.CONFUSION_CLASS
            P = desc.C - desc.first_class if cls else desc.C
            ws = torch.empty((L.confusion_workspace_bytes(desc) + 7) // 8, dtype=torch.float64, device=device)
            out = torch.zeros(desc.N, P, 8, dtype=torch.float32, device=device)
            if cls:
                edges = hist = None
                counts = torch.zeros(desc.N, desc.C, desc.C, dtype=torch.int64, device=device)
            else:
                edges = self.edges.to(device)
                counts = torch.zeros(desc.N, desc.C, 4, dtype=torch.int64, device=device)
                hist = torch.zeros(desc.N, desc.C, 2, self.bins, dtype=torch.int64, device=device)
            plan = self._plans[key] = (desc, ws, edges, counts, hist, out)
        return plan

    # ------------------------------------------------------------------ one call
    def __call__(self, outputs, target: torch.Tensor) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
        _, maps, main = maps_of(outputs)
        x = maps[main]
        if not isinstance(x, torch.Tensor) or not isinstance(target, torch.Tensor):
            raise ValueError("ConfusionMetrics: outputs and target must be tensors (or a dict / list of output tensors)")
        shape = tuple(x.shape)
        if len(shape) != 4:
            raise ValueError(f"ConfusionMetrics: logits must be (N, C, H, W), got shape {shape}")
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"ConfusionMetrics: logits must be float32 or bfloat16, got {x.dtype}")
        if x.numel() == 0:
            raise ValueError("ConfusionMetrics: empty maps")
        if shape[2] > L.CONFUSION_MAX_HW or shape[3] > L.CONFUSION_MAX_HW:
            raise ValueError(f"ConfusionMetrics: maps of {shape[2]} x {shape[3]} pixels, at most {L.CONFUSION_MAX_HW} each way")
        if target.dtype in INT_DTYPES:
            mode = L.CONFUSION_CLASS
            K = shape[1]
            if not 2 <= K <= L.CLASS_MAX_K:
                raise ValueError(f"ConfusionMetrics: K = {K} classes outside [2, {L.CLASS_MAX_K}]")
            want = (shape[0],) + shape[2:]
            if tuple(target.shape) not in (want, (shape[0], 1) + shape[2:]):
                raise ValueError(f"ConfusionMetrics: logits of shape {shape} against a target of shape {tuple(target.shape)}; "
                                 f"expected {want} or {(shape[0], 1) + shape[2:]}")
        elif target.dtype in (torch.float32, torch.bfloat16, torch.float16, torch.float64):
            mode = L.CONFUSION_BINARY
            want = shape
            if tuple(target.shape) != shape:
                raise ValueError(f"ConfusionMetrics: an output map of shape {shape} against a target of shape {tuple(target.shape)}")
        else:
            raise ValueError(f"ConfusionMetrics: the target must be float maps or integer class indices, got {target.dtype}")
        L.require_cuda(x, target)
        if x.device != target.device:
            raise ValueError(f"ConfusionMetrics: an output map on {x.device} against a target on {target.device}")
        xs = x.detach().contiguous().float()
        t = target.detach().reshape(want).contiguous().to(torch.int32 if mode == L.CONFUSION_CLASS else torch.float32)
        desc, ws, edges, counts, hist, out = self._plan(mode, shape, xs.device)
        ops.confusion_metrics(desc, xs, t, edges, counts, hist, out, ws)
        self.counts, self.hist, self.out = counts, hist, out
        return counts, hist, out

    # ------------------------------------------------------------------ views of the last call
    def _col(self, k: int) -> torch.Tensor:
        if self.out is None:
            raise RuntimeError("ConfusionMetrics: no call yet")
        return self.out[..., k]

    dice = property(lambda self: self._col(0))
    iou = property(lambda self: self._col(1))
    precision = property(lambda self: self._col(2))
    recall = property(lambda self: self._col(3))
    specificity = property(lambda self: self._col(4))
    state = property(lambda self: self._col(5))

    # ------------------------------------------------------------------ scores and curves on the host
    @staticmethod
    def scores(tp, fp, fn, tn) -> dict:
        """dice, iou, precision, recall, specificity (float64 arrays) of integer counts, by the kernel's rules: a zero
        denominator gives 0, except dice = iou = 1 where prediction and target are both empty"""
        tp, fp, fn, tn = (np.asarray(v, dtype=np.int64) for v in (tp, fp, fn, tn))

        def ratio(num, den):
            return np.where(den > 0, num / np.maximum(den, 1).astype(np.float64), 0.0)
        both_empty = (tp + fp == 0) & (tp + fn == 0)
        return {"dice": np.where(both_empty, 1.0, ratio(2 * tp, 2 * tp + fp + fn)),
                "iou": np.where(both_empty, 1.0, ratio(tp, tp + fp + fn)),
                "precision": ratio(tp, tp + fp), "recall": ratio(tp, tp + fn), "specificity": ratio(tn, tn + fp)}

    @staticmethod
    def curves(hist_sum, thresholds) -> dict:
        """Threshold-free scores of SUMMED histograms (P, 2, B) (or (2, B): one pair), ``[:, 0]`` the negatives and ``[:, 1]``
        the positives, with the B - 1 threshold probabilities.  Plain float64 arithmetic on the host.  With TP_j = sum of
        pos[b >= j], FP_j = sum of neg[b >= j] (j = 0 .. B: predicting positive from bin j on), n_pos and n_neg the totals:
          roc            (P, B + 1, 2): (FPR_j, TPR_j) for j = B .. 0, from (0, 0) to (1, 1); nan where a total is 0
          auroc          sum_b neg[b] (sum_{b' > b} pos[b'] + pos[b] / 2) / (n_pos n_neg): ties inside a bin count half; nan
                         when n_pos or n_neg is 0
          ap             sum_j (R_j - R_{j+1}) Prec_j over j = B - 1 .. 0, the bins as tie groups (R_B = 0; Prec_j = 0 where
                         nothing is predicted); nan when n_pos is 0
          best_dice      max over j = 1 .. B - 1 of 2 TP_j / (2 TP_j + FP_j + FN_j) (0 where the denominator is 0)
          best_threshold thresholds[j - 1] at that j; ties go to the j nearest B / 2, then to the lower j
          reliability    (P, B, 2): (pos[b], pos[b] + neg[b]) per bin
        """
        h = np.asarray(hist_sum)
        single = h.ndim == 2
        if single:
            h = h[None]
        if h.ndim != 3 or h.shape[1] != 2:
            raise ValueError(f"ConfusionMetrics.curves: histograms must be (P, 2, B), got shape {tuple(np.shape(hist_sum))}")
        if not np.issubdtype(h.dtype, np.integer) and not (h == np.floor(h)).all():
            raise ValueError("ConfusionMetrics.curves: histograms must hold integers")
        if (h < 0).any():
            raise ValueError("ConfusionMetrics.curves: histograms must be non-negative")
        h = h.astype(np.int64)
        th = np.asarray(thresholds, dtype=np.float64).reshape(-1)
        B = h.shape[2]
        if th.size != B - 1:
            raise ValueError(f"ConfusionMetrics.curves: {B} bins need {B - 1} thresholds, got {th.size}")
        neg, pos = h[:, 0], h[:, 1]
        P = h.shape[0]
        zero = np.zeros((P, 1), dtype=np.int64)
        # TP[:, j] = sum of pos[b >= j], j = 0 .. B
        TP = np.concatenate((np.cumsum(pos[:, ::-1], axis=1)[:, ::-1], zero), axis=1)
        FP = np.concatenate((np.cumsum(neg[:, ::-1], axis=1)[:, ::-1], zero), axis=1)
        n_pos, n_neg = TP[:, 0], FP[:, 0]
        fpos, fneg = n_pos.astype(np.float64), n_neg.astype(np.float64)
        nan = float("nan")
        with np.errstate(divide="ignore", invalid="ignore"):
            tpr = np.where(n_pos[:, None] > 0, TP / fpos[:, None], nan)
            fpr = np.where(n_neg[:, None] > 0, FP / fneg[:, None], nan)
            roc = np.stack((fpr[:, ::-1], tpr[:, ::-1]), axis=2)
            # integers below 2^53 for any pass that fits a device: twice the pair count, exact
            above = TP[:, 1:]                                       # sum of pos[b' > b]
            pairs2 = (neg.astype(object) * (2 * above.astype(object) + pos.astype(object))).sum(axis=1)
            auroc = np.array([float(p2) / (2.0 * float(int(a) * int(b))) if a > 0 and b > 0 else nan
                              for p2, a, b in zip(pairs2, n_pos, n_neg)], dtype=np.float64)
            prec = np.where(TP + FP > 0, TP / np.maximum(TP + FP, 1).astype(np.float64), 0.0)
            rec = np.where(n_pos[:, None] > 0, TP / np.maximum(fpos[:, None], 1.0), nan)
            ap = ((rec[:, :-1] - rec[:, 1:]) * prec[:, :-1]).sum(axis=1)
            FN = n_pos[:, None] - TP
            den = 2 * TP + FP + FN
            dice = np.where(den > 0, 2 * TP / np.maximum(den, 1).astype(np.float64), 0.0)[:, 1:B]      # j = 1 .. B - 1
        js = np.arange(1, B)
        best_j = np.empty(P, dtype=np.int64)
        for p in range(P):
            cand = js[dice[p] == dice[p].max()]
            best_j[p] = cand[np.lexsort((cand, np.abs(cand - B // 2)))[0]]
        best_dice = dice[np.arange(P), best_j - 1]
        res = {"roc": roc, "auroc": auroc, "ap": ap, "best_dice": best_dice, "best_threshold": th[best_j - 1],
               "reliability": np.stack((pos, pos + neg), axis=2), "n_pos": n_pos, "n_neg": n_neg}
        if single:
            res = {k: v[0] for k, v in res.items()}
        return res

    def __repr__(self) -> str:
        return (f"ConfusionMetrics(bins={self.bins}, include_background={self.include_background}, "
                f"ignore_index={self.ignore_index})")
