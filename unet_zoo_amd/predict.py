"""Inference as hipGraph replays: ``GraphedPredict``.

The reference's own inference path is ``sigmoid(logits) > 0.5`` on the host (unet_zoo/utils/visualize.py:174); what the
segmentation recipes add before they report a number -- averaging flipped views, keeping the largest component(s), dropping
specks, filling holes -- is host work per image and class.  ``GraphedPredict`` is all of it captured once per input shape:

    pp = unet_zoo_amd.MaskPostprocess(fill_holes=True, keep_largest=1)
    pred = unet_zoo_amd.GraphedPredict(model.eval(), tta=("hflip", "vflip"), postprocess=pp)
    mask = pred(images)                     # (N, P, H, W) uint8, STATIC: the next call with this shape overwrites it
    pred.prob, pred.labels, pred.class_map, pred.stats, pred.comps, pred.outputs
    for mask in pred.predict(loader): ...   # a cloned mask per batch

One graph per input shape, in this order: ``uz_flip_views`` (the flipped copies of the batch, one launch), the V forwards one
after another with batch N each, ``uz_tta_merge`` (``prob`` = the mean over the views of sigmoid or softmax, each view read
through its inverse flip), then ``uz_postproc`` (``postprocess=``) or the plain threshold / argmax (``uz_mask_decide``).  The
identity is always a view; ``tta`` names the others: "hflip" (along W), "vflip" (along H), "hvflip".

The V forwards are NOT stacked along the batch: vnet's eval forward normalises with batch statistics, so a stacked batch would
change its results (and its running statistics, which advance V times per call here, as V eager calls would advance them).

With more than one view the decision is taken on ``prob`` (``> 0.5``, or the argmax over classes).  With the identity alone it
is taken on the logits themselves (``> 0`` / argmax), which is the same decision without the rounding of a sigmoid that is
0.5 in fp32 for a tiny positive logit: the mask then equals ``GraphedEval``'s ``outputs > 0`` exactly.

Parameters are read where they live and the graphs are captured again when their storage moves (``capture.py`` holds the
protocol): an optimizer step between two calls -- ``GraphedStep`` included -- is seen by the next call.
``fold_bn=True`` folds eval-mode BatchNorm into the convolution epilogues as in ``GraphedEval``.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .capture import GraphedRunner, static_copy
from .criterion import maps_of
from .postprocess import MaskPostprocess, resolve_mode


class Predictor(GraphedRunner):
    """what GraphedPredict and SlidingWindowPredict (tiled.py) share: the views, the decision on a probability or logit map,
    the results a call publishes, check() and predict()"""

    def __init__(self, model: nn.Module, tta: Sequence[str], postprocess: Optional[MaskPostprocess], fold_bn: bool, mode: str):
        super().__init__(model, fold_bn)
        name = type(self).__name__
        if isinstance(tta, str):
            raise ValueError(f"{name}: tta must be a sequence of view names, got the string {tta!r}")
        self.views = ops.tta_views(tuple(tta))                   # the bit set; the identity is always in it
        self.n_views = bin(self.views).count("1")
        if postprocess is not None and not isinstance(postprocess, MaskPostprocess):
            raise TypeError(f"{name}: postprocess must be a MaskPostprocess object or None, got {type(postprocess).__name__}")
        if mode not in ("auto", "binary", "class"):
            raise ValueError(f"{name}: mode must be 'auto', 'binary' or 'class', got {mode!r}")
        self.postprocess, self.mode = postprocess, mode
        self.mask = self.prob = self.labels = self.class_map = self.stats = self.comps = None

    def _decide(self, g, src: torch.Tensor, mode: int, threshold: float, from_logits: bool) -> None:
        """uz_postproc, or the plain threshold / argmax, on `src`: fills g.mask, labels, class_map, stats and comps"""
        pp = self.postprocess
        if pp is not None:
            g.mask = pp(src, mode="binary" if mode == L.POST_BINARY else "class", from_logits=from_logits)
            g.labels, g.class_map, g.stats, g.comps = pp.labels, pp.class_map, pp.stats, pp.comps
        else:
            cls = mode == L.POST_CLASS
            if g.mask is None:
                N, C, H, W = src.shape
                g.mask = torch.empty((N, C - 1 if cls else C, H, W), dtype=torch.uint8, device=src.device)
                g.class_map = torch.empty((N, H, W), dtype=torch.uint8, device=src.device) if cls else None
            ops.mask_decide(src, mode, threshold, 1 if cls else 0, g.mask, g.class_map)
            g.labels = g.stats = g.comps = None

    def _replay(self, g, x: torch.Tensor) -> torch.Tensor:
        """`x` into g's static input (unless it IS that tensor), one replay, and g's results published"""
        if x.data_ptr() != g.x.data_ptr():
            g.x.copy_(x)
        g.graph.replay()
        self.mask, self.prob = g.mask, g.prob
        self.labels, self.class_map, self.stats, self.comps = g.labels, g.class_map, g.stats, g.comps
        return g.mask

    def check(self) -> None:
        """the post-process's error words of the last call, read on the host (MaskPostprocess.check)"""
        if self.postprocess is not None and self.stats is not None:
            err = self.stats[..., 6]
            if bool((err != 0).any().item()):
                raise RuntimeError(f"{type(self).__name__}: a bounded union-find loop of the post-process ran out; the masks are undefined")

    # ------------------------------------------------------------------ one pass over a loader
    def predict(self, loader):
        """yields a CLONED mask per batch; a batch is an image tensor or an (image, ...) sequence"""
        for batch in loader:
            x = batch if isinstance(batch, torch.Tensor) else batch[0]
            yield self(x).clone()

    def _describe(self) -> Tuple[str, str, str]:
        """what the describe() strings share: the forwards of one batch, the decision, the views"""
        names = [n for n, b in L.TTA_VIEWS.items() if self.views & b]
        fold = ", eval BatchNorm folded into the convolution epilogues" if self.fold_bn else ""
        flip = "flip+" if self.n_views > 1 else ""
        return (f"{flip}{self.n_views} x fwd+merge", "postproc" if self.postprocess is not None else "decide",
                f"views {'/'.join(names)}{fold}")


class _PredictGraph:
    """everything captured for one input shape"""
    __slots__ = ("x", "views", "graph", "outputs", "prob", "mask", "labels", "class_map", "stats", "comps")


class GraphedPredict(Predictor):
    def __init__(self, model: nn.Module, *, tta: Sequence[str] = (), postprocess: Optional[MaskPostprocess] = None, fold_bn: bool = False,
                 mode: str = "auto"):
        super().__init__(model, tta, postprocess, fold_bn, mode)
        self._check_model()
        self.outputs = None

    def _pipeline(self, g: _PredictGraph) -> None:
        """flip -> V forwards -> merge -> decision, on the current stream; fills g's result fields"""
        if self.n_views > 1:
            ops.flip_views(g.x, self.views & ~1, g.views[1:])
        outs = [self._forward(v) for v in g.views]
        g.outputs = outs[0]
        mains = []
        for o in outs:
            _, maps, main = maps_of(o)
            mains.append(maps[main].contiguous())
        shape = tuple(mains[0].shape)
        if len(shape) != 4:
            raise ValueError(f"GraphedPredict: the model's main output map must be (N, C, H, W), got shape {shape}")
        mode = resolve_mode(self.mode, shape[1], "GraphedPredict")
        if g.prob is None:
            g.prob = torch.empty(shape, dtype=torch.float32, device=g.x.device)
        ops.tta_merge(mains, self.views, mode, g.prob)
        single = self.n_views == 1
        self._decide(g, mains[0].float() if single else g.prob, mode, 0.0 if single else 0.5, single)

    def _capture(self, x: torch.Tensor) -> _PredictGraph:
        g = _PredictGraph()
        g.x = x
        g.views = [x] + [torch.empty_like(x) for _ in range(self.n_views - 1)]
        g.prob = g.mask = g.class_map = None

        def warm():      # creates the post-process plan of this shape too, outside the capture
            self._pipeline(g)
            g.outputs = None

        g.graph = self._capture_graph(lambda: self._pipeline(g), "prediction graph", x.device, warm)
        return g

    # ------------------------------------------------------------------ one batch
    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """the mask of one batch, (N, P, H, W) uint8: a static device tensor, no host sync"""
        dev = self._check_model()
        key = tuple(x.shape)
        g = self._lookup(key)
        if g is None:
            if x.dim() != 4:
                raise ValueError(f"GraphedPredict: the input must be (N, C, H, W), got shape {tuple(x.shape)}")
            g = self._graphs[key] = self._capture(static_copy(x, dev).contiguous())
            x = g.x                            # (created from this very batch: nothing to copy)
        mask = self._replay(g, x)
        self.outputs = g.outputs
        return mask

    def describe(self) -> str:
        fwd, tail, views = self._describe()
        return f"hipGraph({fwd}+{tail}) per input shape, {views}"
