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

Parameters are read where they live and the graphs are captured again when parameter or buffer storage moves, by
``GraphedEval``'s rule: an optimizer step between two calls -- ``GraphedStep`` included -- is seen by the next call.
``fold_bn=True`` folds eval-mode BatchNorm into the convolution epilogues as in ``GraphedEval``.
"""
from __future__ import annotations

from itertools import chain
from typing import Dict, Optional, Sequence

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .engine import Engine
from .loss import _maps_of
from .postprocess import MaskPostprocess, resolve_mode
from .step import CAPTURE_MODE, _check_capture, _new_graph, _unwrap


class _PredictGraph:
    """everything captured for one input shape"""
    __slots__ = ("x", "views", "graph", "outputs", "prob", "mask", "labels", "class_map", "stats", "comps")


class GraphedPredict:
    def __init__(self, model: nn.Module, *, tta: Sequence[str] = (), postprocess: Optional[MaskPostprocess] = None, fold_bn: bool = False,
                 mode: str = "auto"):
        self.model = _unwrap(model)
        if isinstance(tta, str):
            raise ValueError(f"GraphedPredict: tta must be a sequence of view names, got the string {tta!r}")
        self.views = ops.tta_views(tuple(tta))                   # the bit set; the identity is always in it
        self.n_views = bin(self.views).count("1")
        if postprocess is not None and not isinstance(postprocess, MaskPostprocess):
            raise TypeError(f"GraphedPredict: postprocess must be a MaskPostprocess object or None, got {type(postprocess).__name__}")
        if mode not in ("auto", "binary", "class"):
            raise ValueError(f"GraphedPredict: mode must be 'auto', 'binary' or 'class', got {mode!r}")
        self.postprocess, self.mode, self.fold_bn = postprocess, mode, bool(fold_bn)
        self._check_model()
        self._graphs: Dict[tuple, _PredictGraph] = {}
        self._sig: Optional[tuple] = None
        self.captures = 0             # graphs captured so far (a new shape, or storage that moved, adds one)
        self.mask = self.prob = self.labels = self.class_map = self.stats = self.comps = self.outputs = None

    # ------------------------------------------------------------------ checks (no GPU call)
    def _check_model(self) -> torch.device:
        m = self.model
        if m.training:
            raise RuntimeError("GraphedPredict is INFERENCE: call model.eval() first (GraphedStep is the training step)")
        p = next(m.parameters(), None)
        if p is None or p.device.type != "cuda":
            raise RuntimeError("GraphedPredict needs the model on an MI355X ('cuda'): unet_zoo_amd has no CPU path")
        return p.device

    def _signature(self) -> tuple:
        """what a captured graph holds by address: parameter / buffer storage and the pack cache's pointer tables"""
        m = self.model
        c = m._pack_cache
        tabs = tuple(t.data_ptr() if t is not None else 0 for t in (c._table, c._table3))
        return (m.run_dtype, tabs, tuple(t.data_ptr() for t in chain(m.parameters(), m.buffers())))

    # ------------------------------------------------------------------ the forward, as GraphedEval runs it
    def _forward(self, x: torch.Tensor):
        m = self.model
        with torch.no_grad():
            m._pack_cache.refresh(m.run_dtype)
            eng = Engine(m.run_dtype, x.device, False, False, None, m._pack_cache, False, fold_bn_eval=self.fold_bn)
            outs = tuple(m.emit(eng, x))
            eng.finish_forward()
        return m.wrap_outputs(tuple(o.detach() for o in outs))

    def _pipeline(self, g: _PredictGraph) -> None:
        """flip -> V forwards -> merge -> decision, on the current stream; fills g's result fields"""
        if self.n_views > 1:
            ops.flip_views(g.x, self.views & ~1, g.views[1:])
        outs = [self._forward(v) for v in g.views]
        g.outputs = outs[0]
        mains = []
        for o in outs:
            _, maps, main = _maps_of(o)
            mains.append(maps[main].contiguous())
        shape = tuple(mains[0].shape)
        if len(shape) != 4:
            raise ValueError(f"GraphedPredict: the model's main output map must be (N, C, H, W), got shape {shape}")
        mode = resolve_mode(self.mode, shape[1], "GraphedPredict")
        if g.prob is None:
            g.prob = torch.empty(shape, dtype=torch.float32, device=g.x.device)
        ops.tta_merge(mains, self.views, mode, g.prob)
        single = self.n_views == 1
        src = mains[0].float() if single else g.prob
        pp = self.postprocess
        if pp is not None:
            g.mask = pp(src, mode="binary" if mode == L.POST_BINARY else "class", from_logits=single)
            g.labels, g.class_map, g.stats, g.comps = pp.labels, pp.class_map, pp.stats, pp.comps
        else:
            cls = mode == L.POST_CLASS
            if g.mask is None:
                N, C, H, W = shape
                g.mask = torch.empty((N, C - 1 if cls else C, H, W), dtype=torch.uint8, device=g.x.device)
                g.class_map = torch.empty((N, H, W), dtype=torch.uint8, device=g.x.device) if cls else None
            ops.mask_decide(src, mode, 0.0 if single else 0.5, 1 if cls else 0, g.mask, g.class_map)
            g.labels = g.stats = g.comps = None

    def _capture(self, x: torch.Tensor) -> _PredictGraph:
        m = self.model
        g = _PredictGraph()
        g.x = x
        g.views = [x] + [torch.empty_like(x) for _ in range(self.n_views - 1)]
        g.prob = g.mask = g.class_map = None
        # one eager pass that changes nothing: creates the kernel-layout weight copies, the pack cache's pointer tables and
        # the post-process plan of this shape (allocations and host-to-device copies, which a capture must not contain)
        saved = [b.detach().clone() for b in m.buffers()]
        rng = torch.cuda.get_rng_state(x.device)
        side = torch.cuda.Stream(device=x.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._pipeline(g)
            g.outputs = None
            m._pack_cache.refresh(m.run_dtype)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize(x.device)
        for b, s in zip(m.buffers(), saved):
            b.copy_(s)
        torch.cuda.set_rng_state(rng, x.device)
        torch.cuda.synchronize(x.device)
        g.graph = _new_graph()
        with torch.cuda.graph(g.graph, capture_error_mode=CAPTURE_MODE):
            self._pipeline(g)
        _check_capture(g.graph, "prediction graph")
        self.captures += 1
        return g

    # ------------------------------------------------------------------ one batch
    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """the mask of one batch, (N, P, H, W) uint8: a static device tensor, no host sync"""
        dev = self._check_model()
        L.load()
        sig = self._signature()
        if sig != self._sig:
            self._graphs.clear()
        key = tuple(x.shape)
        g = self._graphs.get(key)
        if g is None:
            if x.dim() != 4:
                raise ValueError(f"GraphedPredict: the input must be (N, C, H, W), got shape {tuple(x.shape)}")
            sx = x.detach().to(device=dev, dtype=torch.float32, copy=True).contiguous()
            g = self._graphs[key] = self._capture(sx)
            self._sig = self._signature()      # (the warm-up pass may have built the pack cache's tables)
        elif x.data_ptr() != g.x.data_ptr():
            g.x.copy_(x)
        g.graph.replay()
        self.mask, self.prob, self.outputs = g.mask, g.prob, g.outputs
        self.labels, self.class_map, self.stats, self.comps = g.labels, g.class_map, g.stats, g.comps
        return g.mask

    def check(self) -> None:
        """the post-process's error words of the last call, read on the host (MaskPostprocess.check)"""
        if self.postprocess is not None and self.stats is not None:
            err = self.stats[..., 6]
            if bool((err != 0).any().item()):
                raise RuntimeError("GraphedPredict: a bounded union-find loop of the post-process ran out; the masks are undefined")

    # ------------------------------------------------------------------ one pass over a loader
    def predict(self, loader):
        """yields a CLONED mask per batch; a batch is an image tensor or an (image, ...) sequence"""
        for batch in loader:
            x = batch if isinstance(batch, torch.Tensor) else batch[0]
            yield self(x).clone()

    def describe(self) -> str:
        names = [n for n, b in L.TTA_VIEWS.items() if self.views & b]
        tail = "postproc" if self.postprocess is not None else "decide"
        fold = ", eval BatchNorm folded into the convolution epilogues" if self.fold_bn else ""
        flip = "flip+" if self.n_views > 1 else ""
        return f"hipGraph({flip}{self.n_views} x fwd+merge+{tail}) per input shape, views {'/'.join(names)}{fold}"
