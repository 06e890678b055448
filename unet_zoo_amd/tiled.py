"""Sliding-window inference as hipGraph replays: ``SlidingWindowPredict``.

``GraphedPredict`` feeds the model the image as it arrives.  Three graphs of the zoo are built for one ``image_size``
(swin_unet_v2, uctransnet, unext / unext_s) and raise on any other, and the convolutional ones are tuned at the sizes they
were trained at.  Sliding-window inference (MONAI's ``sliding_window_inference``, nnU-Net's predictor) closes both gaps: the
image is cut into overlapping windows of the training size, the windows run through the model in batches, and their
probabilities are blended with a window weight and normalised by the summed weight:

    pred = unet_zoo_amd.SlidingWindowPredict(model.eval(), window=(256, 256), overlap=0.5, blend="gaussian", tile_batch=16,
                                             tta=("hflip",), postprocess=unet_zoo_amd.MaskPostprocess(min_area=16))
    mask = pred(images)                     # (N, P, H, W) uint8 for ANY H, W; STATIC: the next call with this shape overwrites it
    pred.prob                               # (N, C, H, W) fp32, blended
    pred.plan                               # the tile starts ys / xs, tiles per image, tiles and forwards per call
    for mask in pred.predict(loader): ...   # a cloned mask per batch

One graph per input shape, in this order: for each batch of at most ``tile_batch`` tiles ``uz_tile_gather`` (the windows as one
contiguous batch; an image smaller than the window is centred on it and padded by ``pad_mode``), ``uz_flip_views`` when ``tta``
names views, the V forwards, and ``uz_tta_merge`` straight into that batch's slice of one static (T, C, th, tw) buffer of tile
probabilities; then one ``uz_tile_blend``; then ``uz_postproc`` (``postprocess=``) or the plain ``> 0.5`` / argmax
(``uz_mask_decide``) on the blended ``prob``.  Tiles of different images share a batch.

Probabilities are blended, not logits: they are bounded, so one tile's large logit cannot outvote its neighbours, and the
result means the same with and without TTA.  The tile starts are MONAI's (``ops.tile_plan``: step
``max(int(window (1 - overlap)), 1)``, the last tile shifted back); the window weight is ``ops.tile_weights`` along each axis,
their product floored at 1e-3.  The sum over the tiles of a pixel has a fixed order, so a call is bit-reproducible.

CAVEAT: a model whose eval forward depends on the batch (vnet normalises with batch statistics) gives tile results that depend
on ``tile_batch`` and on which tiles share a batch; its running statistics advance once per forward, i.e.
``forwards per call`` times per call.

The graphs are captured by the protocol of ``capture.py``, as ``GraphedPredict``'s are: an optimizer step between two calls is
seen by the next call.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .capture import static_copy
from .criterion import maps_of
from .postprocess import MaskPostprocess, resolve_mode
from .predict import Predictor

_BLENDS = ("constant", "gaussian")


class _TiledGraph:
    """everything captured for one input shape"""
    __slots__ = ("x", "plan", "gh", "gw", "views", "tiles", "graph", "prob", "mask", "labels", "class_map", "stats", "comps")


class SlidingWindowPredict(Predictor):
    def __init__(self, model: nn.Module, *, window, overlap: float = 0.5, blend: str = "gaussian", sigma_scale: float = 0.125,
                 pad_mode: str = "constant", tile_batch: int = 16, tta: Sequence[str] = (), postprocess: Optional[MaskPostprocess] = None,
                 fold_bn: bool = False, mode: str = "auto"):
        super().__init__(model, tta, postprocess, fold_bn, mode)
        self._check_model(on_gpu=False)
        if (isinstance(window, (str, bytes)) or not hasattr(window, "__len__") or len(window) != 2
                or any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in window)):
            raise ValueError(f"SlidingWindowPredict: window must be two positive ints (height, width), got {window!r}")
        self.window = (int(window[0]), int(window[1]))
        if isinstance(overlap, bool) or not isinstance(overlap, (int, float)) or not 0.0 <= overlap <= 0.75:
            raise ValueError(f"SlidingWindowPredict: overlap must lie in [0, 0.75], got {overlap!r}")
        self.overlap = float(overlap)
        if blend not in _BLENDS:
            raise ValueError(f"SlidingWindowPredict: unknown blend {blend!r}; the window weights are {list(_BLENDS)}")
        if isinstance(sigma_scale, bool) or not isinstance(sigma_scale, (int, float)) or not sigma_scale > 0:
            raise ValueError(f"SlidingWindowPredict: sigma_scale must be positive, got {sigma_scale!r}")
        self.blend, self.sigma_scale = blend, float(sigma_scale)
        if pad_mode not in L.TILE_PADS:
            raise ValueError(f"SlidingWindowPredict: unknown pad_mode {pad_mode!r}; the paddings are {sorted(L.TILE_PADS)}")
        self.pad_mode = pad_mode
        if isinstance(tile_batch, bool) or not isinstance(tile_batch, int) or tile_batch < 1:
            raise ValueError(f"SlidingWindowPredict: tile_batch must be an int >= 1, got {tile_batch!r}")
        self.tile_batch = tile_batch
        self.plan: Optional[dict] = None

    # ------------------------------------------------------------------ the plan (no GPU call)
    def plan_for(self, shape, channels: int = 1) -> dict:
        """the tiling of an (N, C, H, W) input whose probability map has `channels` channels: host arithmetic alone
        (``uz_tile_plan``); raises on what no call with this shape could run"""
        if len(shape) != 4 or any(int(s) < 1 for s in shape):
            raise ValueError(f"SlidingWindowPredict: the input must be a non-empty (N, C, H, W), got shape {tuple(shape)}")
        N, _, H, W = (int(s) for s in shape)
        th, tw = self.window
        if self.pad_mode == "reflect":
            for size, win, axis in ((H, th, "height"), (W, tw, "width")):
                pad = max(win - size, 0)
                if pad - pad // 2 >= size:
                    raise ValueError(f"SlidingWindowPredict: reflect padding needs pad < size, but the {axis} {size} is padded "
                                     f"by {pad - pad // 2} to the window's {win}; use pad_mode='constant'")
        ys, xs = ops.tile_plan(H, th, self.overlap), ops.tile_plan(W, tw, self.overlap)
        per_image = len(ys) * len(xs)
        tiles = N * per_image
        if tiles * int(channels) * th * tw >= 2 ** 31:
            raise ValueError(f"SlidingWindowPredict: {tiles} tiles of {channels} x {th} x {tw} probabilities are 2^31 elements or "
                             f"more; predict fewer images per call")
        batches = [(t0, min(self.tile_batch, tiles - t0)) for t0 in range(0, tiles, self.tile_batch)]
        return {"ys": ys, "xs": xs, "tiles_per_image": per_image, "tiles": tiles, "batches": batches,
                "forwards": len(batches) * self.n_views}

    # ------------------------------------------------------------------ the captured work
    def _pipeline(self, g: _TiledGraph) -> None:
        """per tile batch gather -> flip -> V forwards -> merge, then blend -> decision, on the current stream"""
        plan = g.plan
        ys, xs = plan["ys"], plan["xs"]
        mode = None
        for t0, tn in plan["batches"]:
            views = [v[:tn] for v in g.views]                    # (the last batch may be smaller: a contiguous slice)
            ops.tile_gather(g.x, ys, xs, self.window, self.pad_mode, t0, views[0])
            if self.n_views > 1:
                ops.flip_views(views[0], self.views & ~1, views[1:])
            mains = []
            for v in views:
                _, maps, main = maps_of(self._forward(v))
                mains.append(maps[main].contiguous())
            shape = tuple(mains[0].shape)
            if len(shape) != 4 or shape[0] != tn or shape[2:] != self.window:
                raise ValueError(f"SlidingWindowPredict: the model's main output map of {tn} windows must be "
                                 f"({tn}, C, {self.window[0]}, {self.window[1]}), got shape {shape}")
            mode = resolve_mode(self.mode, shape[1], "SlidingWindowPredict")
            if g.tiles is None:
                self.plan_for(g.x.shape, shape[1])               # the 2^31 check with the true channel count
                g.tiles = torch.empty((plan["tiles"], shape[1]) + self.window, dtype=torch.float32, device=g.x.device)
                g.prob = torch.empty((g.x.shape[0], shape[1]) + tuple(g.x.shape[2:]), dtype=torch.float32, device=g.x.device)
            ops.tta_merge(mains, self.views, mode, g.tiles[t0:t0 + tn])
        ops.tile_blend(g.tiles, ys, xs, g.gh, g.gw, g.prob)
        self._decide(g, g.prob, mode, 0.5, False)

    def _capture(self, x: torch.Tensor, plan: dict) -> _TiledGraph:
        g = _TiledGraph()
        g.x, g.plan = x, plan
        th, tw = self.window
        g.gh = ops.tile_weights(th, self.blend, self.sigma_scale).to(x.device)
        g.gw = ops.tile_weights(tw, self.blend, self.sigma_scale).to(x.device)
        tb = min(self.tile_batch, plan["tiles"])
        g.views = [torch.empty((tb, x.shape[1], th, tw), dtype=torch.float32, device=x.device) for _ in range(self.n_views)]
        g.tiles = g.prob = g.mask = g.class_map = None
        # (the eager pass in front of the capture creates the static buffers and the post-process plan of this shape too)
        g.graph = self._capture_graph(lambda: self._pipeline(g), "sliding-window prediction graph", x.device)
        return g

    # ------------------------------------------------------------------ one batch
    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """the mask of one batch, (N, P, H, W) uint8: a static device tensor, no host sync"""
        key = tuple(x.shape)
        g = self._graphs.get(key)
        plan = g.plan if g is not None else self.plan_for(key)   # (raises before any GPU call)
        dev = self._check_model()
        g = self._lookup(key)
        if g is None:
            g = self._graphs[key] = self._capture(static_copy(x, dev).contiguous(), plan)
            x = g.x                            # (created from this very batch: nothing to copy)
        self.plan = g.plan
        return self._replay(g, x)

    def describe(self) -> str:
        fwd, tail, views = self._describe()
        return (f"hipGraph(tile batches of {self.tile_batch} x (gather+{fwd}) + blend+{tail}) per input shape, "
                f"window {self.window[0]} x {self.window[1]}, overlap {self.overlap:g}, {self.blend} weights, {self.pad_mode} padding, "
                f"{views}")
