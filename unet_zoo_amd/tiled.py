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

The graphs are captured by ``GraphedPredict``'s rules: an eager warm-up pass on a side stream that restores buffers and the
RNG state, no memset node in the capture, and a new capture when parameter or buffer storage or the pack cache's tables move
(the pack cache's pointer tables are rebuilt first) -- an optimizer step between two calls is seen by the next call.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .loss import _maps_of
from .postprocess import MaskPostprocess, resolve_mode
from .predict import GraphedPredict
from .step import CAPTURE_MODE, _check_capture, _new_graph, _unwrap

_BLENDS = ("constant", "gaussian")


class _TiledGraph:
    """everything captured for one input shape"""
    __slots__ = ("x", "plan", "gh", "gw", "views", "tiles", "graph", "prob", "mask", "labels", "class_map", "stats", "comps")


class SlidingWindowPredict:
    def __init__(self, model: nn.Module, *, window, overlap: float = 0.5, blend: str = "gaussian", sigma_scale: float = 0.125,
                 pad_mode: str = "constant", tile_batch: int = 16, tta: Sequence[str] = (), postprocess: Optional[MaskPostprocess] = None,
                 fold_bn: bool = False, mode: str = "auto"):
        self.model = _unwrap(model)
        if self.model.training:
            raise RuntimeError("SlidingWindowPredict is INFERENCE: call model.eval() first (GraphedStep is the training step)")
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
        if isinstance(tta, str):
            raise ValueError(f"SlidingWindowPredict: tta must be a sequence of view names, got the string {tta!r}")
        self.views = ops.tta_views(tuple(tta))                   # the bit set; the identity is always in it
        self.n_views = bin(self.views).count("1")
        if postprocess is not None and not isinstance(postprocess, MaskPostprocess):
            raise TypeError(f"SlidingWindowPredict: postprocess must be a MaskPostprocess object or None, got {type(postprocess).__name__}")
        if mode not in ("auto", "binary", "class"):
            raise ValueError(f"SlidingWindowPredict: mode must be 'auto', 'binary' or 'class', got {mode!r}")
        self.postprocess, self.mode, self.fold_bn = postprocess, mode, bool(fold_bn)
        self._graphs: Dict[tuple, _TiledGraph] = {}
        self._sig: Optional[tuple] = None
        self.captures = 0             # graphs captured so far (a new shape, or storage that moved, adds one)
        self.plan: Optional[dict] = None
        self.mask = self.prob = self.labels = self.class_map = self.stats = self.comps = None

    # the model's forward as the prediction graph runs it, and what a captured graph holds by address (predict.py)
    _forward = GraphedPredict._forward
    _signature = GraphedPredict._signature

    # ------------------------------------------------------------------ checks and the plan (no GPU call)
    def _check_model(self) -> torch.device:
        m = self.model
        if m.training:
            raise RuntimeError("SlidingWindowPredict is INFERENCE: call model.eval() first (GraphedStep is the training step)")
        p = next(m.parameters(), None)
        if p is None or p.device.type != "cuda":
            raise RuntimeError("SlidingWindowPredict needs the model on an MI355X ('cuda'): unet_zoo_amd has no CPU path")
        return p.device

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
                _, maps, main = _maps_of(self._forward(v))
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
        pp = self.postprocess
        if pp is not None:
            g.mask = pp(g.prob, mode="binary" if mode == L.POST_BINARY else "class", from_logits=False)
            g.labels, g.class_map, g.stats, g.comps = pp.labels, pp.class_map, pp.stats, pp.comps
        else:
            cls = mode == L.POST_CLASS
            if g.mask is None:
                N, C, H, W = g.prob.shape
                g.mask = torch.empty((N, C - 1 if cls else C, H, W), dtype=torch.uint8, device=g.x.device)
                g.class_map = torch.empty((N, H, W), dtype=torch.uint8, device=g.x.device) if cls else None
            ops.mask_decide(g.prob, mode, 0.5, 1 if cls else 0, g.mask, g.class_map)
            g.labels = g.stats = g.comps = None

    def _capture(self, x: torch.Tensor, plan: dict) -> _TiledGraph:
        m = self.model
        g = _TiledGraph()
        g.x, g.plan = x, plan
        th, tw = self.window
        g.gh = ops.tile_weights(th, self.blend, self.sigma_scale).to(x.device)
        g.gw = ops.tile_weights(tw, self.blend, self.sigma_scale).to(x.device)
        tb = min(self.tile_batch, plan["tiles"])
        g.views = [torch.empty((tb, x.shape[1], th, tw), dtype=torch.float32, device=x.device) for _ in range(self.n_views)]
        g.tiles = g.prob = g.mask = g.class_map = None
        # one eager pass that changes nothing: creates the kernel-layout weight copies, the pack cache's pointer tables, the
        # static buffers and the post-process plan of this shape (allocations and host-to-device copies, which a capture must
        # not contain)
        saved = [b.detach().clone() for b in m.buffers()]
        rng = torch.cuda.get_rng_state(x.device)
        side = torch.cuda.Stream(device=x.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._pipeline(g)
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
        _check_capture(g.graph, "sliding-window prediction graph")
        self.captures += 1
        return g

    # ------------------------------------------------------------------ one batch
    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """the mask of one batch, (N, P, H, W) uint8: a static device tensor, no host sync"""
        key = tuple(x.shape)
        g = self._graphs.get(key)
        plan = g.plan if g is not None else self.plan_for(key)   # (raises before any GPU call)
        dev = self._check_model()
        L.load()
        sig = self._signature()
        if sig != self._sig:
            if self._sig is not None:
                self.model._pack_cache.repoint()     # storage moved: the pack cache's tables still name the old addresses
            self._graphs.clear()
            g = None
        if g is None:
            sx = x.detach().to(device=dev, dtype=torch.float32, copy=True).contiguous()
            g = self._graphs[key] = self._capture(sx, plan)
            self._sig = self._signature()      # (the warm-up pass may have built the pack cache's tables)
        elif x.data_ptr() != g.x.data_ptr():
            g.x.copy_(x)
        g.graph.replay()
        self.mask, self.prob, self.plan = g.mask, g.prob, g.plan
        self.labels, self.class_map, self.stats, self.comps = g.labels, g.class_map, g.stats, g.comps
        return g.mask

    def check(self) -> None:
        """the post-process's error words of the last call, read on the host (MaskPostprocess.check)"""
        if self.postprocess is not None and self.stats is not None:
            err = self.stats[..., 6]
            if bool((err != 0).any().item()):
                raise RuntimeError("SlidingWindowPredict: a bounded union-find loop of the post-process ran out; the masks are undefined")

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
        return (f"hipGraph(tile batches of {self.tile_batch} x (gather+{flip}{self.n_views} x fwd+merge) + blend+{tail}) per input shape, "
                f"window {self.window[0]} x {self.window[1]}, overlap {self.overlap:g}, {self.blend} weights, {self.pad_mode} padding, "
                f"views {'/'.join(names)}{fold}")
