"""The segmentation itself, cleaned on the device: ``MaskPostprocess``.

What every recipe carried here does to a thresholded map before it reports a number -- fill holes, keep the largest connected
component(s), drop specks -- is ``scipy.ndimage.label`` / ``binary_fill_holes`` / ``numpy.bincount`` per image and class on
the host.  ``MaskPostprocess`` does it in ``uz_postproc.hip`` (lock-free union-find, integer atomics only), with the very
integers scipy gives (include/unetzoo_hip.h):

    pp = unet_zoo_amd.MaskPostprocess(connectivity=1, fill_holes=True, min_area=20, keep_largest=1)
    mask = pp(model(images))                # (N, P, H, W) uint8 on the device, STATIC per shape
    pp.labels, pp.class_map, pp.stats, pp.comps
    pp.check()                              # reads the error words: raises if a bounded loop ran out

Per plane, in this order: (1) ``fill_holes``: scipy's ``binary_fill_holes`` with its default structure (the cross, whatever
``connectivity`` is); (2) components with ``connectivity`` 1 (cross) or 2 (3 x 3 square); (3) components with area <
``min_area`` are dropped; (4) ``keep_largest = k > 0`` keeps the k largest, ties to the component whose first pixel in raster
order comes first.  ``labels`` numbers the survivors 1 .. n in raster order: ``scipy.ndimage.label(mask, structure)[0]``.

``mode="binary"``: every channel is a plane of its own, ``x > 0`` for logits (``from_logits=True``) or ``x > 0.5`` for
probabilities: P = C.  ``mode="class"``: plane c is ``argmax_K == c`` (ties: the lowest index) for the classes 1 .. K-1
(0 .. K-1 with ``include_background=True``).  ``mode="auto"`` is binary for C == 1 and class for C >= 2.

``stats`` is (N, P, 8) int64: components after step 1, components kept, area after step 1, area kept, pixels added by step
1, the largest area among the components of at least ``min_area``, the error word, 0.  ``comps`` is (N, P, 8, 8) int64: the
eight largest kept components in the order of step 4, each area, i_min, j_min, i_max, j_max, sum of i, sum of j, root (the
first pixel, i W + j); unused records are zero -- boxes and centroids without touching the label plane.  ``class_map``
(N, H, W) uint8, class mode: the argmax class where its plane kept the pixel, else the lowest class whose final plane holds
it (a filled hole), else 0.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib as L
from . import ops
from .criterion import maps_of

_MODES = {"binary": L.POST_BINARY, "class": L.POST_CLASS}


def _int(name: str, v, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"MaskPostprocess: {name} must be an int in [{lo}, {hi}], got {v!r}")
    return v


def resolve_mode(mode: str, channels: int, who: str) -> int:
    if mode == "auto":
        return L.POST_BINARY if channels == 1 else L.POST_CLASS
    if mode not in _MODES:
        raise ValueError(f"{who}: mode must be 'auto', 'binary' or 'class', got {mode!r}")
    if mode == "class" and not 2 <= channels <= L.CLASS_MAX_K:
        raise ValueError(f"{who}: K = {channels} classes outside [2, {L.CLASS_MAX_K}]")
    return _MODES[mode]


class MaskPostprocess:
    """``pp(outputs_or_prob, mode="auto", from_logits=True)`` takes any output container of the zoo and works on its MAIN map
    (first value of a dict, last element of a list), fp32 or bf16 (bf16 goes through ``.float()``).  One call is one
    ``uz_postproc``: a number of launches fixed by the settings, no allocation, no host read, so it can be captured
    (``GraphedPredict(..., postprocess=pp)``).  ``labels=False`` leaves the label plane out.

    Descriptor, workspace and results of a (mode, threshold, shape, device) are kept: calls of one object must follow each
    other on one stream or be ordered by the caller, and the results are overwritten by the next call with that shape."""

    def __init__(self, connectivity: int = 1, fill_holes: bool = False, min_area: int = 0, keep_largest: int = 0,
                 include_background: bool = False, labels: bool = True):
        self.connectivity = _int("connectivity", connectivity, 1, 2)
        self.min_area = _int("min_area", min_area, 0, 2 ** 31 - 1)
        self.keep_largest = _int("keep_largest", keep_largest, 0, L.POST_MAX_KEEP)
        for name, v in (("fill_holes", fill_holes), ("include_background", include_background), ("labels", labels)):
            if not isinstance(v, bool):
                raise ValueError(f"MaskPostprocess: {name} must be a bool, got {v!r}")
        self.fill_holes, self.include_background, self.want_labels = fill_holes, include_background, labels
        self._plans: Dict[tuple, tuple] = {}
        self.mask: Optional[torch.Tensor] = None
        self.labels: Optional[torch.Tensor] = None
        self.class_map: Optional[torch.Tensor] = None
        self.stats: Optional[torch.Tensor] = None
        self.comps: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ the plan of a shape
    def describe(self, mode: int, shape, thr: float = 0.0) -> "L.PostprocDesc":
        """the descriptor of a call on a map of this (N, C, H, W) shape"""
        N, C, H, W = (int(s) for s in shape)
        first = (0 if self.include_background else 1) if mode == L.POST_CLASS else 0
        return L.PostprocDesc(mode, N, C, H, W, first, self.connectivity, int(self.fill_holes), self.min_area, self.keep_largest,
                              thr, 0)

    def _plan(self, mode: int, thr: float, shape, device: torch.device):
        key = (mode, thr, tuple(shape), device.index)
        plan = self._plans.get(key)
        if plan is None:
            desc = self.describe(mode, shape, thr)
            cls = mode == L.POST_CLASS
            P = desc.C - desc.first_class if cls else desc.C
            ws = torch.empty((L.postproc_workspace_bytes(desc) + 7) // 8, dtype=torch.float64, device=device)
            mask = torch.zeros(desc.N, P, desc.H, desc.W, dtype=torch.uint8, device=device)
            labels = torch.zeros(desc.N, P, desc.H, desc.W, dtype=torch.int32, device=device) if self.want_labels else None
            cmap = torch.zeros(desc.N, desc.H, desc.W, dtype=torch.uint8, device=device) if cls else None
            stats = torch.zeros(desc.N, P, 8, dtype=torch.int64, device=device)
            comps = torch.zeros(desc.N, P, 8, 8, dtype=torch.int64, device=device)
            plan = self._plans[key] = (desc, ws, mask, labels, cmap, stats, comps)
        return plan

    # ------------------------------------------------------------------ one call
    def __call__(self, outputs_or_prob, *, mode: str = "auto", from_logits: bool = True) -> torch.Tensor:
        _, maps, main = maps_of(outputs_or_prob)
        x = maps[main]
        if not isinstance(x, torch.Tensor):
            raise ValueError("MaskPostprocess: the input must be a tensor (or a dict / list of output tensors)")
        shape = tuple(x.shape)
        if len(shape) != 4:
            raise ValueError(f"MaskPostprocess: the map must be (N, C, H, W), got shape {shape}")
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"MaskPostprocess: the map must be float32 or bfloat16, got {x.dtype}")
        if x.numel() == 0:
            raise ValueError("MaskPostprocess: empty maps")
        if shape[2] > L.POST_MAX_HW or shape[3] > L.POST_MAX_HW:
            raise ValueError(f"MaskPostprocess: maps of {shape[2]} x {shape[3]} pixels, at most {L.POST_MAX_HW} each way")
        m = resolve_mode(mode, shape[1], "MaskPostprocess")
        if m == L.POST_CLASS and not 2 <= shape[1] <= L.CLASS_MAX_K:
            raise ValueError(f"MaskPostprocess: K = {shape[1]} classes outside [2, {L.CLASS_MAX_K}]")
        L.require_cuda(x)
        xs = x.detach().contiguous().float()
        thr = 0.0 if (from_logits or m == L.POST_CLASS) else 0.5
        desc, ws, mask, labels, cmap, stats, comps = self._plan(m, thr, shape, xs.device)
        ops.postproc(desc, xs, mask, labels, cmap, stats, comps, ws)
        self.mask, self.labels, self.class_map, self.stats, self.comps = mask, labels, cmap, stats, comps
        return mask

    def check(self) -> None:
        """read the error words of the last call on the host (a synchronisation); raises when a bounded find / union loop ran
        out -- a bug of the kernels, never a property of the input"""
        if self.stats is None:
            raise RuntimeError("MaskPostprocess: no call yet")
        err = self.stats[..., 6]
        if bool((err != 0).any().item()):
            bad = [tuple(ix) for ix in (err != 0).nonzero().tolist()]
            raise RuntimeError(f"MaskPostprocess: a bounded union-find loop ran out in the (image, plane) pairs {bad}; "
                               f"the results of those planes are undefined")

    def __repr__(self) -> str:
        return (f"MaskPostprocess(connectivity={self.connectivity}, fill_holes={self.fill_holes}, min_area={self.min_area}, "
                f"keep_largest={self.keep_largest}, include_background={self.include_background}, labels={self.want_labels})")
