"""Patch training from a pool of pictures that stays on the device: ``PatchSampler``.

``SlidingWindowPredict`` predicts on pictures larger than the model's window; this is the training side for the same pictures.
The pool -- every picture (fp32, or uint8 to keep a whole data set resident) and its mask -- is moved to the GPU once, a
foreground index is built once (``uz_patch.hip``: per mask plane the running count of foreground pixels over the rows), and
every call draws a batch of windows and cuts them out in two launches:

    pool = unet_zoo_amd.PatchSampler(images, masks, window=(256, 256), batch=16, pos=1 / 3, jitter=1.0)
    x, t = pool()                         # (16, C, 256, 256) fp32 and the mask patches, STATIC: clone what must outlive the next call
    step = unet_zoo_amd.GraphedStep(model, crit, augment=aug, source=pool)
    loss = step()                         # sample + cut (+ augment) + forward + loss + backward from the graphs

Rules of a draw (include/unetzoo_hip.h): with probability `pos` a patch is a FOREGROUND patch when its picture has
any foreground: a non-empty foreground plane is picked uniformly (a channel of an fp32 mask above 0.5; class 1..num_classes-1
of a label map), a foreground pixel of that plane uniformly, and the window is placed so that the pixel lies in it -- at its
centre with jitter = 0, uniformly anywhere in it with jitter = 1 -- and clamped into the picture.  Every other patch is a
window placed uniformly.  ``last_coords`` is the (B, 4) int32 tensor [picture, y0, x0, plane or -1] of the last call.

The draws are torch's: ``torch.rand((B, 8))`` on the device, so ``torch.manual_seed`` reproduces a run and a captured graph
draws fresh patches in every replay (the precedent is ``GpuAugment``).
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import ops
from .criterion import INT_DTYPES
from .data import IMAGENET_MEAN, IMAGENET_STD


class PatchSampler:
    """images: (M, C, H, W) fp32 or uint8, C in 1..4, all pictures of one size (from any device; the pool is held on the current
    cuda device).
    masks: None, fp32 (M, Cm, H, W) with Cm in 1..8, or class indices (M, H, W) of any integer dtype, held and returned as int32
    (``MulticlassLoss.target_dtype``); integer masks need `num_classes` (2..9): classes 1..num_classes-1 are foreground, class 0,
    an ignore index and every other value are background.
    window = (h, w) <= (H, W): pad smaller pictures upstream.  batch: patches per call.  pos: probability of a foreground
    patch.  jitter in [0, 1]: where in the window the chosen foreground pixel lands (0: the centre, 1: anywhere).
    mean / std: uint8 pictures become (v / 255 - mean[c]) / std[c], as one multiply-add with scale = 1 / (255 std) and
    shift = -mean / std formed in float64 and rounded once (C values each: the ImageNet defaults serve C = 3, with another C
    pass your own; mean=None, std=None gives the plain values 0..255).  fp32 pictures are taken as they are.

    ``pool()`` / ``pool.run()``: the two launches on the current stream; returns (pictures, masks), static per sampler.
    ``pool.set_indices(idx)``: the NEXT calls take their pictures from these `batch` indices (an epoch's permutation) instead of
    drawing them; an index outside 0..M-1 gives a patch of zeros.  The choice between drawn and given pictures is part of the
    launch, so it must be made before the first call that a hipGraph captures (``GraphedStep(source=pool)``)."""

    def __init__(self, images: torch.Tensor, masks: Optional[torch.Tensor] = None, window: Tuple[int, int] = (256, 256), batch: int = 16,
                 pos: float = 1.0 / 3.0, jitter: float = 1.0, num_classes: Optional[int] = None,
                 mean: Optional[Sequence[float]] = IMAGENET_MEAN, std: Optional[Sequence[float]] = IMAGENET_STD):
        if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.dtype not in (torch.float32, torch.uint8):
            raise ValueError("PatchSampler: images must be an fp32 or uint8 tensor of shape (M, C, H, W), got "
                             + (f"{images.dtype} {tuple(images.shape)}" if isinstance(images, torch.Tensor) else repr(type(images))))
        M, C, H, W = images.shape
        if M < 1 or not 1 <= C <= 4:
            raise ValueError(f"PatchSampler: images have M = {M} pictures of C = {C} channels; M >= 1 and C in 1..4 are supported")
        try:
            h, w = (int(v) for v in window)
        except (TypeError, ValueError):
            raise ValueError(f"PatchSampler: window is a pair (h, w), got {window!r}") from None
        if not (1 <= h <= H and 1 <= w <= W):
            raise ValueError(f"PatchSampler: window {h} x {w} must lie within the pictures ({H} x {W}); pad smaller pictures upstream")
        if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
            raise ValueError(f"PatchSampler: batch must be a positive int, got {batch!r}")
        for name, p in (("pos", pos), ("jitter", jitter)):
            if not (isinstance(p, (int, float)) and 0.0 <= p <= 1.0):
                raise ValueError(f"PatchSampler: {name} lies in [0, 1], got {p!r}")
        kind, Cm, P = L.PATCH_MASK_NONE, 0, 0
        if masks is not None:
            if not isinstance(masks, torch.Tensor):
                raise ValueError(f"PatchSampler: masks must be a tensor or None, got {type(masks)!r}")
            if masks.dtype == torch.float32:
                if masks.dim() != 4 or masks.shape[0] != M or tuple(masks.shape[2:]) != (H, W) or not 1 <= masks.shape[1] <= 8:
                    raise ValueError(f"PatchSampler: an fp32 masks tensor must be (M, Cm, H, W) = ({M}, 1..8, {H}, {W}) to go with "
                                     f"images {tuple(images.shape)}, got {tuple(masks.shape)}")
                if num_classes is not None:
                    raise ValueError("PatchSampler: num_classes goes with integer masks (class indices) only")
                kind, Cm = L.PATCH_MASK_F32, masks.shape[1]
                P = Cm
            elif masks.dtype in INT_DTYPES:
                if tuple(masks.shape) != (M, H, W):
                    raise ValueError(f"PatchSampler: integer masks (class indices) must be (M, H, W) = ({M}, {H}, {W}) to go with "
                                     f"images {tuple(images.shape)}, got {tuple(masks.shape)}")
                if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 2 <= num_classes <= 9:
                    raise ValueError(f"PatchSampler: integer masks need num_classes, an int in 2..9 (at most 8 foreground "
                                     f"classes), got {num_classes!r}")
                kind, P = L.PATCH_MASK_I32, num_classes - 1
            else:
                raise ValueError(f"PatchSampler: masks must be fp32 or integer, got {masks.dtype}")
        elif num_classes is not None:
            raise ValueError("PatchSampler: num_classes goes with integer masks (class indices) only")
        norm = None
        if images.dtype == torch.uint8 and (mean is not None or std is not None):
            if mean is None or std is None:
                raise ValueError("PatchSampler: mean / std go together (both None: the plain values 0..255)")
            try:
                mu, sd = (np.array([float(v) for v in s], dtype=np.float64) for s in (mean, std))
            except (TypeError, ValueError):
                raise ValueError(f"PatchSampler: mean / std are sequences of C = {C} numbers, got {mean!r} / {std!r}") from None
            if mu.shape != (C,) or sd.shape != (C,) or not np.isfinite(mu).all() or not np.isfinite(sd).all() or (sd <= 0).any():
                raise ValueError(f"PatchSampler: mean / std take C = {C} finite values each, std > 0; got {mean!r} / {std!r}")
            norm = np.concatenate([1.0 / (255.0 * sd), -mu / sd]).astype(np.float32)      # float64, rounded once
        self.window, self.batch, self.pos, self.jitter, self.num_classes = (h, w), batch, float(pos), float(jitter), num_classes
        if not torch.cuda.is_available():
            raise L.HipLibraryError("unet_zoo_amd kernels run on an MI355X only: PatchSampler holds its pool on the current "
                                    "'cuda' device and none is visible (there is no CPU fallback in the product path).")
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.desc = L.PatchDesc(M, C, H, W, L.PATCH_IMAGE_U8 if images.dtype == torch.uint8 else L.PATCH_IMAGE_F32, kind, Cm, P, batch,
                                h, w, 0, self.pos, self.jitter)
        ops.patch_cut_grid(self.desc)        # the library's own refusals (sizes) before anything is moved or allocated
        dev = self.device
        self.images = images.to(dev).contiguous()
        self.masks = None
        if masks is not None:
            self.masks = masks.to(device=dev, dtype=torch.int32 if kind == L.PATCH_MASK_I32 else torch.float32).contiguous()
        self.norm = torch.from_numpy(norm).to(dev) if norm is not None else None
        self.index = None
        if P:
            self.index = torch.empty((M, P, H + 1), dtype=torch.int32, device=dev)
            ops.patch_index(self.desc, self.masks, self.index)
        self.out_image = torch.empty((batch, C, h, w), dtype=torch.float32, device=dev)
        self.out_mask = None
        if kind == L.PATCH_MASK_F32:
            self.out_mask = torch.empty((batch, Cm, h, w), dtype=torch.float32, device=dev)
        elif kind == L.PATCH_MASK_I32:
            self.out_mask = torch.empty((batch, h, w), dtype=torch.int32, device=dev)
        self.coords = torch.empty((batch, 4), dtype=torch.int32, device=dev)
        self.indices = torch.zeros((batch,), dtype=torch.int32, device=dev)
        self.last_coords: Optional[torch.Tensor] = None
        self.u: Optional[torch.Tensor] = None
        self._forced: Optional[torch.Tensor] = None
        self._forced_sticky = False
        self._captured: Optional[int] = None      # use_indices as a hipGraph captured it

    # -- which pictures ---------------------------------------------------------------------------------------------------
    def set_indices(self, indices) -> None:
        """The following calls cut patch b from picture indices[b] (`batch` integers, e.g. a slice of an epoch's permutation),
        written into a static buffer that a captured graph reads; set_indices(None) goes back to drawn pictures.  Switching
        between the two after a hipGraph captured run() is refused: the choice is part of the captured launch."""
        want = 0 if indices is None else 1
        if self._captured is not None and self._captured != want:
            raise RuntimeError("PatchSampler.set_indices: a captured hipGraph draws its pictures " +
                               ("itself" if want else "from set_indices()") + "; choose before the first captured call")
        if indices is not None:
            idx = torch.as_tensor(indices)
            if idx.dtype not in INT_DTYPES or tuple(idx.shape) != (self.batch,):
                raise ValueError(f"PatchSampler.set_indices: {self.batch} integer indices (one per patch), got "
                                 f"{idx.dtype} {tuple(idx.shape)}")
            self.indices.copy_(idx.to(device=self.device, dtype=torch.int32))
        self.desc.use_indices = want

    # -- test seam --------------------------------------------------------------------------------------------------------
    def force_draws(self, u: Optional[torch.Tensor] = None, sticky: bool = False) -> None:
        """Use `u`, (batch, 8) uniforms in [0, 1), in place of the NEXT call's own random draws.  They are cleared by the call
        that uses them unless sticky=True; force_draws() with no arguments clears them (the semantics of
        GpuAugment.force_draws)."""
        if u is None:
            self._forced, self._forced_sticky = None, False
            return
        if not isinstance(u, torch.Tensor) or tuple(u.shape) != (self.batch, 8):
            raise ValueError(f"force_draws: u takes (batch, 8) = ({self.batch}, 8) uniforms, got "
                             f"{tuple(u.shape) if isinstance(u, torch.Tensor) else type(u)!r}")
        self._forced, self._forced_sticky = u.to(device=self.device, dtype=torch.float32).contiguous(), sticky

    # -- the launches -----------------------------------------------------------------------------------------------------
    def bind(self) -> "PatchSampler":
        """The object whose run() GraphedStep captures at the head of its first graph and whose out_image / out_mask it reads:
        the sampler itself, its tensors are static from construction."""
        return self

    def run(self) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """the draw and the cut on the current stream (capturable: no host read, no memset)"""
        u = self._forced
        if u is None:
            u = torch.rand((self.batch, 8), device=self.device)
        elif not self._forced_sticky:
            self._forced = None
        self.u = u          # a captured graph reads it in every replay
        d = self.desc
        if torch.cuda.is_current_stream_capturing():
            self._captured = d.use_indices
        ops.patch_draw(d, u, self.indices if d.use_indices else None, self.index, self.masks if self.index is not None else None,
                       self.coords)
        ops.patch_cut(d, self.images, self.masks, self.coords, self.norm, self.out_image, self.out_mask)
        self.last_coords = self.coords
        return self.out_image, self.out_mask

    __call__ = run

    def __repr__(self) -> str:
        d = self.desc
        return (f"PatchSampler({d.M} pictures {d.C} x {d.H} x {d.W} {'uint8' if d.image_kind else 'fp32'}, window={self.window}, "
                f"batch={self.batch}, pos={self.pos:.4g}, jitter={self.jitter:.4g}, foreground planes={d.P})")
