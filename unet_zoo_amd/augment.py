"""Training-time augmentation on the device: ``GpuAugment``.

``data.GpuPreprocessor`` leaves the resized, normalised batch on the GPU; the reference's dataset does nothing more
(unet_zoo/data/datasets.py:40-59).  Flips, rotations, scalings, translations, an elastic-style grid distortion and an
intensity jitter on the host would feed a 3-6 ms training step from a few CPU cores.  ``GpuAugment`` does them in two
launches (``uz_augment.hip``): one that turns per-sample uniform draws into each sample's inverse map and jitter, and one that
reads picture and mask through that map -- bilinear for the picture, nearest for the mask, so a mask stays a mask.

    aug = unet_zoo_amd.GpuAugment(hflip=0.5, rotate=15.0, scale=(0.9, 1.1), translate=0.05, brightness=0.1, contrast=0.1)
    xa, ta = aug(images, masks)               # device tensors, STATIC per shape: clone what must outlive the next call
    step = unet_zoo_amd.GraphedStep(model, augment=aug)      # or inside the step's first hipGraph

Coordinates (include/unetzoo_hip.h): output pixel (i, j), u = j + 0.5 - W/2, v = i + 0.5 - H/2, reads the source
at sx = a u + b v + ox + Dx(i, j), sy = c u + d v + oy + Dy(i, j) in pixel indices; (a, b, c, d) = (1/s) R(-theta) diag(fx, fy).

The draws are torch's: ``torch.rand((N, 8))`` and, with ``grid_distort=(G, sigma_px)``, ``torch.randn((N, 2, G, G)) * sigma_px``
on the device, so ``torch.manual_seed`` reproduces a run and a captured graph draws fresh values in every replay (the
precedent is VNet's Dropout2d masks and ``Engine.dropout``).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

from . import _lib as L
from . import ops
from .criterion import INT_DTYPES


class _Bound:
    """the static tensors of one (picture, mask) pair: what the two launches read and write"""
    __slots__ = ("aug", "image", "mask", "desc", "params", "out_image", "out_mask", "u", "disp")

    def run(self) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """the two launches on the current stream (capturable: no host read, no memset)"""
        aug, N = self.aug, self.desc.N
        u, disp = aug._draws(N, self.desc.G, self.image.device)
        self.u, self.disp = u, disp          # a captured graph reads them in every replay
        ops.augment_params(self.desc, u, self.params)
        ops.augment_apply(self.desc, self.image, self.mask, self.params, disp, self.out_image, self.out_mask)
        aug.last_params = self.params
        return self.out_image, self.out_mask


class GpuAugment:
    """hflip / vflip: probabilities of a horizontal / vertical flip; rotate: the angle is uniform in [-rotate, rotate] degrees;
    scale = (smin, smax): uniform zoom factor; translate: the shift is uniform in [-translate, translate] of the width / height;
    brightness / contrast: out = (1 + c) * picture + b with b uniform in [-brightness, brightness], c in [-contrast, contrast];
    grid_distort = (G, sigma_px): a (G, G) grid of normal displacements of sigma_px pixels, interpolated bilinearly over the
    picture (align_corners=True) and added to the source coordinates; G in 2..16.
    image_fill / mask_fill / label_fill: what a source position outside the picture contributes -- to the picture (before
    the jitter, so the fill is jittered with the rest), to a float mask, to integer labels (pass the criterion's
    ``ignore_index``).

    ``aug(images, masks=None)``: images (N, C, H, W) fp32 on the device with C in 1..4; masks fp32 (N, Cm, H, W) with Cm in 1..8,
    or class indices (N, H, W) of any integer dtype, held and returned as int32 (``MulticlassLoss.target_dtype``).  Returns
    (pictures, masks) of the same shapes; they are static per shape, the next call with that shape overwrites them.
    ``last_params`` is the (N, 16) tensor of the last call: a, b, ox, c, d, oy, contrast, brightness, zeros.
    With several ranks every rank draws from its own generator: seed the ranks differently (or alike, to augment alike)."""

    def __init__(self, hflip: float = 0.5, vflip: float = 0.0, rotate: float = 15.0, scale: Tuple[float, float] = (0.9, 1.1),
                 translate: float = 0.05, brightness: float = 0.1, contrast: float = 0.1,
                 grid_distort: Optional[Tuple[int, float]] = None, image_fill: float = 0.0, mask_fill: float = 0.0,
                 label_fill: int = -100):
        for name, p in (("hflip", hflip), ("vflip", vflip)):
            if not (isinstance(p, (int, float)) and 0.0 <= p <= 1.0):
                raise ValueError(f"GpuAugment: {name} is a probability in [0, 1], got {p!r}")
        for name, r in (("rotate", rotate), ("translate", translate), ("brightness", brightness), ("contrast", contrast)):
            if not (isinstance(r, (int, float)) and math.isfinite(r) and r >= 0.0):
                raise ValueError(f"GpuAugment: {name} is a non-negative range, got {r!r}")
        try:
            smin, smax = (float(v) for v in scale)
        except (TypeError, ValueError):
            raise ValueError(f"GpuAugment: scale is a pair (smin, smax), got {scale!r}") from None
        if not (0.0 < smin <= smax and math.isfinite(smax)):
            raise ValueError(f"GpuAugment: scale needs 0 < smin <= smax, got {scale!r}")
        G, sigma = 0, 0.0
        if grid_distort is not None:
            try:
                G, sigma = grid_distort
            except (TypeError, ValueError):
                raise ValueError(f"GpuAugment: grid_distort is None or a pair (G, sigma_px), got {grid_distort!r}") from None
            if isinstance(G, bool) or not isinstance(G, int) or not 2 <= G <= 16:
                raise ValueError(f"GpuAugment: grid_distort's G must be an int in 2..16, got {G!r}")
            if not (isinstance(sigma, (int, float)) and math.isfinite(sigma) and sigma >= 0.0):
                raise ValueError(f"GpuAugment: grid_distort's sigma_px is a non-negative range, got {sigma!r}")
        for name, f in (("image_fill", image_fill), ("mask_fill", mask_fill)):
            if not (isinstance(f, (int, float)) and math.isfinite(f)):
                raise ValueError(f"GpuAugment: {name} must be a finite number, got {f!r}")
        if isinstance(label_fill, bool) or not isinstance(label_fill, int) or not -2 ** 31 <= label_fill < 2 ** 31:
            raise ValueError(f"GpuAugment: label_fill must be an int32 value, got {label_fill!r}")
        self.hflip, self.vflip, self.rotate, self.scale = float(hflip), float(vflip), float(rotate), (smin, smax)
        self.translate, self.brightness, self.contrast = float(translate), float(brightness), float(contrast)
        self.grid_distort = None if grid_distort is None else (G, float(sigma))
        self.image_fill, self.mask_fill, self.label_fill = float(image_fill), float(mask_fill), label_fill
        self.last_params: Optional[torch.Tensor] = None
        self._forced: Optional[Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]] = None
        self._forced_sticky = False
        self._bound: Dict[tuple, _Bound] = {}

    # -- test seam --------------------------------------------------------------------------------------------------------
    def force_draws(self, u: Optional[torch.Tensor] = None, disp: Optional[torch.Tensor] = None, sticky: bool = False) -> None:
        """Use these values in place of the NEXT call's own random draws: `u` (N, 8) uniforms in [0, 1), `disp` (N, 2, G, G)
        displacements in pixels.  They are cleared by the call that uses them unless sticky=True; force_draws() with no
        arguments clears them (the semantics of VNet.force_draws)."""
        if u is None and disp is None:
            self._forced, self._forced_sticky = None, False
            return
        if u is not None and (u.dim() != 2 or u.shape[1] != 8):
            raise ValueError(f"force_draws: u takes (N, 8) uniforms, got {tuple(u.shape)}")
        if disp is not None:
            G = self.grid_distort[0] if self.grid_distort is not None else None
            if G is None or disp.dim() != 4 or tuple(disp.shape[1:]) != (2, G, G):
                raise ValueError(f"force_draws: disp takes (N, 2, G, G) displacements with G = {G} (grid_distort), got "
                                 f"{tuple(disp.shape)}")
        self._forced, self._forced_sticky = (u, disp), sticky

    def _draws(self, N: int, G: int, device) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        u, disp = self._forced if self._forced is not None else (None, None)
        for name, t in (("u", u), ("disp", disp)):
            if t is not None and t.shape[0] != N:
                raise ValueError(f"force_draws: the batch size of {name} ({t.shape[0]}) differs from the input's ({N})")
        if not self._forced_sticky:
            self._forced = None
        if u is None:
            u = torch.rand((N, 8), device=device)
        else:
            u = u.to(device=device, dtype=torch.float32).contiguous()
        if G == 0:
            disp = None
        elif disp is None:
            disp = torch.randn((N, 2, G, G), device=device) * self.grid_distort[1]
        else:
            disp = disp.to(device=device, dtype=torch.float32).contiguous()
        return u, disp

    # -- binding to tensors -----------------------------------------------------------------------------------------------
    def bind(self, images: torch.Tensor, masks: Optional[torch.Tensor] = None) -> _Bound:
        """Static outputs and parameters for THESE input tensors (fp32 pictures; an fp32 or int32 mask), which the returned
        object's run() reads in place: GraphedStep captures run() at the head of its first graph."""
        if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.dtype != torch.float32:
            raise ValueError("GpuAugment: images must be an fp32 tensor of shape (N, C, H, W), got "
                             + (f"{images.dtype} {tuple(images.shape)}" if isinstance(images, torch.Tensor) else repr(type(images))))
        N, C, H, W = images.shape
        if not 1 <= C <= 4:
            raise ValueError(f"GpuAugment: images have C = {C} channels; 1..4 are supported")
        kind, Cm = L.AUGMENT_MASK_NONE, 0
        if masks is not None:
            if masks.dtype == torch.float32:
                if masks.dim() != 4 or masks.shape[0] != N or tuple(masks.shape[2:]) != (H, W) or not 1 <= masks.shape[1] <= 8:
                    raise ValueError(f"GpuAugment: an fp32 masks tensor must be (N, Cm, H, W) = ({N}, 1..8, {H}, {W}) to go with "
                                     f"images {tuple(images.shape)}, got {tuple(masks.shape)}")
                kind, Cm = L.AUGMENT_MASK_F32, masks.shape[1]
            elif masks.dtype == torch.int32:
                if tuple(masks.shape) != (N, H, W):
                    raise ValueError(f"GpuAugment: integer masks (class indices) must be (N, H, W) = ({N}, {H}, {W}) to go with "
                                     f"images {tuple(images.shape)}, got {tuple(masks.shape)}")
                kind = L.AUGMENT_MASK_I32
            else:
                raise ValueError(f"GpuAugment: masks must be fp32 or integer, got {masks.dtype}")
        G = self.grid_distort[0] if self.grid_distort is not None else 0
        if G and (H < 2 or W < 2):
            raise ValueError(f"GpuAugment: grid_distort needs images of at least 2 x 2 pixels, got {H} x {W}")
        L.require_cuda(images, masks)        # good arguments on the host: there is no CPU path
        b = _Bound()
        b.aug, b.image, b.mask = self, images.contiguous(), masks.contiguous() if masks is not None else None
        b.desc = L.AugmentDesc(N, C, H, W, kind, Cm, G, self.hflip, self.vflip, self.rotate, self.scale[0], self.scale[1],
                               self.translate, self.brightness, self.contrast, self.image_fill, self.mask_fill, self.label_fill)
        ops.augment_grid(b.desc)        # the library's own refusals (size) before anything is allocated
        b.params = torch.empty((N, 16), dtype=torch.float32, device=images.device)
        b.out_image = torch.empty_like(b.image)
        b.out_mask = torch.empty_like(b.mask) if masks is not None else None
        b.u = b.disp = None
        return b

    def __call__(self, images: torch.Tensor, masks: Optional[torch.Tensor] = None):
        if masks is not None and isinstance(masks, torch.Tensor) and masks.dtype in INT_DTYPES and masks.dtype != torch.int32:
            masks = masks.to(torch.int32)
        key = (tuple(images.shape), None if masks is None else (tuple(masks.shape), masks.dtype), images.device) \
            if isinstance(images, torch.Tensor) else None
        b = self._bound.get(key)
        if b is None:
            b = self.bind(images, masks)
            if key is not None:
                self._bound[key] = b
        else:
            if images.dtype != torch.float32:
                raise ValueError(f"GpuAugment: images must be fp32, got {images.dtype}")
            b.image = images.contiguous()
            b.mask = masks.contiguous() if masks is not None else None
        return b.run()

    def __repr__(self) -> str:
        return (f"GpuAugment(hflip={self.hflip}, vflip={self.vflip}, rotate={self.rotate}, scale={self.scale}, "
                f"translate={self.translate}, brightness={self.brightness}, contrast={self.contrast}, "
                f"grid_distort={self.grid_distort}, image_fill={self.image_fill}, mask_fill={self.mask_fill}, "
                f"label_fill={self.label_fill})")
