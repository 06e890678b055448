"""float64 numpy restatement of GpuAugment's arithmetic (include/unetzoo_hip.h, uz_augment.hip): the checker of
tests/test_augment_gpu.py, itself pinned against torch on the CPU by tests/test_augment.py.

Output pixel (i, j), u = j + 0.5 - W/2, v = i + 0.5 - H/2, reads the source at
    sx = a u + b v + ox + Dx(i, j),  sy = c u + d v + oy + Dy(i, j)            (pixel indices)
(a, b, ox, c, d, oy) = params[:6]; D = the (2, G, G) grid interpolated bilinearly at (j (G-1)/(W-1), i (G-1)/(H-1)).
Picture: bilinear over the four taps around (floor sx, floor sy), a tap outside contributing `fill`, then contrast * value +
brightness.  Mask: the pixel (floor(sx + 0.5), floor(sy + 0.5)), `fill` outside."""
import math

import numpy as np
import torch

# (theta [rad], s, hflip, vflip, tx, ty): the four generic warps of the tests
SETS = ((0.3, 1.1, False, False, 2.3, -1.7),
        (-0.7, 0.8, True, False, 0.4, 3.2),
        (math.radians(17.0), 1.25, False, True, -5.1, 0.6),
        (math.radians(-33.0), 0.9, True, True, 1.9, 2.2))
# ranges of a GpuAugment that contain them (H, W >= 21: translate * min(H, W) >= 5.1)
RANGES = dict(hflip=0.5, vflip=0.5, rotate=45.0, scale=(0.75, 1.3), translate=0.25)
TIE_TOL = 1e-3      # a mask pixel is compared unless sx + 0.5 or sy + 0.5 lies this close to an integer ...
TIE_CAP = 0.01      # ... which may leave out at most this share of a case's pixels


def draws_for_sets(H, W, sets=SETS, ranges=RANGES, u_brightness=0.5, u_contrast=0.5):
    """(N, 8) float32 uniforms from which params_from_draws() / uz_augment_params form (the float32 neighbours of) `sets`"""
    smin, smax = ranges["scale"]
    u = np.zeros((len(sets), 8), np.float64)
    for n, (theta, s, hf, vf, tx, ty) in enumerate(sets):
        u[n] = (0.25 if hf else 0.75, 0.25 if vf else 0.75, (math.degrees(theta) / ranges["rotate"] + 1.0) / 2.0,
                (s - smin) / (smax - smin), (tx / (ranges["translate"] * W) + 1.0) / 2.0,
                (ty / (ranges["translate"] * H) + 1.0) / 2.0, u_brightness, u_contrast)
    assert (u >= 0.0).all() and (u < 1.0).all()
    return u.astype(np.float32)


def params_from_draws(u, H, W, hflip=0.0, vflip=0.0, rotate=0.0, scale=(1.0, 1.0), translate=0.0, brightness=0.0, contrast=0.0):
    """(N, 16) float64 per-sample parameters from (N, 8) uniforms: a, b, ox, c, d, oy, contrast, brightness, zeros.  The two
    flip decisions compare in float32, as the kernel does (u and the probability are float32 there)."""
    u32 = np.asarray(u, np.float32)
    q = u32.astype(np.float64)
    fx = np.where(u32[:, 0] < np.float32(hflip), -1.0, 1.0)
    fy = np.where(u32[:, 1] < np.float32(vflip), -1.0, 1.0)
    theta = np.radians((2.0 * q[:, 2] - 1.0) * rotate)
    s = scale[0] + q[:, 3] * (scale[1] - scale[0])
    tx = (2.0 * q[:, 4] - 1.0) * translate * W
    ty = (2.0 * q[:, 5] - 1.0) * translate * H
    p = np.zeros((len(q), 16), np.float64)
    p[:, 0] = np.cos(theta) * fx / s
    p[:, 1] = np.sin(theta) * fy / s
    p[:, 2] = W / 2.0 + tx - 0.5
    p[:, 3] = -np.sin(theta) * fx / s
    p[:, 4] = np.cos(theta) * fy / s
    p[:, 5] = H / 2.0 + ty - 0.5
    p[:, 6] = 1.0 + (2.0 * q[:, 7] - 1.0) * contrast
    p[:, 7] = (2.0 * q[:, 6] - 1.0) * brightness
    return p


def displacement(disp, H, W):
    """(2, G, G) -> (2, H, W): bilinear, align_corners=True"""
    disp = np.asarray(disp, np.float64)
    G = disp.shape[-1]
    gx = np.arange(W, dtype=np.float64) * (G - 1) / (W - 1)
    gy = np.arange(H, dtype=np.float64) * (G - 1) / (H - 1)
    x0 = np.minimum(np.floor(gx).astype(np.int64), G - 2)
    y0 = np.minimum(np.floor(gy).astype(np.int64), G - 2)
    tx, ty = (gx - x0)[None, None, :], (gy - y0)[None, :, None]
    Y0, X0 = y0[:, None], x0[None, :]
    top = (1.0 - tx) * disp[:, Y0, X0] + tx * disp[:, Y0, X0 + 1]
    bot = (1.0 - tx) * disp[:, Y0 + 1, X0] + tx * disp[:, Y0 + 1, X0 + 1]
    return (1.0 - ty) * top + ty * bot


def source_coords(p, H, W, disp=None):
    """(sx, sy), each (H, W) float64, of one sample with parameters p (>= 6 entries) and displacement grid disp (2, G, G)"""
    p = np.asarray(p, np.float64)
    u = (np.arange(W, dtype=np.float64) + 0.5 - W / 2.0)[None, :]
    v = (np.arange(H, dtype=np.float64) + 0.5 - H / 2.0)[:, None]
    sx = p[0] * u + p[1] * v + p[2]
    sy = p[3] * u + p[4] * v + p[5]
    if disp is not None:
        D = displacement(disp, H, W)
        sx, sy = sx + D[0], sy + D[1]
    return sx, sy


def _taps(img, yy, xx, fill):
    H, W = img.shape[-2:]
    inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
    v = img[..., np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
    return np.where(inside, v, fill)


def bilinear_fill(img, sx, sy, fill):
    """img (..., H, W) read at (sx, sy): four taps, `fill` for a tap outside"""
    img = np.asarray(img, np.float64)
    x0f, y0f = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0f, sy - y0f
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    top = (1.0 - fx) * _taps(img, y0, x0, fill) + fx * _taps(img, y0, x0 + 1, fill)
    bot = (1.0 - fx) * _taps(img, y0 + 1, x0, fill) + fx * _taps(img, y0 + 1, x0 + 1, fill)
    return (1.0 - fy) * top + fy * bot


def nearest_fill(mask, sx, sy, fill):
    """mask (..., H, W) at (floor(sx + 0.5), floor(sy + 0.5)), `fill` outside; keeps the mask's dtype"""
    mask = np.asarray(mask)
    xm, ym = np.floor(sx + 0.5).astype(np.int64), np.floor(sy + 0.5).astype(np.int64)
    return _taps(mask, ym, xm, mask.dtype.type(fill))


def tie_band(sx, sy, tol=TIE_TOL):
    """True where the nearest pixel hangs on less than `tol` of a source coordinate: sx + 0.5 or sy + 0.5 that close to an
    integer (a float32 coordinate may round to the other side)"""
    a, b = sx + 0.5, sy + 0.5
    return (np.abs(a - np.round(a)) < tol) | (np.abs(b - np.round(b)) < tol)


def apply(images, masks, params, disp=None, image_fill=0.0, mask_fill=0.0, label_fill=-100):
    """images (N, C, H, W), masks None / float (N, Cm, H, W) / integer (N, H, W), params (N, >= 8), disp None / (N, 2, G, G)
    -> (pictures float64, masks in their dtype, tie band (N, H, W) bool)"""
    images = np.asarray(images, np.float64)
    N, _, H, W = images.shape
    out = np.empty_like(images)
    mout = None if masks is None else np.empty_like(np.asarray(masks))
    band = np.zeros((N, H, W), bool)
    for n in range(N):
        sx, sy = source_coords(params[n], H, W, None if disp is None else disp[n])
        out[n] = float(params[n][6]) * bilinear_fill(images[n], sx, sy, image_fill) + float(params[n][7])
        band[n] = tie_band(sx, sy)
        if masks is not None:
            m = np.asarray(masks)[n]
            mout[n] = nearest_fill(m, sx, sy, mask_fill if m.dtype.kind == "f" else label_fill)
    return out, mout, band


def ulp32(x):
    """spacing of float32 at |x|"""
    return float(np.spacing(np.float32(abs(x))))


def neighbour_diff(images):
    """D: the largest difference between horizontally or vertically neighbouring pixels"""
    a = np.asarray(images, np.float64)
    return max(float(np.abs(np.diff(a, axis=-1)).max()), float(np.abs(np.diff(a, axis=-2)).max()))


def image_bound(images, H, W, extra_eps=0.0, gain=1.0, top=None):
    """2 D eps + 8 * 2^-23 max|picture|, eps = 4 ulp32(2 max(H, W)) + extra_eps: a bilinear surface moves at most D per pixel
    along each axis (2 D for both), times the float32 error eps of a source coordinate, plus the rounding of the interpolation
    itself.  gain / top: the same for the jittered picture gain * picture + offset (D scales by |gain|, `top` = its max)."""
    eps = 4.0 * ulp32(2.0 * max(H, W)) + extra_eps
    top = float(np.abs(np.asarray(images, np.float64)).max()) if top is None else top
    return 2.0 * abs(gain) * neighbour_diff(images) * eps + 8.0 * 2.0 ** -23 * top


# ---- what a flip and a whole-pixel translation must give, from torch.flip and slices (no arithmetic) -------------------------
def shifted(y, dx, dy, fill):
    """out[..., i, j] = y[..., i + dy, j + dx], `fill` where that lies outside (slices)"""
    H, W = y.shape[-2:]
    out = torch.full_like(y, fill)
    i0, i1, j0, j1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    out[..., i0:i1, j0:j1] = y[..., i0 + dy:i1 + dy, j0 + dx:j1 + dx]
    return out


def flipped_shifted(y, hflip, vflip, tx, ty, fill):
    """what the map of a flip and a whole-pixel translation (tx, ty) reads: flip first; a flipped axis shifts the other way"""
    dims = [d for d, f in ((-1, hflip), (-2, vflip)) if f]
    y = torch.flip(y, dims) if dims else y
    return shifted(y, -tx if hflip else tx, -ty if vflip else ty, fill)
