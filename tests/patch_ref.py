"""Numpy restatement of uz_patch.hip as include/unetzoo_hip.h specifies it: the foreground index, the draw and the cut.

Integer picks are pick(u, n) = min(n - 1, floor(float64(u) * n)) with u a float32 uniform: one IEEE double product, which the
kernel forms in the same way, so index, coordinates and fp32 / mask patches are compared for equality.  The comparison u1 < pos
is made in float32 (pos is a float in the descriptor).  tests/test_patch_sampler.py holds this file to a brute force
(np.flatnonzero for the k-th pixel, slicing for the cut)."""
import numpy as np

NONE, F32, I32 = 0, 1, 2


def planes(mask, num_classes=None):
    """(M, P, H, W) bool foreground planes of an fp32 (M, Cm, H, W) mask or an integer (M, H, W) label map"""
    mask = np.asarray(mask)
    if mask.dtype == np.float32:
        return mask > np.float32(0.5)
    assert num_classes is not None
    return np.stack([mask == p + 1 for p in range(num_classes - 1)], axis=1)


def index(mask, num_classes=None):
    """(M, P, H + 1) int32: the exclusive prefix over rows of each plane's per-row foreground count; entry H is the total"""
    fg = planes(mask, num_classes)
    counts = fg.sum(axis=3, dtype=np.int64)
    out = np.zeros(counts.shape[:2] + (counts.shape[2] + 1,), dtype=np.int64)
    out[:, :, 1:] = np.cumsum(counts, axis=2)
    return out.astype(np.int32)


def pick(u, n):
    return min(n - 1, int(np.floor(np.float64(np.float32(u)) * np.float64(n))))


def anchor(u, jitter, n):
    """patch row / column at which the chosen pixel lands: float64, every operation rounded"""
    t = (np.float64(np.float32(u)) - np.float64(0.5)) * np.float64(np.float32(jitter))
    return min(n - 1, int(np.floor((np.float64(0.5) + t) * np.float64(n))))


def kth_pixel(idx_plane, plane, rank):
    """(py, px) of the rank-th foreground pixel of a (H, W) bool plane in row-major order, the way the kernel finds it: the last
    row whose prefix is <= rank, then the (rank - prefix)-th set pixel of that row"""
    H = plane.shape[0]
    lo, hi = 0, H - 1
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if idx_plane[mid] <= rank:
            lo = mid
        else:
            hi = mid - 1
    cols = np.flatnonzero(plane[lo])
    return lo, int(cols[rank - int(idx_plane[lo])])


def draw(u, idx, fg, M, H, W, h, w, pos, jitter, indices=None):
    """coords (B, 4) int32 [m, y0, x0, plane or -1].  u (B, 8) float32; idx (M, P, H + 1) and fg (M, P, H, W) bool, or None
    without a mask; indices (B,) or None"""
    u = np.asarray(u, dtype=np.float32)
    B = u.shape[0]
    P = 0 if idx is None else idx.shape[1]
    out = np.zeros((B, 4), dtype=np.int32)
    for b in range(B):
        if indices is not None:
            m = int(indices[b])
            if not 0 <= m < M:
                out[b] = (-1, 0, 0, -1)
                continue
        else:
            m = pick(u[b, 0], M)
        y0, x0, plane = pick(u[b, 4], H - h + 1), pick(u[b, 5], W - w + 1), -1
        if P > 0 and u[b, 1] < np.float32(pos):
            present = [p for p in range(P) if idx[m, p, H] > 0]
            if present:
                plane = present[pick(u[b, 2], len(present))]
                rank = pick(u[b, 3], int(idx[m, plane, H]))
                py, px = kth_pixel(idx[m, plane], fg[m, plane], rank)
                ry, rx = anchor(u[b, 4], jitter, h), anchor(u[b, 5], jitter, w)
                y0 = min(max(py - ry, 0), H - h)
                x0 = min(max(px - rx, 0), W - w)
        out[b] = (m, y0, x0, plane)
    return out


def norm_of(mean, std):
    """(2, C) float32 [scale, shift]: scale = 1 / (255 std), shift = -mean / std, in float64 and rounded once"""
    mu, sd = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    return np.stack([1.0 / (255.0 * sd), -mu / sd]).astype(np.float32)


def cut(image, mask, coords, h, w, norm=None):
    """(image_out float64, mask_out): the windows of `coords`; fp32 pictures and masks are copied, uint8 pictures become
    v * scale[c] + shift[c] in float64 (the kernel's fused multiply-add is within half an ulp of it); m = -1 gives zeros"""
    image = np.asarray(image)
    B, C = coords.shape[0], image.shape[1]
    out = np.zeros((B, C, h, w), dtype=np.float64)
    mout = None if mask is None else np.zeros((B,) + mask.shape[1:-2] + (h, w), dtype=mask.dtype)
    for b, (m, y0, x0, _) in enumerate(coords):
        if m < 0:
            continue
        win = image[m, :, y0:y0 + h, x0:x0 + w].astype(np.float64)
        if image.dtype == np.uint8 and norm is not None:
            nrm = np.asarray(norm, dtype=np.float64).reshape(2, C)
            win = win * nrm[0][:, None, None] + nrm[1][:, None, None]
        out[b] = win
        if mask is not None:
            mout[b] = mask[m, ..., y0:y0 + h, x0:x0 + w]
    return out, mout
