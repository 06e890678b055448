"""The surface-distance metrics of unet_zoo_amd.SurfaceMetrics restated in numpy (float64, brute force): what the GPU tests
compare against, pinned to scipy + numpy.percentile by tests/test_surface_metrics.py.

Definition (medpy's hd / hd95 / assd in 2D, connectivity 1; A the prediction, B the target):
    S(X)    = pixels of X with a 4-neighbour outside X, outside the picture counting as outside X
    d2(p,S) = min over s in S of (pi - si)^2 + (pj - sj)^2                      (an integer)
    D       = sorted({d2(p, S(B)) : p in S(A)} + {d2(p, S(A)) : p in S(B)}),  n = |S(A)| + |S(B)|
    hd      = spacing sqrt(D[-1])
    hdq     = spacing (lo + f (hi - lo)),  r = (n - 1) (q / 100.0), k = floor(r), f = r - k, lo = sqrt(D[k]),
              hi = sqrt(D[min(k + 1, n - 1)])
    assd    = spacing / 2 (mean sqrt(D_AB) + mean sqrt(D_BA))
    state   = 0 both non-empty, 1 A empty, 2 B empty, 3 both empty; the values and the d2 statistics are 0 unless state = 0
"""
import math

import numpy as np


def surface(mask: np.ndarray) -> np.ndarray:
    """the pixels of a 2D boolean mask with a 4-neighbour outside it"""
    m = np.pad(np.asarray(mask, dtype=bool), 1)
    inner = m[:-2, 1:-1] & m[2:, 1:-1] & m[1:-1, :-2] & m[1:-1, 2:]
    return m[1:-1, 1:-1] & ~inner


def min_d2(p: np.ndarray, s: np.ndarray) -> np.ndarray:
    """for every point of p (n, 2) the smallest squared distance to a point of s (m, 2), int64; in blocks"""
    out = np.empty(len(p), dtype=np.int64)
    step = max(1, (1 << 22) // max(1, len(s)))
    for a in range(0, len(p), step):
        d = p[a:a + step, None, :].astype(np.int64) - s[None, :, :].astype(np.int64)
        out[a:a + step] = (d * d).sum(-1).min(1)
    return out


def pair(A: np.ndarray, B: np.ndarray, q: float = 95.0, spacing: float = 1.0):
    """((hd, hdq, assd) in float64, the int64 statistics row |S(A)|, |S(B)|, max d2, D_(k), D_(k+1), state, |A|, |B|)"""
    A, B = np.asarray(A, dtype=bool), np.asarray(B, dtype=bool)
    sa, sb = np.argwhere(surface(A)), np.argwhere(surface(B))
    na, nb = int(A.sum()), int(B.sum())
    state = (1 if na == 0 else 0) | (2 if nb == 0 else 0)
    if state:
        return (0.0, 0.0, 0.0), np.array([len(sa), len(sb), 0, 0, 0, state, na, nb], dtype=np.int64)
    dab, dba = min_d2(sa, sb), min_d2(sb, sa)
    D = np.sort(np.concatenate([dab, dba]))
    n = len(D)
    r = (n - 1) * (q / 100.0)
    k = int(math.floor(r))
    f = r - k
    k1 = min(k + 1, n - 1)
    lo, hi = math.sqrt(int(D[k])), math.sqrt(int(D[k1]))
    hd = spacing * math.sqrt(int(D[-1]))
    hdq = spacing * (lo + f * (hi - lo))
    assd = spacing * 0.5 * (np.sqrt(dab.astype(np.float64)).mean() + np.sqrt(dba.astype(np.float64)).mean())
    return (hd, hdq, float(assd)), np.array([len(sa), len(sb), int(D[-1]), int(D[k]), int(D[k1]), 0, na, nb], dtype=np.int64)


def binary(logits: np.ndarray, target: np.ndarray, q: float = 95.0, spacing: float = 1.0):
    """(out (N, C, 3) float64, stats (N, C, 8) int64) of (N, C, H, W) logits against (N, C, H, W) float maps"""
    N, C = logits.shape[:2]
    out, stats = np.zeros((N, C, 3)), np.zeros((N, C, 8), dtype=np.int64)
    for n in range(N):
        for c in range(C):
            out[n, c], stats[n, c] = pair(logits[n, c] > 0, target[n, c] > 0.5, q, spacing)
    return out, stats


def classes(logits: np.ndarray, labels: np.ndarray, q: float = 95.0, spacing: float = 1.0, first_class: int = 1,
            ignore_index: int = -100):
    """(out (N, P, 3), stats (N, P, 8)) of (N, K, H, W) logits against (N, H, W) class indices, P = K - first_class"""
    N, K = logits.shape[:2]
    pred = np.argmax(logits, axis=1)                 # the first of equal maxima
    valid = (labels >= 0) & (labels < K) & (labels != ignore_index)
    P = K - first_class
    out, stats = np.zeros((N, P, 3)), np.zeros((N, P, 8), dtype=np.int64)
    for n in range(N):
        for p in range(P):
            c = first_class + p
            out[n, p], stats[n, p] = pair((pred[n] == c) & valid[n], (labels[n] == c) & valid[n], q, spacing)
    return out, stats


def blobs(shape, seed: int, count: int = 3, rmax: float = 0.3) -> np.ndarray:
    """a boolean (H, W) mask of `count` seeded discs / ellipses, some of which may touch the picture's edge"""
    H, W = shape
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros(shape, dtype=bool)
    for _ in range(count):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        ry, rx = rng.uniform(1.0, max(1.5, rmax * H)), rng.uniform(1.0, max(1.5, rmax * W))
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return m


def ulp32(x) -> np.ndarray:
    """the spacing of float32 at |x| (of the smallest normal number below it)"""
    a = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), float(np.finfo(np.float32).tiny)).astype(np.float32)
    return np.spacing(a).astype(np.float64)
