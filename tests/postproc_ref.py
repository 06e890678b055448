"""unet_zoo_amd.MaskPostprocess restated with numpy / scipy.ndimage: what the GPU tests compare against, pinned to answers
derived by hand by tests/test_postproc.py.  Also here: the adversarial planes of those tests (the planes of
tests/postproc_core_main.cpp, built the same way).

Per plane, in this order:
    1. fill_holes: ndimage.binary_fill_holes (default structure: the cross, whatever the connectivity)
    2. ndimage.label with the cross (connectivity 1) or the 3 x 3 square (2); scipy numbers components in raster order of
       their first pixel, so a component's root (its smallest index i W + j) is where its number first appears
    3. drop area < min_area
    4. keep_largest = k > 0: the first k of a stable sort by (-area, root)
    mask, labels = ndimage.label(mask, structure)[0], stats row, comps records, class_map
"""
import numpy as np
from scipy import ndimage as ndi

CROSS = ndi.generate_binary_structure(2, 1)
SQUARE = ndi.generate_binary_structure(2, 2)


def plane(p: np.ndarray, connectivity: int = 1, fill_holes: bool = False, min_area: int = 0, keep_largest: int = 0):
    """(mask uint8, labels int32, stats int64[8], comps int64[8, 8]) of one boolean plane"""
    p = np.asarray(p, dtype=bool)
    H, W = p.shape
    st = SQUARE if connectivity == 2 else CROSS
    filled = ndi.binary_fill_holes(p) if fill_holes else p
    lab, n = ndi.label(filled, structure=st)
    flat = lab.ravel()
    area = np.bincount(flat, minlength=n + 1)[1:]
    # first occurrence of every label in raster order: the root
    roots = np.full(n, H * W, dtype=np.int64)
    np.minimum.at(roots, flat[flat > 0] - 1, np.nonzero(flat > 0)[0])
    cand = [c for c in range(n) if area[c] >= min_area]
    order = sorted(cand, key=lambda c: (-int(area[c]), int(roots[c])))
    kept = order[:keep_largest] if keep_largest > 0 else order
    keep_flag = np.zeros(n + 1, dtype=bool)
    for c in kept:
        keep_flag[c + 1] = True
    mask = keep_flag[lab]
    labels = ndi.label(mask, structure=st)[0].astype(np.int32)
    stats = np.array([n, len(kept), int(filled.sum()), int(mask.sum()), int(filled.sum() - p.sum()),
                      int(area[order[0]]) if order else 0, 0, 0], dtype=np.int64)
    comps = np.zeros((8, 8), dtype=np.int64)
    for r, c in enumerate(kept[:8]):
        ii, jj = np.nonzero(lab == c + 1)
        comps[r] = [area[c], ii.min(), jj.min(), ii.max(), jj.max(), ii.sum(), jj.sum(), roots[c]]
    return mask.astype(np.uint8), labels, stats, comps


def _stack(planes, **kw):
    """planes: (N, P, H, W) boolean -> mask, labels, stats (N, P, 8), comps (N, P, 8, 8)"""
    N, P = planes.shape[:2]
    res = [[plane(planes[n, p], **kw) for p in range(P)] for n in range(N)]
    pick = lambda k: np.stack([np.stack([res[n][p][k] for p in range(P)]) for n in range(N)])
    return pick(0), pick(1), pick(2), pick(3)


def binary(x: np.ndarray, thr: float = 0.0, **kw):
    """(N, C, H, W) float32 maps, plane = x > thr (compared in float32, as the kernel does)"""
    return _stack(np.asarray(x, dtype=np.float32) > np.float32(thr), **kw)


def classes(x: np.ndarray, include_background: bool = False, **kw):
    """(N, K, H, W) float32 maps, plane c = (argmax_K == c), ties to the lowest index (numpy.argmax's rule); the fifth result
    is class_map (N, H, W) uint8"""
    x = np.asarray(x, dtype=np.float32)
    K = x.shape[1]
    first = 0 if include_background else 1
    am = x.argmax(1)
    planes = np.stack([am == c for c in range(first, K)], axis=1)
    mask, labels, stats, comps = _stack(planes, **kw)
    cmap = np.zeros(am.shape, dtype=np.uint8)
    for c in range(K - 1, first - 1, -1):                  # the lowest class last: it wins
        cmap[mask[:, c - first] != 0] = c
    own = np.zeros(am.shape, dtype=bool)
    for c in range(first, K):
        own |= (am == c) & (mask[:, c - first] != 0)
    cmap[own] = am[own]
    return mask, labels, stats, comps, cmap


# ---- planes ------------------------------------------------------------------------------------------------------------------
def blobs(shape, seed: int, sigma: float = 2.0, level: float = 0.0) -> np.ndarray:
    """smoothed seeded noise as float32 logits: `> level` gives blobs with holes and specks"""
    rng = np.random.RandomState(seed)
    x = ndi.gaussian_filter(rng.randn(*shape), sigma=(0,) * (len(shape) - 2) + (sigma, sigma))
    return ((x / x.std()) - level).astype(np.float32)


def adversarial(H: int = 33, W: int = 70):
    """name -> boolean plane; the planes of tests/postproc_core_main.cpp"""
    out = {}
    out["empty"] = np.zeros((H, W), dtype=bool)
    out["full"] = np.ones((H, W), dtype=bool)
    p = np.zeros((H, W), dtype=bool)
    p[0, 0] = p[0, -1] = p[-1, 0] = p[-1, -1] = True
    out["corners"] = p
    k = np.arange(150)
    out["row"] = (k % 7 != 3)[None, :]
    out["column"] = (k % 7 != 3)[:, None]
    i, j = np.mgrid[0:H, 0:W]
    out["serpentine"] = (i % 2 == 0) | (j == np.where((i // 2) % 2 == 0, W - 1, 0))
    p = np.zeros((H, W), dtype=bool)
    t, b, l, r = 0, H - 1, 0, W - 1
    while t <= b and l <= r:
        p[t, l:r + 1] = True
        p[t:b + 1, r] = True
        if b - t >= 2:
            p[b, l + 2:r + 1] = True
        if r - l >= 2:
            p[t + 2:b + 1, l + 2] = True
        t, b, l, r = t + 2, b - 2, l + 2, r - 2
        if t <= b and l <= r:
            p[t, l] = True
    out["spiral"] = p
    out["comb_last_row"] = (j % 2 == 0) | (i == H - 1)
    i3, j3 = np.mgrid[0:3, 0:130]
    out["comb_last_column"] = (i3 % 2 == 0) | (j3 == 129)
    out["checkerboard"] = (i + j) % 2 == 0
    p = np.zeros((H, W), dtype=bool)
    p[2:10, 3:20] = True
    p[10:20, 20:66] = True
    out["diagonal_touch"] = p
    return out


def squares(H, W, sizes, gap=2):
    """filled squares of the given side lengths from the top-left on, row after row, never touching"""
    p = np.zeros((H, W), dtype=bool)
    i0 = j0 = 1
    rowh = 0
    for s in sizes:
        if j0 + s + 1 > W:
            i0, j0, rowh = i0 + rowh + gap, 1, 0
        assert i0 + s < H, "squares do not fit"
        p[i0:i0 + s, j0:j0 + s] = True
        j0 += s + gap
        rowh = max(rowh, s)
    return p


def ring(p, i0, j0, i1, j1):
    """a one-pixel rectangular ring with corners (i0, j0), (i1, j1), drawn into p"""
    p[i0, j0:j1 + 1] = p[i1, j0:j1 + 1] = True
    p[i0:i1 + 1, j0] = p[i0:i1 + 1, j1] = True
    return p


def holes(H: int = 33, W: int = 70):
    """name -> boolean plane for the hole cases"""
    z = lambda: np.zeros((H, W), dtype=bool)
    out = {"ring": ring(z(), 3, 4, 20, 40)}
    out["ring_in_ring"] = ring(ring(z(), 2, 2, 30, 60), 8, 10, 22, 40)
    p = ring(z(), 3, 4, 20, 40)
    p[3, 4] = False                                         # the corner: the gap is diagonal only
    out["diagonal_gap"] = p
    p = ring(z(), 3, 4, 20, 40)
    p[3, 17] = False
    out["straight_gap"] = p
    p = z()
    p[0:12, 10] = p[0:12, 30] = True
    p[11, 10:31] = True
    out["u_at_edge"] = p
    p = ring(z(), 5, 5, 15, 25)                             # a ring with an island inside it: filling joins them
    p[9:12, 12:16] = True
    out["fill_joins"] = p
    return out
