"""Reference of sliding-window inference in plain float64 torch / numpy: the tile plan (MONAI's rule), the windows by slicing and
F.pad, and the weighted blend as a Python loop over the tiles.  The fp32-rounded weight tables are taken as given."""
import math

import numpy as np
import torch
import torch.nn.functional as F

MAX_COVER = 8


def plan(size: int, window: int, overlap: float) -> list:
    """tile starts along one axis, on the canvas of max(size, window) pixels"""
    D = max(size, window)
    step = max(int(window * (1 - overlap)), 1)
    n = 1 if D == window else math.ceil((D - window) / step) + 1
    return [min(i * step, D - window) for i in range(n)]


def cover(starts, window: int, size: int) -> np.ndarray:
    """tiles over each pixel of the canvas along one axis"""
    D = max(size, window)
    k = np.zeros(D, dtype=np.int64)
    for s in starts:
        k[s:s + window] += 1
    return k


def offsets(size: int, window: int):
    """(before, after): where the image lies on the canvas"""
    pad = max(window - size, 0)
    return pad // 2, pad - pad // 2


def canvas(x: torch.Tensor, window, pad_mode: str) -> torch.Tensor:
    th, tw = window
    (t, b), (l, r) = offsets(x.shape[2], th), offsets(x.shape[3], tw)
    if t + b + l + r == 0:
        return x
    return F.pad(x, (l, r, t, b), mode=pad_mode) if pad_mode == "reflect" else F.pad(x, (l, r, t, b))


def gather(x: torch.Tensor, ys, xs, window, pad_mode: str = "constant") -> torch.Tensor:
    """all tiles (N ny nx, C, th, tw) of x (N, C, H, W), tile t = (n ny + iy) nx + ix"""
    th, tw = window
    cv = canvas(x, window, pad_mode)
    return torch.stack([cv[n, :, y:y + th, x0:x0 + tw] for n in range(x.shape[0]) for y in ys for x0 in xs])


def blend(tiles: torch.Tensor, ys, xs, gh: torch.Tensor, gw: torch.Tensor, shape) -> torch.Tensor:
    """(N, C, H, W) float64 = sum w p / sum w in float64, w = max(gh[y'] gw[x'], 1e-3) from the fp32 tables as given"""
    N, C, H, W = shape
    T, _, th, tw = tiles.shape
    Dh, Dw = max(H, th), max(W, tw)
    w = torch.clamp(gh.double()[:, None] * gw.double()[None, :], min=float(np.float32(1e-3)))
    num = torch.zeros(N, C, Dh, Dw, dtype=torch.float64)
    den = torch.zeros(N, 1, Dh, Dw, dtype=torch.float64)
    t = 0
    for n in range(N):
        for y in ys:
            for x in xs:
                num[n, :, y:y + th, x:x + tw] += w * tiles[t].double()
                den[n, :, y:y + th, x:x + tw] += w
                t += 1
    assert t == T
    oy, ox = offsets(H, th)[0], offsets(W, tw)[0]
    return (num / den)[:, :, oy:oy + H, ox:ox + W]


def ulp_distance(got: torch.Tensor, ref64: torch.Tensor) -> float:
    """largest distance of fp32 `got` from the fp32-rounded float64 reference, in float32 ulp of the reference"""
    r32 = ref64.float()
    ulp = torch.from_numpy(np.spacing(np.abs(r32.numpy()))).double()
    return float(((got.cpu().double() - r32.double()).abs() / ulp).max())
