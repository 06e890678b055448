"""The definition of unet_zoo_amd.BoundaryLoss restated on the CPU: the signed squared distance transform from
scipy.ndimage.distance_transform_edt (integers), the distance map, and the boundary term with its gradients by torch autograd
in float64.  tests/test_boundary_loss.py pins the transform against a brute force over all pixel pairs and hand-derived
cases; tests/test_boundary_loss_gpu.py compares the kernels with it.  Nothing here touches the library."""
import numpy as np
import torch
import torch.nn.functional as F
from scipy import ndimage as ndi

import multiclass_ref as MR  # tests/multiclass_ref.py (pytest puts this directory on sys.path)


# ------------------------------------------------------------------------------------------------------------ the transform
def sd2_plane(G: np.ndarray) -> np.ndarray:
    """signed squared distance of one boolean plane, int64: +d2 to G outside, -d2 to the complement inside; 0 for an empty or
    a full plane.  d2 is an integer (a sum of two squares) and edt returns its float64 square root: rint(edt ** 2) is exact"""
    G = np.asarray(G, dtype=bool)
    if not G.any() or G.all():
        return np.zeros(G.shape, dtype=np.int64)
    out = np.rint(ndi.distance_transform_edt(~G) ** 2).astype(np.int64)
    inside = np.rint(ndi.distance_transform_edt(G) ** 2).astype(np.int64)
    return np.where(G, -inside, out)


def sd2_brute(G: np.ndarray) -> np.ndarray:
    """the definition itself: a minimum over all pixel pairs"""
    G = np.asarray(G, dtype=bool)
    H, W = G.shape
    if not G.any() or G.all():
        return np.zeros(G.shape, dtype=np.int64)
    ii, jj = np.mgrid[0:H, 0:W]
    d2 = (ii.reshape(-1, 1) - ii.reshape(1, -1)) ** 2 + (jj.reshape(-1, 1) - jj.reshape(1, -1)) ** 2      # (HW, HW)
    g = G.reshape(-1)
    big = np.iinfo(np.int64).max
    to_g = np.where(g[None, :], d2, big).min(1)
    to_c = np.where(~g[None, :], d2, big).min(1)
    return np.where(g, -to_c, to_g).reshape(H, W).astype(np.int64)


def planes_binary(target) -> np.ndarray:
    """(N, C, H, W) float target -> (N C, H, W) boolean planes G = target > 0.5"""
    t = np.asarray(target)
    return (t > 0.5).reshape((-1,) + t.shape[-2:])


def class_set(K: int, include_background: bool):
    return list(range(0 if include_background else 1, K))


def planes_class(y, K: int, include_background: bool = False, ignore_index: int = -100) -> np.ndarray:
    """(N, H, W) labels -> (N |Cset|, H, W) boolean planes G_c = (y == c); an ignored pixel is in none"""
    y = np.asarray(y).reshape((-1,) + tuple(np.asarray(y).shape[-2:]))
    valid = (y != ignore_index) & (y >= 0) & (y < K)
    return np.stack([(y[n] == c) & valid[n] for n in range(y.shape[0]) for c in class_set(K, include_background)])


def sd2_planes(planes: np.ndarray) -> np.ndarray:
    return np.stack([sd2_plane(p) for p in planes])


def phi_of(sd2, spacing: float = 1.0) -> np.ndarray:
    """the distance map (float64) of integer sd2"""
    s = np.asarray(sd2, dtype=np.float64)
    return np.where(s > 0, spacing * np.sqrt(np.abs(s)), np.where(s < 0, -spacing * (np.sqrt(np.abs(s)) - 1.0), 0.0))


def phi_kervadec(G: np.ndarray, spacing: float = 1.0) -> np.ndarray:
    """Kervadec's one_hot2dist for one plane: edt(~G) ~G - (edt(G) - 1) G; zeros for an empty plane -- and, by this project's
    convention, for a full one"""
    G = np.asarray(G, dtype=bool)
    if not G.any() or G.all():
        return np.zeros(G.shape)
    return ndi.distance_transform_edt(~G, sampling=spacing) * ~G - (ndi.distance_transform_edt(G, sampling=spacing) - spacing) * G


# ------------------------------------------------------------------------------------------------- the term and its gradients
def term_binary(x: torch.Tensor, phi: torch.Tensor) -> torch.Tensor:
    """B = sum sigmoid(x) phi / (N C H W); phi (N C, H, W)"""
    return (torch.sigmoid(x.double()) * phi.reshape(x.shape)).sum() / x.numel()


def term_class(x: torch.Tensor, y: torch.Tensor, phi: torch.Tensor, include_background: bool = False, ignore_index: int = -100) -> torch.Tensor:
    """B = sum over n, c in Cset, valid pixels of softmax(x)_c phi_c / (N |Cset| H W); phi (N |Cset|, H, W)"""
    N, K, H, W = x.shape
    cs = class_set(K, include_background)
    y = y.reshape(N, H, W).long()
    valid = MR.valid_mask(y, K, ignore_index).double()
    p = torch.softmax(x.double(), dim=1)[:, cs[0]:]
    return (p * phi.reshape(N, len(cs), H, W) * valid.unsqueeze(1)).sum() / (N * len(cs) * H * W)


def region_map(x, t, w_bce=1.0, w_region=1.0, alpha=0.5, beta=0.5, smooth=1.0, gamma=1.0, reduce="image", pos_weight=None):
    """RegionLoss's documented formula for one map, float64"""
    x, t = x.double(), t.double()
    pw = 1.0 if pos_weight is None else pos_weight
    p = torch.sigmoid(x)
    bce = (-(pw * t * F.logsigmoid(x) + (1 - t) * F.logsigmoid(-x))).mean()
    groups = {"batch": 1, "image": x.shape[0], "channel": x.shape[0] * x.shape[1]}[reduce]
    pf, tf = p.reshape(groups, -1), t.reshape(groups, -1)
    I, S, T = (pf * tf).sum(1), pf.sum(1), tf.sum(1)
    q = 1 - (I + smooth) / (I + alpha * (S - I) + beta * (T - I) + smooth)
    return w_bce * bce + w_region * (q if gamma == 1 else q ** gamma).mean()


def base_map(kind: str, x, t, **kw):
    """the base criterion of one map in float64: "bce_dice" (BCEWithLogits, mean), "region" or "multiclass" """
    if kind == "bce_dice":
        return F.binary_cross_entropy_with_logits(x.double(), t.double())
    if kind == "region":
        return region_map(x, t, **kw)
    if kind == "multiclass":
        return MR.loss_map(x, t, **kw)
    raise ValueError(kind)


def reference(kind: str, maps, target, ow, weight: float, base_scale: float = 1.0, spacing: float = 1.0,
              include_background: bool = False, base_kw=None):
    """(loss, [d loss / d map], B of every map, sd2) of base_scale * sum_m ow_m base(map_m) + weight * sum_m ow_m B_m in
    float64, phi computed once from the target"""
    base_kw = dict(base_kw or {})
    cls = kind == "multiclass"
    ignore = base_kw.get("ignore_index", -100)
    leaves = [m.detach().double().requires_grad_(True) for m in maps]
    if cls:
        K = maps[0].shape[1]
        sd2 = sd2_planes(planes_class(target.numpy(), K, include_background, ignore))
    else:
        sd2 = sd2_planes(planes_binary(target.numpy()))
    phi = torch.from_numpy(phi_of(sd2, spacing))
    terms = [term_class(v, target, phi, include_background, ignore) if cls else term_binary(v, phi) for v in leaves]
    base = sum(w * base_map(kind, v, target, **base_kw) for w, v in zip(ow, leaves))
    loss = base_scale * base + weight * sum(w * b for w, b in zip(ow, terms))
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [torch.zeros_like(l) if g is None else g for l, g in zip(leaves, grads)]
    return loss.detach(), grads, [b.detach() for b in terms], sd2
