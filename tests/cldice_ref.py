"""The definition of unet_zoo_amd.ClDiceLoss restated with torch on the CPU in float64: the soft skeleton from
max_pool2d, torch.min and relu, the centreline Dice per segment, and the gradients by torch autograd -- whose subgradients at
ties (relu'(0) = 0, the first maximum of a pooling window in row-major order, half to each side of an equal torch.min) are the
definition's.  tests/test_cldice_loss.py pins those; tests/test_cldice_loss_gpu.py compares the kernels with this file.
Nothing here touches the library.

Ties: probabilities are computed from the UNIQUE logits and gathered back, so equal logits give bit-equal probabilities
whatever torch's vectorised sigmoid does with the lanes and the tail of a row."""
import torch
import torch.nn.functional as F

import boundary_ref as BR  # tests/boundary_ref.py: the base criteria in float64 (pytest puts this directory on sys.path)
import multiclass_ref as MR


# ------------------------------------------------------------------------------------------------------------ the soft skeleton
def erode(a: torch.Tensor) -> torch.Tensor:
    """min(v, h) on (N, C, H, W): v, h the minima of the vertical and the horizontal 3-window, clipped to the picture"""
    v = -F.max_pool2d(-a, (3, 1), (1, 1), (1, 0))
    h = -F.max_pool2d(-a, (1, 3), (1, 1), (0, 1))
    return torch.min(v, h)


def dilate(a: torch.Tensor) -> torch.Tensor:
    return F.max_pool2d(a, (3, 3), (1, 1), (1, 1))


def soft_open(a: torch.Tensor) -> torch.Tensor:
    return dilate(erode(a))


def skel(a: torch.Tensor, iterations: int) -> torch.Tensor:
    s = F.relu(a - soft_open(a))
    for _ in range(iterations):
        a = erode(a)
        d = F.relu(a - soft_open(a))
        s = s + F.relu(d - s * d)
    return s


# ------------------------------------------------------------------------------------------------------------ the probabilities
def tied(x: torch.Tensor, fn, dfn) -> torch.Tensor:
    """fn(x) whose equal inputs give bit-equal outputs (evaluated once per unique value), with the derivative dfn of the value"""
    u, inv = torch.unique(x.detach(), return_inverse=True)
    val = fn(u)[inv]
    return val + dfn(val) * (x - x.detach())          # x - x.detach() is exactly 0: the value is val, the gradient dfn(val)


def sigmoid_tied(x: torch.Tensor) -> torch.Tensor:
    return tied(x, torch.sigmoid, lambda p: p * (1.0 - p))


def class_planes(x: torch.Tensor, y: torch.Tensor, include_background: bool, ignore_index: int, probs=None):
    """(p, t) of the classes that count, (N, K', H, W): softmax and one-hot with the invalid pixels zeroed in every plane;
    `probs` given (N, K, H, W): those in place of the softmax"""
    N, K, H, W = x.shape
    y = y.reshape(N, H, W).long()
    valid = MR.valid_mask(y, K, ignore_index).unsqueeze(1)
    p = (torch.softmax(x, dim=1) if probs is None else probs) * valid
    t = ((y.unsqueeze(1) == torch.arange(K).reshape(1, K, 1, 1)) & valid).to(x.dtype)
    c0 = 0 if include_background else 1
    return p[:, c0:], t[:, c0:]


# -------------------------------------------------------------------------------------------------------------------- the term
def cl_term(p: torch.Tensor, t: torch.Tensor, iterations: int, smooth: float, per_image: bool):
    """(V, skel(p), skel(t)) for planes p, t (N, C, H, W); skel(t) gets no gradient"""
    sp, st = skel(p, iterations), skel(t, iterations).detach()
    dims = (2, 3) if per_image else (0, 2, 3)
    tprec = ((sp * t).sum(dims) + smooth) / (sp.sum(dims) + smooth)
    tsens = ((st * p).sum(dims) + smooth) / (st.sum(dims) + smooth)
    cl = 1.0 - 2.0 * tprec * tsens / (tprec + tsens)
    return cl.mean(), sp, st


def term(x, target, class_mode: bool, iterations: int = 3, smooth: float = 1.0, per_image: bool = False,
         include_background: bool = False, ignore_index: int = -100):
    """(V, p, skel(p), skel(t)) of one map of logits x in x's dtype (the planes that count in the class mode)"""
    if class_mode:
        p, t = class_planes(x, target, include_background, ignore_index)
    else:
        p, t = sigmoid_tied(x), target.to(x.dtype)
    V, sp, st = cl_term(p, t, iterations, smooth, per_image)
    return V, p.detach(), sp.detach(), st


def reference(kind: str, maps, target, ow, weight: float, base_scale: float = 1.0, iterations: int = 3, smooth: float = 1.0,
              per_image: bool = False, include_background: bool = False, base_kw=None):
    """(loss, [d loss / d map], V of every map, p of every map, skel(p) of every map, skel(t)) of
    base_scale * sum_m ow_m base(map_m) + weight * sum_m ow_m V_m in float64"""
    base_kw = dict(base_kw or {})
    cls = kind == "multiclass"
    ignore = base_kw.get("ignore_index", -100)
    leaves = [m.detach().double().requires_grad_(True) for m in maps]
    res = [term(v, target, cls, iterations, smooth, per_image, include_background, ignore) for v in leaves]
    base = sum(w * BR.base_map(kind, v, target, **base_kw) for w, v in zip(ow, leaves))
    loss = base_scale * base + weight * sum(w * r[0] for w, r in zip(ow, res))
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [torch.zeros_like(l) if g is None else g for l, g in zip(leaves, grads)]
    return loss.detach(), grads, [r[0].detach() for r in res], [r[1] for r in res], [r[2] for r in res], res[0][3]


def class_term_from_probs(x, y, probs, iterations=3, smooth=1.0, per_image=False, include_background=True, ignore_index=-100):
    """(V, dV/dx) of the class mode in float64 evaluated FROM GIVEN probabilities (the device's own, whose exp is not the
    CPU's): V and g = dV/dp by autograd from `probs`, carried to the logits with the float64 Jacobian of the softmax,
    dV/dx_k = p_k (g_k - sum_c p_c g_c), and dropped at the invalid pixels"""
    N, K, H, W = x.shape
    leaf = probs.detach().double().requires_grad_(True)
    p, t = class_planes(x.double(), y, include_background, ignore_index, probs=leaf)
    V, _, _ = cl_term(p, t, iterations, smooth, per_image)
    (g,) = torch.autograd.grad(V, leaf)
    p64 = torch.softmax(x.double(), dim=1)
    valid = MR.valid_mask(y.reshape(N, H, W).long(), K, ignore_index).unsqueeze(1)
    grad = p64 * (g - (p64 * g).sum(1, keepdim=True)) * valid
    return V.detach(), grad


def term_float32(x, target, class_mode, iterations=3, smooth=1.0, per_image=False, include_background=False, ignore_index=-100):
    """(V, dV/dx) evaluated by torch in FLOAT32 throughout: how far a plain float32 evaluation is from the float64 one, to judge
    the bounds of the GPU tests by.  Only for tie-free inputs: float32 CPU torch is no comparator on ties."""
    leaf = x.detach().float().requires_grad_(True)
    if class_mode:
        p, t = class_planes(leaf, target, include_background, ignore_index)
    else:
        p, t = torch.sigmoid(leaf), target.float()
    V, _, _ = cl_term(p, t, iterations, smooth, per_image)
    assert V.dtype == torch.float32
    (grad,) = torch.autograd.grad(V, leaf)
    return V.detach(), grad


# ---------------------------------------------------------------------------------- the cases of tests/test_cldice_loss_gpu.py
# (here so that tests/test_cldice_loss.py can hold torch's own float32 evaluation of the same inputs against the same bounds)
REGION_KW = dict(alpha=0.5, beta=0.5, smooth=0.5)                          # RegionLoss.dice()
CLASS_KW = dict(w_ce=0.4, w_dice=0.6, smooth=1.0, include_background=True, reduce="image")
MIN_GAP = 1e-5        # between distinct probabilities of a plane: fp32 rounding (6e-8 near 1) cannot reorder or merge them


def bands(shape) -> torch.Tensor:
    """thin diagonal bands, 2-3 pixels wide: ((y + 2x) % 11 < 3) | ((3y - x) % 13 < 2); image 0 shifted, channels offset"""
    N, C, H, W = shape
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    t = torch.zeros(shape)
    for n in range(N):
        for c in range(C):
            ys, xs = yy + (4 if n == 0 else 0) + 5 * c, xx + 3 * c
            t[n, c] = ((((ys + 2 * xs) % 11) < 3) | (((3 * ys - xs) % 13) < 2)).float()
    return t


def plane_gap(p: torch.Tensor) -> float:
    """the smallest gap between distinct values inside one (H, W) plane, over all planes of (N, C, H, W)"""
    gap = float("inf")
    for plane in p.reshape((-1,) + p.shape[-2:]):
        u = torch.unique(plane)
        if len(u) > 1:
            gap = min(gap, (u[1:] - u[:-1]).min().item())
    return gap


def make_inputs(shape, seed=0):
    """target: thin bands; logits (2t - 1) 2 + noise replaced by their ranks INSIDE THE PLANE spread evenly over [-4, 4] (the
    morphology compares values of one plane only), each plane shifted by a fraction of the rank step so that all logits of the
    tensor are distinct.  Asserts: all logits distinct in fp32, distinct float64 probabilities of a plane >= MIN_GAP apart"""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    t = bands(shape)
    raw = ((2.0 * t - 1.0) * 2.0 + torch.randn(shape, generator=g).double()).reshape(N * C, H * W)
    ranks = torch.empty_like(raw)
    ranks.scatter_(1, torch.sort(raw, dim=1, stable=True).indices, torch.arange(H * W, dtype=torch.float64).expand(N * C, -1))
    step = 8.0 / max(H * W - 1, 1)
    x = -4.0 + step * ranks + (step / (2 * N * C)) * torch.arange(N * C, dtype=torch.float64).unsqueeze(1)
    x = x.reshape(shape).float()
    assert len(torch.unique(x)) == x.numel()
    assert plane_gap(torch.sigmoid(x.double())) >= MIN_GAP
    return x, t


def make_tied_inputs(shape, seed=0):
    """the same logits snapped to multiples of 1/8 and clamped to [-6, 6]: exact in bf16, at most 97 distinct values"""
    x, t = make_inputs(shape, seed)
    x = ((x * 8.0).round() / 8.0).clamp(-6.0, 6.0)
    assert torch.equal(x.bfloat16().float(), x)
    for plane in x.reshape((-1,) + x.shape[-2:]):         # equal values INSIDE a plane are what the windows meet
        counts = torch.unique(plane, return_counts=True)[1]
        assert counts[counts > 1].sum() >= 100
    assert plane_gap(sigmoid_tied(x.double())) >= MIN_GAP
    return x, t


def make_labels(N, K, H, W, seed=0):
    """thin bands of the classes 1 .. K-1 on background 0, an ignored stripe (-100), out-of-range labels (K + 3, -7) and the
    last image without class 1"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    y = torch.zeros(N, H, W, dtype=torch.int64)
    for n in range(N):
        band = (((yy + 2 * xx + 3 * n) % 11) < 3) | (((3 * yy - xx) % 13) < 2)
        cls = 1 + ((yy // 5 + xx // 7 + n) % (K - 1))
        y[n] = torch.where(band, cls, torch.zeros_like(cls))
    y[:, H // 3, :] = -100
    y[0, 0, 0] = K + 3
    y[-1, H - 1, W // 2] = -7
    y[-1][y[-1] == 1] = 2
    return y


def make_class_inputs(K, N=2, H=33, W=20, seed=0):
    """foreground probabilities p_1 .. p_(K-1) per pixel from independent rank grids (per plane, evenly over
    [0.02, 0.9] / (K - 1): sum < 1), p_0 = 1 - sum, x = log p.  Asserts the gaps of every foreground plane >= MIN_GAP, on the
    float64 softmax of the fp32 logits"""
    g = torch.Generator().manual_seed(seed + K)
    y = make_labels(N, K, H, W, seed)
    p = torch.zeros(N, K, H, W, dtype=torch.float64)
    for c in range(1, K):
        raw = (2.0 * (y == c).double() + torch.randn(N, H, W, generator=g).double()).reshape(N, H * W)
        ranks = torch.empty_like(raw)
        ranks.scatter_(1, torch.sort(raw, dim=1, stable=True).indices, torch.arange(H * W, dtype=torch.float64).expand(N, -1))
        p[:, c] = ((0.02 + 0.88 * ranks / (H * W - 1)) / (K - 1)).reshape(N, H, W)
    p[:, 0] = 1.0 - p[:, 1:].sum(1)
    assert p[:, 0].min() > 0.05
    x = p.log().float()
    assert plane_gap(torch.softmax(x.double(), dim=1)[:, 1:]) >= MIN_GAP
    assert (y == -100).any() and (y >= K).any() and (y < 0).any() and not (y[-1] == 1).any() and (y[0] == 1).any()
    return x, y
