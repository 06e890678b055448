"""The definition of unet_zoo_amd.LovaszLoss restated on the CPU in float64: segments of (error, membership bit),
ranks from a stable descending sort, the Jaccard differences along the ranks, and the gradients by torch autograd through the
fixed permutation.  tests/test_lovasz_loss.py pins it against Berman's published form, the closed-form weights, a brute-force
Jaccard and hand-derived segments; tests/test_lovasz_loss_gpu.py compares the kernels with it.  Nothing here touches the
library."""
import torch

import boundary_ref as BR  # tests/boundary_ref.py: the base criteria in float64 (pytest puts this directory on sys.path)
import multiclass_ref as MR


# ------------------------------------------------------------------------------------------------------------- one segment list
def ranks_of(e: torch.Tensor) -> torch.Tensor:
    """(S, L) errors -> (S, L) int64 ranks: descending e, ties by ascending position, -1 where e <= 0 (or NaN)"""
    e = e.detach()
    order = torch.sort(e, dim=1, descending=True, stable=True).indices
    ranks = torch.empty_like(order)
    ranks.scatter_(1, order, torch.arange(e.shape[1]).expand_as(order))
    return torch.where(e > 0, ranks, torch.full_like(ranks, -1))      # the unranked sort behind every ranked element


def order_of(ranks: torch.Tensor) -> torch.Tensor:
    """the permutation that lists the ranked elements by rank, then the unranked ones by position"""
    L = ranks.shape[1]
    key = torch.where(ranks >= 0, ranks, L + torch.arange(L).expand_as(ranks))
    return torch.sort(key, dim=1, stable=True).indices


def weights_sorted(b_sorted: torch.Tensor, G: torch.Tensor) -> torch.Tensor:
    """g = J_r - J_{r-1}, J_r = 1 - (G - c) / (G + n), J_{-1} = 0, along sorted membership bits (S, L); G (S, 1)"""
    b = b_sorted.double()
    c = b.cumsum(1)
    n = torch.arange(1, b.shape[1] + 1, dtype=torch.float64) - c
    J = 1.0 - (G - c) / (G + n)            # G + n >= 1: rank 0 has c = 1 (G >= 1) or n = 1
    return torch.cat([J[:, :1], J[:, 1:] - J[:, :-1]], dim=1)


def weights_closed_form(b_sorted: torch.Tensor, G: torch.Tensor) -> torch.Tensor:
    """the same from the integers: 1 / (G + n) for a member, (G - c) / ((G + n - 1)(G + n)) otherwise, 1 at rank 0 if G = 0"""
    b = b_sorted.double()
    c = b.cumsum(1)
    n = torch.arange(1, b.shape[1] + 1, dtype=torch.float64) - c
    Gn = G + n
    other = (G - c) / torch.where(Gn > 1, (Gn - 1) * Gn, torch.ones_like(Gn))
    g = torch.where(b > 0, 1.0 / Gn, other)
    first = torch.zeros_like(g)
    first[:, 0] = 1.0
    return torch.where((G == 0).expand_as(g), first, g)


def segment_values(e: torch.Tensor, b: torch.Tensor, ranks: torch.Tensor = None):
    """(L_s of every segment (differentiable in e), ranks, g by POSITION) for errors e (S, L) and membership bits b (S, L)"""
    if ranks is None:
        ranks = ranks_of(e)
    order = order_of(ranks)
    G = b.double().sum(1, keepdim=True)                   # members of the whole segment, ranked or not
    g = weights_sorted(torch.gather(b, 1, order), G) * (torch.gather(ranks, 1, order) >= 0)
    values = (torch.gather(e, 1, order) * g).sum(1)       # g is a constant: the gradient goes through the permutation
    return values, ranks, torch.zeros_like(g).scatter_(1, order, g)


# ------------------------------------------------------------------------------------------------------------ the two modes
def binary_segments(x: torch.Tensor, t: torch.Tensor, per_image: bool = True):
    """(e, b) as (S, L): e = 1 - x s, whose VALUE is the fp32 one of the definition (x s is exact, one rounding) and whose
    gradient is -s"""
    N, C, H, W = x.shape
    b = t > 0.5
    x32 = x.detach().float()
    e32 = torch.where(b, 1.0 - x32, 1.0 + x32)
    assert e32.dtype == torch.float32
    e64 = 1.0 - x.double() * torch.where(b, 1.0, -1.0).double()
    e = e64 + (e32.double() - e64).detach()
    if per_image:
        return e.reshape(N * C, H * W), b.reshape(N * C, H * W)
    return e.permute(1, 0, 2, 3).reshape(C, N * H * W), b.permute(1, 0, 2, 3).reshape(C, N * H * W)


def class_segments(x: torch.Tensor, y: torch.Tensor, per_image: bool = True, ignore_index: int = -100):
    """(e, b) as (S, L): e = |b - softmax(x)_c| at a valid pixel, 0 (unranked, no member) at an ignored one"""
    N, K, H, W = x.shape
    y = y.reshape(N, H, W).long()
    valid = MR.valid_mask(y, K, ignore_index)
    b = (y.unsqueeze(1) == torch.arange(K).reshape(1, K, 1, 1)) & valid.unsqueeze(1)
    e = (b.double() - torch.softmax(x.double(), dim=1)).abs() * valid.unsqueeze(1)
    if per_image:
        return e.reshape(N * K, H * W), b.reshape(N * K, H * W)
    return e.permute(1, 0, 2, 3).reshape(K, N * H * W), b.permute(1, 0, 2, 3).reshape(K, N * H * W)


def combine(values: torch.Tensor, b: torch.Tensor, C: int, present_only: bool) -> torch.Tensor:
    """V = mean over lines of the mean over the line's classes P; P: the classes with a member, or all C; empty P adds 0"""
    lines = values.shape[0] // C
    vals = values.reshape(lines, C)
    member = b.reshape(lines, C, -1).any(2)
    P = member if present_only else torch.ones_like(member)
    count = P.sum(1)
    per_line = (vals * P).sum(1) / count.clamp(min=1)
    return (per_line * (count > 0)).sum() / lines


def term(x, target, class_mode: bool, per_image: bool = True, classes: str = "present", ignore_index: int = -100, ranks=None):
    """(V, errors (S, L) float64, ranks (S, L) int64) of one map; `ranks` given: that permutation in place of the reference's"""
    if class_mode:
        e, b = class_segments(x, target, per_image, ignore_index)
    else:
        e, b = binary_segments(x, target, per_image)
    values, ranks, _ = segment_values(e, b, ranks)
    V = combine(values, b, x.shape[1], class_mode and classes == "present")
    return V, e.detach(), ranks


def reference(kind: str, maps, target, ow, weight: float, base_scale: float = 1.0, per_image: bool = True,
              classes: str = "present", base_kw=None, ranks=None):
    """(loss, [d loss / d map], V of every map, errors of every map, ranks of every map) of
    base_scale * sum_m ow_m base(map_m) + weight * sum_m ow_m V_m in float64; `ranks`: per map, ranks to use"""
    base_kw = dict(base_kw or {})
    cls = kind == "multiclass"
    ignore = base_kw.get("ignore_index", -100)
    leaves = [m.detach().double().requires_grad_(True) for m in maps]
    res = [term(v, target, cls, per_image, classes, ignore, None if ranks is None else ranks[i]) for i, v in enumerate(leaves)]
    base = sum(w * BR.base_map(kind, v, target, **base_kw) for w, v in zip(ow, leaves))
    loss = base_scale * base + weight * sum(w * r[0] for w, r in zip(ow, res))
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [torch.zeros_like(l) if g is None else g for l, g in zip(leaves, grads)]
    return loss.detach(), grads, [r[0].detach() for r in res], [r[1] for r in res], [r[2] for r in res]


# ---------------------------------------------------------------------------------- the cases of tests/test_lovasz_loss_gpu.py
# (here so that tests/test_lovasz_loss.py can hold torch's own float32 evaluation of the same inputs against the same bounds)
SHAPES = [(1, 1, 4, 4), (3, 1, 17, 23), (5, 1, 64, 48), (2, 3, 33, 20)]
REGION_KW = dict(alpha=0.5, beta=0.5, smooth=0.5)                          # RegionLoss.dice()
FOCAL_KW = dict(alpha=0.7, beta=0.3, gamma=4 / 3, smooth=1e-3, pos_weight=2.5)
CLASS_KW = dict(w_ce=0.4, w_dice=0.6, smooth=1.0, include_background=True, reduce="image")


def make_inputs(shape, seed=0):
    """as tests/test_region_loss_gpu.py: x = 3 randn, t = rand > 0.7; image 1: empty target; image 2 (N > 2): all foreground"""
    g = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(shape, generator=g)
    t = (torch.rand(shape, generator=g) > 0.7).float()
    if shape[0] > 1:
        t[1] = 0.0
    if shape[0] > 2:
        t[2] = 1.0
        x[2] = x[2].abs() + 2.0
    return x, t


def make_tied_inputs(shape, seed=5):
    """logits snapped to multiples of 0.25 (exact in bf16 too for |x| < 64): hundreds of equal errors"""
    x, t = make_inputs(shape, seed)
    return (x * 4.0).round() / 4.0, t


def make_spread_inputs(shape, seed=6):
    """randn * 10 ** uniform(-3, 6): the keys spread over the exponent range, every digit pass of the sort has work"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * 10.0 ** (torch.rand(shape, generator=g) * 9.0 - 3.0)
    return x, (torch.rand(shape, generator=g) > 0.6).float()


def make_labels(N, K, H, W, seed=0):
    """blocky labels 0 .. K-1 with an ignored stripe (-100), out-of-range labels (K + 3, -7) and one image without class 1"""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, K, (N, (H + 3) // 4, (W + 3) // 4), generator=g)
    y = coarse.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :H, :W].contiguous()
    y[:, H // 3, :] = -100
    y[0, 0, 0] = K + 3
    y[-1, H - 1, W // 2] = -7
    y[-1][y[-1] == 1] = 2
    return y


def make_class_inputs(K, N=3, H=33, W=20):
    g = torch.Generator().manual_seed(K)
    return 2.0 * torch.randn(N, K, H, W, generator=g), make_labels(N, K, H, W, seed=K)


def term_float32(x, target, class_mode, per_image=True, classes="present", ignore_index=-100):
    """(V, dV/dx) evaluated by torch in FLOAT32 throughout, with the float64 reference's ranks (the permutation is not what is
    being measured): how far a plain float32 evaluation is from the float64 one, to judge the bounds of the GPU tests by"""
    leaf = x.detach().float().requires_grad_(True)
    if class_mode:
        N, K, H, W = x.shape
        y = target.reshape(N, H, W).long()
        valid = MR.valid_mask(y, K, ignore_index)
        b = (y.unsqueeze(1) == torch.arange(K).reshape(1, K, 1, 1)) & valid.unsqueeze(1)
        e = (b.float() - torch.softmax(leaf, dim=1)).abs() * valid.unsqueeze(1)
        ranks = ranks_of(class_segments(x, target, per_image, ignore_index)[0])
    else:
        N, K, H, W = x.shape
        b = target > 0.5
        e = torch.where(b, 1.0 - leaf, 1.0 + leaf)
        ranks = ranks_of(binary_segments(x, target, per_image)[0])
    if per_image:
        e, b = e.reshape(N * K, H * W), b.reshape(N * K, H * W)
    else:
        e, b = e.permute(1, 0, 2, 3).reshape(K, N * H * W), b.permute(1, 0, 2, 3).reshape(K, N * H * W)
    order = order_of(ranks)
    G = b.double().sum(1, keepdim=True)
    g = (weights_closed_form(torch.gather(b, 1, order), G) * (torch.gather(ranks, 1, order) >= 0)).float()
    values = (torch.gather(e, 1, order) * g).sum(1)
    V = combine(values, b, K, class_mode and classes == "present")
    assert V.dtype == torch.float32
    (grad,) = torch.autograd.grad(V, leaf)
    return V.detach(), grad


def class_grad_float32_top(x, y, per_image=True, classes="present", ignore_index=-100):
    """dV/dx of the class mode in FLOAT32 in the form the kernel takes: dV/dx_k = p_k (d_k - sum_c p_c d_c), but for the class
    `top` of the largest logit -- the only one whose p can be near 1, where that difference cancels -- as
    p_top (d_top (1 - p_top) - sum_{c != top} p_c d_c) with 1 - p_top = sum_{c != top} p_c"""
    N, K, H, W = x.shape
    e, b = class_segments(x, y, per_image, ignore_index)
    _, ranks, g = segment_values(e, b)
    lines = e.shape[0] // K
    member = b.reshape(lines, K, -1).any(2)
    P = member if classes == "present" else torch.ones_like(member)
    share = (P / (lines * P.sum(1, keepdim=True).clamp(min=1))).reshape(lines * K, 1)
    d = (torch.where(b, -g, g) * share).float()                                # sign(p - b) g / (lines |P|), by position
    d = d.reshape(N, K, H, W) if per_image else d.reshape(K, N, H, W).permute(1, 0, 2, 3)
    p = torch.softmax(x.float(), dim=1)
    top = torch.zeros_like(p, dtype=torch.bool).scatter_(1, x.argmax(1, keepdim=True), True)
    pd_rest = (p * d * ~top).sum(1, keepdim=True)
    p_top, d_top = (p * top).sum(1, keepdim=True), (d * top).sum(1, keepdim=True)
    q_top = (p * ~top).sum(1, keepdim=True)
    t = torch.where(top, d_top * q_top - pd_rest, d - (p_top * d_top + pd_rest))
    grad = p * t
    assert grad.dtype == torch.float32
    return grad
