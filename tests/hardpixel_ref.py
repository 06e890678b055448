"""The definition of unet_zoo_amd.HardPixelLoss restated on the CPU in float64: the plain pixel losses, the focal
modulation, the kept count, the m-th largest value with its tie counts, the position-free tie weights, and the gradients by
torch autograd through the fixed weights.  Two entry points: `reference` is fully independent; given `losses` (the fp32
array a device wrote) it takes the kept set -- m, tau, the ties -- from THAT array and evaluates value and gradient in
float64 with it.  tests/test_hardpixel_loss.py pins it against plain torch; tests/test_hardpixel_loss_gpu.py compares the
kernels with it.  Nothing here touches the library."""
import math

import torch

import boundary_ref as BR  # tests/boundary_ref.py: the base criteria in float64 (pytest puts this directory on sys.path)
import multiclass_ref as MR


# ------------------------------------------------------------------------------------------------------------ the pixel losses
def pixel_losses(x, target, class_mode: bool, gamma: float = 0.0, ignore_index: int = -100, dtype=torch.float64):
    """(f, l, valid) in the f layout -- (N, C, H, W) in the binary mode, (N, H, W) in the class mode --, differentiable in x;
    f and l are 0 at a pixel that is in no segment"""
    x = x.to(dtype)
    if class_mode:
        N, K, H, W = x.shape
        y = target.reshape(N, H, W).long()
        valid = MR.valid_mask(y, K, ignore_index)
        ys = torch.where(valid, y, torch.zeros_like(y))
        l = torch.logsumexp(x, dim=1) - torch.gather(x, 1, ys.unsqueeze(1)).squeeze(1)
        l = l * valid
    else:
        s = torch.where(target > 0.5, 1.0, -1.0).to(dtype)
        l = torch.nn.functional.softplus(-s * x)
        valid = torch.ones_like(target, dtype=torch.bool)
    if gamma == 0:
        return l, l, valid
    q = -torch.expm1(-l)                                   # 1 - p_t
    return q ** gamma * l, l, valid


def fp32(v: float) -> float:
    return torch.tensor(v, dtype=torch.float32).item()


def threshold(max_prob) -> float:
    """-log(max_prob) with max_prob and the result rounded to fp32, as the descriptor holds them; +inf: off"""
    return math.inf if not max_prob else fp32(-math.log(fp32(max_prob)))


def kept_count(n: int, c: int, keep: float, min_kept: int) -> int:
    """m = max(k, c), k = clamp(max(min_kept, ceil(keep n)), 1, n) with the product keep n in fp32 (one rounding)"""
    if n == 0:
        return 0
    k = int(torch.ceil(torch.tensor(keep, dtype=torch.float32) * torch.tensor(float(n), dtype=torch.float32)).item())
    return max(min(max(k, min_kept, 1), n), c)


def select(f: torch.Tensor, m: int):
    """(tau, n_above, n_tie) of the valid values f (1-D): tau the m-th largest"""
    tau = torch.sort(f, descending=True).values[m - 1]
    return tau, int((f > tau).sum()), int((f == tau).sum())


def weights_of(fsel, lsel, valid, S: int, keep: float, min_kept: int = 0, max_prob=None):
    """(w, rows): the weight of every pixel as (S, L) float64 -- 1 / m above tau, (m - n_above) / (n_tie m) at tau, 0
    elsewhere and at invalid pixels -- and per segment (m, n_above, n_tie, tau); fsel is what is selected on, lsel the plain
    loss that the count c looks at"""
    fsel, lsel, valid = fsel.detach().reshape(S, -1), lsel.detach().reshape(S, -1), valid.reshape(S, -1)
    thr = threshold(max_prob)
    w = torch.zeros(fsel.shape, dtype=torch.float64)
    rows = []
    for s in range(S):
        v = valid[s]
        n = int(v.sum())
        c = int((lsel[s][v] > thr).sum())
        m = kept_count(n, c, keep, min_kept)
        if m == 0:
            rows.append((0, 0, 0, fsel.new_zeros(())))
            continue
        tau, above, tie = select(fsel[s][v], m)
        w[s] = (v & (fsel[s] > tau)).double() * (1.0 / m) + (v & (fsel[s] == tau)).double() * ((m - above) / (tie * m))
        rows.append((m, above, tie, tau))
    return w, rows


def selection_of(losses32: torch.Tensor, valid, S: int, keep: float, min_kept: int = 0, max_prob=None) -> torch.Tensor:
    """(S, 4) int64 -- m, n_above, n_tie, the bit pattern of tau -- of an fp32 array of f (gamma = 0 where max_prob is set: c
    is counted on the array itself)"""
    assert losses32.dtype == torch.float32
    _, rows = weights_of(losses32, losses32, valid, S, keep, min_kept, max_prob)
    return torch.tensor([[m, a, t, int(tau.float().view(torch.int32))] for m, a, t, tau in rows], dtype=torch.int64)


def term(x, target, class_mode: bool, keep: float = 0.1, min_kept: int = 0, max_prob=None, gamma: float = 0.0,
         per_image: bool = False, ignore_index: int = -100, losses=None, dtype=torch.float64, weights=None):
    """(V, f, rows, w) of one map; `losses` (fp32, the f layout): the kept set is that array's, and with gamma = 0 the count c
    too; `weights`: these in place of any selection (for an evaluation in another dtype)"""
    f, l, valid = pixel_losses(x, target, class_mode, gamma, ignore_index, dtype)
    S = x.shape[0] if per_image else 1
    rows = None
    if weights is None:
        if losses is None:
            weights, rows = weights_of(f, l, valid, S, keep, min_kept, max_prob)
        else:
            lsel = losses if gamma == 0 else l
            weights, rows = weights_of(losses.cpu(), lsel.cpu(), valid, S, keep, min_kept, max_prob)
    nseg = int(valid.reshape(S, -1).any(1).sum())
    V = (weights.to(dtype) * f.reshape(S, -1)).sum() / max(nseg, 1)
    return V, f.detach(), rows, weights


def reference(kind: str, maps, target, ow, weight: float, base_scale: float = 1.0, base_kw=None, losses=None, **kw):
    """(loss, [d loss / d map], V of every map, f of every map, rows of every map) of
    base_scale * sum_m ow_m base(map_m) + weight * sum_m ow_m V_m in float64; `losses`: per map, the fp32 f to select on
    (or None); kw: keep, min_kept, max_prob, gamma, per_image"""
    base_kw = dict(base_kw or {})
    cls = kind == "multiclass"
    ignore = base_kw.get("ignore_index", -100)
    leaves = [m.detach().double().requires_grad_(True) for m in maps]
    res = [term(v, target, cls, ignore_index=ignore, losses=None if losses is None else losses[i], **kw) for i, v in enumerate(leaves)]
    base = sum(w * BR.base_map(kind, v, target, **base_kw) for w, v in zip(ow, leaves))
    loss = base_scale * base + weight * sum(w * r[0] for w, r in zip(ow, res))
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [torch.zeros_like(l) if g is None else g for l, g in zip(leaves, grads)]
    return loss.detach(), grads, [r[0].detach() for r in res], [r[1] for r in res], [r[2] for r in res]


def term_float32(x, target, class_mode, **kw):
    """(V, dV/dx) evaluated by torch in FLOAT32 throughout, with the float64 reference's weights (the kept set is not what
    is being measured): how far a plain float32 evaluation is from the float64 one, to judge the bounds of the GPU tests by"""
    _, _, _, w = term(x.double(), target, class_mode, **kw)
    leaf = x.detach().float().requires_grad_(True)
    V, _, _, _ = term(leaf, target, class_mode, dtype=torch.float32, weights=w.float(), **kw)
    assert V.dtype == torch.float32
    (grad,) = torch.autograd.grad(V, leaf)
    return V.detach(), grad


# ------------------------------------------------------------------------------- the cases of tests/test_hardpixel_loss_gpu.py
# (here so that tests/test_hardpixel_loss.py can hold torch's own float32 evaluation of the same inputs against the same bounds)
BINARY_SHAPES = [(3, 1, 17, 23), (2, 3, 40, 40)]
REGION_KW = dict(alpha=0.5, beta=0.5, smooth=0.5)                          # RegionLoss.dice()
FOCAL_KW = dict(alpha=0.7, beta=0.3, gamma=4 / 3, smooth=1e-3, pos_weight=2.5)
CLASS_KW = dict(w_ce=0.4, w_dice=0.6, smooth=1.0, include_background=True, reduce="image")
CLASS_KS = (2, 4, 19, 32)
# name -> (keep, min_kept, max_prob): topk(0.1), ohem(0.7, min_kept=50) where fewer than 50 pixels lie below 0.7 (min_kept
# decides), ohem(0.9, min_kept=5) where more than 5 lie below 0.9 (c > k: max_prob decides)
MIN_KEEP = 2.0 ** -126
CLASS_MODES = {"topk": (0.1, 0, None), "ohem": (MIN_KEEP, 50, 0.7), "ohem_c": (MIN_KEEP, 5, 0.9)}


def make_inputs(shape, seed=0):
    """x = 3 randn, t = rand > 0.7; image 1: empty target"""
    g = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(shape, generator=g)
    t = (torch.rand(shape, generator=g) > 0.7).float()
    if shape[0] > 1:
        t[1] = 0.0
    return x, t


def make_tied_inputs(shape=(2, 1, 64, 64), seed=5):
    """logits snapped to multiples of 0.25 (exact in bf16 too for |x| < 64): hundreds of equal losses"""
    x, t = make_inputs(shape, seed)
    return (x * 4.0).round() / 4.0, t


def make_narrow_inputs(shape=(2, 1, 24, 20), seed=6):
    """softplus(z) = 1 at z = log(e - 1); z = that + (1.5 +- 1.2)e-5 / sigmoid(z): every l lies between 1 and 1 + 256 ulps, so
    all f share their first three digits and only the last round of the select tells them apart"""
    g = torch.Generator().manual_seed(seed)
    t = (torch.rand(shape, generator=g) > 0.5).float()
    z0 = math.log(math.e - 1.0)
    z = z0 + (1.5e-5 + 1.2e-5 * (2.0 * torch.rand(shape, generator=g) - 1.0)) / (1.0 / (1.0 + math.exp(-z0)))
    return torch.where(t > 0.5, -z, z).float(), t


def make_labels(N, K, H, W, seed=0):
    """blocky labels 0 .. K-1 with ignored rows (-100) and labels outside [0, K) (K + 3, -7)"""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, K, (N, (H + 3) // 4, (W + 3) // 4), generator=g)
    y = coarse.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :H, :W].contiguous()
    y[:, H // 3:H // 3 + 5, :] = -100
    y[0, 0, 0] = K + 3
    y[-1, H - 1, W // 2] = -7
    y[0, 2, 5] = K
    return y


def class_shape(K):
    return (2, K, 33, 47) if K <= 4 else (2, K, 16, 24)


def make_class_inputs(K, seed=None, lift=12.0):
    """logits of a mostly trained network: 3 randn + `lift` on the labelled class, so that few pixels have p_t < 0.7"""
    N, _, H, W = class_shape(K)
    g = torch.Generator().manual_seed(K if seed is None else seed)
    y = make_labels(N, K, H, W, seed=K)
    x = 3.0 * torch.randn(N, K, H, W, generator=g)
    hit = (y.unsqueeze(1) == torch.arange(K).reshape(1, K, 1, 1)) & (y != -100).unsqueeze(1)
    return x + lift * hit, y


TIED_KEEP = 0.5      # the threshold falls where the snapped logits are densest: more than 100 equal f at tau
BINARY_BASES = ("bce_dice", "region_dice", "focal_tversky")
# (shape, per_image, base, keep, gamma): both shapes, per_image both ways, keep in {0.1, 1.0}, gamma in {0, 2}, the bases in turn
BINARY_CASES = [(s, p, BINARY_BASES[i % 3], k, g) for i, (s, p, k, g) in enumerate(
    (s, p, k, g) for s in BINARY_SHAPES for p in (False, True) for k in (0.1, 1.0) for g in (0.0, 2.0))]
# the class mode with the focal modulation: (K, keep, gamma, per_image) -- HardPixelLoss.focal and a focal top-k
FOCAL_CLASS_CASES = [(4, 1.0, 2.0, False), (4, 0.1, 2.0, True), (19, 1.0, 1.5, False)]
# (K, mode, per_image, image 1 fully ignored)
CLASS_CASES = [(K, mode, False, False) for K in CLASS_KS for mode in CLASS_MODES] + [(K, "topk", True, True) for K in CLASS_KS]


def class_case_inputs(K, blank):
    x, y = make_class_inputs(K)
    if blank:
        y = y.clone()
        y[1] = -100
    return x, y


def term_cases():
    """(id, x, target, class_mode, kw) of every term the GPU tests evaluate"""
    for s, p, _, k, g in BINARY_CASES:
        x, t = make_inputs(s)
        yield f"binary-{'x'.join(map(str, s))}-{'image' if p else 'batch'}-keep{k}-gamma{g}", x, t, False, dict(keep=k, gamma=g, per_image=p)
    for K, mode, p, blank in CLASS_CASES:
        x, y = class_case_inputs(K, blank)
        keep, min_kept, max_prob = CLASS_MODES[mode]
        yield f"class-K{K}-{mode}-{'image' if p else 'batch'}", x, y, True, dict(keep=keep, min_kept=min_kept, max_prob=max_prob, per_image=p)
    for K, keep, gamma, p in FOCAL_CLASS_CASES:
        x, y = make_class_inputs(K, lift=4.0)
        yield f"class-K{K}-focal{gamma:g}-keep{keep:g}-{'image' if p else 'batch'}", x, y, True, dict(keep=keep, gamma=gamma, per_image=p)
    for p in (False, True):
        x, t = make_tied_inputs()
        yield f"tied-{'image' if p else 'batch'}", x, t, False, dict(keep=TIED_KEEP, per_image=p)
    x, t = make_narrow_inputs()
    yield "narrow", x, t, False, dict(keep=0.25, per_image=True)
