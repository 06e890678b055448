"""Helpers of tests/test_bn_walk.py (CPU) and tests/test_bn_walk_gpu.py: the element passes of BatchNorm in uz_eltwise.hip --
bn_finalize_kernel, bn_relu_apply_kernel, bn_relu_bwd_kernel (reduce pass and apply pass), bn_bwd_finalize_kernel and
bn_relu_bwd_head_kernel -- where every workgroup makes several trips through its loop and all four pixel slots are live.

  * the launch plans restated in plain Python from the host code (grid_for, reduce_shape, bnbwd_shape, the EW choice of the
    finalize kernels), and the walk of the backward kernels restated unit by unit: which workgroup row, trip and slot
    holds which pixel or window, for the walk from the front and for the walk from the end (bit 2 of the flag word);
  * dyadic operands on which every fp32 operation of the forward pass and of the reduce pass is exact, so that order
    cannot matter and the comparison is bit for bit;
  * float64 references written with torch ops (no function of the library is called), on whichever device the operands
    are on;
  * comparators that say where a difference lies: pixel, channel, workgroup row, trip and slot;
  * the case table.

Nothing here needs a GPU or the kernel library."""
from collections import namedtuple
from functools import lru_cache
from types import SimpleNamespace

import torch
import torch.nn.functional as F

BF16, F32 = torch.bfloat16, torch.float32
CUS_HW, RESERVE = 256, 128
CUS = CUS_HW - RESERVE
SENTINEL = -77.0                 # exact in bf16; no case can produce it (|act| < 16, |dy| far below)
NPIX = 4                         # pixel slots of a thread of the non-pooled backward kernels, one grid stride apart
SCALES = (-1.0, -0.5, 0.0, 0.25, 0.5, 1.0, 1.5, 2.0)


def vec_of(dt):
    return 8 if dt == BF16 else 4


def cdiv(a, b):
    return -(-a // b)


def dt_name(dt):
    return "bf16" if dt == BF16 else "fp32"


# ---- restated plans ---------------------------------------------------------------------------------------------------------
ApplyPlan = namedtuple("ApplyPlan", "units grid trips")
BwdPlan = namedtuple("BwdPlan", "units bx by gy gx ustride per_trip trips slots pool")
FinPlan = namedtuple("FinPlan", "ew ng trips blocks")


def pool_hw(H, W, pool):
    """the pooled map of a pool mode ("floor" / "ceil")"""
    return ((H + 1) // 2, (W + 1) // 2) if pool == "ceil" else (H // 2, W // 2)


def n_units(N, H, W, pool):
    """pixels, or 2x2 windows counted on the CEIL grid whatever the mode: every pixel lies in exactly one window"""
    return N * cdiv(H, 2) * cdiv(W, 2) if pool else N * H * W


def apply_plan(dt, N, H, W, C, pool, cus=CUS):
    """bn_relu_apply_t with grid_for(total, 256): one thread per (pixel or window, channel chunk)"""
    units = n_units(N, H, W, pool) * (C // vec_of(dt))
    grid = max(1, min(cdiv(units, 256), 8 * cus))
    return ApplyPlan(units, grid, cdiv(units, 256 * grid))


def bwd_plan(dt, N, H, W, C, pool, pass_, cus=CUS):
    """bnbwd_shape -> reduce_shape; pass_ 1: the reduce pass (4 workgroups per CU), 2: the apply pass and the head's (8)"""
    cc = C // vec_of(dt)
    bx = 1
    while bx < cc and bx < 64:
        bx *= 2
    by, gy = 256 // bx, cdiv(cc, bx)
    units = n_units(N, H, W, pool)
    wg = 8 if pass_ == 2 else 4
    gx = max(1, min(cdiv(units, by), max(1, cus * wg // gy)))
    ustride = gx * by
    per_trip = ustride * (1 if pool else NPIX)
    return BwdPlan(units, bx, by, gy, gx, ustride, per_trip, cdiv(units, per_trip), min(NPIX, cdiv(units, ustride)), bool(pool))


def fin_plan(rows, C):
    """uz_bn_finalize / bnbwd_finalize: EW channels per block of 1024 threads, NG row groups, four groups per trip"""
    ew = 8 if rows >= 128 and C <= 512 else 32
    ng = 1024 // ew
    return FinPlan(ew, ng, cdiv(rows, 4 * ng), cdiv(C, ew))


Walk = namedtuple("Walk", "unit row trip slot")


def walk(plan, rev):
    """the loops of bn_relu_bwd_kernel / bn_relu_bwd_head_kernel followed literally: thread row ty of workgroup b starts at
    u0 = b * by + ty and advances by (4 or 1) * ustride; non-pooled, slot k of a trip holds q = u0 + k * ustride; the walk
    from the end mirrors q (or u0) by units - 1 - q.  One entry per unit VISITED, in visiting order"""
    base = torch.arange(plan.ustride)
    step = 1 if plan.pool else NPIX
    unit, row, trip, slot = [], [], [], []
    for j in range(plan.trips):
        u0 = base + j * step * plan.ustride
        live = u0 < plan.units                       # the loop condition
        for k in range(step):
            q = u0 + k * plan.ustride
            ok = live & (q < plan.units)             # in[k]
            qq = q[ok]
            unit.append(plan.units - 1 - qq if rev else qq)
            row.append(base[ok] // plan.by)
            trip.append(torch.full_like(qq, j))
            slot.append(torch.full_like(qq, k))
    return Walk(torch.cat(unit), torch.cat(row), torch.cat(trip), torch.cat(slot))


def owners(plan, rev):
    """per unit: (workgroup row, trip, slot) -- (units, 3) int64; -1 where the walk never comes"""
    w = walk(plan, rev)
    out = torch.full((plan.units, 3), -1, dtype=torch.int64)
    out[w.unit] = torch.stack([w.row, w.trip, w.slot], 1)
    return out


def unit_of_pixels(N, H, W, pool):
    """per pixel (NHW order): its unit -- itself, or its window on the ceil grid"""
    P = N * H * W
    p = torch.arange(P)
    if not pool:
        return p
    Ho, Wo = cdiv(H, 2), cdiv(W, 2)
    w_, t = p % W, p // W
    h_, n_ = t % H, t // H
    return (n_ * Ho + h_ // 2) * Wo + w_ // 2


def plan_line(form, dt, shape, C, plan):
    if isinstance(plan, ApplyPlan):
        return f"    {form} {dt_name(dt)} {shape} x {C}: {plan.units} threads' units on a grid of {plan.grid} x 256, {plan.trips} trips"
    return (f"    {form} {dt_name(dt)} {shape} x {C}: block {plan.bx} x {plan.by}, grid {plan.gx} x {plan.gy}, {plan.units} units, "
            f"stride {plan.ustride}, {plan.trips} trips" + ("" if plan.pool else f", {plan.slots} slots"))


# ---- the case table ---------------------------------------------------------------------------------------------------------
# claims, per form (False: no pool, True: pooled): trips of the forward apply pass, of the reduce pass and of the backward apply
# pass, and (no pool) the live slots of the reduce and of the backward apply pass -- at 128 CUs
Case = namedtuple("Case", "id dt shape C pools claims")
Claim = namedtuple("Claim", "apply reduce bwd rslots bslots")
HeadCase = namedtuple("HeadCase", "id shape C K trips slots")

CASES = {c.id: c for c in (
    Case("W1", BF16, (3, 97, 113), 512, (None,), {False: Claim(9, 5, 3, 4, 4)}),
    Case("W2", F32, (3, 97, 113), 256, (None,), {False: Claim(9, 5, 3, 4, 4)}),
    Case("W3", BF16, (2, 65, 127), 512, ("floor", "ceil"), {True: Claim(2, 3, 2, None, None)}),
    Case("W4", F32, (2, 65, 127), 256, ("floor", "ceil"), {True: Claim(2, 3, 2, None, None)}),
    Case("W5", BF16, (1, 131, 139), 96, (None,), {False: Claim(1, 1, 1, 3, 2)}),
    Case("W6", BF16, (1, 89, 95), 520, (None, "ceil", "floor"), {False: Claim(3, 3, 2, 4, 4), True: Claim(1, 3, 2, None, None)}),
    Case("S1b", BF16, (2, 9, 13), 8, (None, "ceil", "floor"), {False: Claim(1, 1, 1, 1, 1), True: Claim(1, 1, 1, None, None)}),
    Case("S1f", F32, (2, 9, 13), 4, (None, "ceil", "floor"), {False: Claim(1, 1, 1, 1, 1), True: Claim(1, 1, 1, None, None)}),
    Case("S2rb", BF16, (1, 1, 37), 64, ("ceil",), {True: Claim(1, 1, 1, None, None)}),
    Case("S2rf", F32, (1, 1, 37), 64, ("ceil",), {True: Claim(1, 1, 1, None, None)}),
    Case("S2cb", BF16, (1, 37, 1), 64, ("ceil",), {True: Claim(1, 1, 1, None, None)}),
    Case("S2cf", F32, (1, 37, 1), 64, ("ceil",), {True: Claim(1, 1, 1, None, None)}),
    Case("S3b", BF16, (2, 3, 3), 64, ("floor",), {True: Claim(1, 1, 1, None, None)}),
    Case("S3f", F32, (2, 3, 3), 64, ("floor",), {True: Claim(1, 1, 1, None, None)}),
)}
WALKING = ("W1", "W2", "W3", "W4", "W5", "W6")
SMALL = tuple(i for i in CASES if i.startswith("S"))
# block shapes the table claims: id -> (bx, by, gy)
BLOCKS = {"W1": (64, 4, 1), "W2": (64, 4, 1), "W3": (64, 4, 1), "W4": (64, 4, 1), "W5": (16, 16, 1), "W6": (64, 4, 2),
          "S1b": (1, 256, 1), "S1f": (1, 256, 1)}

# the head's apply pass (bf16, no pool): trips and live slots at 128 CUs.  W8: slots 0 and 1 are live on the table's map
# (34571 pixels on a stride of 32768); W8w is that case on the smallest square map on which slot 2 is live as well
HEAD_CASES = {c.id: c for c in (
    HeadCase("W7", (4, 255, 257), 64, (3,), 2, 4),
    HeadCase("W8", (1, 181, 191), 64, (1, 8), 1, 2),
    HeadCase("W8w", (1, 257, 257), 64, (8,), 1, 3),
)}

HEAD_ROWS = 600                  # partial rows the head cases hand to the finalize kernel: pixel p in row p % 600 (two trips at EW = 8)
FIN_ROWS = (1, 127, 128, 512, 513, 1024)
FIN_C = (8, 96, 512, 520)


def forms(case):
    """(pool mode, pooled?) of a case, in table order"""
    return [(p, p is not None) for p in case.pools]


# ---- exact operands ---------------------------------------------------------------------------------------------------------
def _quarters(shape, lo, hi, g):
    """multiples of 1/4 in [lo, hi], fp32"""
    return torch.randint(4 * lo, 4 * hi + 1, shape, generator=g, dtype=torch.int16).float() / 4


def channel_vectors(C, g):
    """(scale, shift, mean, invstd) as a (4, C) fp32 tensor: every run of eight channels holds every scale of SCALES, the
    negative ones and zero among them; a zero scale makes pre = shift for every pixel, so all four taps of every window tie:
    with shift = +1 (channels 0, 16, ..) at a positive value, with shift = -1 (channels 8, 24, ..) below the ReLU, where
    dz, S0, S1 and dy are all exactly 0"""
    c = torch.arange(C)
    scale = torch.tensor(SCALES)[(3 * c + 2) % 8]
    shift = _quarters((C,), -2, 2, g)
    zero = scale == 0
    shift[zero] = torch.where((c[zero] // 8) % 2 == 0, 1.0, -1.0)
    mean = _quarters((C,), -1, 1, g)
    invstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)]
    return torch.stack([scale, shift, mean, invstd])


def _seed(key):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(key)) + 20260


@lru_cache(maxsize=1)
def operands(case_id):
    """y, res, g0, g1: (P, C); gp: (N, Ho, Wo, C) on the ceil grid (gp_rows() cuts the mode's map out); vec: (4, C).
    fp32 on the CPU, every value exact in bf16"""
    c = CASES[case_id]
    N, H, W = c.shape
    P = N * H * W
    g = torch.Generator().manual_seed(_seed(case_id))
    o = SimpleNamespace()
    o.vec = channel_vectors(c.C, g)
    o.y = _quarters((P, c.C), -4, 4, g)
    o.res = _quarters((P, c.C), -4, 4, g)
    o.g0 = _quarters((P, c.C), -2, 2, g)
    o.g1 = _quarters((P, c.C), -2, 2, g)
    o.gp = _quarters((N, cdiv(H, 2), cdiv(W, 2), c.C), -2, 2, g)
    return o


def gp_rows(gp, shape, pool):
    Hp, Wp = pool_hw(shape[1], shape[2], pool)
    return gp[:, :Hp, :Wp].reshape(-1, gp.shape[-1])


@lru_cache(maxsize=1)
def head_operands(case_id, K):
    """y: (P, C); g: (N, K, H, W) logit gradients and w: (K, C) head weights, multiples of 1/2 in [-1, 1]: the head's input
    gradient sum_k g w is a multiple of 1/4 of magnitude <= 8, exact in bf16 after any order of additions"""
    c = HEAD_CASES[case_id]
    N, H, W = c.shape
    gen = torch.Generator().manual_seed(_seed(case_id) + K)
    o = SimpleNamespace()
    o.vec = channel_vectors(c.C, gen)
    o.y = _quarters((N * H * W, c.C), -4, 4, gen)
    o.g = torch.randint(-2, 3, (N, K, H, W), generator=gen, dtype=torch.int16).float() / 2
    o.w = torch.randint(-2, 3, (K, c.C), generator=gen, dtype=torch.int16).float() / 2
    return o


def head_gradient(o, shape, dt=BF16):
    """bf16(sum_k g[n, k, hw] * w[k, c]), added in ascending k, as a (P, C) float64 tensor"""
    N, H, W = shape
    K = o.w.shape[0]
    g = o.g.double().permute(0, 2, 3, 1).reshape(N * H * W, K)
    d = torch.zeros(N * H * W, o.w.shape[1], dtype=torch.float64, device=g.device)
    for k in range(K):
        d += g[:, k:k + 1] * o.w[k].double()
    return d.to(dt).double()


# ---- float64 references -----------------------------------------------------------------------------------------------------
def nchw(rows, shape):
    N, H, W = shape
    return rows.reshape(N, H, W, -1).permute(0, 3, 1, 2).contiguous()


def nhwc(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def forward_ref(y, vec, shape, dt, relu=True, res=None, pool=None):
    """act = relu?(y * scale + shift) [+ res], rounded once to the run dtype; pooled = max_pool2d of the STORED act"""
    v = y.double() * vec[0].double() + vec[1].double()
    if relu:
        v = torch.relu(v)
    if res is not None:
        v = v + res.double()
    act = v.to(dt)
    pooled = None
    if pool:
        pooled = nhwc(F.max_pool2d(nchw(act.double(), shape), 2, 2, ceil_mode=pool == "ceil")).to(dt)
    return act, pooled


def backward_terms(y, vec, shape, g0=None, g1=None, gp=None, pool=None, relu=True):
    """(dz, xhat) in float64; the pool's gradient goes where F.max_pool2d(return_indices=True) on relu?(pre) points: ATen's
    first maximum in (0,0), (0,1), (1,0), (1,1) order"""
    N, H, W = shape
    yd = y.double()
    pre = yd * vec[0].double() + vec[1].double()
    g = torch.zeros_like(yd)
    if g0 is not None:
        g = g + g0.double()
    if g1 is not None:
        g = g + g1.double()
    if gp is not None:
        a = nchw(torch.relu(pre) if relu else pre, shape)
        _, idx = F.max_pool2d(a, 2, 2, ceil_mode=pool == "ceil", return_indices=True)
        Hp, Wp = pool_hw(H, W, pool)
        src = nchw(gp.double(), (N, Hp, Wp))
        routed = torch.zeros(N, a.shape[1], H * W, dtype=torch.float64, device=yd.device)
        routed.scatter_(2, idx.flatten(2), src.flatten(2))
        g = g + nhwc(routed.reshape(N, -1, H, W))
    dz = torch.where(pre > 0, g, torch.zeros_like(g)) if relu else g
    xhat = (yd - vec[2].double()) * vec[3].double()
    return dz, xhat


def totals(dz, xhat):
    return torch.stack([dz.sum(0), (dz * xhat).sum(0)])


def rows_ref(dz, xhat, plan, shape, rev):
    """the partial rows (gx, 2, C) of the reduce pass by the restated ownership, float64"""
    own = owners(plan, rev)[:, 0][unit_of_pixels(*shape, plan.pool)].to(dz.device)
    out = torch.zeros(plan.gx, 2, dz.shape[1], dtype=torch.float64, device=dz.device)
    out[:, 0].index_add_(0, own, dz)
    out[:, 1].index_add_(0, own, dz * xhat)
    return out


def dy_ref(dz, xhat, vec, S, P):
    """dy = scale * (dz - S0 / P - xhat * S1 / P) and the magnitude A its fp32 roundings are relative to"""
    sc = vec[0].double()
    k0, k1 = S[0] / P, S[1] / P
    return sc * (dz - k0 - xhat * k1), sc.abs() * (dz.abs() + k0.abs() + (xhat * k1).abs())


def finalize_ref(stats, count, gamma, beta, eps, momentum, rm, rv):
    """the formulas of bn_finalize_kernel in float64; eps and momentum are the kernel's fp32 arguments widened.  Returns
    (scale, shift, mean, invstd, running_mean, running_var)"""
    eps = float(torch.tensor(eps, dtype=F32))
    momentum = float(torch.tensor(momentum, dtype=F32))
    t1, t2 = stats[:, 0].double().sum(0), stats[:, 1].double().sum(0)
    m = t1 / count
    var = (t2 / count - m * m).clamp_min(0.0)
    istd = 1.0 / torch.sqrt(var + eps)
    ga, be = gamma.double(), beta.double()
    unbiased = var * count / (count - 1.0) if count > 1 else var
    return (ga * istd, be - m * ga * istd, m, istd, (1.0 - momentum) * rm.double() + momentum * m,
            (1.0 - momentum) * rv.double() + momentum * unbiased)


def finalize_inputs(rows, C, kind="plain"):
    """partial rows of exact integers: every row stands for 16 samples x + offset_c, x in -3 .. 3, offset_c in -2 .. 2, so
    the variance is about 4 against a squared mean of at most 4 (var >= mean^2 / 16 is asserted by the CPU file).
    kind "clamp": the sums of squares are zero -- a negative variance, clamped to 0; "count1": one row, count 1, with
    sum x^2 = (sum x)^2 + 5: a variance of 5 that a count of 1 must not unbias (it would divide by zero).
    Returns (stats (rows, 2, C) fp32, count, gamma, beta, running_mean, running_var)"""
    g = torch.Generator().manual_seed(rows * 1000 + C + len(kind))
    x = torch.randint(-3, 4, (rows, 16, C), generator=g).float() + torch.randint(-2, 3, (C,), generator=g).float()
    stats = torch.stack([x.sum(1), (x * x).sum(1)], 1)
    count = 16.0 * rows
    if kind == "clamp":
        stats[:, 1] = 0.0
    elif kind == "count1":
        assert rows == 1
        stats[:, 0] = x[:, 0]                         # one sample: |mean| <= 5
        stats[:, 1] = stats[:, 0] ** 2 + 5.0
        count = 1.0
    gamma = torch.randn(C, generator=g)
    gamma[::5] = 0.0
    return stats, count, gamma, torch.randn(C, generator=g), torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5


def bwd_finalize_inputs(rows, C):
    g = torch.Generator().manual_seed(rows * 1000 + C + 7)
    return torch.randint(-1000, 1001, (rows, 2, C), generator=g).float()


# ---- preconditions of exactness ---------------------------------------------------------------------------------------------
def assert_exact_preconditions(case, o, pool, plans):
    """conditions on the INPUTS (a case that fails one gets other inputs, never another bound): rounding to the run dtype
    changes nothing; per workgroup row and in total the sums of |dz| (in quarters) and of |dz * xhat| (in 1/32) stay below
    2^24, so that every fp32 partial sum is exact in any order; pooled: at least 5 % of the (window, channel) pairs have
    two taps tied at a positive maximum.  plans: the reduce-pass plans to check the rows of.  Returns the figures"""
    for name in ("y", "res", "g0", "g1", "gp", "vec"):
        t = getattr(o, name)
        assert torch.equal(t.to(case.dt).float(), t), name
    gp = gp_rows(o.gp, case.shape, pool) if pool else None
    for res in (None, o.res):
        act, _ = forward_ref(o.y, o.vec, case.shape, case.dt, True, res, None)
        full = torch.relu(o.y.double() * o.vec[0].double() + o.vec[1].double()) + (0 if res is None else res.double())
        assert torch.equal(act.double(), full) and float(full.abs().max()) < 16
        assert torch.equal(full * 16, (full * 16).round())
    dz, xhat = backward_terms(o.y, o.vec, case.shape, o.g0, o.g1, gp, pool)
    a0, a1 = dz.abs() * 4, (dz * xhat).abs() * 32
    assert torch.equal(a0, a0.round()) and torch.equal(a1, a1.round())
    fig = {"sum |dz| / 2^24": float(a0.sum(0).max()) / 2 ** 24, "sum |dz xhat| / 2^24": float(a1.sum(0).max()) / 2 ** 24}
    assert max(fig.values()) < 1, fig
    for plan in plans:
        own = owners(plan, False)[:, 0][unit_of_pixels(*case.shape, plan.pool)]   # (rows are parts of the totals either way)
        for a in (a0, a1):
            assert float(torch.zeros(plan.gx, a.shape[1], dtype=torch.float64).index_add_(0, own, a).max()) < 2 ** 24
    if pool:
        fig["tied windows"] = tie_fraction(o.y, o.vec, case.shape, pool)
        assert fig["tied windows"] >= 0.05, fig
    return fig


def tie_fraction(y, vec, shape, pool):
    """the fraction of (pooled window, channel) pairs in which the maximum is positive and held by two taps or more"""
    a = nchw(torch.relu(y.double() * vec[0].double() + vec[1].double()), shape)
    ceil = pool == "ceil"
    m = F.max_pool2d(a, 2, 2, ceil_mode=ceil)
    Hp, Wp = m.shape[2:]
    pad = F.pad(a, (0, 2 * Wp - a.shape[3] if ceil else 0, 0, 2 * Hp - a.shape[2] if ceil else 0), value=-1.0)[:, :, :2 * Hp, :2 * Wp]
    taps = pad.reshape(a.shape[0], a.shape[1], Hp, 2, Wp, 2)
    hits = (taps == m[:, :, :, None, :, None]).sum((3, 5))
    return float(((hits >= 2) & (m > 0)).double().mean())


# ---- comparators ------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _where_apply(pixels, chans, shape, dt, C, pool, plan, rev):
    """trip and workgroup of the forward apply pass for (pixel, channel) pairs"""
    cc = C // vec_of(dt)
    u = unit_of_pixels(*shape, pool)[pixels]
    idx = u * cc + chans // vec_of(dt)
    idx0 = plan.units - 1 - idx if rev else idx
    return [f"pixel {int(p)} channel {int(ch)}: trip {int(i) // (256 * plan.grid)}, workgroup {(int(i) // 256) % plan.grid}"
            for p, ch, i in zip(pixels, chans, idx0)]


def _where_bwd(pixels, chans, shape, plan, rev):
    own = owners(plan, rev)[unit_of_pixels(*shape, plan.pool)[pixels]]
    return [f"pixel {int(p)} channel {int(ch)}: trip {int(o[1])}, slot {int(o[2])}, workgroup row {int(o[0])}"
            for p, ch, o in zip(pixels, chans, own)]


def report(bad, what, where):
    nz = bad.nonzero()[:4].cpu()
    lines = where(nz[:, 0], nz[:, 1])
    return f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in {int(bad.any(1).sum())} pixels; first: " + "; ".join(lines)


def assert_same(got, ref, what, where):
    """bit for bit; where(pixels, channels) -> descriptions"""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = _bits(got) != _bits(ref)
    assert not bool(bad.any()), report(bad, what, where)


def where_apply(case, pool, plan, rev=False):
    return lambda p, ch: _where_apply(p, ch, case.shape, case.dt, case.C, pool, plan, rev)


def where_bwd(shape, plan, rev=False):
    return lambda p, ch: _where_bwd(p, ch, shape, plan, rev)


def check_rows(got, want, what="partial rows"):
    """the reduce pass's rows (gx, 2, C) fp32 against the restated ownership, bit for bit, row by row"""
    want32 = want.float()
    assert torch.equal(want32.double(), want), "the reference rows are not exact in fp32"
    assert got.shape == want32.shape, (got.shape, want32.shape)
    bad = (_bits(got) != _bits(want32)).flatten(1).any(1)
    if bool(bad.any()):
        first = bad.nonzero().flatten()[:6].tolist()
        b = first[0]
        k, ch = (_bits(got[b]) != _bits(want32[b])).nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.shape[0]} workgroup rows differ (first {first}); row {b}, "
                             f"{('sum dz', 'sum dz xhat')[k]}, channel {ch}: got {float(got[b, k, ch])}, want {float(want32[b, k, ch])}")


def check_totals(sums, dgamma, dbeta, S, what="totals"):
    """sums (2, C) float64, dbeta = float(S0), dgamma = float(S1): bit for bit"""
    bad = _bits(sums) != _bits(S)
    assert not bool(bad.any()), f"{what}: sums differ in {int(bad.sum())} entries, first {bad.nonzero()[0].tolist()}"
    if dgamma is not None:
        assert torch.equal(_bits(dbeta), _bits(S[0].float())), f"{what}: dbeta"
        assert torch.equal(_bits(dgamma), _bits(S[1].float())), f"{what}: dgamma"


def check_dy(got, ref, A, dz, S, dt, where, extra=None, what="dy"):
    """|got - ref| <= 2^-21 A (at most eight fp32 roundings, each relative to a quantity A bounds) [+ 2^-8 |ref| in bf16: one
    ulp] [+ extra]; exactly 0 wherever dz, S0 and S1 are all 0"""
    assert got.shape == ref.shape and got.dtype == dt, (what, got.shape, ref.shape, got.dtype)
    gd = got.double()
    bound = 2.0 ** -21 * A
    if dt == BF16:
        bound = bound + 2.0 ** -8 * ref.abs()
    if extra is not None:
        bound = bound + extra
    bad = ~((gd - ref).abs() <= bound)                # a NaN is a difference
    zero = (dz == 0) & (S[0] == 0) & (S[1] == 0)
    bad |= zero & (gd != 0)
    assert not bool(bad.any()), report(bad, what, where)


def check_ulp(got, ref, what):
    """a finalize output: at most one fp32 ulp (of the reference's magnitude) from the float64 formula"""
    r32 = ref.float().abs()
    ulp = (torch.nextafter(r32, torch.full_like(r32, float("inf"))) - r32).double()
    err = (got.double() - ref).abs()
    bad = ~(err <= ulp)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} channels off by more than one ulp, first channel " \
                                f"{int(bad.nonzero()[0])}: got {float(got[bad][0])!r}, want {float(ref[bad][0])!r}"
