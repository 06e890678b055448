"""TEST INFRASTRUCTURE.  What tests/test_conv_pp_walk.py (CPU) and tests/test_conv_pp_walk_gpu.py share about
conv3x3_pp_kernel (csrc/uz_conv3x3_pp.hip) where its workgroups walk several tiles: the restatement of uz_pp_plan(), the
table of shapes at which every configuration walks, integer operands with their exact references, and comparators that
name the tiles and trips of a mismatch.  No GPU use.

Why integers: x from {-1, 0, 1} (the XF form: -2..2 before the transform, 0..7 after it), thinned weights from {-1, 0, 1},
an integer bias.  Every product and every fp32 partial sum is then an integer far below 2^24, whatever the order of the
sum, so F.conv2d in fp32 on the CPU IS the float64 result and the kernel's output must be that value, bit for bit; the
checks of assert_exact_preconditions() (from the reference alone) extend that to the bf16 store and to the statistics
however tiles are dealt to lanes, waves and workgroups."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

CUS_HW = 256                     # UZ_NUM_CU_HW
RESERVE = 128                    # uz_set_cu_reserve() of the walking cases
CUS = CUS_HW - RESERVE           # UZ_NUM_CU under that reserve
KU = 32                          # input channels per slab
SENTINEL = -77.0                 # exact in bf16; what a buffer holds where no case may write
BF16 = torch.bfloat16

# configuration: (tile height, tile width, channels per N tile), as PpCfg<TH, TW, ...> and BN = 64 * WN
TILE = {"pp512": (16, 32, 128), "pp512x64": (16, 32, 64), "pp256": (8, 32, 128), "pp256w16": (16, 16, 128),
        "pp128w16": (8, 16, 128)}

Plan = namedtuple("Plan", "cfg th tw ntiles tiles_n grid_m ksplit")


def cdiv(a, b):
    return -(-a // b)


def pp_plan(N, H, W, Cin, Nout, cus, up=False):
    """(cfg, th, tw, ntiles, tiles_n, grid_m, ksplit) as uz_pp_plan() decides for a bf16 3x3 convolution (padding 1, plain
    store; up: the nearest x2 upsampled read, H x W the OUTPUT grid), or None where the ping-pong kernel does not apply.
    `cus` is UZ_NUM_CU = 256 - reserve: rounds(), the pp512x64 threshold and the cap follow it; the pp128w16 demotion and the
    split-K rule use the hardware's 256:
        tiles(th, tw) = N * ceil(H / th) * ceil(W / tw);  rounds(t) = ceil(t / UZ_NUM_CU);  tn = ceil(Nout / 128)
        Nout >= 128:  W >= 32 && H >= 8:  pp512 if H >= 16 && rounds(tiles(16,32) tn) * 16 < rounds(tiles(8,32) tn) * 10, else pp256
                      9 <= W <= 16 && H >= 8:  pp256w16
        32 < Nout < 128 && W >= 32 && H >= 16:  pp512x64 if tiles(16,32) >= UZ_NUM_CU / 2
        pp256 / pp256w16:  tot = tiles * tn;  splits = tot * 4 <= 256 && Cin / 32 >= 16;  tot * 2 <= 256 && !splits -> pp128w16
        grid_m = min(ntiles, max(1, UZ_NUM_CU / tiles_n))
        pp256 / pp256w16 with ntiles * tiles_n * 4 <= 256 && Cin / 32 >= 16:  s = min(256 / tot, (Cin / 32) / 4, 8);
            s >= 4 -> cps = ceil(ncb / s), ksplit = ceil(ncb / cps)"""
    if Cin % KU != 0 or Nout % 8 != 0:
        return None
    if up and (H % 2 or W % 2):
        return None

    def tiles(th, tw):
        return N * cdiv(H, th) * cdiv(W, tw)

    def rounds(t):
        return cdiv(t, cus)

    cfg = None
    if Nout >= 128:
        tn = cdiv(Nout, 128)
        if W >= 32 and H >= 8:
            r512, r256 = rounds(tiles(16, 32) * tn), rounds(tiles(8, 32) * tn)
            cfg = "pp512" if (H >= 16 and r512 * 16 < r256 * 10) else "pp256"
        elif 9 <= W <= 16 and H >= 8:
            cfg = "pp256w16"
    elif Nout > 32 and W >= 32 and H >= 16:
        if tiles(16, 32) >= cus // 2:
            cfg = "pp512x64"
    if cfg is None:
        return None
    ncb = Cin // KU
    if cfg in ("pp256", "pp256w16"):
        tot = tiles(*TILE[cfg][:2]) * cdiv(Nout, 128)
        splits = tot * 4 <= CUS_HW and ncb >= 16
        if tot * 2 <= CUS_HW and not splits:
            cfg = "pp128w16"
    th, tw, bn = TILE[cfg]
    ntiles, tiles_n = tiles(th, tw), cdiv(Nout, bn)
    cap = max(1, cus // tiles_n)
    ksplit = 1
    tot = ntiles * tiles_n
    if cfg in ("pp256", "pp256w16") and tot * 4 <= CUS_HW and ncb >= 16:
        s = min(CUS_HW // tot, ncb // 4, 8)
        if s >= 4:
            ksplit = cdiv(ncb, cdiv(ncb, s))
    return Plan(cfg, th, tw, ntiles, tiles_n, min(ntiles, cap), ksplit)


def kernel_name(cfg, up=False):
    """what uz_conv_igemm_kernel_name() answers for an unsplit launch of the configuration"""
    return f"conv3x3_{cfg}_bf16" + ("_up2" if up else "")


# ---- the shapes at which the configurations walk under a reserve of 128 CUs ------------------------------------------------
# map: (cfg, (N, H, W), widest Nout, rows ragged, columns ragged); the Nout of a case is a prefix of the widest one's channels
Map = namedtuple("Map", "cfg shape nout_max rows_ragged cols_ragged")
MAPS = {
    # 224 tiles / 64: rows 120 = 7 * 16 + 8, columns 218 = 6 * 32 + 26; Nout 200 and 136 leave a channel tail in N tile 2
    "m512": Map("pp512", (4, 120, 218), 200, True, True),
    # 260 tiles / 128: rows 16 + 4, columns 32 + 4; Nout 40: channel tail
    "m512x64": Map("pp512x64", (65, 20, 36), 64, True, True),
    # 240 tiles / 64: rows 8 + 4, columns 2 * 32 + 8
    "m256": Map("pp256", (40, 12, 72), 200, True, True),
    # 330 tiles / 64: columns only (72 = 2 * 32 + 8), 40 rows = 5 * 8: interior tiles exist
    "m256c": Map("pp256", (22, 40, 72), 256, False, True),
    # 130 tiles / 64: both ways, channel tail
    "m256w16": Map("pp256w16", (130, 12, 14), 136, True, True),
    # 66 tiles / 32: whole 16 x 16 maps, four N tiles
    "m256w16n": Map("pp256w16", (66, 16, 16), 512, False, False),
    # 256 tiles / 128: rows 8 + 4, columns 14: every workgroup exactly two trips
    "m128w16": Map("pp128w16", (128, 12, 14), 128, True, True),
    # 100 tiles / 64: two N tiles; some workgroups one trip, some two
    "m128w16n": Map("pp128w16", (50, 12, 14), 256, True, True),
}

# A case: a map, the input channels (Cin / 32 slabs per tile), the output channels, whether the input is read upsampled,
# the operand family ("int": x from {-1, 0, 1}; "xf": the raw input of the transformed read)
Case = namedtuple("Case", "map cin nout up kind")


def _c(m, cin, nout=None, up=False, kind="int"):
    return Case(m, cin, MAPS[m].nout_max if nout is None else nout, up, kind)


# (a) plain forward, bias + statistics.  Slabs: pp512 (NPH = 9, DPH = 4) and pp256 (UPP = 3: NPH = 3, DPH = 2) take one, two
# and a count with a middle slab (three / four); the rest one and two
PLAIN = [_c("m512", 32), _c("m512", 64), _c("m512", 96), _c("m512", 64, 136),
         _c("m512x64", 32, 40), _c("m512x64", 64),
         _c("m256", 32), _c("m256", 64), _c("m256", 128), _c("m256c", 64),
         _c("m256w16", 32), _c("m256w16", 64), _c("m256w16n", 64),
         _c("m128w16", 32), _c("m128w16", 64), _c("m128w16n", 32)]
# (b) the nearest x2 upsampled read
UP2 = [_c("m512", 64, up=True), _c("m512x64", 32, 40, up=True), _c("m256", 64, up=True)]
# (c) fused BatchNorm-backward sums (operands of (a) without the bias)
BNRED = [_c("m512", 64, 136), _c("m512x64", 32, 40), _c("m256", 128), _c("m256w16", 64), _c("m128w16", 64)]
# (d) eval-mode epilogue (operands of (a))
BNACT = [_c("m512", 96), _c("m512x64", 32, 40), _c("m256", 64), _c("m256w16", 32), _c("m128w16", 32)]
# (e) input transform: pp512x64 only; one, two, four slabs and once upsampled
XF = [_c("m512x64", 32, 40, kind="xf"), _c("m512x64", 64, kind="xf"), _c("m512x64", 128, 40, kind="xf"),
      _c("m512x64", 64, up=True, kind="xf")]
# (f) normal operands, one case per configuration
NORMAL = [_c("m512", 64), _c("m512x64", 64), _c("m256c", 64), _c("m256w16", 64), _c("m128w16", 64)]

ALL_CASES = list(dict.fromkeys(PLAIN + UP2 + BNRED + BNACT + XF + NORMAL))


def case_id(c):
    return f"{MAPS[c.map].cfg}-{c.map}-cin{c.cin}-n{c.nout}" + ("-up2" if c.up else "") + ("-xf" if c.kind == "xf" else "")


def case_plan(c, cus=CUS):
    N, H, W = MAPS[c.map].shape
    return pp_plan(N, H, W, c.cin, c.nout, cus, c.up)


def assert_walks(c, plan):
    """the walk conditions from the restated plan alone: the configuration the case claims, unsplit; every workgroup makes
    at least two trips and some make three (pp128w16: some make two, none three -- it cannot, see the GPU file's docstring);
    ragged as the map claims"""
    m = MAPS[c.map]
    N, H, W = m.shape
    assert plan is not None and plan.cfg == m.cfg, (plan, m.cfg)
    assert plan.ksplit == 1, plan
    assert (plan.th, plan.tw) == TILE[m.cfg][:2]
    if m.cfg == "pp128w16":
        assert plan.grid_m + 1 <= plan.ntiles <= 2 * plan.grid_m, plan
    else:
        assert plan.ntiles >= 2 * plan.grid_m + 1, plan
    assert (H % plan.th != 0) == m.rows_ragged and (W % plan.tw != 0) == m.cols_ragged, (H, W, plan)
    assert c.nout <= m.nout_max and c.cin % KU == 0
    if c.up:
        assert H % 2 == 0 and W % 2 == 0


# ---- integer operands and their exact references ---------------------------------------------------------------------------
def ints(g, shape, lo=-1, hi=1):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def nhwc(t):
    """(N, C, H, W) -> (N H W, C)"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def density(cin, kind):
    """share of the weights kept.  var(y) = 9 Cin * density * E[w^2] E[a^2] with E[w^2] = 2/3: "int" (E[a^2] = 2/3) 4 Cin density
    = 48, sigma 7; "xf" (a in 0..7, a variance of about 5 around a channel's mean, the signs of a channel's weights balanced, see
    int_operands()) about 12 weights per output channel, sigma 8.  The largest map has 104640 pixels: sum y^2 about 5e6 ("xf":
    46800 pixels, 3e6) against the 2^24 = 1.7e7 of the exact-statistics precondition, and |y| stays below 100 of the 256 a
    bf16 integer may reach"""
    return min(1.0, (12.0 if kind == "int" else 2.0) / cin)


Operands = namedtuple("Operands", "x w b prod scale shift")


@functools.lru_cache(maxsize=1)
def int_operands(map_name, cin, up, kind):
    """x (N, Cin, Hi, Wi) as the kernel reads it (half resolution when up), w (widest Nout, Cin, 3, 3), integer bias, the exact
    product (N H W, widest Nout) WITHOUT the bias in fp32, and for "xf" the per-input-channel (scale, shift) of the transform
    relu(x * scale + shift) that the product was formed on (zero padding AFTER the transform).  Shared by the variants of a
    shape, which follow each other"""
    m = MAPS[map_name]
    N, H, W = m.shape
    Hi, Wi = (H // 2, W // 2) if up else (H, W)
    g = torch.Generator().manual_seed(1000 * cin + 7 * H + W + (1 if up else 0) + (2 if kind == "xf" else 0))
    w = ints(g, (m.nout_max, cin, 3, 3))
    w = w * (torch.rand(w.shape, generator=g) < density(cin, kind)).float()
    if kind == "xf":
        # the transformed activation has a mean of about 2.5: an output channel whose weights lean to one sign would carry
        # that mean times its imbalance into every pixel, and sum y^2 with it.  The kept weights of a channel therefore take
        # alternating signs along a random order: they sum to 0 or 1
        flat = w.reshape(m.nout_max, -1)
        keys = torch.where(flat != 0, torch.rand(flat.shape, generator=g), torch.full((), 2.0))
        rank = keys.argsort(1).argsort(1)
        w = ((1 - 2 * (rank % 2)).float() * (flat != 0).float()).reshape(w.shape)
    b = ints(g, (m.nout_max,), -3, 3)
    scale = shift = None
    if kind == "xf":
        x = ints(g, (N, cin, Hi, Wi), -2, 2)
        scale = (ints(g, (cin,), 0, 1) * 2 - 1) * ints(g, (cin,), 1, 2)        # {+-1, +-2}
        shift = ints(g, (cin,), 1, 3)                                          # > 0: a transformed zero pad would show
        a = torch.relu(x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))  # integers in 0..7
    else:
        x = ints(g, (N, cin, Hi, Wi))
        a = x
    ain = F.interpolate(a, scale_factor=2, mode="nearest") if up else a
    prod = nhwc(F.conv2d(ain, w, None, padding=1))
    assert bool((prod == prod.round()).all()) and prod.abs().max().item() < 2 ** 20     # fp32 on integers: exact
    return Operands(x, w, b, prod, scale, shift)


def operands(c):
    return int_operands(c.map, c.cin, c.up, c.kind)


def plain_ref(c, with_bias=True):
    """float64 (N H W, Nout): the exact convolution [+ bias] of a case"""
    o = operands(c)
    y = o.prod[:, :c.nout].double()
    return y + o.b[:c.nout].double() if with_bias else y


def assert_exact_preconditions(ref64, sums=True):
    """from the reference alone: rounding it to bf16 changes nothing (integers up to 256, half-integers below 128), and per
    channel sum |y| < 2^24 and sum y^2 < 2^24 over all pixels -- no fp32 partial sum of the statistics can round, however
    the tiles are dealt to lanes, waves and workgroups.  sums=False: a form without statistics (the eval-mode epilogue)"""
    assert ref64.dtype == torch.float64
    assert torch.equal(ref64.to(BF16).double(), ref64), f"max |y| {ref64.abs().max().item():g}: not exact in bf16"
    if not sums:
        return None
    s1, s2 = ref64.abs().sum(0).max().item(), (ref64 * ref64).sum(0).max().item()
    assert s1 < 2 ** 24 and s2 < 2 ** 24, (s1, s2)
    return s1, s2


BnRed = namedtuple("BnRed", "bn_y vec dz want0 want1")


def bnred_operands(c, dx64):
    """the BatchNorm whose backward sums ride in the epilogue of the gradient dx (float64, exact): bn_y integers in -3..3,
    scale = +-1 and shift = 0.5 (the mask has no ties), integer mean in -2..2, invstd a power of two in 2^-2..2.  Every term
    dz and dz * ((y - mean) * invstd) -- the per-element form the epilogue accumulates -- is a multiple of 2^-2; with
    sum |term| < 2^22 per channel (asserted) no fp32 partial sum can round.  Returns bn_y (P, Nout), vec (4, Nout) =
    (scale, shift, mean, invstd), dz, and the two exact sums in float64"""
    g = torch.Generator().manual_seed(31 * c.cin + c.nout)
    P, n = dx64.shape
    bn_y = ints(g, (P, n), -3, 3)
    scale = ints(g, (n,), 0, 1) * 2 - 1
    shift = torch.full((n,), 0.5)
    mean = ints(g, (n,), -2, 2)
    invstd = 2.0 ** ints(g, (n,), -2, 1)
    dz = torch.where(bn_y * scale + shift > 0, dx64, torch.zeros((), dtype=torch.float64))
    term = dz * ((bn_y.double() - mean.double()) * invstd.double())
    assert dz.abs().sum(0).max().item() < 2 ** 22 and term.abs().sum(0).max().item() < 2 ** 22, \
        (dz.abs().sum(0).max().item(), term.abs().sum(0).max().item())
    assert bool((term * 4 == (term * 4).round()).all())
    return BnRed(bn_y, torch.stack([scale, shift, mean, invstd]), dz, dz.sum(0), term.sum(0))


def act_vectors(c):
    """eval-mode BatchNorm folded to (scale, shift): scale from {+-0.5, +-1, +-2}, shift integers in -3..3"""
    g = torch.Generator().manual_seed(17 * c.cin + c.nout)
    scale = (ints(g, (c.nout,), 0, 1) * 2 - 1) * 2.0 ** ints(g, (c.nout,), -1, 1)
    return scale, ints(g, (c.nout,), -3, 3)


def act_ref(pre64, scale, shift, relu):
    y = pre64 * scale.double() + shift.double()
    return y.clamp_min(0.0) if relu else y


# ---- comparators ---------------------------------------------------------------------------------------------------------------
def tile_of_pixels(shape, plan):
    """(N H W,) the tile of every pixel, numbered as the kernel's decode() does: tile = (image * th_n + tile row) * tw_n +
    tile column"""
    N, H, W = shape
    th_n, tw_n = cdiv(H, plan.th), cdiv(W, plan.tw)
    n = torch.arange(N).view(N, 1, 1)
    ti = (torch.arange(H) // plan.th).view(1, H, 1)
    tj = (torch.arange(W) // plan.tw).view(1, 1, W)
    return ((n * th_n + ti) * tw_n + tj).reshape(-1)


def decode(tile, shape, plan):
    """tile -> (image, tile row, tile column), as decode() of the kernel"""
    _, H, W = shape
    per = cdiv(H, plan.th) * cdiv(W, plan.tw)
    im, rem = divmod(tile, per)
    return (im,) + divmod(rem, cdiv(W, plan.tw))


def _where(got, ref, shape, plan):
    """which pixels of a (N H W, n) result differ: their tiles as (image, tile row, tile column), the trips tile // grid_m of
    the workgroups that computed them (a fault of the walk shows in trips >= 1 only), the channels"""
    bad = got != ref
    rows = bad.any(1).nonzero().flatten()
    if rows.numel() == 0:
        return "equal"
    tiles = torch.unique(tile_of_pixels(shape, plan)[rows])
    trips = torch.unique(tiles // plan.grid_m).tolist()
    chans = bad.any(0).nonzero().flatten()
    diff = (got.double() - ref.double()).abs()
    diff = diff[~torch.isnan(diff)]
    return (f"{rows.numel()} of {got.shape[0]} pixels differ in {tiles.numel()} of {plan.ntiles} {plan.th} x {plan.tw} tiles, "
            f"trips {trips} of a grid of {plan.grid_m}; first tiles (image, tile row, tile column) "
            f"{[decode(t, shape, plan) for t in tiles[:6].tolist()]}; {chans.numel()} channels (first {chans[:8].tolist()}); "
            f"max |diff| {diff.max().item() if diff.numel() else float('nan'):g}")


def assert_same(got, ref, shape, plan, what="y"):
    """bit for bit; the failure names tiles and trips"""
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert torch.equal(got, ref), f"{what}: {_where(got, ref, shape, plan)}"


def stats_rows(ref64, shape, plan):
    """(grid_m, 2, n) float64: the partial rows an exact kernel writes -- workgroup b sums the tiles b, b + grid_m, ..."""
    wg = tile_of_pixels(shape, plan) % plan.grid_m
    rows = torch.zeros((plan.grid_m, 2, ref64.shape[1]), dtype=torch.float64)
    rows[:, 0].index_add_(0, wg, ref64)
    rows[:, 1].index_add_(0, wg, ref64 * ref64)
    return rows


def check_sums(rows, want0, want1, plan, names=("sum y", "sum y^2")):
    """partial rows (grid_m, 2, n) summed in float64 against two exact per-channel sums; the failure gives the error as a
    share of the largest tile's part of the sum, which is what one tile lost from a workgroup's running sums amounts to"""
    assert tuple(rows.shape) == (plan.grid_m, 2, want0.shape[0]), (tuple(rows.shape), plan.grid_m)
    s = rows.double().sum(0).cpu()
    for k, want in enumerate((want0, want1)):
        if not torch.equal(s[k], want):
            err = (s[k] - want).abs()
            ch = int(err.argmax())
            raise AssertionError(f"{names[k]}: {int((err > 0).sum())} of {want.numel()} channels off, worst channel {ch} by "
                                 f"{err[ch].item():g} of {want[ch].item():g} ({plan.ntiles} tiles, grid of {plan.grid_m})")


def check_stats(rows, ref64, plan):
    """the BatchNorm partial rows of the STORED values, exactly (assert_exact_preconditions(ref64) is the caller's)"""
    check_sums(rows, ref64.sum(0), (ref64 * ref64).sum(0), plan)
