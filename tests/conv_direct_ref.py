"""TEST INFRASTRUCTURE.  What tests/test_conv_direct_walk.py (CPU) and tests/test_conv_direct_walk_gpu.py share about the two
persistent kernels of csrc/uz_conv3x3.hip -- conv3x3_direct_kernel (weights resident in LDS, streaming with 64 or 128 output
channels) and conv3x3_res64_kernel -- where their workgroups walk several tiles: the restatement of uz_direct_plan(), the
table of maps and cases at which every instantiation walks, integer operands with their exact references, and a comparator
of the per-workgroup statistics rows.  No GPU use.

Everything that does not depend on the kernel comes from tests/conv_pp_ref.py and is used as it stands: both kernels'
decode() numbers tiles as the ping-pong kernel's does, (image * th_n + tile row) * tw_n + tile column, so tile_of_pixels,
decode, assert_same, stats_rows, check_sums, check_stats and the _where diagnostics serve with the Plan of this file (they
read th, tw, ntiles, grid_m of it), and so do ints, nhwc, density, assert_exact_preconditions, bnred_operands, act_vectors,
act_ref.

Why integers (as there): x from {-1, 0, 1}, thinned weights from {-1, 0, 1}, an integer bias in -3..3.  Every product and
every fp32 partial sum is an integer far below 2^24 whatever the order of the sum, so F.conv2d in fp32 on the CPU IS the
float64 result, and that value, rounded once to the run dtype (which changes nothing: asserted), is the only correct output
in bf16 and in fp32 alike.  The operands do not depend on the dtype: a bf16 and an fp32 case of one (map, Cin) share them."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

import conv_pp_ref as P  # tests/conv_pp_ref.py (pytest puts this directory on sys.path)
from conv_pp_ref import (SENTINEL, act_ref, act_vectors, assert_exact_preconditions, assert_same, bnred_operands,  # noqa: F401
                         cdiv, check_stats, check_sums, decode, density, ints, nhwc, stats_rows, tile_of_pixels, _where)

CUS_HW = P.CUS_HW                # UZ_NUM_CU_HW
RESERVE = P.RESERVE              # uz_set_cu_reserve() of the walking cases
CUS = P.CUS                      # UZ_NUM_CU under that reserve: 128
BF16, F32 = torch.bfloat16, torch.float32
DT_NAME = {BF16: "bf16", F32: "f32"}             # as uz_conv_igemm_kernel_name() spells them

Plan = namedtuple("Plan", "form tw th bn ntiles tiles_n grid_m slabs")


def direct_plan(dt, N, H, W, Cin, Nout, cus, up=False, ldy=None):
    """(form, tw, th, bn, ntiles, tiles_n, grid_m, slabs) as uz_direct_plan() decides for a 3x3 convolution (padding 1,
    dilation 1, plain store; up: the nearest x2 upsampled read, H x W the OUTPUT grid) that conv_pp_ref.pp_plan does not take,
    or None where it does (bf16) or where the channel multiples fail.  form: "resident" | "stream" | "res64".  `cus` is
    UZ_NUM_CU = 256 - reserve.  From the source:
        vec = 8 (bf16) | 4 (fp32);  bk = 8 * vec;  Cin, Nout, ldy multiples of vec
        tw = W >= 32 ? 32 : 16;  th = 256 / tw;  ntiles = N * ceil(H / th) * ceil(W / tw)
        bn = Nout <= 64 ? 64 : 128;  bn == 128 && ntiles * ceil(Nout / 128) <= UZ_NUM_CU / 2  ->  bn = 64
        resident iff bn == 64 && Cin == bk
        bf16 && Cin <= 64 && !(Cin == 64 && Nout <= 64)  ->  res64, bn = 64
        tiles_n = ceil(Nout / bn);  grid_m = min(ntiles, max(1, UZ_NUM_CU / tiles_n));  slabs = ceil(Cin / bk)"""
    vec = 8 if dt == BF16 else 4
    bk = 8 * vec
    if Cin % vec or Nout % vec or (Nout if ldy is None else ldy) % vec:
        return None
    if up and (H % 2 or W % 2):
        return None
    if dt == BF16 and P.pp_plan(N, H, W, Cin, Nout, cus, up) is not None:
        return None
    tw = 32 if W >= 32 else 16
    th = 256 // tw
    ntiles = N * cdiv(H, th) * cdiv(W, tw)
    bn = 64 if Nout <= 64 else 128
    if bn == 128 and ntiles * cdiv(Nout, 128) <= cus // 2:
        bn = 64
    form = "resident" if (bn == 64 and Cin == bk) else "stream"
    if dt == BF16 and Cin <= 64 and not (Cin == 64 and Nout <= 64):
        form, bn = "res64", 64
    tiles_n = cdiv(Nout, bn)
    return Plan(form, tw, th, bn, ntiles, tiles_n, min(ntiles, max(1, cus // tiles_n)), cdiv(Cin, bk))


def kernel_name(dt, form, bn, up=False):
    """what uz_conv_igemm_kernel_name() answers: conv3x3_direct_<dt>_bn<bn>[_resident][_up2] | conv3x3_res64_<dt>[_up2]"""
    tail = "_up2" if up else ""
    if form == "res64":
        return f"conv3x3_res64_{DT_NAME[dt]}{tail}"
    return f"conv3x3_direct_{DT_NAME[dt]}_bn{bn}" + ("_resident" if form == "resident" else "") + tail


# ---- the maps: the smallest at which every workgroup makes two trips and some make three, under a reserve of 128 CUs -------
# (N, H, W), tile (th x tw), widest Nout (the Nout of a case is a prefix of the widest one's channels), rows / columns ragged
Map = namedtuple("Map", "shape th tw nout_max rows_ragged cols_ragged")
MAPS = {
    # 258 tiles / 128: rows 12 < 16, columns 16 + 4
    "A16": Map((129, 12, 20), 16, 16, 64, True, True),
    # 260 tiles / 128: rows 8 + 4, columns 32 + 8
    "A32": Map((65, 12, 40), 8, 32, 64, True, True),
    # 198 tiles / 64 at two N tiles (res64, four N tiles: / 32): rows 2 * 8 + 4, columns 32 + 8; tile (0, 0) is whole
    "B32": Map((33, 20, 40), 8, 32, 200, True, True),
    # 132 tiles / 64 at two N tiles (res64, three N tiles: / 42): rows 16 + 4, columns 16 + 4
    "B16": Map((33, 20, 20), 16, 16, 200, True, True),
}
MAX_PIXELS = 31200               # no map is larger

# A case: run dtype, the form and bn it claims, a map, Cin -> Nout, the slabs per tile it claims, the upsampled read
Case = namedtuple("Case", "dt form bn map cin nout slabs up")


def _c(dt, form, bn, m, cin, nout, slabs, up=False):
    return Case(dt, form, bn, m, cin, nout, slabs, up)


def _key(c):
    """cases that share operands follow each other (int_operands keeps one set)"""
    return (c.map, c.cin, c.up)


# Plain forward, bias + statistics.  Slabs per tile ncb = 1 .. 4 give every combination of the two parities the streaming
# form carries from tile to tile: ncb odd flips `par`; ndbl = ceil(9 ncb / 2) = 5, 9, 14, 18 flips, flips, keeps, keeps `dpar`.
# A bf16 streaming tile cannot have one slab (Cin <= 64 goes to res64 or the resident form), so only fp32 holds flip / flip.
PLAIN = sorted([
    # fp32 resident (Cin == 32), one slab
    _c(F32, "resident", 64, "A16", 32, 64, 1), _c(F32, "resident", 64, "A32", 32, 40, 1),
    _c(F32, "resident", 64, "A32", 32, 40, 1, up=True),
    # fp32 streaming, 64 channels
    _c(F32, "stream", 64, "A16", 64, 64, 2), _c(F32, "stream", 64, "A32", 96, 40, 3), _c(F32, "stream", 64, "A32", 128, 64, 4),
    # fp32 streaming, 128 channels
    _c(F32, "stream", 128, "B32", 32, 200, 1), _c(F32, "stream", 128, "B32", 64, 200, 2),
    _c(F32, "stream", 128, "B16", 96, 136, 3), _c(F32, "stream", 128, "B16", 128, 200, 4),
    # bf16 resident (Cin == 64), one slab
    _c(BF16, "resident", 64, "A16", 64, 64, 1), _c(BF16, "resident", 64, "A32", 64, 64, 1),
    _c(BF16, "resident", 64, "A32", 64, 32, 1), _c(BF16, "resident", 64, "A32", 64, 64, 1, up=True),
    # bf16 streaming, 64 channels; 72: the last slab is 8 channels, the rest zero-filled by the descriptor range
    _c(BF16, "stream", 64, "A16", 128, 64, 2), _c(BF16, "stream", 64, "A32", 72, 40, 2),
    _c(BF16, "stream", 64, "A32", 192, 40, 3), _c(BF16, "stream", 64, "A32", 256, 32, 4),
    # bf16 streaming, 128 channels; 72 and 136: partial last slab
    _c(BF16, "stream", 128, "B32", 72, 200, 2), _c(BF16, "stream", 128, "B16", 128, 200, 2),
    _c(BF16, "stream", 128, "B32", 136, 200, 3), _c(BF16, "stream", 128, "B16", 192, 136, 3),
    _c(BF16, "stream", 128, "B16", 256, 200, 4), _c(BF16, "stream", 128, "B32", 72, 200, 2, up=True),
    # res64 (bf16, Cin <= 64); 64 -> 136: three N tiles, grid 42; 40 -> 200: four N tiles, grid 32
    _c(BF16, "res64", 64, "A16", 16, 64, 1), _c(BF16, "res64", 64, "A32", 48, 40, 1), _c(BF16, "res64", 64, "A32", 32, 32, 1),
    _c(BF16, "res64", 64, "B16", 64, 136, 1), _c(BF16, "res64", 64, "B32", 40, 200, 1),
    _c(BF16, "res64", 64, "A32", 32, 32, 1, up=True),
], key=_key)
# x's neighbours in the wider buffer NaN instead of 5.0, once per kernel family: a partial last slab (bf16 streaming), a
# Cin below the slab (res64), fp32
NAN_NEIGHBOURS = [_c(BF16, "stream", 64, "A32", 72, 40, 2), _c(BF16, "res64", 64, "A32", 48, 40, 1),
                  _c(F32, "stream", 64, "A32", 96, 40, 3)]
# fused BatchNorm-backward sums: bf16 only, not res64 (operands of PLAIN without the bias)
BNRED = sorted([_c(BF16, "resident", 64, "A32", 64, 64, 1), _c(BF16, "stream", 64, "A16", 128, 64, 2),
                _c(BF16, "stream", 128, "B32", 136, 200, 3), _c(BF16, "stream", 128, "B16", 192, 136, 3)], key=_key)
# eval-mode epilogue, with and without the ReLU: not res64 (operands of PLAIN)
ACT = sorted([_c(F32, "resident", 64, "A16", 32, 64, 1), _c(F32, "stream", 128, "B32", 64, 200, 2),
              _c(BF16, "resident", 64, "A32", 64, 32, 1), _c(BF16, "stream", 64, "A32", 192, 40, 3),
              _c(BF16, "stream", 128, "B16", 128, 200, 2)], key=_key)
# normal operands, one case per (dtype, form)
NORMAL = [_c(F32, "resident", 64, "A16", 32, 64, 1), _c(F32, "stream", 64, "A16", 64, 64, 2),
          _c(F32, "stream", 128, "B16", 96, 136, 3), _c(BF16, "resident", 64, "A16", 64, 64, 1),
          _c(BF16, "stream", 64, "A16", 128, 64, 2), _c(BF16, "stream", 128, "B16", 128, 200, 2),
          _c(BF16, "res64", 64, "A16", 16, 64, 1), _c(BF16, "res64", 64, "B16", 64, 136, 1)]

ALL_CASES = sorted(dict.fromkeys(PLAIN + NAN_NEIGHBOURS + BNRED + ACT + NORMAL), key=_key)


def case_id(c):
    form = c.form if c.form == "res64" else f"{c.form}{c.bn}"
    return f"{DT_NAME[c.dt]}-{form}-{c.map}-cin{c.cin}-n{c.nout}" + ("-up2" if c.up else "")


def case_plan(c, cus=CUS):
    N, H, W = MAPS[c.map].shape
    return direct_plan(c.dt, N, H, W, c.cin, c.nout, cus, c.up)


def case_kernel_name(c):
    return kernel_name(c.dt, c.form, c.bn, c.up)


def assert_walks(c, plan):
    """the walk conditions from the restated plan alone: the form, tile and bn the case claims; every workgroup makes at
    least two trips through the tile loop and some make three; ragged as the map claims"""
    m = MAPS[c.map]
    N, H, W = m.shape
    assert plan is not None, c
    assert (plan.form, plan.bn, plan.tw, plan.th, plan.slabs) == (c.form, c.bn, m.tw, m.th, c.slabs), (plan, c)
    assert plan.ntiles >= 2 * plan.grid_m + 1, plan
    assert (H % plan.th != 0) == m.rows_ragged and (W % plan.tw != 0) == m.cols_ragged, (H, W, plan)
    assert c.nout <= m.nout_max and N * H * W <= MAX_PIXELS
    if c.up:
        assert H % 2 == 0 and W % 2 == 0


# ---- integer operands and their exact references ---------------------------------------------------------------------------
Operands = namedtuple("Operands", "x w b prod")


@functools.lru_cache(maxsize=1)
def int_operands(map_name, cin, up):
    """x (N, Cin, Hi, Wi) as the kernel reads it (half resolution when up), w (widest Nout, Cin, 3, 3), integer bias, and the
    exact product (N H W, widest Nout) WITHOUT the bias in fp32 -- as conv_pp_ref.int_operands, for any Cin.  density(): 4 Cin
    density = 48 from Cin 12 on, sigma 7: |y| stays far below the 256 a bf16 integer may reach, and sum y^2 over the at most
    31200 pixels of a map about 1.5e6 against the 2^24 of the exact-statistics precondition (both asserted by the CPU file)"""
    m = MAPS[map_name]
    N, H, W = m.shape
    Hi, Wi = (H // 2, W // 2) if up else (H, W)
    g = torch.Generator().manual_seed(1000 * cin + 7 * H + W + (1 if up else 0))
    w = ints(g, (m.nout_max, cin, 3, 3))
    w = w * (torch.rand(w.shape, generator=g) < density(cin, "int")).float()
    b = ints(g, (m.nout_max,), -3, 3)
    x = ints(g, (N, cin, Hi, Wi))
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    prod = nhwc(F.conv2d(xin, w, None, padding=1))
    assert bool((prod == prod.round()).all()) and prod.abs().max().item() < 2 ** 20     # fp32 on integers: exact
    return Operands(x, w, b, prod)


def operands(c):
    return int_operands(c.map, c.cin, c.up)


def plain_ref(c, with_bias=True):
    """float64 (N H W, Nout): the exact convolution [+ bias] of a case"""
    o = operands(c)
    y = o.prod[:, :c.nout].double()
    return y + o.b[:c.nout].double() if with_bias else y


# ---- the per-workgroup rows ------------------------------------------------------------------------------------------------
def check_rows(rows, ref64, shape, plan):
    """the BatchNorm partial rows (grid_m, 2, n) of the STORED values against stats_rows(), row for row and exactly
    (assert_exact_preconditions(ref64) is the caller's): workgroup b owns the tiles b, b + grid_m, ...  A workgroup that
    loses the sums of one tile shows here even if another workgroup gains them; the failure names the workgroups, and for
    the first of them what its rows lack as a share of each of its trips"""
    assert tuple(rows.shape) == (plan.grid_m, 2, ref64.shape[1]), (tuple(rows.shape), plan.grid_m, ref64.shape[1])
    got = rows.double().cpu()
    want = stats_rows(ref64, shape, plan)
    if torch.equal(got, want):
        return
    bad = (got != want).any(2).any(1).nonzero().flatten()
    b = int(bad[0])
    ch = int((got[b] != want[b]).any(0).nonzero().flatten()[0])
    tiles = tile_of_pixels(shape, plan)
    trips = []
    for t in range(b, plan.ntiles, plan.grid_m):
        part = ref64[tiles == t, ch]
        trips.append((t // plan.grid_m, part.sum().item(), (part * part).sum().item()))
    raise AssertionError(f"statistics rows: {bad.numel()} of {plan.grid_m} workgroups differ (first {bad[:8].tolist()}); workgroup "
                         f"{b}, channel {ch}: (sum y, sum y^2) got {got[b, :, ch].tolist()}, want {want[b, :, ch].tolist()}; its "
                         f"tiles' parts as (trip, sum y, sum y^2): {trips}")
