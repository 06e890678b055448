"""Helper of tests/test_wgrad_walk.py and tests/test_wgrad_walk_gpu.py (not a test module): the launch plans of the
weight-gradient family restated in Python, and the ONE table of cases both files walk.

Restated (tune flags 0, as in every production build):
  plan9()      uz_wgrad9_plan     (uz_wgrad9.hip): which nine-tap problems the row walk takes, and its split rule
  plan_g4()    uz_wgrad_g4_plan   (uz_wgrad_g4.hip): the bf16 2 x 2 gather
  plan3x3()    uz_wgrad3x3_plan   (uz_wgrad3x3.hip): one-tap / batched / stride-2 / dilated / short-map nine-tap forms
  make_plan()  make_plan          (uz_wgrad.hip): the generic kernel's tile, split and chunk
  multi_plan() multi_plan         (uz_wgrad.hip): per-problem split of the shared one-tap launches of uz_wgrad_multi
  reduce_form()                   which of the six slab reductions wgrad_phases() launches

A case is a descriptor (D), the reserve it runs under, the kernel name it claims and a dict of claims about the loop state
it exists for; check_claims() asserts them from the restated plan alone."""
import heapq
from collections import namedtuple

CUS_HW = 256
CONV, GATHER2X2, CONV_UP2, CONV_S2 = 0, 1, 2, 3

D = namedtuple("D", "dt N H W Hr Wr Ci ldl Cj ldr ntaps mode dil")


def cdiv(a, b):
    return -(-a // b)


def desc(dt, N, H, W, Ci, Cj, ntaps=1, mode=CONV, dil=1, Hr=None, Wr=None, ldl=None, ldr=None):
    if Hr is None:
        Hr, Wr = {CONV: (H, W), CONV_UP2: (H // 2, W // 2), GATHER2X2: (2 * H, 2 * W)}[mode]
    return D(dt, N, H, W, Hr, Wr, Ci, ldl or Ci, Cj, ldr or Cj, ntaps, mode, dil)


def _lds_width(W):
    return W == 16 or W == 32 or (W >= 64 and W % 64 == 0)


def _ranges(units, upb):
    """K-steps of every pixel range: [upb, upb, ..., last]"""
    split = cdiv(units, upb)
    return [min(upb, units - z * upb) for z in range(split)]


def plan9(d, cus):
    up = d.mode == CONV_UP2
    if d.dt != "bf16" or not (d.mode == CONV or up) or d.ntaps != 9 or d.dil != 1:
        return None
    if d.Ci % 8 or d.Cj % 8 or not _lds_width(d.W):
        return None
    kw = min(d.W, 64)
    g = 64 // kw
    if d.H % g:
        return None
    nsl = 5 if kw == 16 else 6                     # W9<64, KW>::NSL
    hsteps = d.H // g
    if hsteps < nsl - 1:
        return None
    units = d.N * (d.W // kw) * hsteps
    ntiles = cdiv(d.Ci, 64) * cdiv(d.Cj, 64)
    split = 1 if ntiles >= cus else cus // ntiles
    split = min(split, max(units // 8, 1))
    if split > 8:
        split -= split % 8
    split = max(split, 1)
    upb = cdiv(units, split)
    return dict(kind="v9", name="wgrad9_bf16_64x64_rowwalk", units=units, upb=upb, split=cdiv(units, upb),
                nslabs=cdiv(units, upb))


def plan_g4(d, cus):
    if d.dt != "bf16" or d.mode != GATHER2X2 or d.ntaps != 4 or d.Ci % 8 or d.Cj % 8 or not _lds_width(d.W):
        return None
    kw = min(d.W, 64)
    g = 64 // kw
    if d.H % g:
        return None
    units = d.N * (d.W // kw) * (d.H // g)
    bi = 128 if d.Ci > 64 else 64
    ntiles = cdiv(d.Ci, bi) * cdiv(d.Cj, 64)
    split = 1 if ntiles >= cus else cus // ntiles
    split = min(split, max(units // 4, 1))
    if split > 8:
        split -= split % 8
    split = max(split, 1)
    upb = cdiv(units, split)
    return dict(kind="g4", name=f"wgrad_g4_bf16_{bi}x64_4tap", units=units, upb=upb, split=cdiv(units, upb),
                nslabs=cdiv(units, upb))


def plan3x3(d, cus, batch=1):
    """uz_wgrad3x3_plan: None where the LDS-DMA kernels decline.  Keys: name, tile (bi, bj), tiles, kw, kr, H, W (as the
    kernel walks them), units, upb, split = nslabs, nus (K-steps of every range), upi / upr (K-steps per image / per row
    block), remap (the XCD id remap of the three-tap form is on)"""
    if batch == 1:
        p = plan9(d, cus) or plan_g4(d, cus)
        if p:
            return p
    up = d.mode == CONV_UP2
    s2 = d.mode == CONV_S2 and d.ntaps == 9
    dil9 = d.mode == CONV and d.ntaps == 9 and d.dil > 1
    gather = (d.mode == GATHER2X2 and d.ntaps == 4) or s2 or dil9
    if d.dt != "bf16" or not (d.mode == CONV or up or gather):
        return None
    if not ((d.ntaps == 9 and d.dil == 1) or (d.ntaps == 1 and not up) or gather):
        return None
    one_tap = d.ntaps == 1 or gather
    gcode = 3 if dil9 else (2 if s2 else (1 if gather else 0))
    if d.Ci % 8 or d.Cj % 8:
        return None
    W, H, nimg = d.W, d.H, d.N
    P = d.N * d.H * d.W
    if one_tap and not gather:
        W, H, nimg = 64, cdiv(P, 64), 1
    if not _lds_width(W):
        return None
    kw = min(W, 64)
    ok9 = not one_tap and not gather
    wide9 = 0
    if ok9 and d.Ci % 128 == 0 and d.Cj % 64 == 0 and ((d.Cj == 64 and P >= 1 << 19) or (d.Cj >= 1024 and d.Ci >= 512)):
        wide9 = 1
    elif ok9 and d.Ci == 64 and d.Cj % 128 == 0:
        wide9 = 2
    if wide9 and W >= 32:
        kw = 16
    if not wide9 and not one_tap and W >= 64 and not (d.Ci % 128 == 0 and d.Cj % 128 == 0):
        kw = 16
    kr = 64 // kw
    if H % kr:
        return None
    if ((P - 1) * d.ldl + d.Ci) * 2 >= 1 << 31 or ((d.N * d.Hr * d.Wr - 1) * d.ldr + d.Cj) * 2 >= 1 << 31:
        return None
    big = d.Ci % 128 == 0 and d.Cj % 128 == 0 and not wide9
    if one_tap and not big:
        t64 = d.Ci * cdiv(d.Cj, 64) + d.Cj * cdiv(d.Ci, 64)
        t128 = d.Ci * cdiv(d.Cj, 128) + d.Cj * cdiv(d.Ci, 128)
        big = t128 < t64
    b = 128 if big else 64
    bi, bj = (128 if wide9 == 1 else b), (128 if wide9 == 2 else b)
    tiles = cdiv(d.Ci, bi) * cdiv(d.Cj, bj)
    units = nimg * H * W // 64
    if batch > 1 and not (one_tap and not gather):
        return None
    base = tiles * (3 if (big and not one_tap) else (d.ntaps if gather else 1)) * batch
    split = 1 if base >= cus else cus // base
    split = max(1, min(split, max(units // 8, 1), 256))
    upb = cdiv(units, split)
    sp = cdiv(units, upb)
    if big and not one_tap:
        for ds in range(8):
            s = split - ds
            if s < 1:
                break
            upb2 = cdiv(units, s)
            sp2 = cdiv(units, upb2)
            if (tiles * sp2) % 8 == 0:
                upb, sp = upb2, sp2
                break
    tile = f"{bi}x{bj}"
    if gcode == 3:
        name = f"wgrad3x3_bf16_{tile}_dilated9"
    elif gcode:
        name = f"wgrad3x3_bf16_{tile}_gather{d.ntaps}"
    elif one_tap:
        name = f"wgrad3x3_bf16_{tile}_1tap"
    else:
        name = f"wgrad3x3_bf16_{tile}_{'3tap' if big else '9tap'}"
    return dict(kind="3x3", name=name, tile=(bi, bj), tiles=tiles, kw=kw, kr=kr, H=H, W=W, units=units, upb=upb, split=sp,
                nslabs=sp, nus=_ranges(units, upb), upi=(H * W) // 64, upr=W // kw,
                remap=bool(big and not one_tap and (tiles * sp) % 8 == 0), base=base)


def make_plan(d, cus):
    """make_plan of uz_wgrad.hip: (tile edge, tiles, split, chunk, nks) -- nks the K-steps of every pixel range"""
    bkp = 64 if d.dt == "bf16" else 32
    P = d.N * d.H * d.W
    b = 128 if (d.Ci > 64 and d.Cj > 64) else 64
    tiles = cdiv(d.Ci, b) * cdiv(d.Cj, b)
    base = tiles * d.ntaps
    split = cdiv(4 * cus, base)
    split = max(1, min(split, min(max(P // (4 * bkp), 1), 64)))
    chunk = cdiv(cdiv(P, split), bkp) * bkp
    split = cdiv(P, chunk)
    nks = [cdiv(min(chunk, P - z * chunk), bkp) for z in range(split)]
    return dict(kind="generic", name=f"wgrad_{d.dt}_{b}x{b}", b=b, tiles=tiles, split=split, nslabs=split, chunk=chunk,
                bkp=bkp, nks=nks, P=P)


def plan(d, cus):
    """the plan uz_wgrad runs for d: the LDS-DMA family's where it applies, else the generic kernel's"""
    return plan3x3(d, cus) or make_plan(d, cus)


def workspace_bytes(d, cus):
    return plan(d, cus)["nslabs"] * d.ntaps * d.Ci * d.Cj * 4


def batched_workspace_bytes(d, batch, cus):
    p = plan3x3(d, cus, batch)
    return batch * p["nslabs"] * d.Ci * d.Cj * 4 if p else workspace_bytes(d, cus)


def reduce_form(d, nslabs):
    cicj = d.Ci * d.Cj
    if d.ntaps == 9:
        if nslabs >= 32 and cicj % 4 == 0 and cicj <= 64 * 128:
            return "flat<9,16>"
        return "reduce<9,16>" if nslabs >= 32 else "reduce<9,4>"
    return "reduce<4,4>" if d.ntaps == 4 else "reduce<1,4>"


def _makespan(plans, T):
    cu = [0] * CUS_HW
    end = 0
    for p in plans:
        upb = min(p["units"], T)
        upb = cdiv(p["units"], cdiv(p["units"], upb))
        for _ in range(p["tiles"] * cdiv(p["units"], upb)):
            t = heapq.heappop(cu) + upb + 6
            end = max(end, t)
            heapq.heappush(cu, t)
    return end


def multi_plan(descs, cus):
    """per problem: None (goes through uz_wgrad on its own) or dict(big, tiles, units, upb, split, first, launch) for the
    shared launches; plus the workspace total.  Launch order: tile shape, longest pixel list first (stable); 24 per launch"""
    p2 = [plan3x3(d, cus) for d in descs]
    tog = [p is not None and p["kind"] == "3x3" and p["name"].endswith("_1tap") and d.ntaps == 1 for p, d in zip(p2, descs)]
    steps = sum(p["units"] * p["tiles"] for p, t in zip(p2, tog) if t)
    Tmax = min(max(steps // (4 * cus), 8), 64)
    order = []
    for big in (False, True):
        idx = [i for i in range(len(descs)) if tog[i] and (p2[i]["tile"][0] == 128) == big]
        order += sorted(idx, key=lambda i: -p2[i]["units"])          # sorted() is stable
    out = [None] * len(descs)
    launch = 0
    beg = 0
    while beg < len(order):
        end = beg
        while end < len(order) and end - beg < 24 and p2[order[end]]["tile"] == p2[order[beg]]["tile"]:
            end += 1
        best, bestT = -1, Tmax
        T = Tmax
        while T >= (Tmax + 1) // 2 and T >= 8:
            m = _makespan([p2[i] for i in order[beg:end]], T)
            if best < 0 or m < best:
                best, bestT = m, T
            T -= 2
        first = 0
        for i in order[beg:end]:
            p = p2[i]
            upb = min(p["units"], bestT)
            upb = cdiv(p["units"], cdiv(p["units"], upb))
            split = cdiv(p["units"], upb)
            out[i] = dict(big=p["tile"][0] == 128, tiles=p["tiles"], units=p["units"], upb=upb, split=split, first=first,
                          launch=launch, nus=_ranges(p["units"], upb))
            first += p["tiles"] * split
        launch += 1
        beg = end
    total = 0
    for i, d in enumerate(descs):
        b = out[i]["split"] * d.Ci * d.Cj * 4 if out[i] else workspace_bytes(d, cus)
        total += (b + 255) & ~255
    return out, total


# ---- the cases ----------------------------------------------------------------------------------------------------------------
# Product cases of uz_wgrad (sections 1, 4, 5, 6 of the GPU file).  claims:
#   nus / nks      exact list of K-steps per pixel range (LDS-DMA kernels / generic kernel)
#   nslabs         number of slabs
#   remap          the three-tap form's XCD remap is on / off
#   mid_image      some range starts inside an image (u_beg % upi != 0)
#   mid_row        some range starts at the second 64-column strip of a row (kw = 64, W = 128, odd u_beg)
#   ragged         P % 64
#   img_wraps      generic kernel: images per K-step >= 2 (H * W < BKP, N >= 5)
#   row_wraps      generic kernel: rows per K-step >= this
#   ragged_chunks  generic kernel: split > 1, P % chunk != 0 and P % BKP != 0
Case = namedtuple("Case", "id d reserve name claims window phase1 random")


def _c(id, d, name, reserve=0, window=False, phase1=False, random=False, **claims):
    return Case(id, d, reserve, name, claims, window, phase1, random)


B, F = "bf16", "fp32"
T64, T128 = "wgrad3x3_bf16_64x64_", "wgrad3x3_bf16_128x128_"

PRODUCT_CASES = [
    # -- 1. one-tap, 64 x 64 tile (Ci, Cj <= 64: the only channels at which t128 < t64 fails) and 128 x 128 tile
    _c("1tap64-nu1-whole", desc(B, 1, 1, 64, 64, 64), T64 + "1tap", nus=[1]),
    _c("1tap64-nu1-ragged1", desc(B, 1, 1, 1, 64, 64), T64 + "1tap", window=True, nus=[1], ragged=1),
    _c("1tap64-nu2", desc(B, 1, 2, 64, 64, 64), T64 + "1tap", nus=[2]),
    _c("1tap64-nu3-ragged63", desc(B, 1, 1, 191, 64, 64), T64 + "1tap", window=True, nus=[3], ragged=63),
    _c("1tap64-nu4", desc(B, 1, 4, 64, 64, 64), T64 + "1tap", nus=[4]),
    _c("1tap64-nu7", desc(B, 1, 7, 64, 64, 64), T64 + "1tap", nus=[7], phase1=True),
    _c("1tap64-nu10", desc(B, 1, 10, 64, 64, 64), T64 + "1tap", nus=[10], random=True),
    _c("1tap64-8x9+1-ragged1", desc(B, 1, 1, 72 * 64 + 1, 64, 64), T64 + "1tap", window=True, nus=[9] * 8 + [1], ragged=1),
    _c("1tap64-tails-40x24", desc(B, 1, 1, 16 * 64 + 63, 40, 24), T64 + "1tap", window=True, nus=[9, 8], ragged=63),
    _c("1tap128-nu1-whole", desc(B, 1, 1, 64, 128, 128), T128 + "1tap", nus=[1]),
    _c("1tap128-nu2", desc(B, 1, 2, 64, 128, 128), T128 + "1tap", nus=[2]),
    _c("1tap128-nu3", desc(B, 1, 3, 64, 256, 128), T128 + "1tap", nus=[3]),
    _c("1tap128-nu4", desc(B, 1, 4, 64, 128, 128), T128 + "1tap", nus=[4]),
    _c("1tap128-nu5-ragged1", desc(B, 1, 1, 257, 128, 128), T128 + "1tap", window=True, nus=[5], ragged=1),
    _c("1tap128-nu6", desc(B, 1, 6, 64, 128, 256), T128 + "1tap", nus=[6], phase1=True, random=True),
    _c("1tap128-8x9+1-ragged63", desc(B, 1, 1, 72 * 64 + 63, 128, 128), T128 + "1tap", window=True, nus=[9] * 8 + [1], ragged=63),
    _c("1tap128-tails-72x40", desc(B, 7, 7, 14, 72, 40), T128 + "1tap", window=True, nus=[11], ragged=46),
    _c("1tap128-288x96", desc(B, 3, 14, 14, 288, 96), T128 + "1tap", window=True, nus=[10], ragged=12),
    # the same problem under two reserves: 16 tiles, split 256 / 16 = 16 against 128 / 16 = 8
    _c("1tap128-512x512-r0", desc(B, 2, 64, 64, 512, 512), T128 + "1tap", nus=[8] * 16),
    _c("1tap128-512x512-r128", desc(B, 2, 64, 64, 512, 512), T128 + "1tap", reserve=128, nus=[16] * 8),
    # -- 4. stride-2 and dilated gathers, both tiles; odd Hr x Wr for stride 2
    _c("s2-64-odd", desc(B, 3, 4, 16, 64, 64, 9, CONV_S2, Hr=7, Wr=31), T64 + "gather9", nus=[3], mid_image=False, phase1=True),
    _c("s2-64-split", desc(B, 7, 6, 32, 64, 64, 9, CONV_S2, Hr=11, Wr=63), T64 + "gather9", nus=[11, 10], mid_image=True,
       random=True),
    _c("s2-128-even", desc(B, 3, 16, 16, 128, 128, 9, CONV_S2, Hr=32, Wr=32), T128 + "gather9", nus=[12], mid_image=False, phase1=True, random=True),
    _c("s2-128-split-odd", desc(B, 7, 12, 16, 128, 256, 9, CONV_S2, Hr=23, Wr=31), T128 + "gather9", window=True, nus=[11, 10],
       mid_image=True),
    _c("dil2-64", desc(B, 3, 12, 16, 64, 64, 9, dil=2), T64 + "dilated9", nus=[9], phase1=True, random=True),
    _c("dil8-64-split", desc(B, 7, 12, 16, 64, 40, 9, dil=8), T64 + "dilated9", window=True, nus=[11, 10], mid_image=True),
    _c("dil2-128-split", desc(B, 3, 8, 64, 128, 128, 9, dil=2), T128 + "dilated9", nus=[8, 8, 8], mid_image=False, random=True),
    _c("dil8-128-split", desc(B, 9, 4, 32, 128, 128, 9, dil=8), T128 + "dilated9", nus=[9, 9], mid_image=True, phase1=True),
    # -- 5. nine-tap forms on short maps
    _c("3tap-w16h4-noremap", desc(B, 8, 4, 16, 128, 128, 9), T128 + "3tap", nus=[8], remap=False),
    _c("3tap-w16h12-remap", desc(B, 7, 12, 16, 256, 256, 9), T128 + "3tap", nus=[11, 10], remap=True, mid_image=True,
       phase1=True, random=True),
    _c("3tap-w32h2", desc(B, 9, 2, 32, 128, 128, 9), T128 + "3tap", nus=[9], remap=False),
    _c("3tap-w32h8", desc(B, 5, 8, 32, 128, 128, 9), T128 + "3tap", nus=[10, 10], remap=False, mid_image=True),
    _c("3tap-w64h3", desc(B, 7, 3, 64, 128, 128, 9), T128 + "3tap", nus=[11, 10], remap=False, mid_image=True),
    _c("3tap-w128h3-midrow", desc(B, 3, 3, 128, 128, 128, 9), T128 + "3tap", nus=[9, 9], remap=False, mid_row=True),
    _c("3tap-w128h2-up2", desc(B, 4, 2, 128, 128, 128, 9, CONV_UP2), T128 + "3tap", nus=[8, 8], remap=False),
    _c("9tap64-w16h8", desc(B, 5, 8, 16, 64, 64, 9), T64 + "9tap", nus=[10], phase1=True, random=True),
    _c("9tap64-w32h4", desc(B, 9, 4, 32, 72, 40, 9), T64 + "9tap", window=True, nus=[9, 9], mid_image=True),
    _c("9tap64-w64h4", desc(B, 5, 4, 64, 64, 64, 9), T64 + "9tap", nus=[10, 10], mid_image=True),
    _c("9tap64-w128h4-up2", desc(B, 3, 4, 128, 64, 64, 9, CONV_UP2), T64 + "9tap", nus=[8, 8, 8], mid_image=False),
    _c("9tap64x128-w16h4", desc(B, 9, 4, 16, 64, 128, 9), "wgrad3x3_bf16_64x128_9tap", nus=[9], phase1=True),
    _c("9tap64x128-w32h8", desc(B, 5, 8, 32, 64, 128, 9), "wgrad3x3_bf16_64x128_9tap", nus=[10, 10], mid_image=True, random=True),
    _c("9tap128x64-w64h4", desc(B, 1, 4, 64, 512, 1024, 9), "wgrad3x3_bf16_128x64_9tap", nus=[4], phase1=True),
    _c("9tap128x64-w16h4", desc(B, 3, 4, 16, 512, 1024, 9), "wgrad3x3_bf16_128x64_9tap", nus=[3], random=True),
    # -- 6. the generic kernel: fp32 everywhere, bf16 on widths the LDS-DMA plans decline
    _c("gen-f32-64-4x4-wraps", desc(F, 7, 4, 4, 64, 64, 9), "wgrad_fp32_64x64", nks=[4], img_wraps=2, phase1=True),
    _c("gen-f32-128-3x5-wraps", desc(F, 9, 3, 5, 68, 132, 9), "wgrad_fp32_128x128", window=True, nks=[5], img_wraps=2, phase1=True),
    _c("gen-bf16-64-4x4-wraps", desc(B, 21, 4, 4, 64, 64, 9), "wgrad_bf16_64x64", nks=[6], img_wraps=4, phase1=True),
    _c("gen-bf16-128-3x5-wraps", desc(B, 19, 3, 5, 72, 136, 9), "wgrad_bf16_128x128", window=True, nks=[5], img_wraps=4, phase1=True),
    _c("gen-f32-64-w5-split", desc(F, 3, 19, 5, 64, 64, 1), "wgrad_fp32_64x64", nks=[5, 4], row_wraps=6, ragged_chunks=True),
    _c("gen-f32-128-w7-split", desc(F, 2, 39, 7, 68, 132, 9), "wgrad_fp32_128x128", window=True, nks=[5, 5, 5, 3], row_wraps=4,
       ragged_chunks=True, random=True),
    _c("gen-f32-64-dil2", desc(F, 3, 9, 7, 68, 36, 9, dil=2), "wgrad_fp32_64x64", window=True, nks=[6], row_wraps=4),
    _c("gen-f32-64-dil-beyond", desc(F, 2, 6, 5, 64, 64, 9, dil=7), "wgrad_fp32_64x64", nks=[2], row_wraps=6, random=True),
    _c("gen-f32-64-up2", desc(F, 3, 6, 10, 64, 36, 9, CONV_UP2), "wgrad_fp32_64x64", window=True, nks=[6]),
    _c("gen-f32-128-up2", desc(F, 2, 8, 14, 68, 132, 9, CONV_UP2), "wgrad_fp32_128x128", nks=[7]),
    _c("gen-f32-64-gather-2h", desc(F, 3, 5, 7, 64, 36, 4, GATHER2X2), "wgrad_fp32_64x64", window=True, nks=[4], row_wraps=4),
    _c("gen-f32-128-gather-2h+1", desc(F, 3, 5, 7, 68, 132, 4, GATHER2X2, Hr=11, Wr=15), "wgrad_fp32_128x128", nks=[4], row_wraps=4),
    _c("gen-bf16-64-w8", desc(B, 3, 9, 8, 64, 64, 9), "wgrad_bf16_64x64", nks=[4], row_wraps=8),
    _c("gen-bf16-128-w12-split", desc(B, 5, 21, 12, 72, 136, 9), "wgrad_bf16_128x128", window=True, nks=[5, 5, 5, 5],
       ragged_chunks=True, random=True),
    _c("gen-bf16-64-w20-tails", desc(B, 2, 7, 20, 72, 40, 9), "wgrad_bf16_64x64", window=True, nks=[5]),
    _c("gen-bf16-64-w20-split", desc(B, 13, 5, 20, 40, 24, 9), "wgrad_bf16_64x64", window=True, nks=[5, 5, 5, 5, 1], ragged_chunks=True,
       random=True),
]


def check_claims(c, p):
    """the loop state the case exists for, from the restated plan p of c.d under c.reserve"""
    d, cl = c.d, c.claims
    assert p["name"] == c.name, (c.id, p["name"])
    said = []
    if "nus" in cl:
        assert p["kind"] == "3x3" and p["nus"] == cl["nus"], (c.id, p["nus"])
        said.append(f"nu {p['nus']}")
    if "nks" in cl:
        assert p["kind"] == "generic" and p["nks"] == cl["nks"], (c.id, p["nks"], p)
        said.append(f"nk {p['nks']}")
    if "nslabs" in cl:
        assert p["nslabs"] == cl["nslabs"], (c.id, p["nslabs"])
    if "remap" in cl:
        assert p["name"].endswith("3tap") and p["remap"] == cl["remap"], (c.id, p["tiles"], p["split"])
        said.append(f"remap {'on' if p['remap'] else 'off'} ({p['tiles']} tiles x {p['split']})")
    if "mid_image" in cl:
        got = any((z * p["upb"]) % p["upi"] for z in range(1, p["split"]))
        assert got == cl["mid_image"] and (d.N > 1 or not got), (c.id, p["upb"], p["upi"])
        said.append("a range starts inside an image" if got else "ranges start on images")
    if cl.get("mid_row"):
        assert p["kw"] == 64 and p["upr"] == 2 and any((z * p["upb"]) % 2 for z in range(1, p["split"])), (c.id, p)
        said.append("a range starts at the second strip of a row")
    if "ragged" in cl:
        assert (d.N * d.H * d.W) % 64 == cl["ragged"], c.id
        said.append(f"P % 64 = {cl['ragged']}")
    if "img_wraps" in cl:
        assert d.N >= 5 and p["bkp"] // (d.H * d.W) >= cl["img_wraps"], c.id
        said.append(f"{p['bkp'] // (d.H * d.W)} image wraps per K-step")
    if "row_wraps" in cl:
        assert p["bkp"] // d.W >= cl["row_wraps"], c.id
        said.append(f"{p['bkp'] // d.W} row wraps per K-step")
    if cl.get("ragged_chunks"):
        assert p["split"] > 1 and p["P"] % p["chunk"] and p["P"] % p["bkp"], (c.id, p)
        said.append(f"P {p['P']} in chunks of {p['chunk']}")
    return f"{c.id}: {p['name']}, nslabs {p['nslabs']}, " + ", ".join(said)


# ---- reduction cases (section 7): descriptors whose plan gives the wanted slab count ---------------------------------------------
# (id, descriptor, reserve, form, nslabs).  The row-walk plan of a 64 x 64-channel, W = 64 problem gives nslabs =
# min(cus, units / 8) rounded down to a multiple of 8 above 8: the map's height and the reserve select the count.
RCase = namedtuple("RCase", "id d reserve form nslabs random")


def _rw(C1, C2, units):
    """bf16 nine-tap row-walk descriptor with `units` K-steps: one image of `units` rows of 64 pixels"""
    return desc(B, 1, units, 64, C1, C2, 9)


REDUCE_CASES = [RCase(f"r94-{s}", _rw(64, 64, 8 * s + 3), 0, "reduce<9,4>", s, s == 5) for s in (1, 2, 4, 5, 8)] + [
    RCase("r94-9", desc(F, 1, 36, 32, 64, 64, 9), 0, "reduce<9,4>", 9, False),           # generic kernel: P / 128 ranges
    RCase("r94-31", desc(F, 1, 124, 32, 64, 64, 9), 0, "reduce<9,4>", 31, False),
] + [RCase(f"flat-{s}", _rw(64, 64, 8 * s), 0, "flat<9,16>", s, s == 40) for s in (32, 40, 48, 56)] + [
    RCase("flat-cicj64-33", desc(B, 132, 8, 16, 8, 8, 9), 0, "flat<9,16>", 33, False),    # 144 columns of four: 2.25 workgroups
    RCase("flat-straddle-64", _rw(24, 8, 512), 0, "flat<9,16>", 64, True),               # Ci Cj = 192: columns 0 .. 255 of a workgroup straddle a tap
    RCase("flat-tail-12x20", desc(F, 8, 32, 32, 12, 20, 9), 0, "flat<9,16>", 64, False),
] + [RCase(f"r916-{s}", _rw(128, 128, 8 * s), 0, "reduce<9,16>", s, s == 40) for s in (32, 40, 48, 56)] + [
    RCase(f"r44-{s}", desc(B, 1, 4 * s, 64, 64, 64, 4, GATHER2X2), 0, "reduce<4,4>", s, s == 5) for s in (1, 3, 4, 5, 8)
] + [RCase("r44-9", desc(F, 1, 36, 32, 64, 64, 4, GATHER2X2), 0, "reduce<4,4>", 9, False)] + [
    RCase(f"r14-{s}", desc(B, 1, 8 * s, 64, 64, 64, 1), 0, "reduce<1,4>", s, s == 5) for s in (1, 3, 4, 5, 8, 9)
] + [
    # fp32, Ci Cj % 64 != 0: the last workgroup's e < CiCj tail
    RCase("r94-tail-12x20", desc(F, 1, 12, 32, 12, 20, 9), 0, "reduce<9,4>", 3, True),
    RCase("r916-tail-100x84", desc(F, 8, 32, 32, 100, 84, 9), 0, "reduce<9,16>", 64, False),
    RCase("r44-tail-12x20", desc(F, 1, 20, 32, 12, 20, 4, GATHER2X2), 0, "reduce<4,4>", 5, False),
    RCase("r14-tail-12x20", desc(F, 1, 36, 32, 12, 20, 1), 0, "reduce<1,4>", 9, False),
]


# ---- batched one-tap products (section 2): uz_wgrad_batched2 on bf16 token maps -----------------------------------------------
# P tokens per problem, batch x heads problems of C x KV channels; gap: floats between results (ob = C * KV + gap).
# claims: nus (K-steps of every range of one problem), forced (base >= cus alone brings the split down to 1)
BCase = namedtuple("BCase", "id P batch heads C KV reserve gap name nus forced")

BATCHED_CASES = [
    BCase("direct-64-gap", 200, 5, 1, 64, 64, 0, 24, T64 + "1tap", [4], False),            # nslabs 1: written in place, ob > Ci Cj
    BCase("direct-128-gap", 330, 3, 1, 128, 136, 0, 8, T128 + "1tap", [6], False),
    BCase("split-64", 1100, 3, 1, 64, 64, 0, 0, T64 + "1tap", [9, 9], False),               # wgrad_reduce_kernel<1,4>, gridDim.y 3
    BCase("split-128-gap", 1217, 3, 1, 128, 128, 0, 40, T128 + "1tap", [10, 10], False),
    BCase("heads-direct", 200, 2, 3, 64, 32, 0, 0, T64 + "1tap", [4], False),               # lb2 = 64 against rb2 = 32
    BCase("heads-split", 1100, 2, 3, 64, 32, 0, 16, T64 + "1tap", [9, 9], False),           # gridDim.y = 6
    BCase("batch-forces-split-1", 1100, 130, 1, 64, 64, 128, 0, T64 + "1tap", [18], True),
]


def batched_desc(c):
    return desc(B, 1, 1, c.P, c.C, c.KV, ldl=c.heads * c.C, ldr=c.heads * c.KV)


def check_batched_claims(c):
    cus = CUS_HW - c.reserve
    p = plan3x3(batched_desc(c), cus, c.batch * c.heads)
    assert p and p["name"] == c.name and p["nus"] == c.nus, (c.id, p)
    if c.forced:
        assert p["base"] >= cus and p["units"] // 8 >= 2 and p["split"] == 1, (c.id, p)
    return f"{c.id}: {p['name']} x {c.batch * c.heads}, nslabs {p['nslabs']}, nu {p['nus']}" + (", base >= CUs" if c.forced else "")


# ---- uz_wgrad_multi (section 3): (P, Ci, Cj) per problem, bf16 one-tap ----------------------------------------------------------
# claims: odd_first (some problem with n & 7 != 0 workgroups, n > 8, starts at first % 8 != 0), flushes (more than 64 split
# problems), launches (shared launches of the 64 / 128 tile), misalign (destinations are views at an odd float offset)
MCase = namedtuple("MCase", "id probs misalign odd_first flushes launches")

MULTI_CASES = [
    MCase("permutation", [(20 * 64, 64, 64), (37 * 64 - 5, 64, 64), (88 * 64, 40, 24), (37 * 64, 256, 128), (20 * 64 + 1, 128, 128),
                          (83 * 64, 72, 40), (85 * 64 - 63, 64, 64)], False, True, False, (1, 1)),
    MCase("misaligned", [(17 * 64, 64, 64), (20 * 64, 128, 128), (4 * 64, 64, 64)], True, False, False, (1, 1)),
    MCase("many", [(17 * 64 + (i % 3), 64, 64) for i in range(70)] + [(17 * 64 - (i % 2), 128, 128) for i in range(26)], False, False,
          True, (3, 2)),
]


def multi_descs(c):
    return [desc(B, 1, 1, P, Ci, Cj) for P, Ci, Cj in c.probs]


def check_multi_claims(c, cus=CUS_HW):
    plans, total = multi_plan(multi_descs(c), cus)
    assert all(p is not None for p in plans), c.id
    said = []
    if c.odd_first:
        odd = [(p["first"], p["tiles"] * p["split"]) for p in plans
               if p["first"] % 8 and (p["tiles"] * p["split"]) & 7 and p["tiles"] * p["split"] > 8]
        assert odd, (c.id, plans)
        said.append(f"(first, n) with first % 8 != 0, n & 7 != 0, n > 8: {odd}")
    nsplit = sum(p["split"] > 1 for p in plans)
    if c.flushes:
        assert nsplit > 64, (c.id, nsplit)
        said.append(f"{nsplit} split problems: the reduction flushes")
    nl = (len({p["launch"] for p in plans if not p["big"]}), len({p["launch"] for p in plans if p["big"]}))
    assert nl == c.launches, (c.id, nl)
    if c.misalign:
        assert nsplit >= 1, c.id
    said.append(f"launches (64, 128) {nl}; splits {[p['split'] for p in plans][:8]}")
    return f"{c.id}: " + "; ".join(said), plans, total
