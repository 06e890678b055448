"""GPU: the weight-gradient family where workgroups walk several K-steps and where the slab sums switch form.

Kernels: wgrad3x3_body of uz_wgrad3x3.hip (two K-steps per barrier in a four-stage ring, haveA / haveB look-ahead, waves 4-7
trailing, hand-counted waits, the XCD remap of the three-tap form, the column permutation of wgrad3x3_multi_kernel),
wgrad_kernel of uz_wgrad.hip (per-row coordinate advance over rows and images) and the six slab reductions.  The cases, the
restated plans and the loop state each case claims live in tests/wgrad_walk_cases.py; tests/test_wgrad_walk.py proves the
claims without a GPU.  Here every case asserts its kernel family by name (and, through the workspace size, its slab count)
before it compares.

References:
  1. integer operands from {-2 .. 2}: the test first asserts from the operands alone that max_i sum_p |L[p][i]| * max |R| --
     an upper bound of max(|L|^T |R|) over every tap -- is below 2^24, so no fp32 partial sum can round whatever the order;
     the result must then EQUAL the float64 product: L^T R for one tap, autograd's weight gradient of F.conv2d /
     F.conv_transpose2d in float64 for the tap forms (as tests/test_wgrad9_gpu.py).  Every case runs twice: same bits.
  2. operand windows: both operands are channel windows of wider buffers whose other columns are NaN, with 70 NaN rows behind
     the last pixel: a tail that is zero by luck rather than by the descriptor's byte range shows as NaN.
  3. normal operands, one case per kernel form: 2e-5 (fp32) / 2e-2 (bf16) of the reference's max, as tests/test_ops_gpu.py.
  4. reductions alone (uz_wgrad_phase(..., 2)): the test writes the slabs, slab z holds +-(z + 1): dropping or doubling any
     slab changes every sum.  Random slabs: |error| <= nslabs * 2^-24 * sum_z |slab_z| per element (every one of the at most
     nslabs additions rounds by at most 2^-24 of a partial sum that sum_z |slab_z| bounds).
  5. phase 1 alone: a NaN workspace with a guard behind it; all nslabs * ntaps * Ci * Cj floats finite afterwards, the guard
     untouched, the float64 sum over slabs equal to reference 1.

Forms left out: every form the family launches through uz_wgrad, uz_wgrad_batched2 and uz_wgrad_multi has a case.  One
instantiation has none because the ABI cannot reach it: wgrad3x3_body's 2 x 2 gather (MODE 2, name ..._gather4).
uz_wgrad3x3_plan asks uz_wgrad_g4_plan first, and that plan accepts every bf16 UZ_TAPS_GATHER2X2 descriptor the
LDS-DMA plan would (the same conditions on channels, width, H % kr and byte ranges), so such problems run in
uz_wgrad_g4.hip (tests/test_wgrad9_gpu.py); with batch > 1 only one-tap problems are planned.  The 128 x 64 nine-tap form
is reached through its Cj >= 1024 and Ci >= 512 branch only: the other branch of the same plan line (Cj == 64) needs 2^19
pixels of at least 128 dy channels, 128 MB for one operand, and launches the same kernel."""
import functools
from ctypes import byref

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import wgrad_walk_cases as C  # tests/wgrad_walk_cases.py (pytest puts this directory on sys.path)
from unet_zoo_amd import _lib as L
from unet_zoo_amd import ops

DEV = "cuda"
SENTINEL = -77.0
GUARD = 64
NAN_ROWS = 70


@pytest.fixture(autouse=True)
def _restore():
    yield
    L.set_cu_reserve(0)


@pytest.fixture(scope="module", autouse=True)
def _free_references():
    yield
    _int_case.cache_clear()


def tdt(d):
    return torch.bfloat16 if d.dt == "bf16" else torch.float32


def cdesc(d):
    return L.WgradDesc(L.dtype_code(tdt(d)), d.N, d.H, d.W, d.Hr, d.Wr, d.Ci, d.ldl, d.Cj, d.ldr, d.ntaps, d.mode, d.dil)


def windowed(c):
    """the descriptor as run: operands are windows of wider buffers where the case says so"""
    return c.d._replace(ldl=c.d.Ci + 40, ldr=c.d.Cj + 24) if c.window else c.d


def place(vals, dt, ld):
    """(rows, C) values -> a device buffer (rows [+ NAN_ROWS], ld) and the address of the window; everything else NaN"""
    rows, ch = vals.shape
    if ld == ch:
        buf = vals.to(dt).to(DEV).contiguous()
        return buf, buf.data_ptr()
    buf = torch.full((rows + NAN_ROWS, ld), float("nan"), dtype=dt, device=DEV)
    buf[:rows, 8:8 + ch] = vals.to(dt).to(DEV)
    return buf, buf.data_ptr() + 8 * buf.element_size()


def reference(d, Lv, Rv):
    """float64 out[i][j][tap] of uz_wgrad for operands Lv (N H W, Ci), Rv (N Hr Wr, Cj)"""
    Lv, Rv = Lv.double(), Rv.double()
    if d.ntaps == 1:
        return (Lv.t() @ Rv).reshape(d.Ci, d.Cj, 1)
    lm = Lv.view(d.N, d.H, d.W, d.Ci).permute(0, 3, 1, 2)
    rm = Rv.view(d.N, d.Hr, d.Wr, d.Cj).permute(0, 3, 1, 2)
    if d.mode == C.GATHER2X2:      # L the coarse input of a ConvTranspose2d(k2, s2), R the gradient on the fine grid
        w = torch.zeros(d.Ci, d.Cj, 2, 2, dtype=torch.float64, requires_grad=True)
        y = F.conv_transpose2d(lm, w, None, stride=2)
        F.pad(y, [0, d.Wr - 2 * d.W, 0, d.Hr - 2 * d.H]).backward(rm)
        return w.grad.reshape(d.Ci, d.Cj, 4)
    w = torch.zeros(d.Ci, d.Cj, 3, 3, dtype=torch.float64, requires_grad=True)
    if d.mode == C.CONV_UP2:
        y = F.conv2d(F.interpolate(rm, scale_factor=2, mode="nearest"), w, None, padding=1)
    elif d.mode == C.CONV_S2:
        y = F.conv2d(rm, w, None, stride=2, padding=1)
    else:
        y = F.conv2d(rm, w, None, padding=d.dil, dilation=d.dil)
    assert y.shape == lm.shape
    y.backward(lm)
    return w.grad.reshape(d.Ci, d.Cj, 9)


def assert_exact_in_fp32(Lv, Rv):
    """from the operands alone: an upper bound of max(|L|^T |R|), every tap's pixel subset included"""
    assert Lv.double().abs().sum(0).max().item() * Rv.double().abs().max().item() < 2 ** 24


@functools.lru_cache(maxsize=None)
def _int_case(cid):
    c = next(c for c in C.PRODUCT_CASES if c.id == cid)
    d = c.d
    g = torch.Generator().manual_seed(sum(map(ord, cid)))
    Lv = torch.randint(-2, 3, (d.N * d.H * d.W, d.Ci), generator=g).float()
    Rv = torch.randint(-2, 3, (d.N * d.Hr * d.Wr, d.Cj), generator=g).float()
    assert_exact_in_fp32(Lv, Rv)
    return Lv, Rv, reference(d, Lv, Rv)


def guarded_out(n):
    return torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)


def check_guards(buf, what="out"):
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), f"{what}: a guard float changed"


def assert_family(c, d):
    """the kernel by name and, through the workspace size, the slab count of the restated plan; returns the plan"""
    L.set_cu_reserve(c.reserve)
    p = C.plan(d, C.CUS_HW - c.reserve)
    assert ops.wgrad_kernel_name(cdesc(d)) == c.name == p["name"]
    lib = L.load()
    assert L.check_count(lib.uz_wgrad_split(byref(cdesc(d))), "uz_wgrad_split") == p["nslabs"]
    C.check_claims(c, p)
    return p


def run_wgrad(d, lptr, rptr, phase=0, ws=None):
    lib = L.load()
    cd = cdesc(d)
    n = d.Ci * d.Cj * d.ntaps
    out = guarded_out(n)
    if ws is None:
        ws = torch.empty(max(L.check_count(lib.uz_wgrad_workspace_bytes(byref(cd)), "workspace") // 4, 64), dtype=torch.float32,
                         device=DEV)
    optr = out.data_ptr() + 4 * GUARD
    if phase == 0:
        L.check(lib.uz_wgrad(byref(cd), lptr, rptr, optr, ws.data_ptr(), L.stream_ptr()), "uz_wgrad")
    else:
        L.check(lib.uz_wgrad_phase(byref(cd), lptr, rptr, optr, ws.data_ptr(), L.stream_ptr(), phase), "uz_wgrad_phase")
    torch.cuda.synchronize()
    check_guards(out)
    return out[GUARD:GUARD + n].cpu().view(d.Ci, d.Cj, d.ntaps)


def where(got, ref):
    bad = (got.double() != ref).nonzero()
    if bad.numel() == 0:
        return "equal"
    per_tap = [(t, int((got[:, :, t].double() != ref[:, :, t]).sum())) for t in range(ref.shape[2])]
    i = tuple(bad[0].tolist())
    return (f"{bad.shape[0]} of {ref.numel()} elements differ; per tap {per_tap}; first (i, j, tap) = {i}: {got[i].item()} vs "
            f"{ref[i].item()}; max |diff| {(got.double() - ref).abs().max().item():g}")


# ---- sections 1, 4, 5, 6: uz_wgrad on integers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in C.PRODUCT_CASES])
def test_product_is_exact_on_integers(cid):
    c = next(c for c in C.PRODUCT_CASES if c.id == cid)
    d = windowed(c)
    Lv, Rv, ref = _int_case(cid)
    assert_family(c, d)
    lbuf, lptr = place(Lv, tdt(d), d.ldl)
    rbuf, rptr = place(Rv, tdt(d), d.ldr)
    got = run_wgrad(d, lptr, rptr)
    assert torch.equal(got.double(), ref), where(got, ref)
    assert torch.equal(run_wgrad(d, lptr, rptr), got), "two launches on the same bytes differ"


def test_two_reserves_two_splits_same_bits():
    """512 x 512 channels over 8192 tokens: 16 ranges of 8 K-steps on 256 CUs, 8 of 16 on 128 -- exact, so equal"""
    a, b = [c for c in C.PRODUCT_CASES if c.id.startswith("1tap128-512x512")]
    Lv, Rv, ref = _int_case(a.id)
    lbuf, lptr = place(Lv, tdt(a.d), a.d.ldl)
    rbuf, rptr = place(Rv, tdt(a.d), a.d.ldr)
    outs = []
    for c in (a, b):
        p = assert_family(c, c.d)
        outs.append((p["nslabs"], run_wgrad(c.d, lptr, rptr)))
    assert outs[0][0] != outs[1][0]
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][1].double(), ref)


@pytest.mark.parametrize("cid", [c.id for c in C.PRODUCT_CASES if c.random])
def test_product_on_normal_operands(cid):
    c = next(c for c in C.PRODUCT_CASES if c.id == cid)
    d = windowed(c)
    dt = tdt(d)
    g = torch.Generator().manual_seed(len(cid))
    Lv = torch.randn(d.N * d.H * d.W, d.Ci, generator=g).to(dt)
    Rv = torch.randn(d.N * d.Hr * d.Wr, d.Cj, generator=g).to(dt)
    ref = reference(d, Lv, Rv)
    assert_family(c, d)
    lbuf, lptr = place(Lv, dt, d.ldl)
    rbuf, rptr = place(Rv, dt, d.ldr)
    got = run_wgrad(d, lptr, rptr)
    e = ((got.double() - ref).abs().max() / ref.abs().max()).item()
    tol = 2e-5 if dt == torch.float32 else 2e-2
    print(f"  {cid}: {e:.3e} of the max (tolerance {tol:g})")
    assert e < tol, e
    assert torch.equal(run_wgrad(d, lptr, rptr), got)


@pytest.mark.parametrize("Ci,name", [(64, C.T64 + "9tap"), (128, C.T128 + "3tap")])
def test_short_map_border_taps_see_zero_padding(Ci, name):
    """all ones, N = 3, a 4 x 64 map: a tap counts the pixels it sees -- (H - |dy|) (W - |dx|) per image"""
    N, H, W = 3, 4, 64
    d = C.desc("bf16", N, H, W, Ci, Ci, 9)
    assert ops.wgrad_kernel_name(cdesc(d)) == name
    ones = torch.ones(N * H * W, Ci, dtype=torch.bfloat16, device=DEV)
    got = run_wgrad(d, ones.data_ptr(), ones.data_ptr())
    rows = torch.tensor([H - 1, H, H - 1]).float()
    cols = torch.tensor([W - 1, W, W - 1]).float()
    want = (N * rows[:, None] * cols[None, :]).reshape(9).expand(Ci, Ci, 9)
    assert torch.equal(got, want), where(got, want.double())


# ---- section 8: phase 1 alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in C.PRODUCT_CASES if c.phase1])
def test_phase1_fills_exactly_its_slabs(cid):
    c = next(c for c in C.PRODUCT_CASES if c.id == cid)
    d = windowed(c)
    Lv, Rv, ref = _int_case(cid)
    p = assert_family(c, d)
    lbuf, lptr = place(Lv, tdt(d), d.ldl)
    rbuf, rptr = place(Rv, tdt(d), d.ldr)
    n = p["nslabs"] * d.ntaps * d.Ci * d.Cj
    assert 4 * n == L.check_count(L.load().uz_wgrad_workspace_bytes(byref(cdesc(d))), "workspace")
    ws = torch.full((n + 1024,), float("nan"), dtype=torch.float32, device=DEV)
    ws[n:] = SENTINEL
    run_wgrad(d, lptr, rptr, phase=1, ws=ws)
    slabs = ws.cpu()
    assert bool((slabs[n:] == SENTINEL).all()), "the guard behind the workspace changed"
    assert bool(torch.isfinite(slabs[:n]).all()), f"{int((~torch.isfinite(slabs[:n])).sum())} slab floats were never written"
    got = slabs[:n].double().view(p["nslabs"], d.ntaps, d.Ci, d.Cj).sum(0).permute(1, 2, 0)
    assert torch.equal(got, ref), where(got, ref)


# ---- section 7: the slab reductions alone --------------------------------------------------------------------------------------------
def _unused_operands(d):
    dt = tdt(d)
    return (torch.zeros(d.N * d.H * d.W, d.ldl, dtype=dt, device=DEV), torch.zeros(d.N * d.Hr * d.Wr, d.ldr, dtype=dt, device=DEV))


def _reduce(c, slabs):
    d = c.d
    L.set_cu_reserve(c.reserve)
    nsl = L.check_count(L.load().uz_wgrad_split(byref(cdesc(d))), "uz_wgrad_split")
    assert nsl == c.nslabs == slabs.shape[0] and C.reduce_form(d, nsl) == c.form
    lz, rz = _unused_operands(d)
    ws = slabs.to(DEV).contiguous()
    got = run_wgrad(d, lz.data_ptr(), rz.data_ptr(), phase=2, ws=ws)
    assert torch.equal(ws.cpu(), slabs), "the reduction wrote into its slabs"
    return got.reshape(d.Ci * d.Cj, d.ntaps)


@pytest.mark.parametrize("cid", [c.id for c in C.REDUCE_CASES])
def test_reduction_sums_every_slab_once(cid):
    c = next(c for c in C.REDUCE_CASES if c.id == cid)
    d = c.d
    g = torch.Generator().manual_seed(c.nslabs)
    sign = torch.randint(0, 2, (c.nslabs, d.ntaps, d.Ci * d.Cj), generator=g).float() * 2 - 1
    slabs = sign * torch.arange(1, c.nslabs + 1).float()[:, None, None]
    ref = slabs.double().sum(0).t()                    # parameter layout: out[e * NT + t]
    got = _reduce(c, slabs)
    bad = (got.double() != ref).nonzero()
    assert bad.numel() == 0, (f"{bad.shape[0]} of {ref.numel()} sums differ, first (e, tap) = {bad[0].tolist()}: "
                              f"{got[tuple(bad[0])].item()} vs {ref[tuple(bad[0])].item()}")
    assert torch.equal(_reduce(c, slabs), got)


@pytest.mark.parametrize("cid", [c.id for c in C.REDUCE_CASES if c.random])
def test_reduction_on_random_slabs(cid):
    c = next(c for c in C.REDUCE_CASES if c.id == cid)
    d = c.d
    g = torch.Generator().manual_seed(c.nslabs + 100)
    slabs = torch.randn(c.nslabs, d.ntaps, d.Ci * d.Cj, generator=g)
    ref = slabs.double().sum(0).t()
    bound = c.nslabs * 2.0 ** -24 * slabs.double().abs().sum(0).t()
    got = _reduce(c, slabs)
    err = (got.double() - ref).abs()
    print(f"  {cid}: max error / bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())


# ---- section 2: batched and two-level batched one-tap products ------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in C.BATCHED_CASES])
def test_batched_products_are_exact_on_integers(cid):
    c = next(c for c in C.BATCHED_CASES if c.id == cid)
    lib = L.load()
    d = C.batched_desc(c)
    nprob = c.batch * c.heads
    L.set_cu_reserve(c.reserve)
    p = C.plan3x3(d, C.CUS_HW - c.reserve, nprob)
    assert ops.wgrad_kernel_name(cdesc(d)) == c.name == p["name"] and p["nus"] == c.nus
    ws_bytes = L.check_count(lib.uz_wgrad_batched_workspace_bytes(byref(cdesc(d)), nprob), "workspace")
    assert ws_bytes == nprob * p["nslabs"] * c.C * c.KV * 4
    g = torch.Generator().manual_seed(c.P + nprob)
    Lv = torch.randint(-2, 3, (c.batch, c.P, c.heads, c.C), generator=g).float()
    Rv = torch.randint(-2, 3, (c.batch, c.P, c.heads, c.KV), generator=g).float()
    assert c.P * Lv.abs().max().item() * Rv.abs().max().item() < 2 ** 24      # P products per sum
    ref = torch.einsum("bphc,bphk->bhck", Lv.double(), Rv.double()).reshape(nprob, c.C * c.KV)
    ld, rd = Lv.to(torch.bfloat16).to(DEV), Rv.to(torch.bfloat16).to(DEV)
    ob = c.C * c.KV + c.gap

    def run():
        out = guarded_out(nprob * ob)
        ws = torch.empty(max(ws_bytes // 4, 64), dtype=torch.float32, device=DEV)
        L.check(lib.uz_wgrad_batched2(byref(cdesc(d)), c.batch, c.heads, ld.data_ptr(), c.P * d.ldl, c.C if c.heads > 1 else 0,
                                      rd.data_ptr(), c.P * d.ldr, c.KV if c.heads > 1 else 0, out.data_ptr() + 4 * GUARD, ob,
                                      ws.data_ptr(), L.stream_ptr()), "uz_wgrad_batched2")
        torch.cuda.synchronize()
        check_guards(out)
        return out[GUARD:-GUARD].cpu().view(nprob, ob)

    got = run()
    bad = (got[:, :c.C * c.KV].double() != ref).any(1).nonzero().flatten().tolist()
    assert not bad, f"problems {bad[:8]} of {nprob} differ"
    assert bool((got[:, c.C * c.KV:] == SENTINEL).all()), "a float between two results changed"
    assert torch.equal(run(), got)


def test_wgrad_heads_and_wgrad_batched_entry_points():
    """the ops-level callers on the shapes of the heads-split case: one launch for (image, head) pairs against a per-head loop"""
    c = next(c for c in C.BATCHED_CASES if c.id == "heads-split")
    g = torch.Generator().manual_seed(3)
    Lv = torch.randint(-2, 3, (c.batch * c.P, c.heads * c.C), generator=g).float()
    Rv = torch.randint(-2, 3, (c.batch * c.P, c.heads * c.KV), generator=g).float()
    la = ops.Act(Lv.to(torch.bfloat16).to(DEV), 0, c.heads * c.C, c.batch, 1, c.P)
    ra = ops.Act(Rv.to(torch.bfloat16).to(DEV), 0, c.heads * c.KV, c.batch, 1, c.P)
    ref = torch.einsum("bphc,bphk->bhck", Lv.double().view(c.batch, c.P, c.heads, c.C), Rv.double().view(c.batch, c.P, c.heads, c.KV))
    got = ops.wgrad_heads(la, ra, c.heads).cpu()
    assert torch.equal(got.double(), ref)
    for h in range(c.heads):
        one = ops.wgrad_batched(la.window(h * c.C, c.C), ra.window(h * c.KV, c.KV)).cpu()
        assert torch.equal(one.double(), ref[:, h])


# ---- section 3: uz_wgrad_multi ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in C.MULTI_CASES])
def test_multi_products_are_exact_on_integers(cid):
    c = next(c for c in C.MULTI_CASES if c.id == cid)
    lib = L.load()
    ds = C.multi_descs(c)
    _, plans, total = C.check_multi_claims(c)
    g = torch.Generator().manual_seed(len(ds))
    ops_l, ops_r, refs, offs = [], [], [], []
    off = GUARD + (1 if c.misalign else 0)
    for d in ds:
        assert ops.wgrad_kernel_name(cdesc(d)).endswith("_1tap")
        Lv = torch.randint(-2, 3, (d.H * d.W, d.Ci), generator=g).float()
        Rv = torch.randint(-2, 3, (d.H * d.W, d.Cj), generator=g).float()
        assert_exact_in_fp32(Lv, Rv)
        refs.append((Lv.double().t() @ Rv.double()).flatten())
        ops_l.append(Lv.to(torch.bfloat16).to(DEV))
        ops_r.append(Rv.to(torch.bfloat16).to(DEV))
        offs.append(off)
        off += d.Ci * d.Cj + GUARD
    arr = (L.WgradItem * len(ds))()

    def run():
        flat = torch.full((off,), SENTINEL, dtype=torch.float32, device=DEV)
        assert flat.data_ptr() % 16 == 0
        for i, d in enumerate(ds):
            arr[i] = L.WgradItem(cdesc(d), ops_l[i].data_ptr(), ops_r[i].data_ptr(), flat.data_ptr() + 4 * offs[i])
            assert ((flat.data_ptr() + 4 * offs[i]) % 16 != 0) == c.misalign
        ws_bytes = L.check_count(lib.uz_wgrad_multi_workspace_bytes(arr, len(ds)), "workspace")
        assert ws_bytes == total                       # the restated per-problem splits are the library's
        ws = torch.empty(max(ws_bytes, 256) // 4, dtype=torch.float32, device=DEV)
        assert ws.data_ptr() % 256 == 0
        L.check(lib.uz_wgrad_multi(arr, len(ds), ws.data_ptr(), L.stream_ptr()), "uz_wgrad_multi")
        torch.cuda.synchronize()
        return flat.cpu()

    got = run()
    keep = torch.ones(off, dtype=torch.bool)
    bad = []
    for i, d in enumerate(ds):
        n = d.Ci * d.Cj
        keep[offs[i]:offs[i] + n] = False
        if not torch.equal(got[offs[i]:offs[i] + n].double(), refs[i]):
            nbad = int((got[offs[i]:offs[i] + n].double() != refs[i]).sum())
            bad.append((i, c.probs[i], plans[i]["split"], plans[i]["first"], nbad))
    assert not bad, f"(problem, (P, Ci, Cj), split, first workgroup, wrong elements): {bad[:6]}"
    assert bool((got[keep] == SENTINEL).all()), "a float beside a result changed"
    assert torch.equal(run(), got)
