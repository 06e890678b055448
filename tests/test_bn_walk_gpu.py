"""GPU: the BatchNorm element passes of uz_eltwise.hip -- bn_finalize_kernel, bn_relu_apply_kernel (plain, pooled, residual,
without the ReLU), bn_relu_bwd_kernel (reduce pass and apply pass), bn_bwd_finalize_kernel and bn_relu_bwd_head_kernel --
where workgroups walk the map, held to float64 references (helpers, case table and the restated plans: tests/bn_walk_ref.py;
their own checks: tests/test_bn_walk.py).

What the other tests of these kernels never execute, because their maps stay below the grid cap
(gx = min(ceil(units / by), UZ_NUM_CU * wg / gy)):
  * slots 1 to 3 of the non-pooled backward kernels and of the head's apply pass (four pixels one grid stride apart): the
    clamped dummy pixel `units - 1`, the `in[k]` selects, the index arithmetic of the walk from the end on
    q = u0 + k * ustride, the stores of slots 1 to 3;
  * a second trip of any loop: `u0 += NPIX * ustride`, `u0 += ustride` (pooled), `idx0 += gridDim.x * blockDim.x` (forward),
    `r += 4 * NG` (both finalize kernels);
  * idle channel lanes that still take part in the LDS reduction (C = 96 in bf16: 12 chunks on 16 lanes), gy = 2 (C = 520),
    bx = 1 (C = 8 / 4).

Here uz_set_cu_reserve(128) leaves the plans 128 CUs.  Every test restates its plan, prints it (kernel form, trips, slots,
grid), asserts the trips and slots the case table claims, asserts that the library's reduce-pass grid
(uz_bn_relu_bwd_workspace_bytes / (8 C)) is the restated one, and only then launches.  The operands are dyadic, so every
fp32 operation of the forward pass and of the reduce pass is exact and order cannot matter:
  act, pooled                     bit for bit, both dtypes; the bytes outside a channel window still hold the sentinel
  partial rows of the reduce pass bit for bit, row by row against the restated ownership (front walk and end walk)
  sums, dgamma, dbeta             bit for bit
  dy                              |got - ref| <= 2^-21 A, A = |scale| (|dz| + |S0 / P| + |xhat S1 / P|) (eight fp32 roundings;
                                  k0 = float(S0 / P) is not dyadic), + 2^-8 |ref| in bf16; exactly 0 where dz, S0, S1 are 0
  finalize outputs                at most one fp32 ulp from the float64 formula; the backward finalize bit for bit

Cases (tests/bn_walk_ref.py CASES; trips of forward apply / reduce / backward apply, live slots of reduce / backward apply):
  W1 bf16 (3,97,113) x 512 and W2 fp32 x 256: no pool, 9 / 5 / 3 trips (the last one partial), 4 / 4 slots
  W3 bf16 (2,65,127) x 512 and W4 fp32 x 256: pooled, floor and ceil, 2 / 3 / 2 trips, both borders clipped
  W5 bf16 (1,131,139) x 96: bx = 16 with 4 idle lanes, one trip, 3 / 2 slots
  W6 bf16 (1,89,95) x 520: gy = 2, the second column with one live lane; no pool 3 / 3 / 2 trips and 4 / 4 slots, pooled 1 / 3 / 2
  W7 bf16 (4,255,257) x 64: head apply, K = 3, 2 trips, 4 slots, img = p / HW across images
  W8 bf16 (1,181,191) x 64: head apply, K = 1 and K = 8, one trip, slots 0 and 1; W8w (1,257,257): slots 0 to 2
  S1 (2,9,13) x 8 / 4: bx = 1, by = 256;  S2 (1,1,37) and (1,37,1) x 64: ceil pool of one row / one column (a floor pool
  is refused by the host);  S3 (2,3,3) x 64: floor pool with a clipped row and column
Each W1 .. W6 and S case runs once in full form: channel windows of wider buffers on all eight strides (y, res, act, pooled,
g0, g1, gpool, dy: wider by 1, 3, .. 15 vectors), the neighbours holding 5.0 (W5, W6 ceil and S3 once more with NaN), the
outputs pre-filled with the sentinel, the forward with and without the residual.  The variants run on W5 and W6.

Not reachable through the ABI: no query gives the grid of the forward apply pass, of the backward apply pass or of the head's
(those plans are restated only; the reduce pass's is asked).  The fused finalize (uz_bn_relu_add_apply_fin,
uz_bn_relu_bwd_apply_fin) is out of scope: tests/test_bn_fin_gpu.py pins it bit for bit to the launches pinned here."""
from ctypes import byref

import pytest
import torch

pytestmark = pytest.mark.gpu

import bn_walk_ref as R  # tests/bn_walk_ref.py (pytest puts this directory on sys.path)
from unet_zoo_amd import _lib as L
from unet_zoo_amd import ops
from unet_zoo_amd.ops import Act

DEV = "cuda"
BF16, F32 = R.BF16, R.F32
SENTINEL = R.SENTINEL
# the eight strides: buffers wider than the window by these (odd) numbers of 16-byte vectors
M_Y, M_RES, M_ACT, M_POOLED, M_G0, M_G1, M_GP, M_DY = 1, 3, 5, 7, 9, 11, 13, 15


@pytest.fixture(autouse=True)
def _restore():
    yield
    L.set_cu_reserve(0)


@pytest.fixture(scope="module", autouse=True)
def _free_references():
    yield
    R.operands.cache_clear()
    R.head_operands.cache_clear()


def _form_id(c, pool):
    return f"{c.id}-{pool or 'nopool'}"


def _forms(ids):
    return [pytest.param(R.CASES[i], pool, id=_form_id(R.CASES[i], pool)) for i in ids for pool, _ in R.forms(R.CASES[i])]


# ---- windows of wider buffers -----------------------------------------------------------------------------------------------
def _off(dt, m):
    return R.vec_of(dt) * ((m + 1) // 2)


def _in(rows, dt, shape, m, fill):
    """rows (P, C) fp32 on the device as a channel window of a buffer m vectors wider, whose other channels hold `fill`"""
    P, C = rows.shape
    buf = torch.full((P, C + m * R.vec_of(dt)), fill, dtype=dt, device=DEV)
    buf[:, _off(dt, m):_off(dt, m) + C] = rows.to(dt)
    return Act(buf, _off(dt, m), C, *shape)


def _out(shape, C, dt, m):
    P = shape[0] * shape[1] * shape[2]
    buf = torch.full((P, C + m * R.vec_of(dt)), SENTINEL, dtype=dt, device=DEV)
    return Act(buf, _off(dt, m), C, *shape)


def _split(a):
    """(the window, everything else) of an output Act"""
    return a.buf[:, a.off:a.off + a.C], torch.cat([a.buf[:, :a.off], a.buf[:, a.off + a.C:]], 1)


def _untouched(a):
    return bool((_split(a)[1] == SENTINEL).all())


def _to_dev(o):
    d = type(o)()
    for k, v in vars(o).items():
        setattr(d, k, v.to(DEV))
    return d


def _cus():
    return R.CUS_HW - L.get_cu_reserve()


def _pooled_where(p, ch):
    return [f"pooled pixel {int(a)} channel {int(b)}" for a, b in zip(p, ch)]


# ---- the passes -------------------------------------------------------------------------------------------------------------
def _forward(c, o, pool, res=False, relu=True, rev=False, fill=5.0):
    """launch uz_bn_relu_add_apply on windows and hold act / pooled to the reference bit for bit; returns the two buffers"""
    N, H, W = c.shape
    plan = R.apply_plan(c.dt, N, H, W, c.C, pool, _cus())
    print(R.plan_line("apply" + (" pooled " + pool if pool else "") + (" +res" if res else "") + ("" if relu else " no relu")
                      + (" from the end" if rev else ""), c.dt, c.shape, c.C, plan))
    y = _in(o.y, c.dt, c.shape, M_Y, fill)
    r = _in(o.res, c.dt, c.shape, M_RES, fill) if res else None
    act = _out(c.shape, c.C, c.dt, M_ACT)
    pooled = _out((N,) + R.pool_hw(H, W, pool), c.C, c.dt, M_POOLED) if pool else None
    ops.bn_relu_apply(y, o.vec[0], o.vec[1], act, pooled, r, pool == "ceil", relu=relu, reverse=rev)
    want_act, want_pooled = R.forward_ref(o.y, o.vec, c.shape, c.dt, relu, o.res if res else None, pool)
    R.assert_same(_split(act)[0], want_act, "act", R.where_apply(c, pool, plan, rev))
    assert _untouched(act)
    if pool:
        R.assert_same(_split(pooled)[0], want_pooled, "pooled", _pooled_where)
        assert _untouched(pooled)
    return act.buf, pooled.buf if pool else None


def _desc(c, y, g0, g1, gp, dy, pool, relu, rev):
    return L.BnBwdDesc(L.dtype_code(c.dt), *c.shape, c.C, y.ld, g0.ld if g0 else 0, g1.ld if g1 else 0, gp.ld if gp else 0,
                       dy.ld if dy else 0, int(pool == "ceil") | (0 if relu else 2) | (4 if rev else 0))


def _backward(c, o, pool, subset=("g0", "g1", "gp"), relu=True, rev=False, fill=5.0, frozen=False):
    """the reduce pass alone (rows), then ops.bn_relu_bwd: reduce + finalize + apply, the apply pass walking the other way
    (ops.BN_BWD_ALTERNATE); every output against the reference.  Returns (sums, dgamma, dbeta, dy buffer)"""
    lib = L.load()
    N, H, W = c.shape
    P = N * H * W
    use_gp = pool is not None and "gp" in subset
    assert use_gp == (pool is not None) and ops.BN_BWD_ALTERNATE
    rp, bp = R.bwd_plan(c.dt, N, H, W, c.C, pool, 1, _cus()), R.bwd_plan(c.dt, N, H, W, c.C, pool, 2, _cus())
    tag = (" pooled " + pool if pool else "") + " " + "+".join(subset) + ("" if relu else " no relu")
    print(R.plan_line("bwd reduce" + tag + (" from the end" if rev else ""), c.dt, c.shape, c.C, rp))
    print(R.plan_line("bwd apply" + tag + ("" if rev else " from the end"), c.dt, c.shape, c.C, bp))
    gp_rows = R.gp_rows(o.gp, c.shape, pool) if use_gp else None
    y = _in(o.y, c.dt, c.shape, M_Y, fill)
    g0 = _in(o.g0, c.dt, c.shape, M_G0, fill) if "g0" in subset else None
    g1 = _in(o.g1, c.dt, c.shape, M_G1, fill) if "g1" in subset else None
    gp = _in(gp_rows, c.dt, (N,) + R.pool_hw(H, W, pool), M_GP, fill) if use_gp else None
    dy = _out(c.shape, c.C, c.dt, M_DY)
    d = _desc(c, y, g0, g1, gp, dy, pool, relu, rev)
    wsb = L.check_count(lib.uz_bn_relu_bwd_workspace_bytes(byref(d), int(use_gp)), "uz_bn_relu_bwd_workspace_bytes")
    assert wsb == rp.gx * 8 * c.C, (wsb, rp)                                       # the library's grid is the restated one
    # the reference
    dz, xhat = R.backward_terms(o.y, o.vec, c.shape, o.g0 if g0 else None, o.g1 if g1 else None, gp_rows, pool, relu)
    S = R.totals(dz, xhat)
    # the reduce pass alone: its rows
    rows = torch.full((rp.gx, 2, c.C), float("nan"), device=DEV)
    L.check(lib.uz_bn_relu_bwd_reduce_rows(byref(d), y.ptr(), *(o.vec[i].data_ptr() for i in range(4)), g0.ptr() if g0 else None,
                                           g1.ptr() if g1 else None, gp.ptr() if gp else None, rows.data_ptr(), L.stream_ptr()),
            "uz_bn_relu_bwd_reduce_rows")
    R.check_rows(rows, R.rows_ref(dz, xhat, rp, c.shape, rev))
    # reduce + finalize + apply
    sums = torch.full((2, c.C), float("nan"), dtype=torch.float64, device=DEV)
    dgamma, dbeta = torch.full((c.C,), float("nan"), device=DEV), torch.full((c.C,), float("nan"), device=DEV)
    ops.bn_relu_bwd(y, o.vec, g0, g1, gp, sums, dy, dgamma, dbeta, pool == "ceil", relu=relu, frozen=frozen, reverse=rev)
    got = _split(dy)[0]
    where = R.where_bwd(c.shape, bp, not rev)
    if frozen:
        # running statistics are constants: dy = scale * dz, which is exact on these operands; the sums are zeroed in between
        R.check_totals(sums, None, None, torch.zeros_like(S))
        R.check_totals(S, dgamma, dbeta, S)
        want = o.vec[0].double() * dz
        bad = got.double() != want
        assert not bool(bad.any()), R.report(bad, "dy (frozen)", where)
    else:
        R.check_totals(sums, dgamma, dbeta, S)
        want, A = R.dy_ref(dz, xhat, o.vec, S, P)
        R.check_dy(got, want, A, dz, S, c.dt, where)
    assert _untouched(dy)
    return sums, dgamma, dbeta, dy.buf


def _assert_claims(c, pool):
    """before anything is launched: under the reserve in force the case walks as the table says"""
    assert L.get_cu_reserve() == R.RESERVE
    N, H, W = c.shape
    claim = c.claims[pool is not None]
    ap, rp, bp = (R.apply_plan(c.dt, N, H, W, c.C, pool), R.bwd_plan(c.dt, N, H, W, c.C, pool, 1), R.bwd_plan(c.dt, N, H, W, c.C, pool, 2))
    assert (ap.trips, rp.trips, bp.trips) == (claim.apply, claim.reduce, claim.bwd), (ap, rp, bp)
    if pool is None:
        assert (rp.slots, bp.slots) == (claim.rslots, claim.bslots), (rp, bp)
    if c.id in R.BLOCKS:
        assert (rp.bx, rp.by, rp.gy) == R.BLOCKS[c.id]


def _full_form(c, pool, fill=5.0):
    o = _to_dev(R.operands(c.id))
    L.set_cu_reserve(R.RESERVE)
    _assert_claims(c, pool)
    fwd = [_forward(c, o, pool, res=res, fill=fill) for res in (False, True)]
    bwd = _backward(c, o, pool, ("g0", "g1", "gp") if pool else ("g0", "g1"), fill=fill)
    return o, fwd, bwd


# ---- every case in full form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,pool", _forms(R.WALKING + R.SMALL))
def test_full_form_against_float64(c, pool):
    """windows on all eight strides beside neighbours holding 5.0, outputs pre-filled with the sentinel; forward without and
    with the residual; backward with g0 + g1 (+ the pool's gradient): rows, totals, dgamma / dbeta, dy"""
    _full_form(c, pool)


@pytest.mark.parametrize("c,pool", [pytest.param(R.CASES[i], p, id=f"{i}-{p or 'nopool'}") for i, p in
                                    (("W5", None), ("W6", "ceil"), ("S3b", "floor"))])
def test_full_form_next_to_nan_neighbours(c, pool):
    """the channels beside every input window hold NaN: a lane past the last chunk (`cok` false: 4 of 16 at C = 96, 63 of 64 in
    the second grid column at C = 520) must add nothing to the LDS reduction and store nothing"""
    _full_form(c, pool, fill=float("nan"))


@pytest.mark.parametrize("c,pool", [pytest.param(R.CASES[i], p, id=f"{i}-{p or 'nopool'}") for i, p in (("W1", None), ("W3", "ceil"))])
def test_the_whole_chip_gives_the_same_bytes(c, pool):
    """exact operands: act, pooled, sums, dgamma, dbeta do not depend on the grid -- the launch without a reserve (a grid
    twice as wide, half the trips) equals the launch under it"""
    o = _to_dev(R.operands(c.id))
    L.set_cu_reserve(R.RESERVE)
    _assert_claims(c, pool)
    sub = ("g0", "g1", "gp") if pool else ("g0", "g1")
    a1, p1 = _forward(c, o, pool)
    s1, dg1, db1, _ = _backward(c, o, pool, sub)
    L.set_cu_reserve(0)
    full = R.bwd_plan(c.dt, *c.shape, c.C, pool, 1, R.CUS_HW)
    assert full.gx >= 2 * R.bwd_plan(c.dt, *c.shape, c.C, pool, 1).gx
    a2, p2 = _forward(c, o, pool)
    s2, dg2, db2, _ = _backward(c, o, pool, sub)
    assert torch.equal(a1, a2) and (p1 is None or torch.equal(p1, p2))
    assert torch.equal(s1, s2) and torch.equal(dg1, dg2) and torch.equal(db1, db2)


# ---- variants on the cheap walking cases ------------------------------------------------------------------------------------
VARIANT_FORMS = [pytest.param(R.CASES[i], p, id=f"{i}-{p or 'nopool'}") for i, p in (("W5", None), ("W6", None), ("W6", "ceil"), ("W6", "floor"))]


@pytest.mark.parametrize("c,pool", VARIANT_FORMS)
def test_walk_from_the_end(c, pool):
    """bit 2 of the flag word, every pass: the forward stores the same bytes; the reduce pass's rows are those of the MIRRORED
    ownership (units - 1 - q); the apply pass then walks from the front"""
    o = _to_dev(R.operands(c.id))
    L.set_cu_reserve(R.RESERVE)
    _assert_claims(c, pool)
    _forward(c, o, pool, rev=True)
    if pool != "floor":
        _forward(c, o, pool, res=True, rev=True)
    _backward(c, o, pool, ("g0", "g1", "gp") if pool else ("g0", "g1"), rev=True)


SUBSETS = ([("W5", None, s) for s in (("g0",), ("g1",))] + [("W6", None, s) for s in (("g0",), ("g1",))]
           + [("W6", "ceil", s) for s in (("gp",), ("g0", "gp"), ("g1", "gp"))] + [("W6", "floor", ("gp",))])


@pytest.mark.parametrize("cid,pool,subset", [pytest.param(i, p, s, id=f"{i}-{p or 'nopool'}-{'+'.join(s)}") for i, p, s in SUBSETS])
def test_every_subset_of_the_gradients(cid, pool, subset):
    """g0 / g1 / gpool absent in every combination the host accepts (the full sets run in the full form); a pool gradient
    alone: the pooled kernel reads pixel 0 of y in place of both missing gradients and drops it"""
    c = R.CASES[cid]
    o = _to_dev(R.operands(cid))
    L.set_cu_reserve(R.RESERVE)
    _assert_claims(c, pool)
    _backward(c, o, pool, subset)


def test_no_gradient_at_all_is_refused():
    c = R.CASES["S1b"]
    o = _to_dev(R.operands(c.id))
    y, dy = _in(o.y, c.dt, c.shape, M_Y, 5.0), _out(c.shape, c.C, c.dt, M_DY)
    d = _desc(c, y, None, None, None, dy, None, True, False)
    ws = torch.full((8, 2, c.C), SENTINEL, device=DEV)
    rc = L.load().uz_bn_relu_bwd_reduce_rows(byref(d), y.ptr(), *(o.vec[i].data_ptr() for i in range(4)), None, None, None,
                                            ws.data_ptr(), L.stream_ptr())
    assert rc != 0 and bool((ws == SENTINEL).all())


@pytest.mark.parametrize("cid", ["W5", "W6"])
def test_batchnorm_without_the_relu(cid):
    """bit 1 of the flag word (non-pooled): the forward stores fma(y, scale, shift) unclamped, the backward masks nothing"""
    c = R.CASES[cid]
    o = _to_dev(R.operands(cid))
    L.set_cu_reserve(R.RESERVE)
    _assert_claims(c, None)
    _forward(c, o, None, relu=False)
    _backward(c, o, None, ("g0", "g1"), relu=False)
    _backward(c, o, None, ("g0",), relu=False, rev=True)


@pytest.mark.parametrize("c,pool", VARIANT_FORMS[:3])
def test_frozen_statistics(c, pool):
    """ops.bn_relu_bwd(frozen=True): the same kernels with the sums zeroed between the passes: dy = scale * dz exactly, dgamma
    and dbeta the reduce pass's"""
    o = _to_dev(R.operands(c.id))
    L.set_cu_reserve(R.RESERVE)
    _assert_claims(c, pool)
    _backward(c, o, pool, ("g0", "g1", "gp") if pool else ("g0", "g1"), frozen=True)


@pytest.mark.parametrize("c,pool", [VARIANT_FORMS[0], VARIANT_FORMS[2]])
def test_reduce_without_dgamma_and_dbeta(c, pool):
    """uz_bn_relu_bwd_reduce(dgamma = dbeta = NULL): the totals alone; one of the two alone is refused"""
    lib = L.load()
    o = _to_dev(R.operands(c.id))
    L.set_cu_reserve(R.RESERVE)
    _assert_claims(c, pool)
    N, H, W = c.shape
    rp = R.bwd_plan(c.dt, N, H, W, c.C, pool, 1)
    print(R.plan_line("bwd reduce" + (" pooled " + pool if pool else ""), c.dt, c.shape, c.C, rp))
    gp_rows = R.gp_rows(o.gp, c.shape, pool) if pool else None
    y, g0 = _in(o.y, c.dt, c.shape, M_Y, 5.0), _in(o.g0, c.dt, c.shape, M_G0, 5.0)
    gp = _in(gp_rows, c.dt, (N,) + R.pool_hw(H, W, pool), M_GP, 5.0) if pool else None
    d = _desc(c, y, g0, None, gp, None, pool, True, False)
    ws = torch.empty(rp.gx, 2, c.C, device=DEV)
    sums = torch.full((2, c.C), float("nan"), dtype=torch.float64, device=DEV)
    one = torch.full((c.C,), SENTINEL, device=DEV)
    args = (byref(d), y.ptr(), *(o.vec[i].data_ptr() for i in range(4)), g0.ptr(), None, gp.ptr() if gp else None, ws.data_ptr(),
            sums.data_ptr())
    assert lib.uz_bn_relu_bwd_reduce(*args, one.data_ptr(), None, L.stream_ptr()) != 0
    assert lib.uz_bn_relu_bwd_reduce(*args, None, one.data_ptr(), L.stream_ptr()) != 0
    L.check(lib.uz_bn_relu_bwd_reduce(*args, None, None, L.stream_ptr()), "uz_bn_relu_bwd_reduce")
    dz, xhat = R.backward_terms(o.y, o.vec, c.shape, o.g0, None, gp_rows, pool)
    R.check_totals(sums, None, None, R.totals(dz, xhat))
    assert bool((one == SENTINEL).all())


# ---- edges of the pool ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["S2rb", "S2rf", "S2cb", "S2cf"])
def test_floor_pool_of_a_one_row_map_is_refused(cid):
    """H = 1 or W = 1: the floor-mode pooled map is empty; the host says so and launches nothing"""
    c = R.CASES[cid]
    o = _to_dev(R.operands(cid))
    N, H, W = c.shape
    y, act = _in(o.y, c.dt, c.shape, M_Y, 5.0), _out(c.shape, c.C, c.dt, M_ACT)
    pooled = torch.full((max(1, N * (H // 2) * (W // 2)), c.C), SENTINEL, dtype=c.dt, device=DEV)
    rc = L.load().uz_bn_relu_add_apply(L.dtype_code(c.dt), y.ptr(), y.ld, o.vec[0].data_ptr(), o.vec[1].data_ptr(), N, H, W, c.C,
                                       None, 0, act.ptr(), act.ld, pooled.data_ptr(), c.C, 0, L.stream_ptr())
    assert rc != 0
    torch.cuda.synchronize()
    assert bool((act.buf == SENTINEL).all()) and bool((pooled == SENTINEL).all())
    with pytest.raises(L.HipLibraryError, match="floor-mode pool"):
        L.check(rc, "uz_bn_relu_add_apply")


# ---- the head's apply pass --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hid,K,rev", [("W7", 3, False), ("W8", 1, False), ("W8", 1, True), ("W8", 8, False), ("W8", 8, True),
                                       ("W8w", 8, False)])
def test_head_apply_against_float64(hid, K, rev):
    """uz_bn_relu_bwd_apply_head: the gradient is bf16(sum_k g[n, k, hw] w[k, c]) added in ascending k (exact on these
    operands), then treated as g0.  The rows handed to the finalize are the reference's sums over every 600th pixel: exact
    in fp32, two trips of bn_bwd_finalize_kernel<8>"""
    h = R.HEAD_CASES[hid]
    assert K in h.K
    N, H, W = h.shape
    P = N * H * W
    o = _to_dev(R.head_operands(hid, K))
    L.set_cu_reserve(R.RESERVE)
    plan = R.bwd_plan(BF16, N, H, W, h.C, None, 2)
    assert (plan.trips, plan.slots) == (h.trips, h.slots), plan
    print(R.plan_line(f"head apply K={K}" + (" from the end" if rev else ""), BF16, h.shape, h.C, plan))
    dx = R.head_gradient(o, h.shape)
    dz, xhat = R.backward_terms(o.y, o.vec, h.shape, dx)
    S = R.totals(dz, xhat)
    own = torch.arange(P, device=DEV) % R.HEAD_ROWS
    rows64 = torch.zeros(R.HEAD_ROWS, 2, h.C, dtype=torch.float64, device=DEV)
    rows64[:, 0].index_add_(0, own, dz)
    rows64[:, 1].index_add_(0, own, dz * xhat)
    rows = rows64.float()
    assert torch.equal(rows.double(), rows64) and R.fin_plan(R.HEAD_ROWS, h.C) == (8, 128, 2, 8)
    y, dy = _in(o.y, BF16, h.shape, M_Y, 5.0), _out(h.shape, h.C, BF16, M_DY)
    assert ops.bn_bwd_head_supported(y, K)
    sums = torch.full((2, h.C), float("nan"), dtype=torch.float64, device=DEV)
    dgamma, dbeta = torch.full((h.C,), float("nan"), device=DEV), torch.full((h.C,), float("nan"), device=DEV)
    ops.bn_relu_bwd_head(y, o.vec, ops.HeadGrad(o.g.contiguous(), o.w.contiguous(), rows), sums, dy, dgamma, dbeta, reverse=rev)
    R.check_totals(sums, dgamma, dbeta, S)
    want, A = R.dy_ref(dz, xhat, o.vec, S, P)
    R.check_dy(_split(dy)[0], want, A, dz, S, BF16, R.where_bwd(h.shape, plan, rev))
    assert _untouched(dy)


# ---- the finalize kernels ---------------------------------------------------------------------------------------------------
EPS, MOMENTUM = 1e-5, 0.1


def _finalize(rows, C, kind):
    stats, count, gamma, beta, rm, rv = (t.to(DEV) if torch.is_tensor(t) else t for t in R.finalize_inputs(rows, C, kind))
    plan = R.fin_plan(rows, C)
    print(f"    bn_finalize_kernel<{plan.ew}> rows {rows} x C {C}: {plan.blocks} blocks, {plan.ng} row groups, {plan.trips} trips")
    want = R.finalize_ref(stats, count, gamma, beta, EPS, MOMENTUM, rm, rv)
    rm1, rv1 = rm.clone(), rv.clone()
    vec = ops.bn_finalize(stats, count, gamma, beta, EPS, MOMENTUM, rm1, rv1)
    for name, got, ref in zip(("scale", "shift", "mean", "invstd", "running_mean", "running_var"), (*vec, rm1, rv1), want):
        R.check_ulp(got, ref, f"{name} ({kind}, rows {rows}, C {C})")
    assert torch.equal(ops.bn_finalize(stats, count, gamma, beta, EPS, MOMENTUM, None, None), vec)   # without running statistics
    return vec, want


@pytest.mark.parametrize("C", R.FIN_C)
@pytest.mark.parametrize("rows", R.FIN_ROWS)
def test_finalize_kernels_against_float64(rows, C):
    """both EW choices, one trip of `r += 4 * NG` and several, a last channel block that is partly empty.  Forward: partial
    rows of exact integers, every output within one fp32 ulp of the float64 formula.  Backward: integer rows, the totals and
    dgamma / dbeta bit for bit, with and without dgamma / dbeta"""
    L.set_cu_reserve(R.RESERVE)
    _finalize(rows, C, "plain")
    lib = L.load()
    part = R.bwd_finalize_inputs(rows, C).to(DEV)
    S = torch.stack([part[:, 0].double().sum(0), part[:, 1].double().sum(0)])
    for with_vectors in (True, False):
        sums = torch.full((2, C), float("nan"), dtype=torch.float64, device=DEV)
        dgamma, dbeta = torch.full((C,), SENTINEL, device=DEV), torch.full((C,), SENTINEL, device=DEV)
        L.check(lib.uz_bn_bwd_finalize(part.data_ptr(), rows, C, sums.data_ptr(), dgamma.data_ptr() if with_vectors else None,
                                       dbeta.data_ptr() if with_vectors else None, L.stream_ptr()), "uz_bn_bwd_finalize")
        R.check_totals(sums, dgamma if with_vectors else None, dbeta if with_vectors else None, S)
        if not with_vectors:
            assert bool((dgamma == SENTINEL).all()) and bool((dbeta == SENTINEL).all())


def test_finalize_clamps_a_negative_variance():
    """sums of squares of zero beside nonzero sums: var = -mean^2 is clamped to 0, invstd = 1 / sqrt(eps)"""
    vec, want = _finalize(127, 96, "clamp")
    eps = float(torch.tensor(EPS, dtype=F32))
    assert torch.equal(want[3], torch.full_like(want[3], 1.0 / eps ** 0.5))


def test_finalize_does_not_unbias_a_count_of_one():
    """count == 1: running_var takes the biased variance (count / (count - 1) would divide by zero)"""
    vec, want = _finalize(1, 96, "count1")
    assert bool(torch.isfinite(want[5]).all())


# ---- normal operands --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,C", [(BF16, 520), (F32, 260)])
def test_normal_operands_against_float64(dt, C):
    """randn operands on the smallest walking map ((1, 89, 95), gy = 2: 3 trips of the reduce pass with 4 slots, 2 of the
    apply pass), the true batch statistics from uz_colstats + uz_bn_finalize.  The totals within the forward error of a sum,
    |S - S_ref| <= (L + by + 2) 2^-24 sum |terms| with L = 4 * trips the longest per-thread chain and by the LDS chain; dy
    within the dyadic cases' bound plus the totals' share, |scale| (dS0 + |xhat| dS1) / P"""
    shape = R.CASES["W6"].shape
    N, H, W = shape
    P = N * H * W
    L.set_cu_reserve(R.RESERVE)
    rp, bp = R.bwd_plan(dt, N, H, W, C, None, 1), R.bwd_plan(dt, N, H, W, C, None, 2)
    assert (rp.trips, rp.slots, rp.gy, bp.trips, bp.slots) == (3, 4, 2, 2, 4), (rp, bp)
    print(R.plan_line("bwd reduce", dt, shape, C, rp))
    print(R.plan_line("bwd apply from the end", dt, shape, C, bp))
    g = torch.Generator().manual_seed(C)
    yv = (torch.randn(P, C, generator=g) * 1.5 + 0.3).to(dt).to(DEV)
    gv = torch.randn(P, C, generator=g).to(dt).to(DEV)
    gamma, beta = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
    y, g0 = Act(yv, 0, C, N, H, W), Act(gv, 0, C, N, H, W)
    vec = ops.bn_finalize(ops.colstats(y), P, gamma, beta, EPS, MOMENTUM, None, None)
    dy = _out(shape, C, dt, M_DY)
    sums = torch.full((2, C), float("nan"), dtype=torch.float64, device=DEV)
    dgamma, dbeta = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    ops.bn_relu_bwd(y, vec, g0, None, None, sums, dy, dgamma, dbeta)
    dz, xhat = R.backward_terms(yv, vec, shape, gv)
    S = R.totals(dz, xhat)
    T = torch.stack([dz.abs().sum(0), (dz * xhat).abs().sum(0)])
    dS = (R.NPIX * rp.trips + rp.by + 2) * 2.0 ** -24 * T
    err = (sums - S).abs()
    ratio = float((err / dS.clamp_min(1e-300)).max())        # (a channel the ReLU closes everywhere has no terms: 0 <= 0)
    print(f"    totals: max |S - S_ref| / bound = {ratio:.3e}")
    assert bool((err <= dS).all()), ratio
    assert torch.equal(dbeta, sums[0].float()) and torch.equal(dgamma, sums[1].float())
    want, A = R.dy_ref(dz, xhat, vec, S, P)
    extra = vec[0].double().abs() * (dS[0] + xhat.abs() * dS[1]) / P
    R.check_dy(_split(dy)[0], want, A, dz, S, dt, R.where_bwd(shape, bp, True), extra=extra)
    assert _untouched(dy)
