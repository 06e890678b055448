"""CPU: the ground tests/test_bn_walk_gpu.py stands on, checked without a GPU (helpers: tests/bn_walk_ref.py).

  * every case of the table gets the trips, live slots and block shape it claims from the restated plans (apply_plan,
    bwd_plan: grid_for and reduce_shape of uz_eltwise.hip) at 128 CUs; the restatement at 256 CUs is printed beside it;
  * the restated grid of the reduce pass is the library's: uz_bn_relu_bwd_workspace_bytes(d, pool) / (8 C) -- a host-side
    query that answers without a device -- under a reserve of 128 CUs and of none, for every case, dense and as channel
    windows of wider buffers;
  * the EW choice and the trips of the finalize kernels on rows and channel counts worked by hand;
  * the preconditions of exactness hold for every case: rounding to the run dtype changes nothing, the sums of |dz| and of
    |dz xhat| in their units stay below 2^24, at least 5 % of the pooled (window, channel) pairs tie at a positive maximum;
    the finalize inputs have var >= mean^2 / 16.  These are conditions on the inputs, not measurements;
  * the float64 backward reference is torch.autograd's through F.batch_norm(training=True), relu and max_pool2d, to 1e-12;
  * the restated walk visits every unit exactly once, from the front and from the end;
  * the comparators see planted faults of the kind a wrong walk leaves, and say where."""
from ctypes import byref

import pytest
import torch
import torch.nn.functional as F

import bn_walk_ref as R  # tests/bn_walk_ref.py (pytest puts this directory on sys.path)
from unet_zoo_amd import _lib as L

BF16, F32 = R.BF16, R.F32
FORMS = [pytest.param(c, pool, id=f"{c.id}-{pool or 'nopool'}") for c in R.CASES.values() for pool, _ in R.forms(c)]
HEADS = [pytest.param(h, id=h.id) for h in R.HEAD_CASES.values()]


@pytest.fixture(autouse=True)
def _restore():
    yield
    L.set_cu_reserve(0)


@pytest.fixture(scope="module", autouse=True)
def _free_references():
    yield
    R.operands.cache_clear()
    R.head_operands.cache_clear()


# ---- plans ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,pool", FORMS)
def test_case_walks_as_the_table_claims(c, pool):
    N, H, W = c.shape
    claim = c.claims[pool is not None]
    ap, rp, bp = (R.apply_plan(c.dt, N, H, W, c.C, pool), R.bwd_plan(c.dt, N, H, W, c.C, pool, 1),
                  R.bwd_plan(c.dt, N, H, W, c.C, pool, 2))
    assert (ap.trips, rp.trips, bp.trips) == (claim.apply, claim.reduce, claim.bwd), (ap, rp, bp)
    if pool is None:
        assert (rp.slots, bp.slots) == (claim.rslots, claim.bslots), (rp, bp)
    if c.id in R.BLOCKS:
        assert (rp.bx, rp.by, rp.gy) == (bp.bx, bp.by, bp.gy) == R.BLOCKS[c.id]
    assert rp.bx * rp.by == 256 and rp.ustride == rp.gx * rp.by
    for cus in (R.CUS, R.CUS_HW):
        print(f"  at {cus} CUs:")
        for form, plan in (("apply", R.apply_plan(c.dt, N, H, W, c.C, pool, cus)), ("bwd reduce", R.bwd_plan(c.dt, N, H, W, c.C, pool, 1, cus)),
                           ("bwd apply", R.bwd_plan(c.dt, N, H, W, c.C, pool, 2, cus))):
            print(R.plan_line(form + (" pooled " + pool if pool else ""), c.dt, c.shape, c.C, plan))


def test_walking_cases_are_the_smallest_that_walk():
    """what each W row of the table is for, by name: several trips of every loop, all four slots, a partial last trip, idle
    channel lanes, a second grid column with one live lane"""
    p = {i: R.CASES[i] for i in R.WALKING}
    for i in ("W1", "W2"):
        c = p[i]
        rp, bp = R.bwd_plan(c.dt, *c.shape, c.C, None, 1), R.bwd_plan(c.dt, *c.shape, c.C, None, 2)
        assert 0 < bp.units - (bp.trips - 1) * bp.per_trip < bp.ustride          # the last trip: slot 0 alone, and not all of it
        assert rp.units > (rp.trips - 1) * rp.per_trip and rp.trips >= 2 and rp.slots == 4
    for i in ("W3", "W4"):
        c = p[i]
        assert c.shape[1] % 2 and c.shape[2] % 2                                 # both borders clipped
    c = p["W5"]
    cc = c.C // 8
    assert R.bwd_plan(c.dt, *c.shape, c.C, None, 1).bx - cc == 4                 # four lanes fail `cok`
    c = p["W6"]
    rp = R.bwd_plan(c.dt, *c.shape, c.C, None, 1)
    assert rp.gy == 2 and c.C // 8 - rp.bx == 1                                  # the second column: one live lane
    for c in p.values():
        assert c.shape[0] * c.shape[1] * c.shape[2] * c.C <= 17_000_000


@pytest.mark.parametrize("h", HEADS)
def test_head_case_walks_as_the_table_claims(h):
    """uz_bn_relu_bwd_apply_head launches on bnbwd_shape(d, false, pass 2): the grid and walk of the plain apply pass"""
    plan = R.bwd_plan(BF16, *h.shape, h.C, None, 2)
    assert (plan.trips, plan.slots) == (h.trips, h.slots), plan
    assert (plan.bx, plan.by, plan.gy) == (8, 32, 1)
    if h.id == "W7":
        assert h.shape[0] > 1 and plan.trips == 2                               # img = p / HW across images, two trips
    for cus in (R.CUS, R.CUS_HW):
        print(R.plan_line(f"head apply at {cus} CUs", BF16, h.shape, h.C, R.bwd_plan(BF16, *h.shape, h.C, None, 2, cus)))


def _desc(c, pool, wide=False):
    N, H, W = c.shape
    v = R.vec_of(c.dt)
    lds = [c.C + (2 * i + 1) * v for i in range(5)] if wide else [c.C] * 5
    flags = (1 if pool == "ceil" else 0)
    return L.BnBwdDesc(L.dtype_code(c.dt), N, H, W, c.C, *lds, flags)


@pytest.mark.parametrize("c,pool", FORMS)
def test_restated_reduce_grid_is_the_library_grid(c, pool):
    lib = L.load()
    for reserve in (R.RESERVE, 0):
        L.set_cu_reserve(reserve)
        plan = R.bwd_plan(c.dt, *c.shape, c.C, pool, 1, R.CUS_HW - reserve)
        for wide in (False, True):
            d = _desc(c, pool, wide)
            wsb = L.check_count(lib.uz_bn_relu_bwd_workspace_bytes(byref(d), int(pool is not None)), "workspace")
            assert wsb % (8 * c.C) == 0 and wsb // (8 * c.C) == plan.gx, (reserve, wsb, plan)


@pytest.mark.parametrize("rows,C,ew,trips,blocks", [
    (1, 8, 32, 1, 1), (127, 512, 32, 1, 16), (128, 512, 8, 1, 64), (128, 520, 32, 1, 17), (512, 96, 8, 1, 12),
    (513, 96, 8, 2, 12), (513, 520, 32, 5, 17), (1024, 8, 8, 2, 1), (1024, 520, 32, 8, 17), (129, 520, 32, 2, 17)])
def test_finalize_plan_on_hand_worked_shapes(rows, C, ew, trips, blocks):
    """EW = 8 when rows >= 128 and C <= 512, else 32; a trip covers 4 * 1024 / EW rows; one block per EW channels"""
    assert R.fin_plan(rows, C) == (ew, 1024 // ew, trips, blocks)


def test_finalize_table_covers_both_widths_and_several_trips():
    plans = {(r, C): R.fin_plan(r, C) for r in R.FIN_ROWS for C in R.FIN_C}
    assert {p.ew for p in plans.values()} == {8, 32}
    for ew in (8, 32):
        assert {min(p.trips, 2) for p in plans.values() if p.ew == ew} == {1, 2}
    assert any(C % p.ew for (r, C), p in plans.items())                         # a last channel block that is partly empty


# ---- preconditions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,pool", FORMS)
def test_preconditions_of_exactness(c, pool):
    o = R.operands(c.id)
    fig = R.assert_exact_preconditions(c, o, pool, [R.bwd_plan(c.dt, *c.shape, c.C, pool, 1)])
    print("   ", {k: round(v, 4) for k, v in fig.items()})
    sc, sh = o.vec[0], o.vec[1]
    assert bool((sc < 0).any()) and bool((sc == 0).any())
    assert bool(((sc == 0) & (sh > 0)).any())                                    # every tap ties at a positive value
    if c.C >= 16:
        assert bool(((sc == 0) & (sh < 0)).any())                                # dz, S0, S1 and dy exactly 0


@pytest.mark.parametrize("h", HEADS)
def test_preconditions_of_exactness_head(h):
    for K in h.K:
        o = R.head_operands(h.id, K)
        for t in (o.y, o.vec):
            assert torch.equal(t.to(BF16).float(), t)
        g = o.g.double().permute(0, 2, 3, 1).reshape(-1, K)
        exact = g @ o.w.double()
        assert torch.equal(R.head_gradient(o, h.shape), exact)                   # exact in bf16, in any order
        dz, xhat = R.backward_terms(o.y, o.vec, h.shape, exact)
        a0, a1 = dz.abs() * 4, (dz * xhat).abs() * 32
        assert torch.equal(a0, a0.round()) and torch.equal(a1, a1.round())
        # the rows this case hands to the finalize kernel are sums over every R.HEAD_ROWS-th pixel: exact in fp32
        for a in (a0, a1):
            r = torch.zeros(R.HEAD_ROWS, h.C, dtype=torch.float64).index_add_(0, torch.arange(a.shape[0]) % R.HEAD_ROWS, a)
            assert float(r.max()) < 2 ** 24


@pytest.mark.parametrize("kind,rows,C", [("plain", r, C) for r in R.FIN_ROWS for C in R.FIN_C] + [("clamp", 127, 96), ("count1", 1, 96)])
def test_finalize_inputs(kind, rows, C):
    stats, count, gamma, beta, rm, rv = R.finalize_inputs(rows, C, kind)
    assert torch.equal(stats, stats.round()) and float(stats.abs().max()) < 2 ** 24
    t1, t2 = stats[:, 0].double().sum(0), stats[:, 1].double().sum(0)
    m = t1 / count
    var = t2 / count - m * m
    if kind == "clamp":
        assert bool((var <= 0).all()) and bool((var < 0).any())
    else:
        assert bool((var >= m * m / 16).all()) and bool((var > 0).all())
    if kind == "count1":
        assert count == 1.0 and torch.equal(var, torch.full_like(var, 5.0))
    assert bool((gamma == 0).any()) and bool((gamma < 0).any())
    p = R.bwd_finalize_inputs(rows, C)
    assert torch.equal(p, p.round()) and float(p.abs().sum(0).max()) < 2 ** 24


# ---- the reference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", [None, "floor", "ceil"])
def test_backward_reference_is_autograd(pool):
    shape, C, eps = (2, 7, 9), 8, 1e-5
    N, H, W = shape
    P = N * H * W
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    gamma = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    beta = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    a = torch.relu(F.batch_norm(x, None, None, gamma, beta, training=True, eps=eps))
    g0, g1 = torch.randn(P, C, generator=g, dtype=torch.float64), torch.randn(P, C, generator=g, dtype=torch.float64)
    loss = (a * R.nchw(g0, shape)).sum() + (a * R.nchw(g1, shape)).sum()
    gp = None
    if pool:
        Hp, Wp = R.pool_hw(H, W, pool)
        gp = torch.randn(N * Hp * Wp, C, generator=g, dtype=torch.float64)
        loss = loss + (F.max_pool2d(a, 2, 2, ceil_mode=pool == "ceil") * R.nchw(gp, (N, Hp, Wp))).sum()
    loss.backward()
    with torch.no_grad():
        y = R.nhwc(x)
        mean, var = y.mean(0), y.var(0, unbiased=False)
        invstd = 1.0 / torch.sqrt(var + eps)
        vec = torch.stack([gamma * invstd, beta - mean * gamma * invstd, mean, invstd])
        dz, xhat = R.backward_terms(y, vec, shape, g0, g1, gp, pool)
        S = R.totals(dz, xhat)
        dy, _ = R.dy_ref(dz, xhat, vec, S, P)
        for got, want in ((dy, R.nhwc(x.grad)), (S[0], beta.grad), (S[1], gamma.grad)):
            assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_forward_reference_pools_the_stored_value():
    """the pool sees act as stored: with a residual in bf16 the sum is rounded before the maximum is taken"""
    shape, C = (1, 4, 4), 8
    g = torch.Generator().manual_seed(5)
    y, res = torch.randn(16, C, generator=g).to(BF16), (torch.randn(16, C, generator=g) * 100).to(BF16)
    vec = torch.stack([torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C)])
    act, pooled = R.forward_ref(y, vec, shape, BF16, True, res, "floor")
    assert act.dtype == pooled.dtype == BF16
    assert torch.equal(pooled.float(), R.nhwc(F.max_pool2d(R.nchw(act.float(), shape), 2, 2)))


# ---- the walk ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,pool", FORMS)
def test_walk_visits_every_unit_once(c, pool):
    for pass_ in (1, 2):
        for cus in (R.CUS, R.CUS_HW):
            plan = R.bwd_plan(c.dt, *c.shape, c.C, pool, pass_, cus)
            for rev in (False, True):
                w = R.walk(plan, rev)
                assert torch.equal(w.unit.sort().values, torch.arange(plan.units)), (plan, rev)
                assert int(w.row.max()) < plan.gx and int(w.trip.max()) == plan.trips - 1
                if not pool:
                    assert int(w.slot.max()) == plan.slots - 1
                own = R.owners(plan, rev)
                assert int(own.min()) >= 0
                # from the front, the owner of unit q is workgroup row (q mod ustride) / by
                q = torch.arange(plan.units)
                q = plan.units - 1 - q if rev else q
                assert torch.equal(own[:, 0], (q % plan.ustride) // plan.by)


@pytest.mark.parametrize("h", HEADS)
def test_head_walk_visits_every_pixel_once(h):
    plan = R.bwd_plan(BF16, *h.shape, h.C, None, 2)
    for rev in (False, True):
        w = R.walk(plan, rev)
        assert torch.equal(w.unit.sort().values, torch.arange(plan.units))
        assert int(w.slot.max()) == h.slots - 1 and int(w.trip.max()) == h.trips - 1


# ---- planted faults ---------------------------------------------------------------------------------------------------------
FC = R.CASES["W6"]
FCUS = 32                     # the comparators take any plan: at 32 CUs the case makes 9 / 5 trips, so a second trip has all four slots


def _ground(pool, rev=False):
    o = R.operands(FC.id)
    gp = R.gp_rows(o.gp, FC.shape, pool) if pool else None
    dz, xhat = R.backward_terms(o.y, o.vec, FC.shape, o.g0, o.g1, gp, pool)
    S = R.totals(dz, xhat)
    P = dz.shape[0]
    dy, A = R.dy_ref(dz, xhat, o.vec, S, P)
    return o, dz, xhat, S, dy, A


@pytest.mark.parametrize("dt", [BF16, F32])
def test_comparators_pass_the_reference_itself(dt):
    o, dz, xhat, S, dy, A = _ground(None)
    rp, bp = R.bwd_plan(FC.dt, *FC.shape, FC.C, None, 1, FCUS), R.bwd_plan(FC.dt, *FC.shape, FC.C, None, 2, FCUS)
    R.check_dy(dy.to(dt), dy, A, dz, S, dt, R.where_bwd(FC.shape, bp))
    rows = R.rows_ref(dz, xhat, rp, FC.shape, False)
    assert torch.equal(rows.sum(0), S)
    R.check_rows(rows.float(), rows)
    R.check_totals(S.clone(), S[1].float(), S[0].float(), S)
    act, _ = R.forward_ref(o.y, o.vec, FC.shape, dt)
    R.assert_same(act, act.clone(), "act", R.where_apply(FC, None, R.apply_plan(dt, *FC.shape, FC.C, None)))


@pytest.mark.parametrize("rev", [False, True])
def test_dy_check_names_a_zeroed_pixel_of_slot_2_of_the_second_trip(rev):
    o, dz, xhat, S, dy, A = _ground(None)
    bp = R.bwd_plan(FC.dt, *FC.shape, FC.C, None, 2, FCUS)
    own = R.owners(bp, rev)
    pix = int(((own[:, 1] == 1) & (own[:, 2] == 2)).nonzero()[7])
    ch = int((dy[pix].abs() > 0.5).nonzero()[0])
    got = dy.to(BF16)
    got[pix, ch] = 0
    with pytest.raises(AssertionError) as e:
        R.check_dy(got, dy, A, dz, S, BF16, R.where_bwd(FC.shape, bp, rev))
    msg = str(e.value)
    assert "1 of" in msg and f"pixel {pix} channel {ch}: trip 1, slot 2, workgroup row {int(own[pix, 0])}" in msg, msg


def test_dy_check_sees_one_ulp_too_many_in_fp32():
    o, dz, xhat, S, dy, A = _ground(None)
    bp = R.bwd_plan(FC.dt, *FC.shape, FC.C, None, 2, FCUS)
    pix, ch = bp.units - 1, 3
    got = dy.float()
    got[pix, ch] += 16 * 2.0 ** -21 * float(A[pix, ch])
    with pytest.raises(AssertionError, match=f"pixel {pix} channel {ch}: trip"):
        R.check_dy(got, dy, A, dz, S, F32, R.where_bwd(FC.shape, bp))


def test_dy_check_sees_a_pool_gradient_sent_to_the_second_of_two_tied_taps():
    """a window whose first two taps tie at a positive maximum: the gradient belongs to tap (0, 0); moved to tap (0, 1), the
    sums are what they were (equal y, equal xhat) and dy differs in exactly those two pixels"""
    pool = "ceil"
    o, dz, xhat, S, dy, A = _ground(pool)
    N, H, W = FC.shape
    gp = R.gp_rows(o.gp, FC.shape, pool)
    pre = R.nchw(o.y.double() * o.vec[0].double() + o.vec[1].double(), FC.shape)
    Wp = R.pool_hw(H, W, pool)[1]
    found = None
    for ch in range(FC.C):
        if float(o.vec[0, ch]) == 0:
            continue
        p = pre[0, ch]
        t00, t01, t10, t11 = p[0:H - 1:2, 0:W - 1:2], p[0:H - 1:2, 1:W:2], p[1:H:2, 0:W - 1:2], p[1:H:2, 1:W:2]
        hit = ((t00 == t01) & (t00 > 0) & (t00 > t10) & (t00 > t11)).nonzero()
        for ho, wo in hit.tolist():
            if float(gp[ho * Wp + wo, ch]) != 0:
                found = (ch, ho, wo)
                break
        if found:
            break
    assert found is not None
    ch, ho, wo = found
    p0, p1 = (2 * ho) * W + 2 * wo, (2 * ho) * W + 2 * wo + 1
    gval = float(gp[ho * Wp + wo, ch])
    assert float(dz[p0, ch]) == float(o.g0[p0, ch] + o.g1[p0, ch]) + gval       # the reference sent it to the first tap
    dz2 = dz.clone()
    dz2[p0, ch] -= gval
    dz2[p1, ch] += gval
    assert torch.equal(R.totals(dz2, xhat), S)
    got, _ = R.dy_ref(dz2, xhat, o.vec, S, dz.shape[0])
    bp = R.bwd_plan(FC.dt, *FC.shape, FC.C, pool, 2, FCUS)
    with pytest.raises(AssertionError) as e:
        R.check_dy(got.float(), dy, A, dz, S, F32, R.where_bwd(FC.shape, bp))
    msg = str(e.value)
    assert "2 of" in msg and "in 2 pixels" in msg and f"pixel {p0} channel {ch}" in msg and f"pixel {p1} channel {ch}" in msg, msg


def test_rows_check_sees_a_unit_moved_between_two_workgroup_rows():
    """the totals are what they were; the rows are not, and check_rows() names both"""
    o, dz, xhat, S, dy, A = _ground(None)
    rp = R.bwd_plan(FC.dt, *FC.shape, FC.C, None, 1, FCUS)
    rows = R.rows_ref(dz, xhat, rp, FC.shape, False)
    own = R.owners(rp, False)
    pix = int(((own[:, 0] == 9) & (own[:, 1] == 2) & (own[:, 2] == 1)).nonzero()[0])
    assert bool((dz[pix] != 0).any())
    moved = rows.clone()
    for k, v in enumerate((dz[pix], dz[pix] * xhat[pix])):
        moved[9, k] -= v
        moved[10, k] += v
    R.check_totals(moved.sum(0), None, None, S)
    with pytest.raises(AssertionError, match=r"2 of 64 workgroup rows differ \(first \[9, 10\]\); row 9, "):
        R.check_rows(moved.float(), rows)


def test_rows_differ_between_the_two_walks():
    """the walk from the end changes WHICH units a workgroup sums: rows of the wrong walk do not pass"""
    o, dz, xhat, S, dy, A = _ground(None)
    rp = R.bwd_plan(FC.dt, *FC.shape, FC.C, None, 1, FCUS)
    fwd, back = R.rows_ref(dz, xhat, rp, FC.shape, False), R.rows_ref(dz, xhat, rp, FC.shape, True)
    assert torch.equal(fwd.sum(0), back.sum(0))
    with pytest.raises(AssertionError, match="workgroup rows differ"):
        R.check_rows(back.float(), fwd)


def test_same_check_names_the_trip_of_the_forward_pass():
    o = R.operands(FC.id)
    ap = R.apply_plan(FC.dt, *FC.shape, FC.C, None)
    act, _ = R.forward_ref(o.y, o.vec, FC.shape, FC.dt)
    got = act.clone()
    pix, ch = (2 * 256 * ap.grid + 256 * 5 + 17) // (FC.C // 8), 0               # third trip, workgroup 5 ...
    idx = pix * (FC.C // 8)
    got.view(torch.int16)[pix, ch] += 1
    with pytest.raises(AssertionError, match=f"pixel {pix} channel 0: trip {idx // (256 * ap.grid)}, workgroup {(idx // 256) % ap.grid}"):
        R.assert_same(got, act, "act", R.where_apply(FC, None, ap))
