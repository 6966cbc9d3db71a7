"""Plan audit on the GPU (`uavac_minsnap_audit_dev`, csrc/minsnap_audit.hip), through the C ABI: per mission the row total, the
peaks of the quantities the control law clips and, per cuboid, the samples inside it -- from coefficients and row counts alone.

What is compared with what:
  * against the PRODUCT'S OWN ROWS everything is exact (no tolerance): the kernel uses the sampler's arithmetic, forms the squares
    as separately rounded products and sums and takes one correctly rounded sqrt of the largest, which is what NumPy computes from
    the sampled rows (`np.sqrt(vx * vx + vy * vy).max()`); max, integer add and min do not depend on order.  Floats are compared by
    value (NaN equal to NaN);
  * against the ORACLE (oracle.c_oracle.plan_threads: its own solve and its own sampler) the peaks hold to 1e-5 of max(1, |peak|)
    -- SURVEY 8(c), the project's bar for sampled velocities and accelerations, applied to every element instead of to a column's
    maximum (so never looser than `conftest.col_err`); a pure ratio is undefined for the peaks that are 0 up to rounding, e.g. the
    climb rate of a mission that only descends.  Row totals, hit counts and first indices are exact; a hit difference is allowed
    only where the oracle's sample nearest a face lies within 1e-9 of it (tests/test_gpu_plan_whole_batch_parity.py's convention),
    such cases are counted and the cap is 0: for these mission sets and cuboids the oracle's nearest sample is >= 7e-5 from every
    face and every mission is >= 1e-3 from every flight limit (checked on the CPU with the oracle).
"""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

VEL, DT = 3.0, 0.01
CUBS = np.array([[6.0, 14.0, 2.0, 9.0, -4.0, -2.8], [10.0, 12.0, 5.0, 7.0, -10.0, 0.0], [3.7, 4.3, 4.0, 10.0, -3.4, -2.8]])
SETS = ((1, 48), (2, 48), (8, 96), (20, 24), (8, 37))       # (m, B); (8, 37): a partial wavefront and a partial workgroup
EXPECT_HIT_MISSIONS = {(1, 48): (8, 1, 2), (2, 48): (13, 1, 4), (8, 96): (32, 10, 6), (20, 24): (9, 4, 3)}
SENT_F, SENT_I, PAD = -1.2345e300, -7777, 96
PEAK_TOL, FACE_TIE = 1e-5, 1e-9


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    e = Engine("cuda:0")
    yield e
    e.ctx.set_option("audit_lanes", 16)


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def audit_abi(eng, coeffs, seg_rows, seg_offsets, B, m, dt, cubs, check_bounds=True):
    """One call of uavac_minsnap_audit_dev on device tensors -> (audit (8, B), hit_rows (n, B), first_hit (n, B)) as NumPy.  The
    outputs are the middle of larger sentinel-filled buffers: nothing outside [rows][B] may be written."""
    import torch
    n = 0 if cubs is None else len(cubs)
    dev = dict(device=eng.device)
    abuf = torch.full((PAD + 8 * B + PAD,), SENT_F, dtype=torch.float64, **dev)
    hbuf = torch.full((PAD + n * B + PAD,), SENT_I, dtype=torch.int32, **dev)
    fbuf = torch.full((PAD + n * B + PAD,), SENT_I, dtype=torch.int32, **dev)
    cub = None if n == 0 else torch.as_tensor(np.ascontiguousarray(cubs, dtype=np.float64)).to(eng.device)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_audit_dev", _p(coeffs), _p(seg_rows), _p(seg_offsets), int(B), int(m), float(dt), _p(cub), n,
                 _p(abuf[PAD:]), _p(hbuf[PAD:]) if n else None, _p(fbuf[PAD:]) if n else None)
    torch.cuda.synchronize()
    a, h, f = abuf.cpu().numpy(), hbuf.cpu().numpy(), fbuf.cpu().numpy()
    if check_bounds:
        assert (a[:PAD] == SENT_F).all() and (a[PAD + 8 * B:] == SENT_F).all()
        for x in (h, f):
            assert (x[:PAD] == SENT_I).all() and (x[PAD + n * B:] == SENT_I).all()
        assert not (a[PAD:PAD + 8 * B] == SENT_F).any() and not (h[PAD:PAD + n * B] == SENT_I).any()
        assert not (f[PAD:PAD + n * B] == SENT_I).any()
    return a[PAD:PAD + 8 * B].reshape(8, B).copy(), h[PAD:PAD + n * B].reshape(n, B).copy(), f[PAD:PAD + n * B].reshape(n, B).copy()


def audit_of_plan(eng, plan, cubs, **kw):
    ragged = hasattr(plan, "seg_offsets")
    return audit_abi(eng, plan.coeffs, plan.seg_rows, plan.seg_offsets if ragged else None, plan.B, plan.max_m if ragged else plan.m,
                     plan.dt, cubs, **kw)


def audit_from_rows(rows, ro, cubs):
    """The same three arrays recomputed with NumPy from sampled rows (N, 11) and row offsets (B + 1,)."""
    B, n = len(ro) - 1, 0 if cubs is None else len(cubs)
    a, h, f = np.empty((8, B)), np.zeros((n, B), np.int32), np.full((n, B), -1, np.int32)
    for b in range(B):
        r = rows[ro[b]:ro[b + 1]]
        x, y, z, vx, vy, vz, ax, ay, az = (r[:, k] for k in range(9))
        a[:, b] = (len(r), np.sqrt(vx * vx + vy * vy).max(), (-vz).max(), vz.max(), np.sqrt(ax * ax + ay * ay).max(), (-az).max(),
                   az.max(), np.sqrt(vx * vx + vy * vy + vz * vz).max())
        for c in range(n):
            q = cubs[c]
            inside = (x >= q[0]) & (x <= q[1]) & (y >= q[2]) & (y <= q[3]) & (z >= q[4]) & (z <= q[5])
            h[c, b] = inside.sum()
            f[c, b] = np.flatnonzero(inside)[0] if inside.any() else -1
    return a, h, f


def same(got, want):
    return all(g.shape == w.shape and np.array_equal(g, w, equal_nan=g.dtype.kind == "f") for g, w in zip(got, want))


def face_margin(rows, cub):
    lo = np.stack([rows[:, 0] - cub[0], cub[1] - rows[:, 0], rows[:, 1] - cub[2], cub[3] - rows[:, 1], rows[:, 2] - cub[4],
                   cub[5] - rows[:, 2]], axis=1)
    return lo.min(axis=1)


_CACHE = {}


def case(eng, m, B):
    """Per mission set, computed once and left unchanged: the plan with rows, the rows-free plan, the rows on the host and what
    they show."""
    if (m, B) not in _CACHE:
        from oracle import minsnap_oracle as mo
        wps = mo.synthetic_missions(B, m)
        plan = eng.plan(wps, VEL, DT)
        free = eng.plan(wps, VEL, DT, rows=False)
        rows, ro = plan.traj.cpu().numpy(), plan.row_offsets.cpu().numpy()
        _CACHE[(m, B)] = dict(wps=wps, plan=plan, free=free, rows=rows, ro=ro, want=audit_from_rows(rows, ro, CUBS))
    return _CACHE[(m, B)]


# ------------------------------------------------------------------------------------------------ 1: the product's own rows
@pytest.mark.parametrize("m, B", SETS)
def test_audit_equals_what_the_products_rows_show(eng, m, B):
    k = case(eng, m, B)
    assert k["free"].traj is None
    for lanes in (16, 64):                                        # lanes per mission: a tuning knob, same results
        eng.ctx.set_option("audit_lanes", lanes)
        got_free = audit_of_plan(eng, k["free"], CUBS)
        got_rows = audit_of_plan(eng, k["plan"], CUBS)
        assert same(got_free, got_rows), (m, B, lanes)
        assert same(got_free, k["want"]), (m, B, lanes, np.abs(got_free[0] - k["want"][0]).max(axis=1))
        no_cub = audit_of_plan(eng, k["free"], None)              # n_cuboids == 0 with NULLs: the other kernel variant
        assert np.array_equal(no_cub[0], k["want"][0]) and no_cub[1].shape == (0, B)
    eng.ctx.set_option("audit_lanes", 16)
    # the public interface gives the same tensors, for both kinds of plan, and never needs the rows
    for plan in (k["free"], k["plan"]):
        a = eng.audit(plan, CUBS)
        fields = (a.rows, a.speed_xy, a.ascent, a.descent, a.accel_xy, a.accel_up, a.accel_down, a.speed)
        assert np.array_equal(np.stack([t.cpu().numpy() for t in fields]), k["want"][0])
        assert same((a.hit_rows.cpu().numpy(), a.first_hit.cpu().numpy()), k["want"][1:])
    none = eng.audit(k["free"])
    assert tuple(none.hit_rows.shape) == tuple(none.first_hit.shape) == (0, B)
    assert np.array_equal(none.block.cpu().numpy(), k["want"][0])


# ------------------------------------------------------------------------------------------------------------ 2: the oracle
@pytest.mark.parametrize("m, B", SETS)
def test_audit_against_the_oracle(eng, m, B):
    import torch
    from oracle import c_oracle as cc
    from uav_ac.scoring import plan_feasibility
    k = case(eng, m, B)
    ref = cc.plan_threads(k["wps"], VEL, DT)
    want = audit_from_rows(ref["rows"], ref["row_offsets"], CUBS)
    a = eng.audit(k["free"], CUBS)
    got = (a.block.cpu().numpy(), a.hit_rows.cpu().numpy(), a.first_hit.cpu().numpy())
    assert np.array_equal(got[0][0], want[0][0])                                     # row totals: exact
    err = np.abs(got[0][1:] - want[0][1:]) / np.maximum(1.0, np.abs(want[0][1:]))
    print(f"audit vs oracle m={m} B={B}: worst peak error {err.max(axis=1)}")
    assert (err <= PEAK_TOL).all(), err.max(axis=1)
    ties = 0
    for c, b in zip(*np.nonzero((got[1] != want[1]) | (got[2] != want[2]))):
        r = ref["rows"][ref["row_offsets"][b]:ref["row_offsets"][b + 1]]
        near = float(np.abs(face_margin(r, CUBS[c])).min())
        assert near <= FACE_TIE, (m, B, int(c), int(b), got[1][c, b], want[1][c, b], got[2][c, b], want[2][c, b], near)
        ties += 1
    assert ties == 0
    hit_missions = tuple(int(v) for v in (want[1] > 0).sum(axis=1))
    assert all(0 < v < B for v in hit_missions)                                      # every cuboid: hit by some, missed by others
    if (m, B) in EXPECT_HIT_MISSIONS:
        assert hit_missions == EXPECT_HIT_MISSIONS[(m, B)]
    # the judge gives every mission the same verdict from the device audit and from the oracle's rows
    from types import SimpleNamespace
    t = lambda v: torch.as_tensor(v)                                                 # noqa: E731
    o = SimpleNamespace(speed_xy=t(want[0][1]), ascent=t(want[0][2]), descent=t(want[0][3]), accel_xy=t(want[0][4]), hit_rows=t(want[1]))
    dev, host = plan_feasibility(a), plan_feasibility(o)
    for key in host:
        assert dev[key].is_cuda and dev[key].cpu().tolist() == host[key].tolist(), key
    if m == 8:
        d = host["descent_ok"]
        assert bool(d.any()) and not bool(d.all())
        assert not bool(host["speed_ok"].any())                                      # the planner knows nothing of max_speed_xy


# ------------------------------------------------------------------------------------------------------------------ 3: ragged
def test_ragged_audit_equals_each_mission_alone_and_its_rows(eng):
    from oracle import minsnap_oracle as mo
    full = mo.synthetic_missions(61, 9)
    missions = [full[b, :2 + (5 * b) % 9] for b in range(61)]                       # 1 .. 9 segments, every count several times
    assert sorted({len(w) - 1 for w in missions}) == list(range(1, 10))
    free = eng.plan_ragged(missions, VEL, DT, rows=False)
    assert free.traj is None
    got = audit_of_plan(eng, free, CUBS)
    with_rows = eng.plan_ragged(missions, VEL, DT)
    assert same(got, audit_from_rows(with_rows.traj.cpu().numpy(), with_rows.row_offsets.cpu().numpy(), CUBS))
    assert same(got, audit_of_plan(eng, with_rows, CUBS))
    for b, w in enumerate(missions):
        alone = audit_of_plan(eng, eng.plan(w[None], VEL, DT, rows=False), CUBS)
        assert same(alone, tuple(x[:, b:b + 1] for x in got)), b
    a = eng.audit(free, CUBS)
    assert same((a.block.cpu().numpy(), a.hit_rows.cpu().numpy(), a.first_hit.cpu().numpy()), got)


@pytest.mark.parametrize("device_loop", [True, False])
def test_collision_free_lab_course_audited_against_all_four_cuboids(eng, device_loop):
    g = load_golden("fixed_missions.npz")
    wp, aabbs = np.asarray(g["lab_wp"], dtype=np.float64), np.asarray(g["lab_aabbs"], dtype=np.float64)
    assert aabbs.shape == (4, 6)
    rp = eng.plan_collision_free([wp, wp[:4], wp[1:]], aabbs, VEL, DT, strict=False, device_loop=device_loop)
    a = eng.audit(rp, aabbs)
    want = audit_from_rows(rp.traj.cpu().numpy(), rp.row_offsets.cpu().numpy(), aabbs)
    print(f"lab course (device_loop={device_loop}): samples inside each cuboid after the obstacle loop\n{want[1]}")
    assert same((a.block.cpu().numpy(), a.hit_rows.cpu().numpy(), a.first_hit.cpu().numpy()), want)


# ---------------------------------------------------------------------------------------------------------------- 4: the walk
def test_long_segments_short_segments_and_a_vertical_mission(eng):
    slow = [np.array([[0.0, 0.0, -1.0], [3.0, 0.0, -1.0]])]                         # one segment of ~9 000 rows at velocity 0.05
    p = eng.plan_ragged(slow, 0.05, DT, strict=False)
    assert 8900 <= p.total_rows <= 9100
    for lanes in (16, 64):
        eng.ctx.set_option("audit_lanes", lanes)
        assert same(audit_of_plan(eng, p, CUBS), audit_from_rows(p.traj.cpu().numpy(), p.row_offsets.cpu().numpy(), CUBS)), lanes
    # segments of 2 .. 5 rows (shorter than a group of lanes) between long ones; a mission that only climbs
    gaps = (0.045, 0.075, 0.105, 0.135)                                              # / 3 m/s / 0.01 s -> 2, 3, 4, 5 rows
    short = []
    for i in range(5):
        pts, x = [[0.0, 0.5 * i, -2.0]], 0.0
        for j, gap in enumerate(gaps[i % 4:] + gaps[:i % 4]):
            x += 3.0 + 0.25 * j
            pts.append([x, 0.5 * i + 0.3 * j, -2.0 - 0.1 * j])
            x += gap
            pts.append([x, 0.5 * i + 0.3 * j, -2.0 - 0.1 * j])
        short.append(np.array(pts + [[x + 3.0, 0.5 * i, -3.0]]))
    vertical = [np.array([[1.0, 1.0, 0.0], [1.0, 1.0, -5.0], [1.0, 1.0, -9.0]])]
    batch = eng.plan_ragged(short + vertical, VEL, DT, strict=False)
    counts = batch.seg_rows.cpu().numpy()
    assert {2, 3, 4, 5} <= set(counts.tolist()) and counts.max() > 100
    rows, ro = batch.traj.cpu().numpy(), batch.row_offsets.cpu().numpy()
    assert np.isfinite(rows).all()
    want = audit_from_rows(rows, ro, CUBS)
    for lanes in (16, 64):
        eng.ctx.set_option("audit_lanes", lanes)
        assert same(audit_of_plan(eng, batch, CUBS), want), lanes
    eng.ctx.set_option("audit_lanes", 16)
    speed_xy, ascent = want[0][1, -1], want[0][2, -1]
    assert speed_xy < 1e-9 and ascent > 1.0                                          # it only climbs


# ------------------------------------------------------------------------------------------------ 5: non-finite plans, bounds
def test_non_finite_missions_report_nan_and_leave_their_neighbours_alone(eng):
    k = case(eng, 8, 37)
    clean = k["want"]
    coeffs = k["free"].coeffs.clone()
    coeffs[5] = float("nan")                                     # what a singular solve writes
    coeffs[36, 8 * 3 + 0, 0] = float("inf")                      # one position coefficient of one segment of the last mission
    coeffs[20, 8 * 7 + 2, 2] = float("-inf")                     # one velocity-only contribution (t^2 and up) in a last segment
    got = audit_abi(eng, coeffs, k["free"].seg_rows, None, 37, 8, DT, CUBS)           # (sentinel-checked: nothing outside [rows][B])
    for b in (5, 36, 20):
        assert got[0][0, b] == clean[0][0, b]                    # the row total does not depend on the coefficients
        assert np.isnan(got[0][1:, b]).all() and (got[1][:, b] == 0).all() and (got[2][:, b] == -1).all(), b
    keep = np.setdiff1d(np.arange(37), (5, 36, 20))
    assert same(tuple(x[:, keep] for x in got), tuple(x[:, keep] for x in clean))
    from uav_ac.scoring import plan_feasibility
    verdict = plan_feasibility(eng.audit(_with_coeffs(k["free"], coeffs), CUBS))
    for key, v in verdict.items():
        assert not v[[5, 36, 20]].any(), key                     # a singular plan never looks feasible


def _with_coeffs(plan, coeffs):
    import copy
    other = copy.copy(plan)
    other.coeffs = coeffs
    return other


# ------------------------------------------------------------------------------------ 6: split invariance and determinism
def test_a_slice_of_the_batch_audits_like_the_whole_and_runs_repeat(eng):
    k = case(eng, 8, 37)
    free = k["free"]
    whole = audit_of_plan(eng, free, CUBS)
    assert same(whole, audit_of_plan(eng, free, CUBS))
    for b0, b1 in ((5, 30), (0, 1), (36, 37), (3, 20)):
        part = audit_abi(eng, free.coeffs[b0:b1], free.seg_rows[b0:b1], None, b1 - b0, 8, DT, CUBS)
        assert same(part, tuple(x[:, b0:b1] for x in whole)), (b0, b1)
    big = case(eng, 8, 96)
    assert same(audit_of_plan(eng, big["free"], CUBS), audit_of_plan(eng, big["free"], CUBS))
    part = audit_abi(eng, big["free"].coeffs[17:81], big["free"].seg_rows[17:81], None, 64, 8, DT, CUBS[::-1].copy())
    assert same(part, tuple(x[:, 17:81] for x in (big["want"][0], big["want"][1][::-1], big["want"][2][::-1])))


# -------------------------------------------------------------------------------------------------------------- 7: validation
def test_invalid_arguments_are_refused_before_anything_is_enqueued(eng):
    import torch
    from uav_ac import _native as nat
    k = case(eng, 8, 37)
    free, B, m = k["free"], 37, 8
    dev = dict(device=eng.device)
    audit = torch.full((8 * B,), SENT_F, dtype=torch.float64, **dev)
    hits = torch.full((3 * B,), SENT_I, dtype=torch.int32, **dev)
    first = torch.full((3 * B,), SENT_I, dtype=torch.int32, **dev)
    cub = torch.as_tensor(CUBS).to(eng.device)
    good = dict(coeffs=free.coeffs, seg_rows=free.seg_rows, seg_offsets=None, B=B, m=m, dt=DT, cuboids=cub, n=3, audit=audit,
                hit_rows=hits, first_hit=first)
    bad = [dict(n=-1), dict(n=17), dict(coeffs=None), dict(seg_rows=None), dict(audit=None), dict(cuboids=None), dict(hit_rows=None),
           dict(first_hit=None), dict(n=0), dict(n=0, cuboids=None), dict(n=0, cuboids=None, hit_rows=None),
           dict(n=0, hit_rows=None, first_hit=None), dict(B=0), dict(B=-3), dict(m=0), dict(m=nat.MAX_SEGMENTS + 1),
           dict(dt=0.0), dict(dt=-0.01), dict(dt=math.inf), dict(dt=math.nan)]
    eng._bind_stream()
    fn = nat.lib().uavac_minsnap_audit_dev
    for change in bad:
        a = {**good, **change}
        rc = fn(eng.ctx._h, _p(a["coeffs"]), _p(a["seg_rows"]), _p(a["seg_offsets"]), a["B"], a["m"], a["dt"], _p(a["cuboids"]), a["n"],
                _p(a["audit"]), _p(a["hit_rows"]), _p(a["first_hit"]))
        assert rc == nat.EINVAL, (change, rc)
        assert (nat.lib().uavac_last_error(eng.ctx._h) or b"") != b"", change
    assert fn(None, _p(free.coeffs), _p(free.seg_rows), None, B, m, DT, _p(cub), 3, _p(audit), _p(hits), _p(first)) == nat.EINVAL
    torch.cuda.synchronize()
    assert bool((audit == SENT_F).all()) and bool((hits == SENT_I).all()) and bool((first == SENT_I).all())
    with pytest.raises(nat.UavacError):
        eng.ctx.set_option("audit_lanes", 32)
    with pytest.raises(ValueError):
        eng.audit(free, np.zeros((17, 6)))
    # the same call with nothing wrong goes through, and so does n_cuboids == 0 with NULLs
    eng.ctx.call("uavac_minsnap_audit_dev", _p(free.coeffs), _p(free.seg_rows), None, B, m, DT, _p(cub), 3, _p(audit), _p(hits), _p(first))
    torch.cuda.synchronize()
    assert same((audit.cpu().numpy().reshape(8, B), hits.cpu().numpy().reshape(3, B), first.cpu().numpy().reshape(3, B)), k["want"])
    audit.fill_(SENT_F)
    eng.ctx.call("uavac_minsnap_audit_dev", _p(free.coeffs), _p(free.seg_rows), None, B, m, DT, None, 0, _p(audit), None, None)
    torch.cuda.synchronize()
    assert np.array_equal(audit.cpu().numpy().reshape(8, B), k["want"][0])
