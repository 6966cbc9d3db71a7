"""Plan demand on the GPU (`uavac_minsnap_demand_dev`, csrc/minsnap_demand.hip), through the C ABI and `Engine.demand`: per mission the
specific thrust, the banks and the roll / pitch rate a perfectly tracked plan needs, the rows that ask for thrust downward and, per
cuboid, the planned clearance with its row -- from coefficients and row counts alone.

What is compared with what:
  * against the PRODUCT'S OWN ROWS AND JERK everything is exact (no tolerance; floats by value, NaN equal to NaN): the kernel evaluates
    the sampler's fma chains, forms every product, sum and quotient separately rounded in the order include/uavac.h states, reduces the
    SQUARES with max, min, integer add and a lexicographic minimum, and takes one sqrt -- which is what `scoring.demand_from_rows` does
    in NumPy on `plan.traj` and `Engine.sample_derivatives(plan)[0]`;
  * against the ORACLE (oracle.c_oracle.plan_threads: its own solve, sampler and jerk) every f64 column holds to 1e-5 of max(1, |value|),
    SURVEY 8(c)'s bar for sampled accelerations and the bar `col_err < TOL` applies to jerk.  The bank and rate columns are ratios over
    the thrust; the bar is valid for them on the 3 m/s sets because the least thrust there is >= 5.18 m/s^2 (NumPy oracle, CPU), and is
    not applied at 6 m/s, where it falls to 0.47.  Row totals and inverted counts are exact.  `clearance_row` is not compared by index
    -- adjacent rows near a minimum differ by as little as 2.7e-10 relative in d2 --: the oracle's distance AT the kernel's row must be
    within the same bar of the oracle's minimum.
"""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT, G = 0.01, 9.81
CUBS = np.array([[6.0, 14.0, 2.0, 9.0, -4.0, -2.8], [10.0, 12.0, 5.0, 7.0, -10.0, 0.0], [3.7, 4.3, 4.0, 10.0, -3.4, -2.8]])
SLOW = ((1, 48, 3.0), (2, 48, 3.0), (8, 37, 3.0))           # (m, B, velocity); (8, 37): a partial wavefront and a partial workgroup
FAST = (8, 37, 6.0)                                         # rows that ask for thrust downward; checked exact only
SENT_F, SENT_I, PAD = -1.2345e300, -7777, 96
TOL = 1e-5
NAMES = ("demand", "idemand", "clearance", "clearance_row")


def sixteen_cuboids():
    """The three cuboids and thirteen smaller ones spread over the missions' airspace."""
    rng = np.random.default_rng(16)
    c = np.stack([rng.uniform(0.0, 16.0, 13), rng.uniform(0.0, 12.0, 13), rng.uniform(-6.0, 0.0, 13)], axis=1)
    h = rng.uniform(0.3, 1.5, (13, 3))
    more = np.stack([c[:, 0] - h[:, 0], c[:, 0] + h[:, 0], c[:, 1] - h[:, 1], c[:, 1] + h[:, 1], c[:, 2] - h[:, 2], c[:, 2] + h[:, 2]], axis=1)
    return np.concatenate([CUBS, more])


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    e = Engine("cuda:0")
    yield e
    e.ctx.set_option("audit_lanes", 16)


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def demand_abi(eng, coeffs, seg_rows, seg_offsets, B, m, dt, cubs, g=G):
    """One call of uavac_minsnap_demand_dev on device tensors -> the four arrays as NumPy, in the order of NAMES.  The outputs are the
    middle of larger sentinel-filled buffers: everything inside is written, nothing outside."""
    import torch
    n = 0 if cubs is None else len(cubs)
    sizes = (6 * B, 2 * B, n * B, n * B)
    bufs = [torch.full((PAD + size + PAD,), SENT_I if k % 2 else SENT_F, dtype=torch.int32 if k % 2 else torch.float64, device=eng.device)
            for k, size in enumerate(sizes)]
    cub = None if n == 0 else torch.as_tensor(np.ascontiguousarray(cubs, dtype=np.float64)).to(eng.device)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_demand_dev", _p(coeffs), _p(seg_rows), _p(seg_offsets), int(B), int(m), float(dt), float(g), _p(cub), n,
                 _p(bufs[0][PAD:]), _p(bufs[1][PAD:]), _p(bufs[2][PAD:]) if n else None, _p(bufs[3][PAD:]) if n else None)
    torch.cuda.synchronize()
    out = []
    for k, (buf, size) in enumerate(zip(bufs, sizes)):
        x, sent = buf.cpu().numpy(), SENT_I if k % 2 else SENT_F
        assert (x[:PAD] == sent).all() and (x[PAD + size:] == sent).all(), NAMES[k]
        assert not (x[PAD:PAD + size] == sent).any(), NAMES[k]
        out.append(x[PAD:PAD + size].reshape(-1, B).copy())
    return tuple(out)


def demand_of_plan(eng, plan, cubs):
    ragged = hasattr(plan, "seg_offsets")
    return demand_abi(eng, plan.coeffs, plan.seg_rows, plan.seg_offsets if ragged else None, plan.B, plan.max_m if ragged else plan.m,
                      plan.dt, cubs)


def spec(rows, jerk, ro, cubs):
    from uav_ac.scoring import demand_from_rows
    d = demand_from_rows(rows, jerk, ro, G, cubs)
    return tuple(d[k] for k in NAMES)


def fields(d):
    """a PlanDemand -> the four arrays"""
    f64 = np.stack([t.cpu().numpy() for t in (d.rows, d.thrust_max, d.thrust_min, d.bank_x, d.bank_y, d.body_rate)])
    return (f64, np.stack([d.inverted_rows.cpu().numpy(), d.first_inverted.cpu().numpy()]), d.clearance.cpu().numpy(),
            d.clearance_row.cpu().numpy())


def same(got, want):
    return all(g.shape == w.shape and np.array_equal(g, w, equal_nan=g.dtype.kind == "f") for g, w in zip(got, want))


def columns(arrays, idx):
    return tuple(x[:, idx] for x in arrays)


_CACHE = {}


def case(eng, m, B, vel):
    """Per mission set, computed once and left unchanged: the plan with rows, the rows-free plan, the rows and the jerk on the host and
    what NumPy makes of them."""
    if (m, B, vel) not in _CACHE:
        from oracle import minsnap_oracle as mo
        wps = mo.synthetic_missions(B, m)
        plan = eng.plan(wps, vel, DT)
        free = eng.plan(wps, vel, DT, rows=False)
        jerk = eng.sample_derivatives(plan)[0].cpu().numpy()
        rows, ro = plan.traj.cpu().numpy(), plan.row_offsets.cpu().numpy()
        _CACHE[(m, B, vel)] = dict(wps=wps, plan=plan, free=free, rows=rows, jerk=jerk, ro=ro, want=spec(rows, jerk, ro, CUBS))
    return _CACHE[(m, B, vel)]


# ------------------------------------------------------------------------------------------------ 1: the product's own rows
@pytest.mark.parametrize("m, B, vel", SLOW + (FAST,))
def test_demand_equals_what_numpy_makes_of_the_products_rows_and_jerk(eng, m, B, vel):
    k = case(eng, m, B, vel)
    want = k["want"]
    assert k["free"].traj is None and np.isfinite(want[0]).all()
    for lanes in (16, 64):                                        # lanes per mission: a tuning knob, same results
        eng.ctx.set_option("audit_lanes", lanes)
        got = demand_of_plan(eng, k["free"], CUBS)
        assert same(got, want), (m, B, vel, lanes, [np.flatnonzero((g != w).any(axis=0)) for g, w in zip(got, want)])
    eng.ctx.set_option("audit_lanes", 16)
    hits, inverted = int((want[2] == 0.0).sum()), int(want[1][0].sum())
    print(f"demand m={m} B={B} v={vel}: {hits} mission-cuboid clearances are 0, peak bank {want[0][3:5].max():.3f}, least thrust "
          f"{want[0][2].min():.3f} m/s^2, {inverted} inverted rows")
    assert hits > 0 and (want[2] > 0.0).any()                     # both kinds of clearance
    assert (inverted > 0) == (vel == FAST[2])
    # the public interface gives the same tensors, for both kinds of plan, and never needs the rows
    for plan in (k["free"], k["plan"]):
        d = eng.demand(plan, CUBS)
        assert same(fields(d), want) and np.array_equal(d.block.cpu().numpy(), want[0])


# ------------------------------------------------------------------------------------------------ 2: independence of form
def test_rows_free_split_no_cuboids_and_sixteen_cuboids(eng):
    k = case(eng, 8, 37, 3.0)
    free, want = k["free"], k["want"]
    assert same(demand_of_plan(eng, k["plan"], CUBS), demand_of_plan(eng, free, CUBS))       # the plan with rows: its rows are not read
    for b0, b1 in ((0, 17), (17, 37)):
        part = demand_abi(eng, free.coeffs[b0:b1], free.seg_rows[b0:b1], None, b1 - b0, 8, DT, CUBS)
        assert same(part, columns(want, slice(b0, b1))), (b0, b1)
    for lanes in (16, 64):
        eng.ctx.set_option("audit_lanes", lanes)
        none = demand_of_plan(eng, free, None)                    # n_cuboids == 0 with NULLs: the other kernel variant
        assert same(none[:2], want[:2]) and none[2].shape == none[3].shape == (0, 37)
        many = sixteen_cuboids()
        assert same(demand_of_plan(eng, free, many), spec(k["rows"], k["jerk"], k["ro"], many)), lanes
    eng.ctx.set_option("audit_lanes", 16)
    d = eng.demand(free)
    assert tuple(d.clearance.shape) == tuple(d.clearance_row.shape) == (0, 37) and same(fields(d)[:2], want[:2])
    with pytest.raises(ValueError):
        eng.demand(free, np.zeros((17, 6)))
    # g comes from the vehicle
    from uav_ac import _native as nat
    moon = nat.Vehicle.default()
    moon.g = 1.62
    from uav_ac.scoring import demand_from_rows
    low = demand_from_rows(k["rows"], k["jerk"], k["ro"], 1.62, CUBS)
    assert same(fields(eng.demand(free, CUBS, vehicle=moon)), tuple(low[n] for n in NAMES))
    assert not np.array_equal(low["demand"], want[0])


# ------------------------------------------------------------------------------------------------ 3: ragged batches
def test_concat_take_and_delay_demand_what_their_gathered_rows_show(eng):
    from uav_ac.scoring import delay_rows, take_rows
    a, b = case(eng, 2, 48, 3.0), case(eng, 8, 37, 3.0)
    both = eng.concat([a["free"], b["free"]])
    ro = np.concatenate([a["ro"], a["ro"][-1] + b["ro"][1:]])
    want = spec(np.concatenate([a["rows"], b["rows"]]), np.concatenate([a["jerk"], b["jerk"]]), ro, CUBS)
    assert same(want, tuple(np.concatenate([x, y], axis=1) for x, y in zip(a["want"], b["want"])))
    for lanes in (16, 64):
        eng.ctx.set_option("audit_lanes", lanes)
        assert same(demand_of_plan(eng, both, CUBS), want), lanes
    eng.ctx.set_option("audit_lanes", 16)
    assert same(fields(eng.demand(both, CUBS)), want)
    # a permutation with duplicates
    index = np.array([36, 0, 5, 5, 20, 1, 36, 11, 3, 30, 29, 5], dtype=np.int32)
    taken = eng.take(b["free"], index)
    rows, tro = take_rows(b["rows"], b["ro"], index)
    jerk, _ = take_rows(b["jerk"], b["ro"], index)
    want = spec(rows, jerk, tro, CUBS)
    assert same(want, columns(b["want"], index))
    assert same(demand_of_plan(eng, taken, CUBS), want)
    # start delays: HOLD rows ask for thrust g, no bank and no rate
    start = (np.arange(37) * 7) % 23
    start[[0, 9]] = 0
    assert (start > 0).sum() > 20
    delayed = eng.delay(b["free"], start.astype(np.int32))
    rows, dro = delay_rows(b["rows"], b["ro"], start, eng.first_yaw(b["free"]))
    jerk = np.concatenate([np.concatenate([np.zeros((start[i], 3)), b["jerk"][b["ro"][i]:b["ro"][i + 1]]]) for i in range(37)])
    want = spec(rows, jerk, dro, CUBS)
    for lanes in (16, 64):
        eng.ctx.set_option("audit_lanes", lanes)
        assert same(demand_of_plan(eng, delayed, CUBS), want), lanes
    eng.ctx.set_option("audit_lanes", 16)
    assert np.array_equal(want[0][0], b["want"][0][0] + start)
    held = start > 0
    assert (want[0][2, held] <= G).all() and (want[0][1, held] >= G).all()
    assert np.array_equal(want[0][3:, ~held], b["want"][0][3:, ~held])
    # a hold row stands where row 0 stands: the clearance keeps every bit, and its row counts the hold rows unless it was row 0
    assert np.array_equal(want[2], b["want"][2])
    assert np.array_equal(want[3], np.where(b["want"][3] == 0, 0, b["want"][3] + start))


# ------------------------------------------------------------------------------------------------ 4: consistent with the audit
@pytest.mark.parametrize("m, B, vel", SLOW + (FAST,))
def test_demand_and_audit_agree_on_rows_and_hits(eng, m, B, vel):
    k = case(eng, m, B, vel)
    a, d = eng.audit(k["free"], CUBS), eng.demand(k["free"], CUBS)
    assert np.array_equal(a.rows.cpu().numpy(), d.rows.cpu().numpy())
    hit_rows, first_hit = a.hit_rows.cpu().numpy(), a.first_hit.cpu().numpy()
    clearance, row = d.clearance.cpu().numpy(), d.clearance_row.cpu().numpy()
    assert np.array_equal(clearance == 0.0, hit_rows > 0) and (hit_rows > 0).any()
    assert np.array_equal(row[hit_rows > 0], first_hit[hit_rows > 0])


# ------------------------------------------------------------------------------------------------ 5: a poisoned mission
def test_a_poisoned_mission_is_excluded_and_its_neighbours_keep_every_bit(eng):
    from uav_ac.scoring import demand_feasibility
    k = case(eng, 8, 37, 3.0)
    clean = k["want"]
    coeffs = k["free"].coeffs.clone()
    coeffs[13, 8 * 4 + 3, 1] = float("nan")                     # one coefficient of one segment of one mission
    for lanes in (16, 64):
        eng.ctx.set_option("audit_lanes", lanes)
        got = demand_abi(eng, coeffs, k["free"].seg_rows, None, 37, 8, DT, CUBS)
        assert got[0][0, 13] == clean[0][0, 13]                  # the row total does not depend on the coefficients
        assert np.isnan(got[0][1:, 13]).all() and got[1][:, 13].tolist() == [0, -1]
        assert np.isnan(got[2][:, 13]).all() and (got[3][:, 13] == -1).all()
        keep = np.setdiff1d(np.arange(37), [13])
        assert same(columns(got, keep), columns(clean, keep)), lanes
    eng.ctx.set_option("audit_lanes", 16)
    verdict = demand_feasibility(dict(zip(NAMES, got)))
    for key, v in verdict.items():
        assert not v[13], key                                     # a singular plan never looks feasible


# ------------------------------------------------------------------------------------------------ 6: the oracle
def _gap(p, cub):
    e = [np.where(p[:, a] < cub[2 * a], cub[2 * a] - p[:, a], np.where(p[:, a] > cub[2 * a + 1], p[:, a] - cub[2 * a + 1], 0.0)) for a in range(3)]
    return np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])


@pytest.mark.parametrize("m, B, vel", SLOW)
def test_demand_against_the_oracle(eng, m, B, vel):
    from oracle import c_oracle as cc
    k = case(eng, m, B, vel)
    ref = cc.plan_threads(k["wps"], vel, DT, derivs=True)
    want = spec(ref["rows"], ref["jerk"], ref["row_offsets"], CUBS)
    got = fields(eng.demand(k["free"], CUBS))
    assert np.array_equal(got[0][0], want[0][0]) and np.array_equal(got[1][0], want[1][0])       # row totals, inverted counts: exact
    assert want[0][2].min() >= 5.18                              # the least thrust: what makes the bar valid for the ratios
    err = np.abs(got[0][1:] - want[0][1:]) / np.maximum(1.0, np.abs(want[0][1:]))
    cerr = np.abs(got[2] - want[2]) / np.maximum(1.0, np.abs(want[2]))
    print(f"demand vs oracle m={m} B={B}: worst error per column {err.max(axis=1)}, clearance {cerr.max()}")
    assert (err <= TOL).all(), err.max(axis=1)
    assert (cerr <= TOL).all(), cerr.max(axis=1)
    # the oracle's distance at the kernel's row is the oracle's minimum, to the same bar
    ro, worst = ref["row_offsets"], 0.0
    for c in range(len(CUBS)):
        for b in range(B):
            p = ref["rows"][ro[b]:ro[b + 1], 0:3]
            assert 0 <= got[3][c, b] < len(p)
            at = float(_gap(p[got[3][c, b]][None], CUBS[c])[0])
            worst = max(worst, abs(at - want[2][c, b]) / max(1.0, want[2][c, b]))
    print(f"  oracle distance at the kernel's row vs the oracle's minimum: worst {worst}")
    assert worst <= TOL


# ------------------------------------------------------------------------------------------------ 7: refusals
def test_invalid_arguments_are_refused_before_anything_is_enqueued(eng):
    import torch
    from uav_ac import _native as nat
    k = case(eng, 8, 37, 3.0)
    free, B, m = k["free"], 37, 8
    dev = dict(device=eng.device)
    demand = torch.full((6 * B,), SENT_F, dtype=torch.float64, **dev)
    idemand = torch.full((2 * B,), SENT_I, dtype=torch.int32, **dev)
    clearance = torch.full((3 * B,), SENT_F, dtype=torch.float64, **dev)
    crow = torch.full((3 * B,), SENT_I, dtype=torch.int32, **dev)
    cub = torch.as_tensor(CUBS).to(eng.device)
    order = ("coeffs", "seg_rows", "seg_offsets", "B", "m", "dt", "g", "cuboids", "n", "demand", "idemand", "clearance", "clearance_row")
    good = dict(coeffs=free.coeffs, seg_rows=free.seg_rows, seg_offsets=None, B=B, m=m, dt=DT, g=G, cuboids=cub, n=3, demand=demand,
                idemand=idemand, clearance=clearance, clearance_row=crow)
    bad = [dict(n=-1), dict(n=17), dict(coeffs=None), dict(seg_rows=None), dict(demand=None), dict(idemand=None), dict(cuboids=None),
           dict(clearance=None), dict(clearance_row=None), dict(n=0), dict(n=0, cuboids=None), dict(n=0, cuboids=None, clearance=None),
           dict(n=0, clearance=None, clearance_row=None), dict(B=0), dict(B=-3), dict(m=0), dict(m=nat.MAX_SEGMENTS + 1),
           dict(dt=0.0), dict(dt=-0.01), dict(dt=math.inf), dict(dt=math.nan),
           dict(g=0.0), dict(g=-9.81), dict(g=math.inf), dict(g=math.nan)]
    eng._bind_stream()
    fn = nat.lib().uavac_minsnap_demand_dev

    def call(ctx, a):
        return fn(ctx, *[_p(a[x]) if x not in ("B", "m", "dt", "g", "n") else a[x] for x in order])
    for change in bad:
        rc = call(eng.ctx._h, {**good, **change})
        assert rc == nat.EINVAL, (change, rc)
        assert (nat.lib().uavac_last_error(eng.ctx._h) or b"") != b"", change
    assert call(None, good) == nat.EINVAL
    torch.cuda.synchronize()
    assert bool((demand == SENT_F).all()) and bool((idemand == SENT_I).all())
    assert bool((clearance == SENT_F).all()) and bool((crow == SENT_I).all())
    # the same call with nothing wrong goes through
    assert call(eng.ctx._h, good) == nat.OK
    torch.cuda.synchronize()
    got = (demand.cpu().numpy().reshape(6, B), idemand.cpu().numpy().reshape(2, B), clearance.cpu().numpy().reshape(3, B),
           crow.cpu().numpy().reshape(3, B))
    assert same(got, k["want"])
