"""Retiming to the tilt and thrust limits on the GPU (`uavac_minsnap_need_dev`, `uavac_minsnap_retime_demand_factors_dev`,
`uavac_minsnap_retime_demand_dev`; csrc/minsnap_need.hip, csrc/minsnap_retime.hip), through the C ABI, `Engine.need` and
`Engine.retime(..., demand=True)`.

What is compared with what -- everything is exact (no tolerance; floats by value, NaN equal to NaN; untouched speeds by their bits):
  * the need kernel against `scoring.need_from_rows` on the PRODUCT'S OWN ROWS: the kernel evaluates the sampler's fma chains, forms every
    product, sum, difference, fmax and sqrt separately rounded in the order include/uavac.h states, reduces the numerators with fmax and
    divides once per mission -- which is what the NumPy specification does on the sampled rows;
  * the factors kernel against `scoring.retime_factors(..., need=...)` on a crafted pair of blocks;
  * the loop against its own replay: `Engine.plan` + `Engine.audit` + `Engine.need` + the NumPy rule, pass by pass.
The vehicles: "fast" is the default vehicle with the four flight limits at 10 / 10 / 10 / 12, so that they are not the bottleneck;
"weak" is the same with max_thrust = 1.6 N per rotor (tests/test_need_host.py has the CPU counts).
"""
import ctypes as C
import math

import numpy as np
import pytest

from test_need_host import MARGIN, crafted, vehicle

pytestmark = pytest.mark.gpu

DT = 0.01
SENT_F, SENT_I, PAD = -1.2345e300, -7777, 96
LIMITS = (3.0, 3.0, 2.0, 12.0)          # max_speed_xy, max_ascent, max_descent, max_horiz_accel of uavac_vehicle_default
UNIFORM = ((8, 37, 3.0), (8, 37, 6.0), (1, 48, 3.0))        # (m, B, velocity); B = 37: two full 16-mission workgroups plus a partial one


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    e = Engine("cuda:0")
    e.take_flags()
    yield e
    e.ctx.set_option("audit_lanes", 16)


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def host(t):
    return t.cpu().numpy()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def limits_of(V):
    from uav_ac.scoring import demand_limits
    return (C.c_double * 4)(*demand_limits(V))


def need_abi(eng, coeffs, seg_rows, seg_offsets, B, m, V=None):
    """One call of uavac_minsnap_need_dev on device tensors -> need (4, B) as NumPy.  The output is the middle of a larger sentinel-filled
    buffer: everything inside is written, nothing outside."""
    import torch
    buf = torch.full((PAD + 4 * B + PAD,), SENT_F, dtype=torch.float64, device=eng.device)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_need_dev", _p(coeffs), _p(seg_rows), _p(seg_offsets), int(B), int(m), DT, limits_of(V), _p(buf[PAD:]))
    torch.cuda.synchronize()
    x = host(buf)
    assert (x[:PAD] == SENT_F).all() and (x[PAD + 4 * B:] == SENT_F).all()
    assert not (x[PAD:PAD + 4 * B] == SENT_F).any()
    return x[PAD:PAD + 4 * B].reshape(4, B).copy()


def need_of_batch(eng, plan, b0, b1, V=None):
    """Missions b0 .. b1 of a Plan or a RaggedBatch, in a call of their own."""
    import torch
    if hasattr(plan, "seg_offsets"):
        so = plan.seg_offsets_host
        part = torch.as_tensor(so[b0:b1 + 1] - so[b0]).to(eng.device)
        return need_abi(eng, plan.coeffs[int(so[b0]):], plan.seg_rows[int(so[b0]):], part, b1 - b0, plan.max_m, V)
    return need_abi(eng, plan.coeffs[b0:b1], plan.seg_rows[b0:b1], None, b1 - b0, plan.m, V)


def both_lane_counts_whole_and_split(eng, plan, want, split, V=None):
    B = int(plan.B)
    for lanes in (16, 64):                                        # lanes per mission: a tuning knob, same results
        eng.ctx.set_option("audit_lanes", lanes)
        assert same(need_of_batch(eng, plan, 0, B, V), want), lanes
        got = np.concatenate([need_of_batch(eng, plan, 0, split, V), need_of_batch(eng, plan, split, B, V)], axis=1)
        assert same(got, want), (lanes, split)
    eng.ctx.set_option("audit_lanes", 16)


_CACHE = {}


def case(eng, m, B, vel):
    """Per mission set, computed once and left unchanged: the waypoints, the rows-free plan, its rows on the host (sampled afterwards
    into a plan of their own) and what NumPy makes of them for the fast vehicle."""
    if (m, B, vel) not in _CACHE:
        from oracle import minsnap_oracle as mo
        from uav_ac.scoring import need_from_rows
        wps = mo.synthetic_missions(B, m)
        free = eng.plan(wps, vel, DT, rows=False)
        sampled = eng.sample_rows(eng.plan(wps, vel, DT, rows=False))
        rows, ro = host(sampled.traj), host(sampled.row_offsets)
        _CACHE[(m, B, vel)] = dict(wps=wps, free=free, sampled=sampled, rows=rows, ro=ro, want=need_from_rows(rows, ro, vehicle(fast=True)))
    return _CACHE[(m, B, vel)]


# ------------------------------------------------------------------------------------------------ 1: the need kernel, the product's own rows
@pytest.mark.parametrize("m, B, vel", UNIFORM)
def test_need_equals_what_numpy_makes_of_the_products_rows(eng, m, B, vel):
    from uav_ac.scoring import need_from_rows
    k = case(eng, m, B, vel)
    fast, want = vehicle(fast=True), k["want"]
    assert k["free"].traj is None and np.isfinite(want).all() and (want.max(axis=0) > 1.0).any()
    both_lane_counts_whole_and_split(eng, k["free"], want, 17, fast)
    # the public interface: both kinds of plan, never the rows; and the vehicle decides
    for plan in (k["free"], k["sampled"]):
        n = eng.need(plan, fast)
        assert same(host(n.block), want) and same(np.stack([host(t) for t in (n.tilt, n.upright, n.thrust_max, n.thrust_min)]), want)
    weak = vehicle(fast=True, max_thrust=1.6)
    low = need_from_rows(k["rows"], k["ro"], weak)
    assert same(host(eng.need(k["free"], weak).block), low) and not same(low[2], want[2]) and same(low[[0, 1, 3]], want[[0, 1, 3]])
    assert same(host(eng.need(k["free"]).block), want)            # the flight limits play no part: the default vehicle asks the same
    print(f"need m={m} B={B} v={vel}: {int((want.max(axis=0) > 1.0).sum())} missions above 1, largest per limit {want.max(axis=1)}")


def test_a_ragged_batch_with_a_singular_mission(eng):
    from oracle import minsnap_oracle as mo
    from uav_ac.scoring import need_from_rows
    B = 40
    full = mo.synthetic_missions(B, 5)
    missions = [full[b, :2 + (3 * b) % 5].copy() for b in range(B)]                  # 1 .. 5 segments
    assert sorted({len(w) - 1 for w in missions}) == [1, 2, 3, 4, 5] and len(missions[21]) == 5
    missions[21][2] = missions[21][1]                                               # a repeated waypoint: a singular knot system
    batch = eng.plan_ragged(missions, 3.0, DT, rows=False, strict=False)
    sampled = eng.sample_rows(eng.plan_ragged(missions, 3.0, DT, rows=False, strict=False))
    flags = eng.take_flags()
    assert flags[1] == 1, flags
    rows, ro = host(sampled.traj), host(sampled.row_offsets)
    fast = vehicle(fast=True)
    want = need_from_rows(rows, ro, fast)
    others = np.setdiff1d(np.arange(B), [21])
    assert np.isnan(want[:, 21]).all() and np.isfinite(want[:, others]).all() and (want.max(axis=0)[others] > 1.0).any()
    both_lane_counts_whole_and_split(eng, batch, want, 21, fast)
    both_lane_counts_whole_and_split(eng, batch, want, 22, fast)
    assert same(host(eng.need(batch, fast).block), want)


# ------------------------------------------------------------------------------------------------ 2: the factors kernel
def crafted_pair(B):
    """The crafted blocks of tests/test_need_host.py with five more columns -- the two terms that do not bind there, r one ulp above 1
    through a need and through a peak, and a need exactly at 1 beside peaks below --, tiled to B columns."""
    audit, need, _, _ = crafted()
    up = math.nextafter(1.0, math.inf)
    more_a = np.array([(2.0, 3.3, 1.0, 5.0), (2.0, 1.0, 1.0, 27.0), (2.0, 1.0, 1.0, 5.0), (2.0, 1.0, 2.0 * up, 5.0), (2.0, 1.0, 1.0, 5.0)]).T
    more_n = np.array([(0.5, 0.2, 0.6, 0.0), (0.5, 0.2, 0.6, 0.0), (0.5, 0.2, up, 0.0), (0.5, 0.2, 0.6, 0.0), (0.5, 0.2, 0.6, 1.0)]).T
    extra = np.full((8, 5), 0.25)
    extra[1:5] = more_a
    audit, need = np.concatenate([audit, extra], axis=1), np.concatenate([need, more_n], axis=1)
    idx = np.arange(B) % audit.shape[1]
    audit, need = audit[:, idx].copy(), need[:, idx].copy()
    audit[0] = 100.0 + np.arange(B)                                                  # row totals: not read
    velocities = 0.5 + 0.013 * np.arange(B) + (np.arange(B) % 7) / 3.0               # no two alike
    return audit, need, velocities


def test_factors_kernel_equals_the_numpy_rule_bit_for_bit(eng):
    import torch
    from uav_ac import _native as nat
    from uav_ac.scoring import retime_factors
    B = 130                                                                          # two wavefronts plus a partial one
    audit, need, vel = crafted_pair(B)
    spec = retime_factors(audit, None, MARGIN, vel, need=need)
    assert set(spec["binding"].tolist()) == {-1, 0, 1, 2, 3, 4, 5, 6, 7}             # every term binds somewhere
    up = math.nextafter(1.0, math.inf)
    assert spec["factors"][14] == up / (1.0 - MARGIN) and spec["binding"][14] == 6 and spec["factors"][15] == up / (1.0 - MARGIN)
    assert spec["factors"][16] == 1.0 and spec["binding"][16] == 7 and spec["factors"][9] == 1.0 and spec["n_nan"] > 0
    dev = dict(device=eng.device)
    d_audit, d_need = torch.as_tensor(audit).to(eng.device), torch.as_tensor(need).to(eng.device)
    limits, dlimits = (C.c_double * 4)(*LIMITS), limits_of(None)
    d_vel = torch.full((PAD + B + PAD,), SENT_F, dtype=torch.float64, **dev)
    d_vel[PAD:PAD + B] = torch.as_tensor(vel)
    d_fac = torch.full((PAD + B + PAD,), SENT_F, dtype=torch.float64, **dev)
    d_bind = torch.full((PAD + B + PAD,), SENT_I, dtype=torch.int32, **dev)
    d_cnt = torch.tensor([0, 0, -7, -7], dtype=torch.int32, **dev)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_retime_demand_factors_dev", _p(d_audit), _p(d_need), B, limits, dlimits, MARGIN, _p(d_vel[PAD:]),
                 _p(d_fac[PAD:]), _p(d_bind[PAD:]), _p(d_cnt))
    torch.cuda.synchronize()
    v, f, bind = host(d_vel), host(d_fac), host(d_bind)
    for x, sent in ((v, SENT_F), (f, SENT_F), (bind, SENT_I)):                       # nothing outside [B]
        assert (x[:PAD] == sent).all() and (x[PAD + B:] == sent).all()
    v, f, bind = v[PAD:PAD + B], f[PAD:PAD + B], bind[PAD:PAD + B]
    assert same_bits(f, spec["factors"]) and same_bits(v, spec["velocities"]) and np.array_equal(bind, spec["binding"])
    assert same_bits(v[~spec["retimed"]], vel[~spec["retimed"]])                      # untouched ones: bit for bit
    assert host(d_cnt).tolist() == [spec["n_retimed"], spec["n_nan"], -7, -7]
    # each argument error: UAVAC_EINVAL, nothing enqueued, nothing written
    o_vel = torch.full((B,), SENT_F, dtype=torch.float64, **dev)
    o_fac = torch.full((B,), SENT_F, dtype=torch.float64, **dev)
    o_bind = torch.full((B,), SENT_I, dtype=torch.int32, **dev)
    o_cnt = torch.full((2,), -7, dtype=torch.int32, **dev)
    DL = tuple(dlimits)
    good = dict(audit=d_audit, need=d_need, B=B, limits=LIMITS, dlimits=DL, margin=MARGIN, vel=o_vel, fac=o_fac, bind=o_bind, cnt=o_cnt)
    bad = [dict(B=0), dict(margin=1.0), dict(margin=-0.001), dict(margin=math.nan), dict(audit=None), dict(need=None), dict(vel=None),
           dict(fac=None), dict(bind=None), dict(cnt=None), dict(limits=None), dict(dlimits=None), dict(limits=(3.0, 0.0, 2.0, 12.0))]
    bad += [dict(dlimits=x) for x in bad_demand_limits(DL)]
    fn = nat.lib().uavac_minsnap_retime_demand_factors_dev
    for change in bad:
        a = {**good, **change}
        lim = None if a["limits"] is None else (C.c_double * 4)(*a["limits"])
        dl = None if a["dlimits"] is None else (C.c_double * 4)(*a["dlimits"])
        rc = fn(eng.ctx._h, _p(a["audit"]), _p(a["need"]), a["B"], lim, dl, a["margin"], _p(a["vel"]), _p(a["fac"]), _p(a["bind"]), _p(a["cnt"]))
        assert rc == nat.EINVAL, (change, rc)
    torch.cuda.synchronize()
    assert bool((o_vel == SENT_F).all()) and bool((o_fac == SENT_F).all()) and bool((o_bind == SENT_I).all()) and bool((o_cnt == -7).all())


def bad_demand_limits(DL):
    """g, max_tilt, Fmax, Fmin that the three calls refuse: g or max_tilt not positive and finite, a vehicle that cannot hover, a least
    thrust below 0 or at g."""
    g, tau, hi, lo = DL
    out = [(x, tau, hi, lo) for x in (0.0, -g, math.inf, math.nan)] + [(g, x, hi, lo) for x in (0.0, -tau, math.inf, math.nan)]
    out += [(g, tau, x, lo) for x in (g, 0.5 * g, math.inf, math.nan)] + [(g, tau, hi, x) for x in (-0.1, g, 2.0 * g, math.nan)]
    return out


# ------------------------------------------------------------------------------------------------ 3: the loop
def replay(eng, wps, v0, V, margin, passes):
    """The loop with `Engine.plan` + `Engine.audit` + `Engine.need` + the NumPy rule: (velocities, product of the factors, the last
    pass's verdict, audit and need)."""
    from uav_ac.scoring import retime_factors
    v, total = np.array(v0, dtype=np.float64), np.ones(len(v0))
    for n in range(passes + 1):
        plan = eng.plan(wps, v, DT, rows=False, strict=False)
        a, need = eng.audit(plan), eng.need(plan, V)
        out = retime_factors(a, V, margin, v, need=need)
        total = np.where(out["nan"], np.nan, total)
        if out["n_retimed"] == 0 or n == passes:
            return v, total, out, a, need
        v, total = out["velocities"], np.where(out["retimed"], total * out["factors"], total)


def test_the_demand_loop_brings_the_fast_vehicles_missions_inside_tilt_and_thrust(eng):
    from uav_ac.scoring import demand_feasibility, plan_feasibility
    k = case(eng, 8, 37, 3.0)
    fast, wps, start = vehicle(fast=True), k["wps"], k["free"]
    four = eng.retime(start, fast, margin=MARGIN, max_passes=4)
    left = ~demand_feasibility(eng.demand(four.plan, vehicle=fast), fast)["tilt_ok"]
    print(f"the four-limit loop: {four.passes} passes, {int((host(four.factors) > 1.0).sum())} missions slowed, {int(left.sum())} of 37 "
          f"still demand more than max_tilt")
    assert left.any() and four.need is None and four.binding is None             # (the CPU check gives 23)
    res = eng.retime(start, fast, margin=MARGIN, max_passes=4, demand=True)
    assert 1 <= res.passes <= 2 and bool(res.converged.all())
    f = demand_feasibility(eng.demand(res.plan, vehicle=fast), fast, slack=0.0)
    assert f["thrust_ok"].all() and f["tilt_ok"].all() and f["upright"].all()
    assert bool(plan_feasibility(res.audit, fast, slack=0)["feasible"].all())
    fac, vel = host(res.factors), host(res.velocities)
    assert (fac[left] > 1.0).all() and (fac >= host(four.factors)).all()
    assert same_bits(vel[fac == 1.0], np.full(int((fac == 1.0).sum()), 3.0)) and (fac == 1.0).any()
    # the returned plan IS the plan at the returned speeds; audit and need are its audit and need
    again = eng.plan(wps, res.velocities, DT, rows=False)
    for name in ("times", "seg_rows", "coeffs", "first_yaw", "row_offsets"):
        assert np.array_equal(host(getattr(res.plan, name)), host(getattr(again, name))), name
    assert res.plan.traj is None and res.plan.velocities is res.velocities and res.plan.total_rows == again.total_rows
    assert same(host(res.audit.block), host(eng.audit(again).block))
    assert same(host(res.need.block), host(eng.need(again, fast).block)) and same(host(res.need.tilt), host(res.need.block)[0])
    worst = host(res.need.block).max(axis=0)
    print(f"the demand loop: {res.passes} passes, {int((fac > 1.0).sum())} missions slowed; afterwards at {worst[fac > 1.0].min():.4f} .. "
          f"{worst[fac > 1.0].max():.4f} of the binding limit")
    assert (worst <= 1.0).all()
    # replayed pass by pass with the NumPy rule: the same speeds, factors and binding, bit for bit
    v, total, last, _, _ = replay(eng, wps, np.full(37, 3.0), fast, MARGIN, 4)
    assert same_bits(vel, v) and same_bits(fac, total) and last["n_retimed"] == 0
    assert np.array_equal(host(res.binding), last["binding"]) and res.binding.dtype.is_floating_point is False
    assert eng.take_flags() == [0, 0, 0, 0]
    assert start.velocities is None and start.velocity == 3.0                     # the input is left as it was


def test_the_weak_vehicle_is_bound_by_thrust_and_the_laboratory_vehicle_by_its_flight_limits(eng):
    from uav_ac.scoring import BINDING_NAMES, demand_feasibility
    k = case(eng, 8, 37, 3.0)
    weak = vehicle(fast=True, max_thrust=1.6)
    judge = eng.retime(k["free"], weak, margin=MARGIN, max_passes=0, demand=True)
    names = [BINDING_NAMES[i] for i in host(judge.binding)]
    print(f"1.6 N per rotor, as planned: binding {dict((n, names.count(n)) for n in set(names))}")
    assert names.count("thrust_max") >= 1 and names.count("tilt") >= 1           # (the CPU check gives 36 and 1)
    res = eng.retime(k["free"], weak, margin=MARGIN, max_passes=4, demand=True)
    f = demand_feasibility(eng.demand(res.plan, vehicle=weak), weak)
    assert bool(res.converged.all()) and 1 <= res.passes <= 2 and f["thrust_ok"].all() and f["tilt_ok"].all() and f["upright"].all()
    assert (host(res.factors) > 1.0).all()
    # the laboratory vehicle at 3 m/s: the demand term is never the larger one, so both loops return the same bits
    lab_four = eng.retime(k["free"], margin=MARGIN, max_passes=4)
    lab = eng.retime(k["free"], margin=MARGIN, max_passes=4, demand=True)
    assert lab.passes == lab_four.passes and same_bits(host(lab.velocities), host(lab_four.velocities))
    assert same_bits(host(lab.factors), host(lab_four.factors)) and np.array_equal(host(lab.converged), host(lab_four.converged))
    assert (host(lab.binding) < 4).all() and (host(lab.binding) >= 0).all()


def test_max_passes_0_only_judges(eng):
    from uav_ac.scoring import retime_factors
    k = case(eng, 8, 37, 3.0)
    fast = vehicle(fast=True)
    res = eng.retime(k["free"], fast, margin=MARGIN, max_passes=0, demand=True)
    spec = retime_factors(eng.audit(k["free"]), fast, MARGIN, need=k["want"])
    assert res.passes == 0 and same_bits(host(res.velocities), np.full(37, 3.0)) and (host(res.factors) == 1.0).all()
    assert np.array_equal(host(res.converged), ~spec["retimed"]) and spec["retimed"].any() and not spec["retimed"].all()
    assert np.array_equal(host(res.binding), spec["binding"]) and same(host(res.need.block), k["want"])
    assert np.array_equal(host(res.plan.coeffs), host(k["free"].coeffs))


def test_plans_come_back_in_kind(eng):
    from uav_ac.fleet import RaggedBatch, RaggedPlan
    k = case(eng, 8, 37, 3.0)
    fast, wps = vehicle(fast=True), k["wps"]
    free = eng.retime(k["free"], fast, margin=MARGIN, demand=True)
    res = eng.retime(k["sampled"], fast, margin=MARGIN, demand=True)              # with rows: sampled once at the end
    again = eng.plan(wps, res.velocities, DT)
    assert same_bits(host(res.velocities), host(free.velocities))
    assert res.plan.traj is not None and res.plan.total_rows == again.total_rows and np.array_equal(host(res.plan.traj), host(again.traj))
    # ragged: every mission as if retimed alone in a uniform batch
    missions = [wps[b, :2 + b % 8] for b in range(24)]
    rag = eng.retime(eng.plan_ragged(missions, 3.0, DT, rows=False), fast, margin=MARGIN, demand=True)
    assert isinstance(rag.plan, RaggedBatch) and rag.plan.traj is None and bool(rag.converged.all()) and rag.passes <= 2
    ref = eng.plan_ragged(missions, rag.velocities, DT, rows=False)
    assert np.array_equal(host(rag.plan.coeffs), host(ref.coeffs)) and np.array_equal(host(rag.plan.row_offsets), host(ref.row_offsets))
    assert same(host(rag.need.block), host(eng.need(ref, fast).block)) and (host(rag.factors) > 1.0).any()
    for b in (1, 7, 14):                                                          # 2, 8 and 7 segments
        alone = eng.retime(eng.plan(missions[b][None], 3.0, DT, rows=False), fast, margin=MARGIN, demand=True)
        assert same_bits(host(alone.velocities), host(rag.velocities)[b:b + 1]) and same_bits(host(alone.factors), host(rag.factors)[b:b + 1])
        assert np.array_equal(host(alone.binding), host(rag.binding)[b:b + 1])
    # a RaggedPlan from the obstacle loop: retimed through its batch, returned as a RaggedPlan with rows
    rp = eng.plan_collision_free([wps[0], wps[1][:4], wps[2][1:]], None, 3.0, DT)
    out = eng.retime(rp, fast, margin=MARGIN, demand=True)
    assert isinstance(out.plan, RaggedPlan) and isinstance(out.plan.batch, RaggedBatch) and out.plan.traj is not None
    assert bool(out.converged.all()) and tuple(out.binding.shape) == (3,) and tuple(out.need.block.shape) == (4, 3)
    assert same(host(out.need.block), host(eng.need(out.plan, fast).block))
    # the refusals are the four-limit call's
    with pytest.raises(ValueError):
        eng.retime(eng.take(k["free"], np.arange(3, dtype=np.int32)), fast, demand=True)      # gathered parts: no waypoints
    assert eng.take_flags() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 4: refusals
def test_invalid_arguments_are_refused_before_anything_is_enqueued(eng):
    import torch
    from uav_ac import _native as nat
    k = case(eng, 8, 37, 3.0)
    p, B, m = k["free"], 37, 8
    dev = dict(device=eng.device)
    DL = tuple(limits_of(None))
    lib = nat.lib()
    eng._bind_stream()
    # the need call
    need = torch.full((4 * B,), SENT_F, dtype=torch.float64, **dev)
    good = dict(coeffs=p.coeffs, seg_rows=p.seg_rows, B=B, m=m, dt=DT, dlimits=DL, need=need)
    bad = [dict(coeffs=None), dict(seg_rows=None), dict(need=None), dict(dlimits=None), dict(B=0), dict(B=-3), dict(m=0),
           dict(m=nat.MAX_SEGMENTS + 1), dict(dt=0.0), dict(dt=-0.01), dict(dt=math.inf), dict(dt=math.nan)]
    bad += [dict(dlimits=x) for x in bad_demand_limits(DL)]

    def call_need(a):
        dl = None if a["dlimits"] is None else (C.c_double * 4)(*a["dlimits"])
        return lib.uavac_minsnap_need_dev(eng.ctx._h, _p(a["coeffs"]), _p(a["seg_rows"]), None, a["B"], a["m"], a["dt"], dl, _p(a["need"]))
    for change in bad:
        assert call_need({**good, **change}) == nat.EINVAL, change
        assert (lib.uavac_last_error(eng.ctx._h) or b"") != b"", change
    torch.cuda.synchronize()
    assert bool((need == SENT_F).all())
    assert call_need(good) == nat.OK
    torch.cuda.synchronize()
    assert same(host(need).reshape(4, B), host(eng.need(p).block))
    # the loop
    vel = torch.full((B,), 3.0, dtype=torch.float64, **dev)
    out = {n: torch.full_like(getattr(p, n), -7) for n in ("times", "seg_rows", "row_offsets", "coeffs")}
    audit = torch.full((8, B), SENT_F, dtype=torch.float64, **dev)
    nblock = torch.full((4, B), SENT_F, dtype=torch.float64, **dev)
    tot = torch.full((B,), SENT_F, dtype=torch.float64, **dev)
    bind = torch.full((B,), SENT_I, dtype=torch.int32, **dev)
    conv = torch.full((B,), -7, dtype=torch.int32, **dev)
    passes = C.c_int(-7)
    fast = vehicle(fast=True)
    FL = (10.0, 10.0, 10.0, 12.0)

    def call(B=B, m=m, dt=DT, limits=FL, dlimits=DL, margin=MARGIN, max_passes=4, vel=vel, audit=audit, nblock=nblock, bind=bind):
        lim = None if limits is None else (C.c_double * 4)(*limits)
        dl = None if dlimits is None else (C.c_double * 4)(*dlimits)
        return lib.uavac_minsnap_retime_demand_dev(eng.ctx._h, _p(p.waypoints), None, B, m, _p(vel), dt, lim, dl, margin, max_passes,
                                                   _p(out["times"]), _p(out["seg_rows"]), _p(out["row_offsets"]), _p(out["coeffs"]), None, None,
                                                   _p(audit), _p(nblock), _p(tot), _p(bind), _p(conv), C.byref(passes))
    changes = [dict(B=0), dict(m=0), dict(m=nat.MAX_SEGMENTS + 1), dict(dt=0.0), dict(limits=None), dict(limits=(3.0, 0.0, 2.0, 12.0)),
               dict(dlimits=None), dict(margin=1.0), dict(margin=-0.1), dict(max_passes=-1), dict(vel=None), dict(audit=None),
               dict(nblock=None), dict(bind=None)] + [dict(dlimits=x) for x in bad_demand_limits(DL)]
    for change in changes:
        assert call(**change) == nat.EINVAL, change
    torch.cuda.synchronize()
    assert bool((vel == 3.0).all()) and bool((audit == SENT_F).all()) and bool((nblock == SENT_F).all()) and bool((tot == SENT_F).all())
    assert bool((bind == SENT_I).all()) and bool((conv == -7).all()) and all(bool((t == -7).all()) for t in out.values())
    # the same call with nothing wrong (status and first_yaw are optional) is Engine.retime(demand=True)
    assert call() == nat.OK and 1 <= passes.value <= 2
    res = eng.retime(p, fast, margin=MARGIN, max_passes=4, demand=True)
    assert same_bits(host(vel), host(res.velocities)) and same_bits(host(tot), host(res.factors)) and bool((conv == 1).all())
    assert np.array_equal(host(bind), host(res.binding)) and same(host(nblock), host(res.need.block))
    assert np.array_equal(host(out["coeffs"]), host(res.plan.coeffs))
