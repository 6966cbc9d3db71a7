"""Plans from given durations, the snap cost of a plan and the optimisation of the segment durations (`uavac_minsnap_row_counts_t_dev`,
`uavac_minsnap_plan_t_dev`, `uavac_minsnap_cost_dev`, `uavac_minsnap_optimize_times_dev`, csrc/minsnap_timeopt.hip), on the GPU.

What is compared with what:
  * the cost against upstream's c^T H c on the GPU's own coefficients (<= 1e-10 relative: the two formulas agree to 5e-13 on the
    host, tests/test_timeopt_host.py, the rest is room for the device's Horner rounding);
  * a plan from the durations of a velocity plan against that plan, bit for bit; from scaled durations against the oracle with the
    project's standing bars (`conftest.col_err`: 1e-9 on coefficients against the dense solve, 1e-5 on rows);
  * the loop's own promises for every mission (cost never rises, total kept, the floor, cost_after is the cost of the returned plan);
  * the loop against its NumPy restatement on the dense KKT solve (tests/timeopt_ref.py): final cost within 1e-5 relative, every
    duration within 1e-3 min(T0) -- 15 to 30 times what replacing `solve` by `lstsq` in the reference moves them;
  * every split against the whole, bit for bit: chunks, sub-batches, ragged against uniform, a run against its repetition.
"""
import ctypes as C

import numpy as np
import pytest

import timeopt_ref as tr
from boundary_ref import dense_coeffs
from conftest import col_err
from oracle import minsnap_oracle as mo

pytestmark = pytest.mark.gpu

VEL, DT = 3.0, 0.01
SENT = -1.2345e300
B65 = 65                  # one full wavefront plus one lane


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    e = Engine("cuda:0")
    e.take_flags()
    return e


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def host(t):
    return t.cpu().numpy()


def dev(eng, a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64).to(eng.device)


def chc(coeffs, times):
    """c^T H c per mission: coeffs (B, 8m, 3), times (B, m) on the host."""
    return np.array([tr.chc_cost(c, t) for c, t in zip(coeffs, times)])


def ragged_missions(counts):
    """Missions of counts[b] segments: the leading waypoints of the bench missions of the largest count."""
    full = mo.synthetic_missions(len(counts), max(counts))
    return [full[b, :c + 1].copy() for b, c in enumerate(counts)]


MIXED = [1, 2, 3, 8] * 4 + [8, 1, 3]


# ------------------------------------------------------------------------------------------------------------- 1: the cost
@pytest.mark.parametrize("m", [1, 2, 8, 20])
def test_cost_is_the_snap_cost_of_the_plans_own_coefficients(eng, m):
    plan = eng.plan(mo.synthetic_missions(B65, m), VEL, DT, rows=False)
    got = host(eng.cost(plan))
    want = chc(host(plan.coeffs), host(plan.times))
    rel = np.abs(got - want) / want
    print(m, rel.max())
    assert rel.max() <= 1e-10
    assert eng.take_flags() == [0, 0, 0, 0]


def test_ragged_cost_equals_the_uniform_call_on_each_mission(eng):
    wps = ragged_missions(MIXED)
    batch = eng.plan_ragged(wps, VEL, DT, rows=False)
    got = host(eng.cost(batch))
    for b, wp in enumerate(wps):
        alone = eng.plan(wp[None], VEL, DT, rows=False)
        assert np.array_equal(host(alone.coeffs).reshape(-1), batch.mission_coeffs(b).reshape(-1))
        assert host(eng.cost(alone))[0] == got[b], b
    assert np.isfinite(got).all() and (got > 0).all()


def test_a_mission_with_nan_coefficients_costs_nan_and_nobody_else(eng):
    plan = eng.plan(mo.synthetic_missions(B65, 8), VEL, DT, rows=False)
    clean = host(eng.cost(plan))
    plan.coeffs[17, 5, 1] = float("nan")
    plan.coeffs[40, 62, 2] = float("inf")
    got = host(eng.cost(plan))
    assert np.isnan(got[17]) and np.isnan(got[40])
    keep = np.ones(B65, bool)
    keep[[17, 40]] = False
    assert np.array_equal(got[keep], clean[keep])


# ------------------------------------------------------------------------------------------------------------- 2: plans from durations
PLAN_FIELDS = ("seg_rows", "row_offsets", "coeffs", "first_yaw", "status")


@pytest.mark.parametrize("rows", [True, False])
def test_plan_from_a_velocity_plans_durations_is_that_plan(eng, rows):
    import torch
    wps = mo.synthetic_missions(B65, 8)
    plan_v = eng.plan(wps, velocity=VEL, dt=DT, rows=rows)
    plan_t = eng.plan(wps, times=plan_v.times, dt=DT, rows=rows)
    assert plan_t.free_times and not plan_v.free_times and np.isnan(plan_t.velocity) and plan_t.velocities is None
    assert plan_t.times is not plan_v.times and torch.equal(plan_t.times, plan_v.times)
    for f in PLAN_FIELDS:
        assert torch.equal(getattr(plan_t, f), getattr(plan_v, f)), f
    assert plan_t.total_rows == plan_v.total_rows
    if rows:
        assert torch.equal(plan_t.traj, plan_v.traj)
    else:
        assert plan_t.traj is None
    assert eng.take_flags() == [0, 0, 0, 0]


@pytest.mark.parametrize("rows", [True, False])
def test_ragged_plan_from_a_velocity_batchs_durations_is_that_batch(eng, rows):
    import torch
    wps = ragged_missions(MIXED)
    batch_v = eng.plan_ragged(wps, VEL, DT, rows=rows)
    tm = host(batch_v.times)
    so = batch_v.seg_offsets_host
    batch_t = eng.plan_ragged(wps, times=[tm[so[b]:so[b + 1]] for b in range(len(wps))], dt=DT, rows=rows)
    assert batch_t.free_times and not batch_v.free_times
    for f in PLAN_FIELDS + ("times",):
        assert torch.equal(getattr(batch_t, f), getattr(batch_v, f)), f
    if rows:
        assert torch.equal(batch_t.traj, batch_v.traj)
    assert eng.take_flags() == [0, 0, 0, 0]


def test_plan_from_scaled_durations_against_the_oracle(eng):
    m = 8
    wps = mo.synthetic_missions(B65, m)
    rng = np.random.default_rng(5)
    times = np.stack([mo.segment_times(wp, VEL) for wp in wps]) * rng.uniform(0.7, 1.4, (B65, m))
    plan = eng.plan(wps, times=times, dt=DT)
    assert np.array_equal(host(plan.times), times)
    want_rows = np.stack([mo.row_counts(t, DT) for t in times])
    assert np.array_equal(host(plan.seg_rows), want_rows)
    ro = host(plan.row_offsets)
    assert np.array_equal(ro, np.concatenate([[0], np.cumsum(want_rows.sum(axis=1))]))
    co = host(plan.coeffs)
    for b in (0, 13, 32, 63, 64):
        ref = dense_coeffs(wps[b], times[b])
        assert col_err(co[b], ref) < 1e-9, b
        pos, vel, acc, _ = mo.sample(ref, times[b], DT)[:4]
        got = plan.mission(b)
        assert got.shape[0] == want_rows[b].sum()
        assert col_err(got[:, 0:3], pos) < 1e-5 and col_err(got[:, 3:6], vel) < 1e-5 and col_err(got[:, 6:9], acc) < 1e-5


def test_a_bad_duration_raises_flag_0_and_costs_only_its_own_mission(eng):
    m = 3
    wps = mo.synthetic_missions(B65, m)
    good = eng.plan(wps, VEL, DT, rows=False)
    times = host(good.times).copy()
    times[7, 1] = -0.5
    times[30, 2] = float("inf")
    with pytest.raises(ValueError, match="positive and finite"):
        eng.plan(wps, times=times, dt=DT)
    assert eng.take_flags() == [0, 0, 0, 0]
    plan = eng.plan(wps, times=times, dt=DT, strict=False)
    flags = eng.take_flags()
    assert flags[0] == 1 and flags[2] == 0 and flags[3] == 0
    sr, want = host(plan.seg_rows), host(good.seg_rows).copy()
    want[[7, 30]] = 0
    assert np.array_equal(sr, want)
    assert np.array_equal(np.diff(host(plan.row_offsets)), want.sum(axis=1))
    keep = np.ones(B65, bool)
    keep[[7, 30]] = False
    assert np.array_equal(host(plan.coeffs)[keep], host(good.coeffs)[keep])
    assert np.array_equal(host(plan.traj), np.concatenate([good_rows for b, good_rows in
                                                           enumerate(np.split(host(eng.sample_rows(good).traj), host(good.row_offsets)[1:-1]))
                                                           if keep[b]]))


def test_a_capacity_one_row_short_refuses_the_whole_plan(eng):
    import torch
    B, m = B65, 3
    wps = mo.synthetic_missions(B, m)
    ref = eng.plan(wps, VEL, DT, dense_yaw=True)
    total = ref.total_rows
    kw = dict(device=eng.device)
    t = dict(seg_rows=torch.full((B, m), -7, dtype=torch.int32, **kw), ro=torch.full((B + 1,), -7, dtype=torch.int64, **kw),
             coeffs=torch.full((B, 8 * m, 3), SENT, dtype=torch.float64, **kw), status=torch.full((B,), -7, dtype=torch.int32, **kw),
             traj=torch.full((total, 11), SENT, dtype=torch.float64, **kw), yaw=torch.full((total,), SENT, dtype=torch.float64, **kw),
             fy=torch.full((B,), SENT, dtype=torch.float64, **kw))
    before = {n: host(v).copy() for n, v in t.items()}
    wp, times = dev(eng, wps), ref.times.clone()

    def chain(capacity):
        eng._bind_stream()
        eng.ctx.call("uavac_minsnap_plan_t_dev", _p(wp), None, B, m, _p(times), DT, _p(t["seg_rows"]), _p(t["ro"]), _p(t["coeffs"]),
                     _p(t["status"]), _p(t["traj"]), capacity, _p(t["yaw"]), _p(t["fy"]))
        return eng.take_flags()

    assert chain(total - 1) == [0, 0, 1, 0]
    for n, v in t.items():
        assert np.array_equal(host(v), before[n]), n
    assert chain(total) == [0, 0, 0, 0]
    for n, name in (("seg_rows", "seg_rows"), ("ro", "row_offsets"), ("coeffs", "coeffs"), ("traj", "traj"), ("yaw", "yaw"),
                    ("fy", "first_yaw"), ("status", "status")):
        assert np.array_equal(host(t[n]), host(getattr(ref, name))), n
    assert torch.equal(times, ref.times)                         # an input: never written


def test_times_do_not_go_with_a_speed_or_a_boundary(eng):
    wps = mo.synthetic_missions(4, 3)
    times = np.full((4, 3), 1.5)
    with pytest.raises(ValueError, match="velocity"):
        eng.plan(wps, 3.0, DT, times=times)
    with pytest.raises(ValueError, match="boundary"):
        eng.plan(wps, dt=DT, times=times, boundary=np.zeros((4, 6, 3)))
    with pytest.raises(ValueError):
        eng.plan(wps, dt=DT, times=times[:, :2])
    with pytest.raises(ValueError, match="velocity"):
        eng.plan_ragged(list(wps), 2.0, DT, times=list(times))


# ------------------------------------------------------------------------------------------------------------- 3: properties of the loop
def assert_loop_properties(eng, plan, res, ragged=False):
    import torch
    T0, T = host(plan.times).reshape(-1), host(res.plan.times).reshape(-1)
    before, after, acc = host(res.cost_before), host(res.cost_after), host(res.accepted)
    so = plan.seg_offsets_host if ragged else np.arange(plan.B + 1) * plan.m
    assert np.all(after <= before) and np.isfinite(after).all()
    assert np.array_equal(after, host(eng.cost(res.plan)))
    assert np.array_equal(before, host(eng.cost(plan)))
    assert res.plan.free_times and res.plan.waypoints is plan.waypoints
    for b in range(plan.B):
        t0, t = T0[so[b]:so[b + 1]], T[so[b]:so[b + 1]]
        assert abs(t.sum() - t0.sum()) <= 1e-12 * t0.sum(), b
        assert t.min() >= 0.2 * t0.min(), b
        if acc[b] == 0:
            assert np.array_equal(t, t0) and after[b] == before[b], b
        else:
            assert after[b] < before[b], b
    return T0, T, before, after, acc


@pytest.mark.parametrize("m,lo,hi", [(2, 2.5, 3.5), (3, 2.5, 3.5), (8, 2.5, 3.5), (8, 1.0, 6.0)])
def test_loop_keeps_its_promises_for_every_mission(eng, m, lo, hi):
    import torch
    wps = mo.synthetic_missions(B65, m, lo, hi)
    plan = eng.plan(wps, VEL, DT, rows=False)
    kept = {f: getattr(plan, f).clone() for f in ("times", "seg_rows", "row_offsets", "coeffs", "first_yaw", "waypoints")}
    res = eng.optimize_times(plan, iterations=6)
    for f, v in kept.items():
        assert torch.equal(getattr(plan, f), v), f                # the input plan is untouched
    _, _, before, after, acc = assert_loop_properties(eng, plan, res)
    r = after / before
    print(m, lo, hi, "cost ratio min / median / max", r.min(), np.median(r), r.max(), "accepted", acc.min(), acc.max())
    assert acc.max() >= 1
    fresh = eng.plan(wps, times=res.plan.times, dt=DT, rows=False)
    for f in PLAN_FIELDS:
        assert torch.equal(getattr(fresh, f), getattr(res.plan, f)), f
    assert res.plan.traj is None and eng.take_flags() == [0, 0, 0, 0]


def test_single_segments_and_zero_iterations_change_nothing(eng):
    import torch
    plan1 = eng.plan(mo.synthetic_missions(B65, 1), VEL, DT, rows=False)
    res = eng.optimize_times(plan1, iterations=3)
    assert torch.equal(res.plan.times, plan1.times) and not bool(res.accepted.any())
    assert torch.equal(res.cost_before, res.cost_after) and torch.equal(res.plan.coeffs, plan1.coeffs)
    plan8 = eng.plan(mo.synthetic_missions(B65, 8), VEL, DT)
    res = eng.optimize_times(plan8, iterations=0)
    assert torch.equal(res.plan.times, plan8.times) and not bool(res.accepted.any())
    assert torch.equal(res.cost_before, res.cost_after) and torch.equal(res.cost_before, eng.cost(plan8))
    assert torch.equal(res.plan.traj, plan8.traj)                  # rows=None: rows as the input has them
    assert eng.optimize_times(plan8, iterations=0, rows=False).plan.traj is None


# ------------------------------------------------------------------------------------------------------------- 4: against the reference
@pytest.fixture(scope="module")
def reference_runs():
    out = {}
    for m in (3, 8):
        wps = mo.synthetic_missions(12, m)                         # exactly these calls: the generator is not prefix-stable in B
        runs = []
        for wp in wps:
            T0 = mo.segment_times(wp, VEL)
            T, history, _ = tr.optimize_times(wp, T0, 6)
            runs.append((T0, T, history[0], history[-1]))
        out[m] = (wps, runs)
    return out


@pytest.mark.parametrize("m", [3, 8])
def test_loop_against_the_numpy_reference(eng, reference_runs, m):
    wps, runs = reference_runs[m]
    plan = eng.plan(wps, VEL, DT, rows=False)
    assert np.array_equal(host(plan.times), np.stack([r[0] for r in runs]))
    res = eng.optimize_times(plan, iterations=6)
    T, before, after = host(res.plan.times), host(res.cost_before), host(res.cost_after)
    for b, (T0, Tref, J0, Jref) in enumerate(runs):
        cost_err = abs(after[b] - Jref) / Jref
        time_err = np.abs(T[b] - Tref).max() / T0.min()
        ratio, ratio_ref = after[b] / before[b], Jref / J0
        print(m, b, "cost_err", cost_err, "time_err / min(T0)", time_err, "ratio", ratio, "reference", ratio_ref)
        assert cost_err <= 1e-5, (m, b)
        assert time_err <= 1e-3, (m, b)
        assert ratio <= ratio_ref * (1 + 1e-5), (m, b)


# ------------------------------------------------------------------------------------------------------------- 5: splits
def result_arrays(res):
    return [host(res.plan.times), host(res.cost_before), host(res.cost_after), host(res.accepted), host(res.plan.coeffs)]


def test_chunks_sub_batches_and_repetitions_give_the_same_bits(eng):
    wps = mo.synthetic_missions(B65, 8, 1.0, 6.0)
    plan = eng.plan(wps, VEL, DT, rows=False)
    whole = result_arrays(eng.optimize_times(plan, iterations=4))
    again = result_arrays(eng.optimize_times(plan, iterations=4))
    eng.ctx.set_option("timeopt_chunk", 7)
    try:
        chunked = result_arrays(eng.optimize_times(plan, iterations=4))
    finally:
        eng.ctx.set_option("timeopt_chunk", 0)
    for a, b, c in zip(whole, again, chunked):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    first = result_arrays(eng.optimize_times(eng.plan(wps[:10], VEL, DT, rows=False), iterations=4))
    for a, b in zip(whole, first):
        assert np.array_equal(a[:10], b)
    assert eng.take_flags() == [0, 0, 0, 0]


def test_ragged_loop_equals_the_uniform_loop_on_each_mission(eng):
    wps = ragged_missions(MIXED)
    batch = eng.plan_ragged(wps, VEL, DT, rows=False)
    res = eng.optimize_times(batch, iterations=4)
    T0, T, before, after, acc = assert_loop_properties(eng, batch, res, ragged=True)
    so = batch.seg_offsets_host
    assert acc[np.array(MIXED) == 1].max() == 0 and acc[np.array(MIXED) == 8].min() >= 1
    for b, wp in enumerate(wps):
        alone = eng.optimize_times(eng.plan(wp[None], VEL, DT, rows=False), iterations=4)
        assert np.array_equal(host(alone.plan.times).reshape(-1), T[so[b]:so[b + 1]]), b
        assert host(alone.cost_before)[0] == before[b] and host(alone.cost_after)[0] == after[b] and host(alone.accepted)[0] == acc[b], b
        assert np.array_equal(host(alone.plan.coeffs).reshape(-1), res.plan.mission_coeffs(b).reshape(-1)), b
    eng.ctx.set_option("timeopt_chunk", 5)
    try:
        chunked = eng.optimize_times(batch, iterations=4)
    finally:
        eng.ctx.set_option("timeopt_chunk", 0)
    for a, b in zip(result_arrays(res), result_arrays(chunked)):
        assert np.array_equal(a, b)
    rows = eng.optimize_times(eng.plan_ragged(wps, VEL, DT), iterations=4).plan       # rows as the input has them
    assert rows.traj is not None and np.array_equal(host(rows.times), T)
    assert np.array_equal(host(rows.traj), host(eng.sample_rows(res.plan).traj))
    assert eng.take_flags() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------- 6: downstream
def test_an_optimised_plan_flies_audits_and_replans_like_any_other(eng):
    import torch
    from test_gpu_plan_audit import audit_from_rows
    B, m, K = 64, 3, 300
    wps = mo.synthetic_missions(B, m)
    plan = eng.plan(wps, VEL, DT)
    res = eng.optimize_times(plan, iterations=4)
    new = res.plan
    assert new.free_times and new.traj is not None and int(res.accepted.max()) >= 1
    # the rollout's standing property (tests/test_gpu_control.py): plan-fed and row-fed flights agree bit for bit in the vehicles' state
    # -- rows 0-25; rows 26-29 hold the yaw scan a plan-fed fleet carries, which a row-fed one leaves alone -- and in every logged tick
    flights = []
    for fed in (True, False):
        fleet = eng.fleet(new, from_plan=fed)
        slog, clog = fleet.rollout(K, state_log=True, cmd_log=True)
        flights.append((fleet.state[:26].clone(), fleet.istate.clone(), slog.clone(), clog.clone()))
    torch.cuda.synchronize()
    for a, b in zip(*flights):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(flights[0][0]).all())
    want = audit_from_rows(host(new.traj), host(new.row_offsets), None)[0]
    assert np.array_equal(host(eng.audit(new).block), want)
    kept = {f: getattr(new, f).clone() for f in ("times", "seg_rows", "row_offsets", "coeffs", "first_yaw", "traj")}
    for again in (eng.replan, eng.solve):
        new.coeffs.fill_(SENT)
        again(new)
        for f, v in kept.items():
            assert torch.equal(getattr(new, f), v), (again.__name__, f)
    assert np.array_equal(host(eng.first_yaw(new)), host(new.first_yaw))
    with pytest.raises(ValueError, match="durations"):
        eng.retime(new)
    bc = np.zeros((B, 6, 3))
    bc[:, 0, 0] = 0.5
    with pytest.raises(ValueError, match="boundary"):
        eng.optimize_times(eng.plan(wps, VEL, DT, rows=False, boundary=bc))
    assert eng.take_flags() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------- 7: the ABI
def test_invalid_arguments_are_refused_before_anything_is_enqueued(eng):
    import torch
    from uav_ac import _native as nat
    B, m = 5, 3
    kw = dict(device=eng.device)
    wp = dev(eng, mo.synthetic_missions(B, m))
    times = torch.full((B, m), 1.5, dtype=torch.float64, **kw)
    outs = dict(before=torch.full((B,), SENT, dtype=torch.float64, **kw), after=torch.full((B,), SENT, dtype=torch.float64, **kw),
                acc=torch.full((B,), -7, dtype=torch.int32, **kw), seg_rows=torch.full((B, m), -7, dtype=torch.int32, **kw),
                ro=torch.full((B + 1,), -7, dtype=torch.int64, **kw), coeffs=torch.full((B, 8 * m, 3), SENT, dtype=torch.float64, **kw),
                cost=torch.full((B,), SENT, dtype=torch.float64, **kw))
    kept = {n: host(v).copy() for n, v in outs.items()}
    kept["times"] = host(times).copy()
    lib = nat.lib()
    c = eng.ctx._h
    eng._bind_stream()

    def opt(wp_=wp, B_=B, m_=m, times_=times, it=2, before=outs["before"], after=outs["after"], acc=outs["acc"]):
        return lib.uavac_minsnap_optimize_times_dev(c, _p(wp_), None, B_, m_, _p(times_), it, _p(before), _p(after), _p(acc))

    assert opt(it=-1) == nat.EINVAL and opt(B_=0) == nat.EINVAL and opt(m_=0) == nat.EINVAL and opt(m_=nat.MAX_SEGMENTS + 1) == nat.EINVAL
    assert opt(wp_=None) == nat.EINVAL and opt(times_=None) == nat.EINVAL and opt(before=None) == nat.EINVAL
    assert opt(after=None) == nat.EINVAL and opt(acc=None) == nat.EINVAL

    def counts(times_=times, B_=B, m_=m, dt=DT, sr=outs["seg_rows"], ro=outs["ro"]):
        return lib.uavac_minsnap_row_counts_t_dev(c, _p(times_), None, B_, m_, dt, _p(sr), _p(ro))

    assert counts(times_=None) == nat.EINVAL and counts(B_=0) == nat.EINVAL and counts(m_=0) == nat.EINVAL and counts(dt=0.0) == nat.EINVAL
    assert counts(sr=None) == nat.EINVAL and counts(ro=None) == nat.EINVAL

    def chain(wp_=wp, B_=B, m_=m, times_=times, dt=DT, sr=outs["seg_rows"], ro=outs["ro"], co=outs["coeffs"], cap=0, yaw=None):
        return lib.uavac_minsnap_plan_t_dev(c, _p(wp_), None, B_, m_, _p(times_), dt, _p(sr), _p(ro), _p(co), None, None, cap, _p(yaw), None)

    assert chain(wp_=None) == nat.EINVAL and chain(times_=None) == nat.EINVAL and chain(B_=0) == nat.EINVAL and chain(m_=65) == nat.EINVAL
    assert chain(dt=-1.0) == nat.EINVAL and chain(sr=None) == nat.EINVAL and chain(ro=None) == nat.EINVAL and chain(co=None) == nat.EINVAL
    assert chain(yaw=outs["cost"]) == nat.EINVAL                  # a dense yaw column without rows

    def cost(co=outs["coeffs"], times_=times, B_=B, m_=m, out=outs["cost"]):
        return lib.uavac_minsnap_cost_dev(c, _p(co), _p(times_), None, B_, m_, _p(out))

    assert cost(co=None) == nat.EINVAL and cost(times_=None) == nat.EINVAL and cost(B_=0) == nat.EINVAL and cost(m_=0) == nat.EINVAL
    assert cost(out=None) == nat.EINVAL
    with pytest.raises(nat.UavacError):
        eng.ctx.set_option("timeopt_chunk", -1)
    assert eng.take_flags() == [0, 0, 0, 0]
    for n, v in outs.items():
        assert np.array_equal(host(v), kept[n]), n
    assert np.array_equal(host(times), kept["times"])
