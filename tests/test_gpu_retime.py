"""Per-mission cruise speeds in the planning chain (`uavac_minsnap_*_v_dev`) and retiming of plans to the flight limits
(`uavac_minsnap_retime_factors_dev`, `uavac_minsnap_retime_dev`, csrc/minsnap_retime.hip), on the GPU through the C ABI.

What is compared with what:
  * a mission planned at its own speed against the SCALAR entry points at that speed: bit for bit (same kernel, same arithmetic);
  * spot missions against oracle.minsnap_oracle at their own speed with the project's standing bars: durations and row counts
    exact, coefficients 1e-9 against method="solve", rows 1e-5, both in the SURVEY 8(c) column metric (`conftest.col_err`);
  * the factors kernel and the loop against `uav_ac.scoring.retime_factors` (NumPy, tests/test_retime_host.py): bit for bit.
"""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import col_err
from test_retime_host import LIMITS, MARGIN, crafted_block, oracle_peaks, same_bits

pytestmark = pytest.mark.gpu

DT = 0.01
SPEEDS = (0.5, 1.3, 2.75, 4.0)
SENT = -1.2345e300


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


def mission_speeds(B, seed):
    return np.array(SPEEDS)[np.random.default_rng(seed).integers(0, len(SPEEDS), B)]


def rows_of(plan):
    return host(plan.traj), host(plan.row_offsets)


def assert_missions_equal(got, ref, pick, seg_slices=None):
    """Missions `pick` of plan `got` equal those of plan `ref`, bit for bit: durations, row counts, coefficients, first headings
    and (when both have rows) rows.  seg_slices: per mission the slice of its segments in a ragged batch."""
    for name in ("times", "seg_rows", "coeffs"):
        a, b = host(getattr(got, name)), host(getattr(ref, name))
        if seg_slices is None:
            assert np.array_equal(a[pick], b[pick], equal_nan=a.dtype.kind == "f"), name
        else:
            for i in pick:
                assert np.array_equal(a[seg_slices[i]], b[seg_slices[i]]), (name, i)
    assert np.array_equal(host(got.first_yaw)[pick], host(ref.first_yaw)[pick])
    if got.traj is not None and ref.traj is not None:
        (ta, ra), (tb, rb) = rows_of(got), rows_of(ref)
        for i in pick:
            assert np.array_equal(ta[ra[i]:ra[i + 1]], tb[rb[i]:rb[i + 1]]), i


def assert_offsets_are_the_exclusive_sum(plan, totals):
    ro = host(plan.row_offsets)
    assert ro[0] == 0 and np.array_equal(np.diff(ro), totals) and plan.total_rows == ro[-1]


# ----------------------------------------------------------------------------------------- 1: per-mission speeds, uniform
_UNIFORM = {}


def uniform_case(eng):
    if not _UNIFORM:
        from oracle import minsnap_oracle as mo
        B, m = 300, 3                                                   # a full 256-mission tile plus a partial one
        wps = mo.synthetic_missions(B, m)
        vel = mission_speeds(B, 1)
        assert all((vel == v).sum() > 40 for v in SPEEDS)
        _UNIFORM.update(B=B, m=m, wps=wps, vel=vel, scalar={v: eng.plan(wps, v, DT) for v in SPEEDS},
                        mixed=eng.plan(wps, vel, DT))
        assert eng.take_flags() == [0, 0, 0, 0]
    return _UNIFORM


def test_uniform_batch_at_per_mission_speeds_equals_the_scalar_calls(eng):
    import torch
    k = uniform_case(eng)
    B, m, vel, mixed = k["B"], k["m"], k["vel"], k["mixed"]
    assert mixed.velocities is not None and math.isnan(mixed.velocity) and np.array_equal(host(mixed.velocities), vel)
    assert k["scalar"][SPEEDS[0]].velocities is None
    totals = np.zeros(B, dtype=np.int64)
    for v in SPEEDS:
        pick = np.flatnonzero(vel == v)
        assert_missions_equal(mixed, k["scalar"][v], pick)
        totals[pick] = host(k["scalar"][v].seg_rows).sum(axis=1)[pick]
    assert_offsets_are_the_exclusive_sum(mixed, totals)
    # the rows-free form: the same plan without the rows
    free = eng.plan(k["wps"], torch.as_tensor(vel), DT, rows=False)
    assert free.traj is None
    assert_missions_equal(free, mixed, np.arange(B))
    assert_offsets_are_the_exclusive_sum(free, totals)
    # replan, both forms: into scrambled buffers, the whole chain by one call
    for plan in (eng.plan(k["wps"], vel, DT), eng.plan(k["wps"], vel, DT, rows=False)):
        for t in (plan.times, plan.coeffs, plan.first_yaw) + (() if plan.traj is None else (plan.traj,)):
            t.fill_(SENT)
        plan.seg_rows.fill_(-7)
        plan.row_offsets.fill_(-7)
        eng.replan(plan)
        assert_missions_equal(plan, mixed, np.arange(B))
        assert_offsets_are_the_exclusive_sum(plan, totals)
    assert eng.take_flags() == [0, 0, 0, 0]
    # the commit guarantee of the form with rows: a buffer one row short refuses the plan as a whole
    plan = eng.plan(k["wps"], vel, DT)
    plan.traj = plan.traj[:-1]
    for t in (plan.times, plan.coeffs, plan.first_yaw, plan.traj):
        t.fill_(SENT)
    plan.seg_rows.fill_(-7)
    plan.row_offsets.fill_(-7)
    eng.replan(plan)
    assert eng.take_flags() == [0, 0, 1, 0]
    assert all(bool((t == SENT).all()) for t in (plan.times, plan.coeffs, plan.first_yaw, plan.traj))
    assert bool((plan.seg_rows == -7).all()) and bool((plan.row_offsets == -7).all())


def test_spot_missions_against_the_oracle_at_their_own_speed(eng):
    from oracle import minsnap_oracle as mo
    k = uniform_case(eng)
    mixed, vel = k["mixed"], k["vel"]
    times, seg_rows, coeffs = host(mixed.times), host(mixed.seg_rows), host(mixed.coeffs)
    spots = [int(np.flatnonzero(vel == v)[j]) for v, j in ((0.5, 0), (2.75, 3), (4.0, -1))]      # (the last one lies in the partial tile)
    assert spots[-1] >= 256
    for b in spots:
        ref_co, ref_t, _, _ = mo.solve_coefficients(k["wps"][b], vel[b], method="solve")
        assert np.array_equal(times[b], ref_t)
        assert np.array_equal(seg_rows[b], mo.row_counts(ref_t, DT))
        e_co = col_err(coeffs[b], ref_co)
        e_rows = col_err(mixed.mission(b), mo.plan(k["wps"][b], vel[b], DT, method="solve"))
        print(f"mission {b} at {vel[b]} m/s: coefficient error {e_co:.3e}, row error {e_rows:.3e}")
        assert e_co < 1e-9 and e_rows < 1e-5, (b, e_co, e_rows)


# ------------------------------------------------------------------------------------------------------------------ 2: ragged
def test_ragged_batch_at_per_mission_speeds_equals_the_scalar_ragged_calls(eng):
    from oracle import minsnap_oracle as mo
    B = 70
    full = mo.synthetic_missions(B, 5)
    missions = [full[b, :2 + (3 * b) % 5] for b in range(B)]                         # 1 .. 5 segments
    assert sorted({len(w) - 1 for w in missions}) == [1, 2, 3, 4, 5]
    vel = mission_speeds(B, 2)
    mixed = eng.plan_ragged(missions, vel, DT)
    free = eng.plan_ragged(missions, vel, DT, rows=False)
    so = mixed.seg_offsets_host
    slices = [slice(int(so[b]), int(so[b + 1])) for b in range(B)]
    totals = np.zeros(B, dtype=np.int64)
    for v in SPEEDS:
        ref = eng.plan_ragged(missions, v, DT)
        pick = np.flatnonzero(vel == v)
        assert len(pick) > 5
        assert_missions_equal(mixed, ref, pick, slices)
        assert_missions_equal(free, ref, pick, slices)
        totals[pick] = np.diff(host(ref.row_offsets))[pick]
    assert_offsets_are_the_exclusive_sum(mixed, totals)
    assert_offsets_are_the_exclusive_sum(free, totals)
    assert np.array_equal(host(mixed.velocities), vel) and math.isnan(mixed.velocity)
    assert eng.take_flags() == [0, 0, 0, 0]


# -------------------------------------------------------------------------------------------------------------- 3: a bad speed
@pytest.mark.parametrize("bad", [0.0, -1.5, float("nan"), float("inf")])
def test_a_bad_speed_raises_flag_0_and_costs_only_its_own_mission(eng, bad):
    k = uniform_case(eng)
    B, at = k["B"], 261
    vel = k["vel"].copy()
    vel[at] = bad
    assert eng.take_flags() == [0, 0, 0, 0]
    for rows in (True, False):
        plan = eng.plan(k["wps"], vel, DT, strict=False, rows=rows)
        flags = eng.take_flags()
        assert flags[0] == 1 and flags[2] == 0 and flags[3] == 0, flags
        assert bool((plan.seg_rows[at] == 0).all())
        ro = host(plan.row_offsets)
        assert ro[at + 1] == ro[at] and np.array_equal(np.diff(ro), host(plan.seg_rows).sum(axis=1))
        assert_missions_equal(plan, k["mixed"], np.setdiff1d(np.arange(B), [at]))
    # ragged form, same kernel: the other template argument
    missions = [k["wps"][b, :2 + b % 3] for b in range(40)]
    v40 = k["vel"][:40].copy()
    good = eng.plan_ragged(missions, v40, DT)
    v40[7] = bad
    batch = eng.plan_ragged(missions, v40, DT, strict=False)
    assert eng.take_flags()[0] == 1
    so = batch.seg_offsets_host
    slices = [slice(int(so[b]), int(so[b + 1])) for b in range(40)]
    assert bool((batch.seg_rows[slices[7]] == 0).all())
    assert_missions_equal(batch, good, np.setdiff1d(np.arange(40), [7]), slices)


# ------------------------------------------------------------------------------------------------------- 4: the factors kernel
def test_factors_kernel_equals_the_numpy_rule_bit_for_bit(eng):
    import torch
    from uav_ac import _native as nat
    from uav_ac.scoring import retime_factors
    B, PAD = 130, 64                                                                 # two wavefronts plus a partial one
    block, want, vel = crafted_block(B)
    spec = retime_factors(block, margin=MARGIN, velocities=vel)
    ok = ~np.isnan(want)
    assert same_bits(spec["factors"][ok], want[ok])
    dev = dict(device=eng.device)
    d_block = torch.as_tensor(block).to(eng.device)
    limits = (C.c_double * 4)(*LIMITS)

    def run(velocities):
        d_vel = torch.full((PAD + B + PAD,), SENT, dtype=torch.float64, **dev)
        d_vel[PAD:PAD + B] = torch.as_tensor(velocities)
        d_fac = torch.full((PAD + B + PAD,), SENT, dtype=torch.float64, **dev)
        d_cnt = torch.tensor([0, 0, -7, -7], dtype=torch.int32, **dev)
        eng._bind_stream()
        eng.ctx.call("uavac_minsnap_retime_factors_dev", _p(d_block), B, limits, MARGIN, _p(d_vel[PAD:]), _p(d_fac[PAD:]), _p(d_cnt))
        torch.cuda.synchronize()
        v, f = host(d_vel), host(d_fac)
        for x in (v, f):                                                             # nothing outside [B]
            assert (x[:PAD] == SENT).all() and (x[PAD + B:] == SENT).all()
        return v[PAD:PAD + B], f[PAD:PAD + B], host(d_cnt).tolist()

    got_v, got_f, cnt = run(vel)
    assert np.array_equal(np.isnan(got_f), spec["nan"]) and same_bits(got_f[ok], spec["factors"][ok])
    assert same_bits(got_v, spec["velocities"])
    assert same_bits(got_v[~spec["retimed"]], vel[~spec["retimed"]])                  # untouched ones: bit for bit
    assert cnt == [spec["n_retimed"], spec["n_nan"], -7, -7]
    assert spec["n_retimed"] == 70 and spec["n_nan"] == 20
    # each argument error: UAVAC_EINVAL, nothing enqueued, nothing written
    d_vel = torch.full((B,), SENT, dtype=torch.float64, **dev)
    d_fac = torch.full((B,), SENT, dtype=torch.float64, **dev)
    d_cnt = torch.full((2,), -7, dtype=torch.int32, **dev)
    good = dict(audit=d_block, B=B, limits=LIMITS, margin=MARGIN, vel=d_vel, fac=d_fac, cnt=d_cnt)
    bad = [dict(B=0), dict(B=-2), dict(margin=1.0), dict(margin=-0.001), dict(margin=math.nan), dict(margin=math.inf),
           dict(audit=None), dict(vel=None), dict(fac=None), dict(cnt=None), dict(limits=None)]
    for i in range(4):
        for value in (0.0, -1.0, math.inf, math.nan):
            bad.append(dict(limits=LIMITS[:i] + (value,) + LIMITS[i + 1:]))
    fn = nat.lib().uavac_minsnap_retime_factors_dev
    eng._bind_stream()
    for change in bad:
        a = {**good, **change}
        lim = None if a["limits"] is None else (C.c_double * 4)(*a["limits"])
        rc = fn(eng.ctx._h, _p(a["audit"]), a["B"], lim, a["margin"], _p(a["vel"]), _p(a["fac"]), _p(a["cnt"]))
        assert rc == nat.EINVAL, (change, rc)
    assert fn(None, _p(d_block), B, limits, MARGIN, _p(d_vel), _p(d_fac), _p(d_cnt)) == nat.EINVAL
    torch.cuda.synchronize()
    assert bool((d_vel == SENT).all()) and bool((d_fac == SENT).all()) and bool((d_cnt == -7).all())


# -------------------------------------------------------------------------------------------------------------------- 5: the loop
_LOOP = {}


def loop_case(eng, m):
    if m not in _LOOP:
        from oracle import minsnap_oracle as mo
        wps = mo.synthetic_missions(64, m)
        start = eng.plan(wps, 3.0, DT, rows=False)
        _LOOP[m] = dict(wps=wps, start=start, result=eng.retime(start, margin=MARGIN, max_passes=4))
        assert eng.take_flags() == [0, 0, 0, 0]
    return _LOOP[m]


def replay(eng, wps, v0, margin, passes):
    """The loop with `Engine.plan` + `Engine.audit` + the NumPy rule: (velocities, product of the factors, audits seen)."""
    from uav_ac.scoring import retime_factors
    v, total = np.array(v0, dtype=np.float64), np.ones(len(v0))
    for n in range(passes + 1):
        a = eng.audit(eng.plan(wps, v, DT, rows=False, strict=False))
        out = retime_factors(a, margin=margin, velocities=v)
        total = np.where(out["nan"], np.nan, total)
        if out["n_retimed"] == 0 or n == passes:
            return v, total, out, a
        v, total = out["velocities"], np.where(out["retimed"], total * out["factors"], total)


@pytest.mark.parametrize("m", [2, 8])
def test_loop_brings_every_bench_mission_inside_the_limits(eng, m):
    from uav_ac.scoring import plan_feasibility
    k = loop_case(eng, m)
    res, wps = k["result"], k["wps"]
    assert not bool(plan_feasibility(eng.audit(k["start"]))["feasible"].any())        # as planned, none is
    assert 1 <= res.passes <= 2 and bool(res.converged.all())
    assert bool(plan_feasibility(res.audit, slack=0)["feasible"].all())
    assert res.plan.traj is None and res.plan.velocities is res.velocities
    # the returned plan IS the plan at the returned speeds, and the audit is its audit
    again = eng.plan(wps, res.velocities, DT, rows=False)
    assert_missions_equal(res.plan, again, np.arange(64))
    assert np.array_equal(host(res.plan.row_offsets), host(again.row_offsets)) and res.plan.total_rows == again.total_rows
    assert np.array_equal(host(res.plan.status), np.zeros(64, dtype=np.int32))
    assert np.array_equal(host(res.audit.block), host(eng.audit(again).block))
    assert tuple(res.audit.hit_rows.shape) == (0, 64)
    # the NumPy rule replayed on each pass's audit gives the same speeds and factors, bit for bit
    v, total, last, _ = replay(eng, wps, np.full(64, 3.0), MARGIN, 4)
    assert same_bits(host(res.velocities), v) and same_bits(host(res.factors), total)
    assert last["n_retimed"] == 0 and (host(res.factors) > 1.0).all()
    # the oracle's own peaks at the returned speeds
    lim = np.array(LIMITS)
    for b in (0, 21, 42, 63):
        peaks = np.array(oracle_peaks(wps[b], v[b], DT))
        print(f"m={m} mission {b}: {v[b]:.4f} m/s, oracle peak / limit {peaks / lim}")
        assert (peaks <= lim).all(), (b, peaks)
    # the input is left as it was
    assert k["start"].velocities is None and k["start"].velocity == 3.0


def test_max_passes_0_only_audits(eng):
    from uav_ac.scoring import plan_feasibility
    k = loop_case(eng, 8)
    vel = np.full(64, 3.0)
    vel[::3] = 1.2                                                                   # slow enough for some, not for all
    start = eng.plan(k["wps"], vel, DT, rows=False)
    res = eng.retime(start, margin=MARGIN, max_passes=0)
    assert res.passes == 0 and same_bits(host(res.velocities), vel)
    feasible = host(plan_feasibility(eng.audit(start))["feasible"])
    assert feasible.any() and not feasible.all()
    assert np.array_equal(host(res.converged), feasible)
    assert (host(res.factors) == 1.0).all()
    assert_missions_equal(res.plan, start, np.arange(64))
    # ... and one pass short of enough says so: margin 0 leaves the sampled peaks of some missions a hair over after a single pass
    one = eng.retime(start, margin=0.0, max_passes=1)
    v, total, last, _ = replay(eng, k["wps"], vel, 0.0, 1)
    assert one.passes == 1 and same_bits(host(one.velocities), v) and same_bits(host(one.factors), total)
    assert np.array_equal(host(one.converged), ~last["retimed"] & ~last["nan"])


def test_a_singular_mission_is_reported_and_costs_nobody_else(eng):
    k = loop_case(eng, 8)
    wps = k["wps"].copy()
    wps[5, 3] = wps[5, 2]                                                            # a repeated waypoint
    assert eng.take_flags() == [0, 0, 0, 0]
    res = eng.retime(eng.plan(wps, 3.0, DT, rows=False, strict=False), margin=MARGIN, max_passes=4)
    flags = eng.take_flags()
    assert flags[1] == 1 and flags[0] == 0, flags
    conv, fac, vel = host(res.converged), host(res.factors), host(res.velocities)
    assert not conv[5] and math.isnan(fac[5]) and vel[5] == 3.0
    assert host(res.plan.status)[5] == 1 and np.isnan(host(res.audit.speed_xy)[5])
    clean, others = k["result"], np.setdiff1d(np.arange(64), [5])
    assert res.passes == clean.passes and conv[others].all()
    assert same_bits(vel[others], host(clean.velocities)[others]) and same_bits(fac[others], host(clean.factors)[others])
    assert_missions_equal(res.plan, clean.plan, others)


def test_plans_with_rows_and_ragged_batches_come_back_in_kind(eng):
    from uav_ac.engine import RaggedBatch
    k = loop_case(eng, 2)
    res = eng.retime(eng.plan(k["wps"], 3.0, DT), margin=MARGIN, max_passes=4)
    assert same_bits(host(res.velocities), host(k["result"].velocities))
    again = eng.plan(k["wps"], res.velocities, DT)
    assert res.plan.traj is not None and res.plan.total_rows == again.total_rows
    assert np.array_equal(host(res.plan.traj), host(again.traj))
    assert_missions_equal(res.plan, again, np.arange(64))
    # ragged: every mission as if retimed alone in a uniform batch
    wps8 = loop_case(eng, 8)["wps"]
    missions = [wps8[b, :2 + b % 8] for b in range(24)]
    batch = eng.plan_ragged(missions, 3.0, DT, rows=False)
    rag = eng.retime(batch, margin=MARGIN, max_passes=4)
    assert isinstance(rag.plan, RaggedBatch) and rag.plan.traj is None and bool(rag.converged.all()) and rag.passes <= 2
    ref = eng.plan_ragged(missions, rag.velocities, DT, rows=False)
    so = ref.seg_offsets_host
    assert_missions_equal(rag.plan, ref, np.arange(24), [slice(int(so[b]), int(so[b + 1])) for b in range(24)])
    assert np.array_equal(host(rag.plan.row_offsets), host(ref.row_offsets))
    for b in (1, 7, 14):                                                             # 2, 8 and 7 segments
        alone = eng.retime(eng.plan(missions[b][None], 3.0, DT, rows=False), margin=MARGIN, max_passes=4)
        assert same_bits(host(alone.velocities), host(rag.velocities)[b:b + 1])
        assert same_bits(host(alone.factors), host(rag.factors)[b:b + 1])
    assert eng.take_flags() == [0, 0, 0, 0]


def test_the_loop_refuses_bad_arguments_before_it_touches_anything(eng):
    import torch
    from uav_ac import _native as nat
    k = loop_case(eng, 2)
    p = k["start"]
    B, m = 64, 2
    dev = dict(device=eng.device)
    vel = torch.full((B,), 3.0, dtype=torch.float64, **dev)
    out = {n: torch.full_like(getattr(p, n), -7) for n in ("times", "seg_rows", "row_offsets", "coeffs")}
    audit = torch.full((8, B), SENT, dtype=torch.float64, **dev)
    tot = torch.full((B,), SENT, dtype=torch.float64, **dev)
    conv = torch.full((B,), -7, dtype=torch.int32, **dev)
    passes = C.c_int(-7)
    fn = nat.lib().uavac_minsnap_retime_dev

    def call(B=B, m=m, dt=DT, limits=LIMITS, margin=MARGIN, max_passes=4, vel=vel, audit=audit):
        lim = None if limits is None else (C.c_double * 4)(*limits)
        return fn(eng.ctx._h, _p(p.waypoints), None, B, m, _p(vel), dt, lim, margin, max_passes, _p(out["times"]), _p(out["seg_rows"]),
                  _p(out["row_offsets"]), _p(out["coeffs"]), None, None, _p(audit), _p(tot), _p(conv), C.byref(passes))

    eng._bind_stream()
    for change in (dict(B=0), dict(m=0), dict(m=nat.MAX_SEGMENTS + 1), dict(dt=0.0), dict(limits=None), dict(limits=(3.0, 0.0, 2.0, 12.0)),
                   dict(limits=(3.0, 3.0, 2.0, math.inf)), dict(margin=1.0), dict(margin=-0.1), dict(max_passes=-1), dict(vel=None),
                   dict(audit=None)):
        assert call(**change) == nat.EINVAL, change
    assert call(dt=math.nan) == nat.ENONFINITE
    torch.cuda.synchronize()
    assert bool((vel == 3.0).all()) and bool((audit == SENT).all()) and bool((tot == SENT).all()) and bool((conv == -7).all())
    assert all(bool((t == -7).all()) for t in out.values())
    # the same call with nothing wrong (status and first_yaw are optional)
    assert call() == nat.OK and 1 <= passes.value <= 2
    assert same_bits(host(vel), host(k["result"].velocities)) and same_bits(host(tot), host(k["result"].factors))
    assert bool((conv == 1).all()) and np.array_equal(host(out["coeffs"]), host(k["result"].plan.coeffs))
