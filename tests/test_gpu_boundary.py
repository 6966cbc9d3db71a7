"""Minimum-snap plans that start and end in motion (`uavac_minsnap_solve_bc_dev`, `uavac_minsnap_plan_bc_dev`,
csrc/minsnap_solve_bc.hip) and the handover of a flying fleet to a new plan (`Fleet.boundary`, `Fleet.follow`), on the GPU.

What is compared with what:
  * every mission's coefficients against the reference-form dense KKT solve with boundary VALUES (tests/boundary_ref.py) with the
    project's standing bars: 1e-9 against `np.linalg.solve`, 1e-5 against `lstsq`, SURVEY 8(c) column metric (`conftest.col_err`);
  * what the construction promises bit for bit: the three start coefficients, ragged against uniform, a split batch against the
    whole, rows against rows-free + sampler, plan-fed against row-fed flight, the audit against NumPy over the rows;
  * the handover: the same flying fleet given the same new route once with its live velocities as the start condition and once
    with the rest start -- the only measured numbers of this file, printed, ordered, not thresholded.
"""
import ctypes as C

import numpy as np
import pytest

import boundary_ref as br
from conftest import col_err

pytestmark = pytest.mark.gpu

VEL, DT = 3.0, 0.01
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


def dev(eng, a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64).to(eng.device)


def durations(eng, wps, velocity=VEL):
    """times (B, m) of uniform missions from the product's own duration kernel (device tensor)."""
    import torch
    B, m = wps.shape[0], wps.shape[1] - 1
    kw = dict(device=eng.device)
    times = torch.empty((B, m), dtype=torch.float64, **kw)
    seg_rows, ro = torch.empty((B, m), dtype=torch.int32, **kw), torch.empty((B + 1,), dtype=torch.int64, **kw)
    wp = dev(eng, wps)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_row_counts_dev", _p(wp), B, m, float(velocity), DT, _p(times), _p(seg_rows), _p(ro))
    return times


def solve_bc(eng, wp, times, bc, B, m, seg_offsets=None, n_seg=None):
    """One call of uavac_minsnap_solve_bc_dev on device tensors -> (coeffs (n_seg * 8, 3) host array, status (B,)).  The coefficients
    are the middle of a larger sentinel-filled buffer: nothing outside may be written, everything inside must be."""
    import torch
    n_seg = B * m if n_seg is None else n_seg
    pad = 96
    buf = torch.full((pad + n_seg * 24 + pad,), SENT, dtype=torch.float64, device=eng.device)
    status = torch.full((B,), -7, dtype=torch.int32, device=eng.device)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_solve_bc_dev", _p(wp), _p(times), _p(seg_offsets), int(B), int(m), _p(bc), _p(buf[pad:]), _p(status))
    torch.cuda.synchronize()
    out = host(buf)
    assert (out[:pad] == SENT).all() and (out[pad + n_seg * 24:] == SENT).all() and not (out[pad:pad + n_seg * 24] == SENT).any()
    return out[pad:pad + n_seg * 24].reshape(n_seg * 8, 3).copy(), host(status)


def solve_rest(eng, wp, times, B, m):
    import torch
    coeffs = torch.empty((B, 8 * m, 3), dtype=torch.float64, device=eng.device)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_solve_dev", _p(wp), _p(times), B, m, _p(coeffs), None)
    return host(coeffs)


# --------------------------------------------------------------------------------- 1: every mission against the dense reference
B_ORACLE = 65                    # a full wave plus one lane
_CASES = {}


def oracle_case(eng, m):
    """Per m, computed once and left unchanged: missions, boundary values, the kernel's coefficients, the two dense references."""
    if m not in _CASES:
        from oracle import minsnap_oracle as mo
        wps = mo.synthetic_missions(B_ORACLE, m)
        bc = br.draw_boundaries(B_ORACLE, 1000 + m)
        times = durations(eng, wps)
        got, status = solve_bc(eng, dev(eng, wps), times, dev(eng, bc), B_ORACLE, m)
        th = host(times)                                          # (the references take the product's own durations)
        _CASES[m] = dict(wps=wps, bc=bc, times=th, got=got.reshape(B_ORACLE, 8 * m, 3), status=status,
                         solve=np.stack([br.dense_coeffs(w, t, c, "solve") for w, t, c in zip(wps, th, bc)]),
                         lstsq=np.stack([br.dense_coeffs(w, t, c, "lstsq") for w, t, c in zip(wps, th, bc)]))
        assert eng.take_flags() == [0, 0, 0, 0]
    return _CASES[m]


@pytest.mark.parametrize("m", [1, 2, 3, 8, 20])
def test_every_mission_against_the_dense_reference_with_boundary_values(eng, m):
    k = oracle_case(eng, m)
    assert (k["status"] == 0).all()
    e_solve = max(col_err(g, r) for g, r in zip(k["got"], k["solve"]))
    e_lstsq = max(col_err(g, r) for g, r in zip(k["got"], k["lstsq"]))
    print(f"m={m}: worst mission col_err {e_solve:.3e} against solve, {e_lstsq:.3e} against lstsq")
    assert e_solve < 1e-9 and e_lstsq < 1e-5


@pytest.mark.parametrize("m", [1, 2, 3, 8, 20])
def test_start_coefficients_are_the_boundary_values_bit_for_bit_and_the_goal_is_met(eng, m):
    k = oracle_case(eng, m)
    got, bc = k["got"], k["bc"]
    assert np.array_equal(got[:, 1], bc[:, 0]) and np.array_equal(got[:, 2], 0.5 * bc[:, 1])
    assert np.array_equal(got[:, 3], bc[:, 2] * (1.0 / 6.0))
    worst = max(np.abs(br.derivatives(g, m - 1, t[-1]) - c[3:]).max() for g, t, c in zip(got, k["times"], bc))
    print(f"m={m}: goal derivatives off by at most {worst:.3e}")
    assert worst < 1e-9


def test_zero_boundaries_give_the_rest_to_rest_plan(eng):
    """Coefficients within 1e-12 of uavac_minsnap_solve_dev (relative to the largest coefficient; another elimination order, so
    not bit-equal); durations, row counts and offsets bit-equal to the _v chain's: they do not depend on bc."""
    import torch
    from oracle import minsnap_oracle as mo
    B, m = 65, 8
    wps = dev(eng, mo.synthetic_missions(B, m))
    speeds = torch.full((B,), VEL, dtype=torch.float64, device=eng.device)
    zero = torch.zeros((B, 6, 3), dtype=torch.float64, device=eng.device)
    out = {}
    for name in ("v", "bc"):
        kw = dict(device=eng.device)
        t = dict(times=torch.empty((B, m), dtype=torch.float64, **kw), seg_rows=torch.empty((B, m), dtype=torch.int32, **kw),
                 ro=torch.empty((B + 1,), dtype=torch.int64, **kw), coeffs=torch.empty((B, 8 * m, 3), dtype=torch.float64, **kw),
                 status=torch.full((B,), -7, dtype=torch.int32, **kw), fy=torch.empty((B,), dtype=torch.float64, **kw))
        eng._bind_stream()
        head = (_p(wps), B, m, _p(speeds), DT)
        tail = (_p(t["times"]), _p(t["seg_rows"]), _p(t["ro"]), _p(t["coeffs"]), _p(t["status"]), None, 0, None, _p(t["fy"]))
        if name == "v":
            eng.ctx.call("uavac_minsnap_plan_v_dev", *head, *tail)
        else:
            eng.ctx.call("uavac_minsnap_plan_bc_dev", *head, _p(zero), *tail)
        out[name] = {k: host(v) for k, v in t.items()}
    for k in ("times", "seg_rows", "ro"):
        assert np.array_equal(out["bc"][k], out["v"][k]), k
    assert (out["bc"]["status"] == 0).all()
    a, b = out["bc"]["coeffs"], out["v"]["coeffs"]
    rel = np.abs(a - b).max() / np.abs(b).max()
    print(f"zero boundaries against the two-ended solve: {rel:.3e} of the largest coefficient")
    assert rel < 1e-12


@pytest.mark.parametrize("k", [1, 7])
def test_tail_resolved_from_an_interior_knot_is_the_tail(eng, k):
    """The property a handover rests on: with the original durations and knot k's own (v, a, j) as the start condition, segments
    k.. of the default (rest-to-rest) solve come back."""
    from oracle import minsnap_oracle as mo
    B, m = 65, 8
    wps = mo.synthetic_missions(B, m)
    times = durations(eng, wps)
    full = solve_rest(eng, dev(eng, wps), times, B, m)
    bc = np.zeros((B, 6, 3))
    bc[:, 0], bc[:, 1], bc[:, 2] = full[:, 8 * k + 1], 2.0 * full[:, 8 * k + 2], 6.0 * full[:, 8 * k + 3]
    tail, status = solve_bc(eng, dev(eng, wps[:, k:]), times[:, k:].contiguous(), dev(eng, bc), B, m - k)
    assert (status == 0).all()
    err = max(col_err(t, f) for t, f in zip(tail.reshape(B, -1, 3), full[:, 8 * k:]))
    print(f"k={k}: tail against the full mission {err:.3e}")
    assert err < 1e-9


def test_ragged_missions_equal_uniform_calls_on_each_alone(eng):
    import torch
    from oracle import minsnap_oracle as mo
    counts = (1, 2, 5, 3)
    wps = [mo.synthetic_missions(4, c)[i] for i, c in enumerate(counts)]
    bc = br.draw_boundaries(4, 77)
    alone, times = [], []
    for w, c, x in zip(wps, counts, bc):
        t = durations(eng, w[None])
        times.append(t.reshape(-1))
        co, st = solve_bc(eng, dev(eng, w[None]), t, dev(eng, x[None]), 1, c)
        assert st[0] == 0
        alone.append(co)
    so = dev(eng, np.concatenate([[0], np.cumsum(counts)]), torch.int64)
    got, status = solve_bc(eng, dev(eng, np.concatenate(wps)), torch.cat(times), dev(eng, bc), 4, max(counts), seg_offsets=so,
                           n_seg=sum(counts))
    assert (status == 0).all() and np.array_equal(got, np.concatenate(alone))
    assert eng.take_flags() == [0, 0, 0, 0]


def test_a_split_batch_equals_the_whole(eng):
    from oracle import minsnap_oracle as mo
    B, m = 130, 8
    wps, bc = mo.synthetic_missions(B, m), br.draw_boundaries(B, 5)
    times = durations(eng, wps)
    whole, _ = solve_bc(eng, dev(eng, wps), times, dev(eng, bc), B, m)
    halves = [solve_bc(eng, dev(eng, wps[s]), times[s].contiguous(), dev(eng, bc[s]), 65, m)[0] for s in (slice(0, 65), slice(65, 130))]
    assert np.array_equal(whole, np.concatenate(halves))


# ------------------------------------------------------------------------------------------------------------- 2: the chain
_CHAIN = {}


def chain_case(eng):
    if not _CHAIN:
        from oracle import minsnap_oracle as mo
        B, m = 65, 3
        wps, bc = mo.synthetic_missions(B, m), br.draw_boundaries(B, 11)
        bc[0, 0, :2] = 0.0                                        # mission 0 starts with no horizontal velocity: its row 0 has no heading of its own
        _CHAIN.update(B=B, m=m, wps=wps, bc=bc, rows=eng.plan(wps, VEL, DT, boundary=bc, dense_yaw=True),
                      free=eng.plan(wps, VEL, DT, boundary=bc, rows=False))
        assert eng.take_flags() == [0, 0, 0, 0]
    return _CHAIN


def test_rows_plan_equals_rows_free_plan_plus_sampler_and_row_0_flies_at_v0(eng):
    k = chain_case(eng)
    rows, free = k["rows"], k["free"]
    assert free.traj is None and free.total_rows == rows.total_rows and rows.boundary is not None
    for name in ("times", "seg_rows", "row_offsets", "coeffs", "first_yaw", "status"):
        assert np.array_equal(host(getattr(rows, name)), host(getattr(free, name))), name
    want = host(rows.traj).copy()
    eng.sample_rows(free)
    assert np.array_equal(host(free.traj), want)
    _CHAIN["free"] = eng.plan(k["wps"], VEL, DT, boundary=k["bc"], rows=False)      # (left as it was for the tests after this one)
    ro = host(rows.row_offsets)
    first = want[ro[:-1]]
    assert np.array_equal(first[:, 3:6], k["bc"][:, 0]) and np.array_equal(first[:, 0:3], k["wps"][:, 0])
    moving = np.hypot(k["bc"][:, 0, 0], k["bc"][:, 0, 1]) >= 1e-3
    assert moving[1:].all() and not moving[0]
    # no back-fill: a mission that moves at its first row has its own heading there.  (atan2 to the last bit is the device
    # library's business: two units in the last place of pi is 9e-16)
    heading = np.arctan2(k["bc"][:, 0, 1], k["bc"][:, 0, 0])
    assert np.abs(first[moving, 9] - heading[moving]).max() < 1e-14
    assert np.array_equal(first[:, 9], host(rows.first_yaw)) and np.array_equal(host(rows.yaw), want[:, 9])


def test_a_capacity_one_row_short_refuses_the_whole_plan(eng):
    import torch
    k = chain_case(eng)
    B, m, total = k["B"], k["m"], k["rows"].total_rows
    kw = dict(device=eng.device)
    t = dict(times=torch.full((B, m), SENT, dtype=torch.float64, **kw), seg_rows=torch.full((B, m), -7, dtype=torch.int32, **kw),
             ro=torch.full((B + 1,), -7, dtype=torch.int64, **kw), coeffs=torch.full((B, 8 * m, 3), SENT, dtype=torch.float64, **kw),
             status=torch.full((B,), -7, dtype=torch.int32, **kw), traj=torch.full((total, 11), SENT, dtype=torch.float64, **kw),
             yaw=torch.full((total,), SENT, dtype=torch.float64, **kw), fy=torch.full((B,), SENT, dtype=torch.float64, **kw))
    before = {n: host(v).copy() for n, v in t.items()}
    speeds = torch.full((B,), VEL, dtype=torch.float64, **kw)
    wps, bc = dev(eng, k["wps"]), dev(eng, k["bc"])

    def chain(capacity):
        eng._bind_stream()
        eng.ctx.call("uavac_minsnap_plan_bc_dev", _p(wps), B, m, _p(speeds), DT, _p(bc), _p(t["times"]),
                     _p(t["seg_rows"]), _p(t["ro"]), _p(t["coeffs"]), _p(t["status"]), _p(t["traj"]), capacity, _p(t["yaw"]), _p(t["fy"]))
        return eng.take_flags()

    assert chain(total - 1) == [0, 0, 1, 0]
    for n, v in t.items():
        assert np.array_equal(host(v), before[n]), n
    assert chain(total) == [0, 0, 0, 0]                          # ... and with the one row more it is the Engine's plan
    for n, name in (("times", "times"), ("seg_rows", "seg_rows"), ("ro", "row_offsets"), ("coeffs", "coeffs"), ("traj", "traj"),
                    ("yaw", "yaw"), ("fy", "first_yaw"), ("status", "status")):
        assert np.array_equal(host(t[n]), host(getattr(k["rows"], name))), n


def test_audit_of_a_boundary_plan_equals_numpy_over_its_rows(eng):
    from test_gpu_plan_audit import audit_from_rows
    k = chain_case(eng)
    want = audit_from_rows(host(k["rows"].traj), host(k["rows"].row_offsets), None)[0]
    for plan in (k["rows"], k["free"]):
        assert np.array_equal(host(eng.audit(plan).block), want)


# ------------------------------------------------------------------------------------------------------------- 3: flight
def test_plan_fed_and_row_fed_fleets_log_the_same_bits_and_retime_refuses(eng):
    import torch
    from oracle import minsnap_oracle as mo
    B, m, K = 64, 3, 400
    wps, bc = mo.synthetic_missions(B, m), br.draw_boundaries(B, 21)
    plan = eng.plan(wps, VEL, DT, boundary=bc)
    logs = []
    for fed in (True, False):
        fleet = eng.fleet(plan, from_plan=fed)
        slog, clog = fleet.rollout(K, state_log=True, cmd_log=True)
        logs.append((slog.clone(), clog.clone(), fleet.state[:26].clone(), fleet.istate.clone()))
    torch.cuda.synchronize()
    for a, b in zip(*logs):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(logs[0][0]).all())
    with pytest.raises(ValueError, match="boundary"):
        eng.retime(plan)
    with pytest.raises(ValueError):
        eng.plan(wps, VEL, DT, boundary=bc[:, :5])
    bad = bc.copy()
    bad[3, 4, 1] = np.inf
    with pytest.raises(ValueError, match="finite"):
        eng.plan(wps, VEL, DT, boundary=bad)
    # replan and solve read plan.boundary again: another start condition in place, other coefficients, the same durations
    before, times = plan.coeffs.clone(), plan.times.clone()
    plan.boundary[:, 0] *= 0.5
    for again in (eng.replan, eng.solve):
        plan.coeffs.fill_(SENT)
        again(plan)
        assert torch.equal(plan.coeffs[:, 1], plan.boundary[:, 0]) and not torch.equal(plan.coeffs, before)
        assert torch.equal(plan.times, times)
    assert eng.take_flags() == [0, 0, 0, 0]


def test_a_singular_mission_reports_status_1_for_itself_alone(eng):
    from oracle import minsnap_oracle as mo
    from uav_ac import _native as nat
    B, m = 64, 3
    wps, bc = mo.synthetic_missions(B, m), br.draw_boundaries(B, 31)
    wps[5, 2] = wps[5, 1]                                         # a repeated waypoint: a segment of zero duration
    plan = eng.plan(wps, VEL, DT, boundary=bc, strict=False, rows=False)
    status, co = host(plan.status), host(plan.coeffs)
    assert status[5] == 1 and status.sum() == 1
    assert np.isnan(co[5]).all() and np.isfinite(np.delete(co, 5, axis=0)).all()
    assert eng.take_flags()[1] == 1
    with pytest.raises(nat.UavacError):
        eng.plan(wps, VEL, DT, boundary=bc, rows=False)
    eng.take_flags()
    # a non-finite boundary value that reaches the kernel (the Engine refuses it; the C ABI cannot without a sync) spoils its own mission only
    wps = mo.synthetic_missions(B, m)
    bc[9, 1, 2] = np.nan
    got, status = solve_bc(eng, dev(eng, wps), durations(eng, wps), dev(eng, bc), B, m)
    got = got.reshape(B, 8 * m, 3)
    assert (status == 0).all() and not np.isfinite(got[9]).all() and np.isfinite(np.delete(got, 9, axis=0)).all()


# ------------------------------------------------------------------------------------------------------------- 4: handover
def test_handover_at_speed_tracks_better_than_a_rest_start_and_finishes_the_course(eng):
    """A fleet flies a rest-to-rest plan until mid-course and is given a new route from where it is: its live positions, then the
    two waypoints it had left.  Once the new plan starts at the vehicles' live velocities (`fleet.boundary()`), once at rest -- both
    from a copy of the same state.  Over the next 300 ticks the worst UAV's peak tracking error with the boundary is strictly below
    the rest start's, where the target waits at the start while the vehicle flies away from it.  Measured on an MI355X:
    0.038 m against 0.523 m.  The fleet with the boundary then finishes within upstream's acceptance (there: mean error at most
    0.033 m, final error at most 0.011 m).
    The cruise speed is 1.5 m/s: the speed peaks of this distribution's minimum-snap curves are 1.74 x the cruise speed, so that at
    3 m/s every mission asks for more than the control law's max_speed_xy = 3 m/s and no flight of it is inside upstream's
    acceptance to begin with; at 1.5 m/s the peaks are 2.61 m/s horizontally, 1.87 m/s up, 1.53 m/s down, inside all limits.
    Mid-course is 3.6 s: the first segment lasts L / 1.5 x 1.5 = 2.5 .. 3.5 s, the first two 4.17 s at least, so every vehicle is
    inside its second segment with 0.5 s of it left at least."""
    import torch
    from oracle import minsnap_oracle as mo
    from uav_ac import scoring
    B, m, cruise = 64, 3, 1.5
    wps = mo.synthetic_missions(B, m)
    first = eng.plan(wps, cruise, DT)
    assert bool(scoring.plan_feasibility(eng.audit(first))["feasible"].all())
    fleet = eng.fleet(first)
    fleet.rollout(3600)
    state, istate = fleet.state.clone(), fleet.istate.clone()
    cursor, seg_rows = host(istate[0]), host(first.seg_rows)      # (the cursor counts the mission's own rows)
    assert ((cursor >= seg_rows[:, 0]) & (cursor < seg_rows[:, 0] + seg_rows[:, 1])).all()       # every vehicle is inside its second segment
    assert float(torch.linalg.norm(state[7:10], dim=0).median()) > 1.0       # ... and the fleet is at speed (one in a sharp corner may be slow)
    route = torch.cat([state[0:3].t()[:, None, :], dev(eng, wps[:, 2:])], dim=1)
    peaks = {}
    for name in ("rest", "boundary"):
        fleet.state.copy_(state)
        fleet.istate.copy_(istate)
        bc = fleet.boundary() if name == "boundary" else None
        if bc is not None:
            assert torch.equal(bc[:, 0], state[7:10].t()) and not bool(bc[:, 1:].any())
        fleet.follow(eng.plan(route, cruise, DT, boundary=bc, rows=False))
        assert not bool(fleet.istate[0:2].any()) and torch.equal(fleet.state[:26], state[:26])
        assert torch.equal(fleet.istate[2:], istate[2:]) and bool((fleet.state[26] == -1.0).all())
        fleet.rollout(300, score=True)
        peaks[name] = float(fleet.score[scoring.MAX].max())
    print(f"handover: worst UAV's peak tracking error over 300 ticks {peaks['boundary']:.4f} m with the live velocities as the "
          f"start condition, {peaks['rest']:.4f} m from a rest start")
    assert peaks["boundary"] < peaks["rest"]
    rows = int((fleet.plan.row_offsets[1:] - fleet.plan.row_offsets[:-1]).max())
    fleet.rollout(10 * rows - 300 + 10, score=True)              # one period per row (inner_per_outer = 10), and the last row's period
    summary = fleet.tracking()
    audit = eng.audit(fleet.plan)
    print(f"handover: to the end of the course mean error at most {float(summary['mean_error'].max()):.4f} m, final error at most "
          f"{float(summary['final_error'].max()):.4f} m, peak error at most {float(summary['max_error'].max()):.4f} m; the new plan's "
          f"peaks: {float(audit.speed_xy.max()):.3f} m/s horizontally, {float(audit.ascent.max()):.3f} up, {float(audit.descent.max()):.3f} down")
    verdict = scoring.acceptance(summary)
    assert bool(verdict["passed"].all()), {k: int((~v).sum()) for k, v in verdict.items()}
    with pytest.raises(ValueError):
        fleet.follow(eng.plan(wps[:32], cruise, DT, rows=False))
