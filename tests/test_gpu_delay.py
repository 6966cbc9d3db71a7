"""Start delays as a plan transform, on the GPU (`uavac_minsnap_delay_offsets_dev` / `uavac_minsnap_delay_dev`, csrc/minsnap_delay.hip),
through the C ABI and `Engine.delay`: every mission with a start row S > 0 gets a leading hold segment, and the existing sampler, audits
and ragged plan-fed rollout fly and audit the delayed plan unchanged.

What is compared with what:
  * the delayed plan's arrays against the construction in NumPy, exactly (they are copies);
  * its sampled rows against `uav_ac.scoring.delay_rows` of the product's own rows, bit for bit in all 11 columns;
  * `Engine.separation` of the delayed plan against `Engine.separation` of the plan with start_rows, bit for bit;
  * the delayed batch flown plan-fed against the same flown row-fed from its sampled rows, bit for bit, and five spot missions against
    the scalar C oracle flown on `delay_rows` of the oracle's own rows at the project's 1e-5.
All cases use synthetic_missions(96, 8) at velocity 3.0 and dt 0.01 -- the stagger tests' missions -- with S mixing 0, 1, 63, 64, 65 and
300 (around the sampler's 64-row chunk)."""
import ctypes as C

import numpy as np
import pytest

from conftest import col_err

pytestmark = pytest.mark.gpu

VEL, DT, B, M = 3.0, 0.01, 96, 8
S_ROWS = np.array([0, 1, 63, 64, 65, 300], dtype=np.int32)[np.arange(B) % 6]
SPOTS = (0, 1, 3, 5, B - 1)                                  # S = 0, 1, 64, 300, and the last lane (300)
PAD, SENT_F, SENT_I = 96, -7777.25, -7777
TOL = 1e-5


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    return Engine("cuda:0")


_CACHE = {}


def case(eng):
    """Computed once and left unchanged: the missions, the plan with rows, the same as a ragged batch, the delayed batch with rows."""
    if not _CACHE:
        from oracle import minsnap_oracle as mo
        wps = mo.synthetic_missions(B, M)
        plan = eng.plan(wps, VEL, DT)
        ragged = eng.plan_ragged(list(wps), VEL, DT, rows=False)
        delayed = eng.delay(plan, S_ROWS, rows=True)
        _CACHE.update(wps=wps, plan=plan, ragged=ragged, delayed=delayed)
    return _CACHE


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def numpy_delay(coeffs, times, seg_rows, counts, S, dt):
    """The construction of the issue in NumPy: per-segment arrays back to back -> the delayed ones and the segment offsets."""
    co, tm, sr, so = [], [], [], [0]
    at = 0
    for b, n in enumerate(counts):
        c, t, r = coeffs[at:at + n], times[at:at + n], seg_rows[at:at + n]
        if S[b] > 0:
            hold = np.zeros((1, 8, 3))
            hold[0, 0] = c[0, 0]
            c, t, r = np.concatenate([hold, c]), np.concatenate([[float(S[b]) * dt], t]), np.concatenate([[S[b]], r])
        co.append(c), tm.append(t), sr.append(r)
        so.append(so[-1] + len(r))
        at += n
    return np.concatenate(co), np.concatenate(tm), np.concatenate(sr).astype(np.int32), np.array(so, dtype=np.int64)


def delay_abi(eng, plan, S, with_times=True):
    """Both calls of the C ABI on a plan, every output the middle of a larger sentinel-filled buffer: nothing outside may be written,
    and everything inside must be.  -> (seg_offsets, coeffs (S', 8, 3), times (S',) | None, seg_rows (S',)) as NumPy."""
    import torch
    ragged = hasattr(plan, "seg_offsets")
    m = plan.max_m if ragged else plan.m
    so_in = plan.seg_offsets if ragged else None
    start = torch.as_tensor(np.ascontiguousarray(S, dtype=np.int32)).to(eng.device)
    so = torch.full((PAD + plan.B + 1 + PAD,), SENT_I, dtype=torch.int64, device=eng.device)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_delay_offsets_dev", _p(so_in), plan.B, m, _p(start), _p(so[PAD:]))
    so_h = so.cpu().numpy()
    assert (so_h[:PAD] == SENT_I).all() and (so_h[PAD + plan.B + 1:] == SENT_I).all()
    so_h = so_h[PAD:PAD + plan.B + 1].copy()
    n = int(so_h[-1])
    co = torch.full((PAD + 24 * n + PAD,), SENT_F, dtype=torch.float64, device=eng.device)
    tm = torch.full((PAD + n + PAD,), SENT_F, dtype=torch.float64, device=eng.device) if with_times else None
    sr = torch.full((PAD + n + PAD,), SENT_I, dtype=torch.int32, device=eng.device)
    eng.ctx.call("uavac_minsnap_delay_dev", _p(plan.coeffs), _p(plan.times) if with_times else None, _p(plan.seg_rows), _p(so_in), plan.B, m,
                 float(plan.dt), _p(start), _p(so[PAD:]), _p(co[PAD:]), _p(tm[PAD:]) if with_times else None, _p(sr[PAD:]))
    torch.cuda.synchronize()
    out = []
    for buf, width, sent in ((co, 24 * n, SENT_F), (tm, n, SENT_F), (sr, n, SENT_I)):
        if buf is None:
            out.append(None)
            continue
        h = buf.cpu().numpy()
        assert (h[:PAD] == sent).all() and (h[PAD + width:] == sent).all()
        out.append(h[PAD:PAD + width].copy())
    return so_h, out[0].reshape(n, 8, 3), out[1], out[2]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64 if a.dtype == np.float64 else a.dtype),
                                                                        b.view(np.int64 if b.dtype == np.float64 else b.dtype))


# ------------------------------------------------------------------------------------------------ 1: the arrays, through the C ABI
def test_the_delayed_arrays_equal_the_numpy_construction(eng):
    k = case(eng)
    plan = k["plan"]
    want = numpy_delay(plan.coeffs.cpu().numpy().reshape(B * M, 8, 3), plan.times.cpu().numpy().reshape(-1),
                       plan.seg_rows.cpu().numpy().reshape(-1), [M] * B, S_ROWS, DT)
    so, co, tm, sr = delay_abi(eng, plan, S_ROWS)
    assert np.array_equal(so, want[3]) and so[-1] == B * M + int((S_ROWS > 0).sum())
    assert same_bits(co, want[0]) and same_bits(tm, want[1]) and same_bits(sr, want[2])
    # the same plan as a ragged batch (the same coefficients bit for bit) gives the same result
    r = k["ragged"]
    assert same_bits(r.coeffs.cpu().numpy(), plan.coeffs.cpu().numpy().reshape(B * M, 8, 3))
    so_r, co_r, tm_r, sr_r = delay_abi(eng, r, S_ROWS)
    assert np.array_equal(so_r, so) and same_bits(co_r, co) and same_bits(tm_r, tm) and same_bits(sr_r, sr)
    # durations are optional: without them the other outputs are the same
    so_n, co_n, tm_n, sr_n = delay_abi(eng, plan, S_ROWS, with_times=False)
    assert tm_n is None and np.array_equal(so_n, so) and same_bits(co_n, co) and same_bits(sr_n, sr)
    # nobody delayed: a copy
    so_0, co_0, tm_0, sr_0 = delay_abi(eng, plan, np.zeros(B, dtype=np.int32))
    assert so_0.tolist() == list(range(0, B * M + 1, M)) and same_bits(co_0, plan.coeffs.cpu().numpy().reshape(B * M, 8, 3))
    assert same_bits(tm_0, plan.times.cpu().numpy().reshape(-1)) and same_bits(sr_0, plan.seg_rows.cpu().numpy().reshape(-1))
    assert eng.take_flags()[0] == 0
    # a truly ragged batch (segment counts 8 and 5 in turn), against the same construction
    wps = [w if b % 2 == 0 else w[:6] for b, w in enumerate(k["wps"][:12])]
    rb = eng.plan_ragged(wps, VEL, DT, rows=False)
    S = S_ROWS[:12][::-1].copy()
    want = numpy_delay(rb.coeffs.cpu().numpy(), rb.times.cpu().numpy(), rb.seg_rows.cpu().numpy(), np.diff(rb.seg_offsets_host), S, DT)
    so, co, tm, sr = delay_abi(eng, rb, S)
    assert np.array_equal(so, want[3]) and same_bits(co, want[0]) and same_bits(tm, want[1]) and same_bits(sr, want[2])


# ------------------------------------------------------------------------------------------------ 2: the rows
def test_the_delayed_rows_equal_delay_rows_of_the_products_own_rows(eng):
    import torch
    from uav_ac.scoring import delay_rows
    k = case(eng)
    plan, d = k["plan"], k["delayed"]
    want, want_ro = delay_rows(plan.traj.cpu().numpy(), plan.row_offsets.cpu().numpy(), S_ROWS, plan.first_yaw.cpu().numpy())
    assert d.B == B and d.max_m == M + 1 and d.free_times and d.waypoints is None and d.velocity == VEL and d.dt == DT
    assert np.array_equal(d.row_offsets.cpu().numpy(), want_ro) and d.total_rows == int(want_ro[-1]) == plan.total_rows + int(S_ROWS.sum())
    assert np.array_equal(d.seg_offsets.cpu().numpy(), d.seg_offsets_host)
    got = d.traj.cpu().numpy()
    for c in range(11):
        assert same_bits(got[:, c], want[:, c]), c
    assert torch.equal(eng.first_yaw(d), plan.first_yaw) and torch.equal(d.first_yaw, plan.first_yaw)
    assert torch.equal(d.start_positions, plan.waypoints[:, 0, :])
    # from the rows-free plan, from the ragged batch and from a device tensor of start rows: the same batch
    free = eng.plan(k["wps"], VEL, DT, rows=False)
    for src in (free, k["ragged"]):
        e = eng.delay(src, torch.as_tensor(S_ROWS).to(eng.device))
        assert e.traj is None and e.total_rows == d.total_rows
        assert torch.equal(e.coeffs, d.coeffs) and torch.equal(e.seg_rows, d.seg_rows) and torch.equal(e.times, d.times)
        assert torch.equal(e.row_offsets, d.row_offsets) and torch.equal(e.first_yaw, d.first_yaw)
    assert eng.take_flags()[0] == 0


# ------------------------------------------------------------------------------------------------ 3: the audit's clock
def test_the_audit_of_the_delayed_plan_equals_the_audit_with_start_rows(eng):
    k = case(eng)
    plan, d = k["plan"], k["delayed"]

    def same_audit(a, b):
        return same_bits(a.min_distance.cpu().numpy(), b.min_distance.cpu().numpy()) and np.array_equal(a.block.cpu().numpy(), b.block.cpu().numpy())

    with_rows = eng.separation(plan, 0.5, 32, start_rows=S_ROWS)
    assert same_audit(eng.separation(d, 0.5, 32), with_rows)
    assert not same_audit(eng.separation(plan, 0.5, 32), with_rows)          # (the delays matter on this set)
    stag = eng.stagger(plan, 0.5, 32)
    assert int((stag.steps > 0).sum()) > 0
    granted = eng.delay(plan, stag.start_rows)
    cleared = eng.separation(granted, 0.5, 32)
    assert same_audit(cleared, eng.separation(plan, 0.5, 32, start_rows=stag.start_rows))
    resolved = (stag.steps >= 0).cpu().numpy()
    assert (cleared.conflicts.cpu().numpy()[resolved] <= (~resolved).sum()).all()      # a resolved mission meets unresolved ones at most


# ------------------------------------------------------------------------------------------------ 4: the flight
def test_the_delayed_batch_flies_plan_fed_as_row_fed_and_as_the_oracle_flies_delayed_rows(eng):
    import torch
    from oracle import c_oracle as co
    from uav_ac.scoring import delay_rows
    k = case(eng)
    d = k["delayed"]
    free = eng.delay(k["plan"], S_ROWS)
    assert free.traj is None
    fed = eng.fleet(free)
    rowed = eng.fleet(d, from_plan=False)
    assert fed.from_plan and not rowed.from_plan
    F = int(fed.vehicle.inner_per_outer)
    K = (int(S_ROWS.max()) + 50) * F                         # every hold ends inside the launch
    slog, _ = fed.rollout(K, state_log=True)
    slog_r, _ = rowed.rollout(K, state_log=True)
    # (the vehicles' state is rows 0-25; rows 26-29 are the yaw scan that only a plan-fed fleet carries)
    assert torch.equal(fed.state[:26], rowed.state[:26]) and torch.equal(fed.istate, rowed.istate) and torch.equal(slog, slog_r)
    # a second fleet, flown from hold end to hold end: after S_b * F ticks the cursor of mission b is exactly S_b
    second = eng.fleet(free)
    S = torch.as_tensor(S_ROWS).to(eng.device)
    done = 0
    for s in sorted(set(S_ROWS.tolist()) - {0}):
        second.rollout(s * F - done)
        done = s * F
        assert bool((second.trajectory_index[S == s] == s).all()), s
    second.rollout(K - done)
    assert torch.equal(second.state, fed.state) and torch.equal(second.istate, fed.istate)
    got = slog.cpu().numpy()
    # spot missions against the scalar C oracle flown on delay_rows of the oracle's own rows
    for b in SPOTS:
        traj, _, _ = co.plan(k["wps"][b], VEL, DT)
        rows, _ = delay_rows(traj, [0, len(traj)], [S_ROWS[b]], [traj[0, 9]])
        state, istate = co.initial_state(rows[0, 0:3])
        s_ref, _ = co.rollout(rows, state, istate, K, log_cmd=False)
        err = col_err(got[:, :, b], s_ref)
        print(f"delayed flight, mission {b} (S = {S_ROWS[b]}): error against the oracle {err:.3e}")
        assert err < TOL, (b, err)


# ------------------------------------------------------------------------------------------------ 5: bad inputs
def test_bad_start_rows_are_clamped_and_flagged_and_a_full_mission_is_refused(eng):
    from oracle import minsnap_oracle as mo
    from uav_ac import _native as nat
    k = case(eng)
    plan = k["plan"]
    eng.take_flags()
    S = S_ROWS.copy()
    S[0], S[1] = -5, 2 ** 29 + 1
    so, co, tm, sr = delay_abi(eng, plan, S)
    flags = eng.take_flags()
    assert flags[0] == 1 and flags[1:] == [0, 0, 0]
    clamped = S.copy()
    clamped[0], clamped[1] = 0, 2 ** 29
    want = numpy_delay(plan.coeffs.cpu().numpy().reshape(B * M, 8, 3), plan.times.cpu().numpy().reshape(-1),
                       plan.seg_rows.cpu().numpy().reshape(-1), [M] * B, clamped, DT)
    assert np.array_equal(so, want[3]) and same_bits(co, want[0]) and same_bits(tm, want[1]) and same_bits(sr, want[2])
    assert so[1] - so[0] == M and so[2] - so[1] == M + 1 and sr[so[1]] == 2 ** 29 and tm[so[1]] == float(2 ** 29) * DT
    # m = 64: a delayed mission would need one more segment than a mission may have
    full = eng.plan(mo.synthetic_missions(2, nat.MAX_SEGMENTS), VEL, DT, rows=False)
    with pytest.raises(ValueError):
        eng.delay(full, [0, 1])
    with pytest.raises(nat.UavacError) as exc:
        delay_abi(eng, full, [0, 1])
    assert exc.value.code == nat.EINVAL
    # the other refusals: a wrong number of start rows, times without out_times, no start rows, a bad dt
    with pytest.raises(ValueError):
        eng.delay(plan, S_ROWS[:-1])
    import torch
    buf = torch.zeros((B * (M + 1) * 24,), dtype=torch.float64, device=eng.device)
    ibuf = torch.zeros((B * (M + 1),), dtype=torch.int32, device=eng.device)
    so_t = torch.zeros((B + 1,), dtype=torch.int64, device=eng.device)
    start = torch.zeros((B,), dtype=torch.int32, device=eng.device)
    for args in ((_p(plan.coeffs), _p(plan.times), _p(plan.seg_rows), None, B, M, DT, _p(start), _p(so_t), _p(buf), None, _p(ibuf)),
                 (_p(plan.coeffs), None, _p(plan.seg_rows), None, B, M, DT, _p(start), _p(so_t), _p(buf), _p(buf), _p(ibuf)),
                 (_p(plan.coeffs), None, _p(plan.seg_rows), None, B, M, DT, None, _p(so_t), _p(buf), None, _p(ibuf)),
                 (_p(plan.coeffs), None, _p(plan.seg_rows), None, B, M, 0.0, _p(start), _p(so_t), _p(buf), None, _p(ibuf)),
                 (_p(plan.coeffs), None, _p(plan.seg_rows), None, 0, M, DT, _p(start), _p(so_t), _p(buf), None, _p(ibuf))):
        with pytest.raises(nat.UavacError) as exc:
            eng.ctx.call("uavac_minsnap_delay_dev", *args)
        assert exc.value.code == nat.EINVAL
    assert eng.take_flags() == [0, 0, 0, 0]
