"""Per-UAV tracking scores of a scored rollout, read back and judged the way upstream's acceptance test does.

The scored rollouts (`Fleet.rollout(K, score=True)`, include/uavac.h uavac_control_rollout_scored_dev) accumulate, per UAV, over
the periods of `inner_per_outer` ticks that start with an outer update: how many of the mission's rows were scored, the next
row to score, the sum, sum of squares, maximum and last of e = |position - target row xyz| at the end of each period.  Upstream
checks one UAV from a full log (tests/integration/test_mujoco_trajectory_tracking.py:26-36): mean tracking error < 0.5 m, final
distance to the goal < 0.5 m, no collision.  `summarize` turns a score block into those quantities for every UAV at once and
`acceptance` applies upstream's three assertions.  Pure torch: works on device and on CPU tensors alike.

`plan_feasibility` is the judge BEFORE the flight: it compares a plan audit (`Engine.audit`, include/uavac.h
uavac_minsnap_audit_dev) with the flight limits the control law clips its targets to.  `retime_factors` says by how much each
mission has to be slowed down to pass it: the CPU statement of the rule the retiming kernel implements (include/uavac.h
uavac_minsnap_retime_factors_dev), NumPy on the host, bit for bit.

`separation_from_rows` is the same kind of statement for the fleet's audit against itself (`Engine.separation`, include/uavac.h
uavac_minsnap_separation_dev): closest approach, partner, clock row, conflicts inside a radius, recomputed from sampled rows in NumPy,
bit for bit; `separation_ok` judges a separation audit.  `conflicts_from_rows` states the audit's conflict LIST the same way
(`Engine.conflicts`, uavac_minsnap_conflicts_dev: every pair inside the radius, from when to when and how near), and `conflict_pairs`
turns such a list into its unique pairs.  `stagger_from_rows` states the rule of the call that acts on that audit
(`Engine.stagger`, uavac_minsnap_stagger_dev: start delays by priority) on sampled rows, and `stagger_ok` judges its result.
`delay_rows` states on sampled rows what the delay transform (`Engine.delay`, uavac_minsnap_delay_dev) makes of a plan and its start
rows, and `separation_from_log` is `separation_from_rows` for a FLIGHT: the rule of `Engine.flown_separation`
(uavac_flown_separation_dev) on the positions of a rollout's state log, `conflicts_from_log` likewise the rule of
`Engine.flown_conflicts` (uavac_flown_conflicts_dev: every pair the flight brought inside the radius), and `conflict_diff` sets a planned
and a flown list side by side: the pairs in both, only planned, only flown.  `layer_from_rows` states the rule of the second lever on
the audit (`Engine.layer`, uavac_minsnap_layer_dev: offset layers by priority at fixed starts), `layer_obstacles_from_rows` the same
search when it also refuses layers inside cuboids (uavac_minsnap_layer_obs_dev), `layer_ok` and `blocked_out` judge the result, and
`shift_coeffs` states the transform that makes granted offsets part of the plan (`Engine.shift`, uavac_minsnap_shift_dev).
`audit_from_log` is the plan audit of a FLIGHT: the rule of `Engine.flown_audit` (uavac_flown_audit_dev) on a rollout's state log --
valid ticks, flown peaks, and per cuboid hits and closest approach --, and `flight_feasibility` judges it as `plan_feasibility` judges a plan.
`demand_from_rows` states what a plan ASKS of the vehicle -- specific thrust, bank, roll / pitch rate, rows that ask for thrust downward,
and per cuboid the planned clearance: the rule of `Engine.demand` (uavac_minsnap_demand_dev) on sampled rows and jerk --,
`demand_feasibility` judges it against what the vehicle can give, and `audit_gap` sets it beside the flight audit of the same missions.
`envelope_from_rows` states every mission's swept box (`Engine.envelope`, uavac_minsnap_envelope_dev), `airspaces_from_envelopes` the
split of a fleet into groups whose boxes can never come within a radius of each other, round for round (`Engine.airspaces`,
uavac_fleet_airspaces_dev), and `airspace_order` the order that puts each of them side by side: what `airspaces=True` on the searches runs on.
"""
from __future__ import annotations

import numpy as np

from . import _native as nat

# score rows (include/uavac.h): callers read 0-5; 6-10 carry a period a launch ended inside of
COUNT, NEXT_ROW, SUM, SUMSQ, MAX, LAST = range(6)


def summarize(score, istate, nrows) -> dict:
    """score [SCORE_ROWS][B] f64, istate [ISTATE_ROWS][B] i32, nrows (B,) rows per mission -> dict of (B,) tensors:
    rows_scored, complete (next_row == nrows), mean_error, rms_error, max_error (NaN where nothing was scored), final_error
    (the last period's error once complete, NaN before), collided (the sticky obstacle flag, or a ground contact after take-off,
    as uav_ac.main.fly_mission counts it)."""
    import torch
    if score.dim() != 2 or score.shape[0] != nat.SCORE_ROWS:
        raise ValueError(f"score must be [{nat.SCORE_ROWS}][B], got {tuple(score.shape)}")
    B = score.shape[1]
    if istate.shape[-1] != B:
        raise ValueError("istate and score hold different batch sizes")
    s = score.to(torch.float64)
    nrows = torch.as_tensor(nrows, device=s.device).to(torch.float64).reshape(-1)
    if nrows.numel() != B:
        raise ValueError("one row count per UAV")
    count = s[COUNT]
    nan = torch.full_like(count, float("nan"))
    scored = count > 0
    safe = torch.where(scored, count, torch.ones_like(count))
    complete = (s[NEXT_ROW] == nrows) & (nrows > 0)
    ist = istate.to(s.device)
    collided = (ist[2] != 0) | ((ist[3] & nat.GROUND_HIT_AFTER_TAKEOFF) != 0)
    return {
        "rows_scored": count.to(torch.int64),
        "complete": complete,
        "mean_error": torch.where(scored, s[SUM] / safe, nan),
        "rms_error": torch.where(scored, torch.sqrt(s[SUMSQ] / safe), nan),
        "max_error": torch.where(scored, s[MAX], nan),
        "final_error": torch.where(complete, s[LAST], nan),
        "collided": collided,
    }


def acceptance(summary: dict, mean_tol: float = 0.5, final_tol: float = 0.5) -> dict:
    """Upstream's three assertions per UAV (test_mujoco_trajectory_tracking.py:26-36) -> dict of (B,) bool tensors:
    mean_ok (mean tracking error < mean_tol), final_ok (complete and final distance < final_tol), no_collision, and passed
    (all three).  A NaN error fails its assertion."""
    mean_ok = summary["mean_error"] < mean_tol
    final_ok = summary["complete"] & (summary["final_error"] < final_tol)
    no_collision = ~summary["collided"]
    return {"mean_ok": mean_ok, "final_ok": final_ok, "no_collision": no_collision, "passed": mean_ok & final_ok & no_collision}


def plan_feasibility(audit, vehicle=None, slack: float = 0.0) -> dict:
    """A plan audit (`Engine.audit` -> PlanAudit, or anything with its fields; device or CPU tensors) against the limits the control
    law silently clips what the planner asks for to (csrc/control_law.h: target climb rate, target horizontal velocity, horizontal
    acceleration command) -> dict of (B,) bool tensors:
    speed_ok (speed_xy <= max_speed_xy + slack), ascent_ok (ascent <= max_ascent + slack), descent_ok (descent <= max_descent +
    slack), accel_ok (accel_xy <= max_horiz_accel + slack), clear (no sample inside any cuboid; all true when none was given),
    feasible (all five).  A NaN peak -- a mission with a non-finite sample, i.e. a singular plan -- fails every test, `clear`
    included.  `vehicle`: a `Vehicle` (or anything with the four limits); None = `uavac_vehicle_default`."""
    import torch
    V = nat.Vehicle.default() if vehicle is None else vehicle
    slack = float(slack)
    speed_ok = audit.speed_xy <= float(V.max_speed_xy) + slack
    ascent_ok = audit.ascent <= float(V.max_ascent) + slack
    descent_ok = audit.descent <= float(V.max_descent) + slack
    accel_ok = audit.accel_xy <= float(V.max_horiz_accel) + slack
    finite = ~(torch.isnan(audit.speed_xy) | torch.isnan(audit.ascent) | torch.isnan(audit.descent) | torch.isnan(audit.accel_xy))
    hits = getattr(audit, "hit_rows", None)
    clear = finite.clone()
    if hits is not None and hits.numel() > 0:
        clear = clear & (hits.reshape(-1, finite.shape[0]) == 0).all(dim=0).to(finite.device)
    return {"speed_ok": speed_ok, "ascent_ok": ascent_ok, "descent_ok": descent_ok, "accel_ok": accel_ok, "clear": clear,
            "feasible": speed_ok & ascent_ok & descent_ok & accel_ok & clear}


DEFAULT_RETIME_MARGIN = 1e-3     # see `retime_factors`; the default of `Engine.retime`


def _host(x, dtype=np.float64) -> np.ndarray:
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=dtype)


def _host_i64(x) -> np.ndarray:
    """offsets and start rows: flat int64"""
    return _host(x, np.int64).reshape(-1)


NEED_TILT, NEED_UPRIGHT, NEED_THRUST_MAX, NEED_THRUST_MIN = range(nat.NEED_ROWS)                # need rows (include/uavac.h)
# the terms of the extended retiming rule, in the order `binding` counts them: the audit's four, then the need block's four
BINDING_NAMES = ("speed_xy", "ascent", "descent", "accel_xy", "tilt", "upright", "thrust_max", "thrust_min")


def demand_limits(vehicle=None):
    """g, max_tilt, Fmax = 4 max_thrust / mass, Fmin = 4 min_thrust / mass (specific thrust, m/s^2) of a `Vehicle` (anything with g,
    max_tilt, mass, max_thrust, min_thrust; None = `uavac_vehicle_default`) -> four floats: the HOST array `demand_limits` of
    `uavac_minsnap_need_dev`, checked as the library checks it (ValueError)."""
    V = nat.Vehicle.default() if vehicle is None else vehicle
    g, tau, mass = float(V.g), float(V.max_tilt), float(V.mass)
    if not (np.isfinite(mass) and mass > 0.0):
        raise ValueError("mass must be finite and > 0")
    hi, lo = (4.0 * float(V.max_thrust)) / mass, (4.0 * float(V.min_thrust)) / mass
    if not (np.isfinite(g) and g > 0.0 and np.isfinite(tau) and tau > 0.0):
        raise ValueError("g and max_tilt must be finite and > 0")
    if not (np.isfinite(hi) and hi > g):
        raise ValueError("the vehicle cannot hover: 4 max_thrust / mass must be finite and > g")
    if not (0.0 <= lo < g):
        raise ValueError("4 min_thrust / mass must be in [0, g)")
    D, E = hi * hi - g * g, g * g - lo * lo
    if not (np.isfinite(D) and D > 0.0 and E > 0.0):
        raise ValueError("thrust limits too close to g")
    return g, tau, hi, lo


def need_from_rows(rows, row_offsets, vehicle=None):
    """The slowdown factor each of the vehicle's tilt and thrust limits asks for, per mission, recomputed from SAMPLED rows -- the
    SPECIFICATION of `uavac_minsnap_need_dev` (csrc/minsnap_need.hip), which is tested against it bit for bit.  NumPy on the host.
    `rows` (N, 11) as the sampler writes them, missions back to back; `row_offsets` (B + 1,); `vehicle` as `demand_limits` takes it.

    Slowing a mission by k > 1 leaves its curve in place and divides its accelerations by u = k^2.  With tau = max_tilt, t2 = tau tau,
    D = Fmax Fmax - g g, E = g g - Fmin Fmin (each one rounded operation), per row, every product, sum, difference, fmax and sqrt one
    rounded operation, in this order:
        xx = ax ax; yy = ay ay; h = xx + yy; A = h + az az; gz = g az
        q  = fmax(fmax(xx - t2 h, yy - t2 h), 0)
        T  = q > 0 ? tau az + sqrt(q) : -inf                tilt:       ax^2 / n2 <= tau^2 and ay^2 / n2 <= tau^2  <=>  u >= T / (tau g)
        U  = az                                             upright:    g u - az >= 0                              <=>  u >= U / g
        H  = sqrt(gz gz + A D) - gz                         thrust max: n2(u) <= Fmax^2                            <=>  u >= H / D
        d  = gz gz - A E
        Lo = (az > 0 and d >= 0) ? gz + sqrt(d) : -inf      thrust min: n2(u) >= Fmin^2 on the interval that reaches to infinity
    and per mission (fmax over its rows from -inf; division by a positive constant is monotone, so it comes once, after the maximum):
        need = sqrt(fmax([max T / (tau g), max U / g, max H / D, max Lo / E], 0))
    -> (NEED_ROWS, B) f64: 0 tilt, 1 upright, 2 thrust_max, 3 thrust_min; hover gives 0, 0, 0, 0.  A mission with a non-finite position,
    velocity or acceleration, and one without rows: NaN in all four -- the audit's rule: a singular plan never looks feasible.
    Known edge: a row in exact free fall with min_thrust = 0 gives upright = 1 and asks for no slowdown, although `demand_feasibility`
    calls it inverted; with min_thrust > 0 the thrust_min row covers it."""
    rows = _host(rows)
    ro = _host_i64(row_offsets)
    B = len(ro) - 1
    if rows.ndim != 2 or rows.shape[1] != nat.TRAJ_COLS:
        raise ValueError(f"rows must be (N, {nat.TRAJ_COLS})")
    if B < 1 or ro[0] != 0 or ro[-1] != len(rows) or (np.diff(ro) < 0).any():
        raise ValueError("row_offsets must ascend from 0 to the number of rows")
    g, tau, hi, lo = demand_limits(vehicle)
    t2, tg, D, E = tau * tau, tau * g, hi * hi - g * g, g * g - lo * lo
    ax, ay, az = rows[:, 6], rows[:, 7], rows[:, 8]
    with np.errstate(all="ignore"):
        xx, yy = ax * ax, ay * ay
        h = xx + yy
        A = h + az * az
        gz = g * az
        q = np.fmax(np.fmax(xx - t2 * h, yy - t2 * h), 0.0)
        T = np.where(q > 0.0, tau * az + np.sqrt(q), -np.inf)
        H = np.sqrt(gz * gz + A * D) - gz
        d = gz * gz - A * E
        Lo = np.where((az > 0.0) & (d >= 0.0), gz + np.sqrt(d), -np.inf)
    finite = np.isfinite(rows[:, 0:9]).all(axis=1)
    need = np.full((nat.NEED_ROWS, B), np.nan)
    over = np.array([tg, g, D, E])
    for b in range(B):
        s = slice(int(ro[b]), int(ro[b + 1]))
        if s.start == s.stop or not finite[s].all():
            continue
        peaks = np.array([np.fmax.reduce(x[s], initial=-np.inf) for x in (T, az, H, Lo)])
        with np.errstate(invalid="ignore"):
            need[:, b] = np.sqrt(np.fmax(peaks / over, 0.0))
    return need


def retime_factors(audit, vehicle=None, margin: float = DEFAULT_RETIME_MARGIN, velocities=None, need=None) -> dict:
    """By how much each mission of an audited plan must be slowed down to stay inside the limits the control law clips its targets
    to -- the SPECIFICATION of `uavac_minsnap_retime_factors_dev` (csrc/minsnap_retime.hip), which is tested against it bit for bit.
    `audit`: a PlanAudit (or anything with speed_xy, ascent, descent, accel_xy), or the (AUDIT_ROWS, B) block itself; tensors (any
    device) or arrays.  `vehicle`: anything with the four limits; None = `uavac_vehicle_default`.

    Scaling every segment duration of a mission by k > 1 -- planning it at velocity / k -- leaves the minimum-snap curve where it is,
    p'(t) = p(t / k): velocity peaks scale by 1 / k, acceleration peaks by 1 / k^2.  Per mission, every step ONE rounded IEEE
    operation (NumPy's elementwise float64 division, sqrt and fmax are exactly that):
        r = max(speed_xy / max_speed_xy, ascent / max_ascent, descent / max_descent, sqrt(accel_xy / max_horiz_accel))
        a NaN among the four peaks (a singular plan, a mission without rows) -> factor NaN, velocity untouched
        r <= 1                                                               -> factor 1.0, velocity untouched bit for bit
        otherwise                                      k = r / (1 - margin)  -> factor k,   velocity / k
    `margin` in [0, 1): the audit's peaks are maxima over SAMPLES and the slower plan is sampled elsewhere on the curve, so its
    sampled peaks can exceed peak / k by the relative gap between sampled and continuous maxima -- about 1e-4 on the bench
    distribution (3 m legs at 3 m/s) at dt = 0.01, growing with dt.  With a margin above the gap one pass suffices; the default 1e-3
    costs 0.1 % of cruise speed.
    -> dict of host arrays / ints: factors (B,) f64, retimed (B,) bool, nan (B,) bool, n_retimed, n_nan -- the kernel's two counters
    -- and, when `velocities` (B,) was given, velocities (B,) f64: the new ones.

    `need`: None (the four limits only, as ever), or the (NEED_ROWS, B) block of `Engine.need` / `need_from_rows`, or a PlanNeed, made
    with the same `vehicle` -- then the SPECIFICATION of `uavac_minsnap_retime_demand_factors_dev`: with r_audit the maximum above,
        r = fmax(r_audit, fmax(fmax(need[0], need[1]), fmax(need[2], need[3])))
    a NaN in either block gives factor NaN, and the dict gains `binding` (B,) i32: the index into `BINDING_NAMES` of the FIRST term that
    attains r, -1 for a NaN mission; given for every mission, also where r <= 1 (the nearest limit)."""
    V = nat.Vehicle.default() if vehicle is None else vehicle
    limits = [float(V.max_speed_xy), float(V.max_ascent), float(V.max_descent), float(V.max_horiz_accel)]
    margin = float(margin)
    if not all(np.isfinite(x) and x > 0.0 for x in limits):
        raise ValueError("every flight limit must be finite and > 0")
    if not (0.0 <= margin < 1.0):
        raise ValueError("margin must be in [0, 1)")
    if hasattr(audit, "speed_xy"):
        peaks = [_host(audit.speed_xy), _host(audit.ascent), _host(audit.descent), _host(audit.accel_xy)]
    else:
        block = _host(audit)
        if block.ndim != 2 or block.shape[0] != nat.AUDIT_ROWS:
            raise ValueError(f"an audit block is [{nat.AUDIT_ROWS}][B], got {block.shape}")
        peaks = [block[1], block[2], block[3], block[4]]
    speed_xy, ascent, descent, accel_xy = (p.reshape(-1) for p in peaks)
    nan = np.isnan(speed_xy) | np.isnan(ascent) | np.isnan(descent) | np.isnan(accel_xy)
    binding = None
    with np.errstate(invalid="ignore"):
        terms = [speed_xy / limits[0], ascent / limits[1], descent / limits[2], np.sqrt(accel_xy / limits[3])]
        r = np.fmax(np.fmax(terms[0], terms[1]), np.fmax(terms[2], terms[3]))
        if need is not None:
            block = _host(need.block if hasattr(need, "block") else need)
            if block.shape != (nat.NEED_ROWS, len(speed_xy)):
                raise ValueError(f"a need block is [{nat.NEED_ROWS}][B] with the audit's B = {len(speed_xy)}, got {block.shape}")
            nan = nan | np.isnan(block).any(axis=0)
            terms += list(block)
            r = np.fmax(r, np.fmax(np.fmax(block[0], block[1]), np.fmax(block[2], block[3])))
            binding = np.where(nan, -1, np.argmax(np.stack(terms) == r, axis=0)).astype(np.int32)      # argmax of bools: the first True
        retimed = ~nan & (r > 1.0)
        k = r / (1.0 - margin)
    factors = np.where(nan, np.nan, np.where(retimed, k, 1.0))
    out = {"factors": factors, "retimed": retimed, "nan": nan, "n_retimed": int(retimed.sum()), "n_nan": int(nan.sum())}
    if binding is not None:
        out["binding"] = binding
    if velocities is not None:
        v = _host(velocities).reshape(-1).copy()
        v[retimed] = v[retimed] / factors[retimed]
        out["velocities"] = v
    return out


SEP_PARTNER, SEP_ROW, SEP_CONFLICTS, SEP_FIRST_CONFLICT, SEP_COMPARED = range(nat.SEP_ROWS)      # isep rows (include/uavac.h)
_MAX_CLOCK = 1 << 29                                                                           # the largest start row the shared clock takes


def _radius(radius) -> float:
    radius = float(radius)
    if not (np.isfinite(radius) and radius >= 0.0):
        raise ValueError("radius must be finite and >= 0")
    return radius


def _group_offsets(group_offsets, B) -> np.ndarray:
    """(G + 1,) offsets that ascend from 0 to B; None = one group of all B"""
    go = np.array([0, B], dtype=np.int64) if group_offsets is None else _host_i64(group_offsets)
    if len(go) < 2 or go[0] != 0 or go[-1] != B or (np.diff(go) < 0).any():
        raise ValueError("group_offsets must ascend from 0 to B")
    return go


def _start_rows(start_rows, B, upper=_MAX_CLOCK) -> np.ndarray:
    """(B,) start rows clamped to 0 .. `upper` (the searches; None: from below only, the separation audit); None = all 0"""
    S = np.zeros(B, dtype=np.int64) if start_rows is None else np.clip(_host_i64(start_rows), 0, upper)
    if len(S) != B:
        raise ValueError("one start row per mission")
    return S


def _included(pos, N, longest=_MAX_CLOCK) -> np.ndarray:
    """(B,) bool: mission b has rows -- at most `longest` (the searches; None: no such term, the separation audit) -- and every
    position pos(b) (N_b, 3) is finite.  Everybody else is EXCLUDED."""
    return np.array([N[b] > 0 and (longest is None or N[b] <= longest) and bool(np.isfinite(pos(b)).all()) for b in range(len(N))],
                    dtype=bool)


def _at(pos, k, s):
    """where a mission with positions `pos` (N, 3) and start row s stands at the clock rows k: it waits on its first row, holds its last"""
    return pos[np.clip(k - s, 0, len(pos) - 1)]


def _inside_any(own, partners, r2) -> bool:
    """is the candidate `own` (H, 3) inside the radius of any decided partner (n, H, 3) at any clock row?"""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (own[None, :, c] - partners[:, :, c] for c in range(3))
        return bool(((dx * dx + dy * dy) + dz * dz < r2).any())


def _max_group(max_group, narrow) -> int:
    """the group limit of a search rule: the narrow call's constant, or the caller's number (>= 1)"""
    if max_group is None:
        return narrow
    if int(max_group) < 1:
        raise ValueError("max_group must be >= 1")
    return int(max_group)


def _prioritised_search(N, included, go, max_group, max_steps, pos, start, r2, blocked=None, committed=None):
    """The search the stagger and the layer rules share.  Candidate q of mission i stands at the positions pos(i, q) (N_i, 3) from
    start row start(i, q) on; per group the included missions in ascending index examine q = 0 .. max_steps against the GRANTED
    candidates of the missions decided before them (candidate 0 for an unresolved one), up to the horizon max(every partner's end,
    the candidate's own end).  `blocked(i, q)`: refused before anybody is compared -- and then the first of a group is examined too.
    pos is only called for a candidate that is compared with somebody, and for a partner's granted one.
    `committed(g)`: the (key, candidate) pairs that count as decided before the group's first mission -- the TRAFFIC of the
    `*_against_rows` rules; a key is B or above, N, pos and start know it, and it is never examined itself.  The group limit counts
    the group's own missions only.
    -> steps (-2: not examined, -1: unresolved), earlier, refused candidates: (B,) each."""
    B = len(included)
    steps, earlier, refused = np.full(B, -2), np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    for g in range(len(go) - 1):
        g0, g1 = int(go[g]), int(go[g + 1])
        if g1 - g0 > max_group:
            continue
        done = [] if committed is None else list(committed(g))                       # (mission, granted candidate) of the included missions decided so far
        for i in range(g0, g1):
            if not included[i]:
                continue
            n, earlier[i], steps[i] = int(N[i]), len(done), -1
            if done:
                h_prev = max(start(j, c) + int(N[j]) for j, c in done)
                k = np.arange(max(h_prev, start(i, max_steps) + n))
                partners = np.stack([_at(pos(j, c), k, start(j, c)) for j, c in done])                # (n, h_max, 3)
            for q in range(max_steps + 1):
                if blocked is not None and blocked(i, q):
                    refused[i] += 1
                    continue
                if done:
                    H = max(h_prev, start(i, q) + n)
                    if _inside_any(_at(pos(i, q), k[:H], start(i, q)), partners[:, :H], r2):
                        continue
                steps[i] = q
                break
            done.append((i, max(int(steps[i]), 0)))
    return steps, earlier, refused


def separation_from_rows(rows, row_offsets, radius, group_offsets=None, start_rows=None):
    """The separation audit recomputed from SAMPLED rows -- the SPECIFICATION of `uavac_minsnap_separation_dev`
    (csrc/minsnap_separation.hip), which is tested against it bit for bit.  NumPy on the host.
    `rows` (N, >= 3): positions in columns 0-2, missions back to back; `row_offsets` (B + 1,); `group_offsets` (G + 1,) or None = one
    group; `start_rows` (B,) or None = all 0 (a negative one counts as 0).

    The missions of a group share a row clock k = 0, 1, ...; mission b stands at its own row clamp(k - S_b, 0, N_b - 1) -- it waits on
    its first row before its start and holds its last row after its end -- and every pair of the group is compared at every k below
    the horizon H_g = max(S_b + N_b).  A mission without rows or with a position that is not finite (what a non-finite coefficient
    gives) is EXCLUDED: compared with nobody, it reports NaN / -1 / -1 / 0 / -1 / 0.  Rounding and ties as the kernel has them: d^2 =
    (dx * dx + dy * dy) + dz * dz with separately rounded products and sums, the minimum taken of the squares, one sqrt at the end, r^2 =
    radius * radius, inside means d^2 < r^2 strictly, and the minimum is the lexicographic one of (d^2, clock row, partner index).
    -> (sep (B,) f64, isep (SEP_ROWS, B) i32): minimum distance (+inf: nobody to compare with); partner, clock row of the minimum (-1
    with +inf / NaN), conflicts (partners that come inside the radius), first clock row with a partner inside (-1: none), compared."""
    rows = _host(rows)
    ro = _host_i64(row_offsets)
    B = len(ro) - 1
    radius = _radius(radius)
    go = _group_offsets(group_offsets, B)
    S = _start_rows(start_rows, B, upper=None)
    r2 = radius * radius
    N = np.diff(ro)
    pos = [rows[ro[b]:ro[b + 1], 0:3] for b in range(B)]
    included = _included(pos.__getitem__, N, longest=None)
    sep = np.full(B, np.nan)
    isep = np.zeros((nat.SEP_ROWS, B), dtype=np.int32)
    isep[[SEP_PARTNER, SEP_ROW, SEP_FIRST_CONFLICT]] = -1
    for g in range(len(go) - 1):
        members = [b for b in range(int(go[g]), int(go[g + 1])) if included[b]]
        if not members:
            continue
        k = np.arange(int(max(S[b] + N[b] for b in members)))
        P = np.stack([_at(pos[b], k, S[b]) for b in members])                            # (n, H, 3): where everybody stands at clock row k
        idx = np.asarray(members)
        for a, b in enumerate(members):
            isep[SEP_COMPARED, b] = len(members) - 1
            if len(members) == 1:
                sep[b] = np.inf
                continue
            others = np.delete(np.arange(len(members)), a)
            dx, dy, dz = (P[a, :, c][:, None] - P[others, :, c].T for c in range(3))     # (H, n - 1): rows first, partners ascending
            d2 = (dx * dx + dy * dy) + dz * dz
            flat = int(np.argmin(d2))                                                     # the first minimum: lowest row, then lowest partner
            row, j = divmod(flat, len(others))
            sep[b] = np.sqrt(d2[row, j])
            isep[SEP_PARTNER, b], isep[SEP_ROW, b] = idx[others[j]], row
            inside = d2 < r2
            isep[SEP_CONFLICTS, b] = int(inside.any(axis=0).sum())
            hit_rows = np.flatnonzero(inside.any(axis=1))
            isep[SEP_FIRST_CONFLICT, b] = hit_rows[0] if len(hit_rows) else -1
    return sep, isep


def conflicts_from_rows(rows, row_offsets, radius, group_offsets=None, start_rows=None):
    """The conflict list recomputed from SAMPLED rows -- the SPECIFICATION of `uavac_minsnap_conflict_offsets_dev` and
    `uavac_minsnap_conflicts_dev` (csrc/minsnap_conflicts.hip), which are tested against it bit for bit.  NumPy on the host; inputs,
    clock, groups, excluded missions and rounding exactly as in `separation_from_rows`.
    Mission i lists every included mission j of its group with d^2(i, j, k) < r^2, strictly, at some clock row k below the group's
    horizon, in ascending j; an excluded mission lists nothing and is listed by nobody.
    -> (offsets (B + 1,) i64, pair_d (E,) f64, pair_i (CONF_ROWS, E) i32): the entries of mission i are [offsets[i], offsets[i + 1]);
    per entry the pair's minimum distance over the clock (the minimum of the squares, one sqrt), and the partner, the first and the
    last clock row inside, the number of rows inside, the clock row of the minimum (the lowest one on a tie)."""
    rows = _host(rows)
    ro = _host_i64(row_offsets)
    B = len(ro) - 1
    radius = _radius(radius)
    go = _group_offsets(group_offsets, B)
    S = _start_rows(start_rows, B, upper=None)
    r2 = radius * radius
    N = np.diff(ro)
    pos = [rows[ro[b]:ro[b + 1], 0:3] for b in range(B)]
    included = _included(pos.__getitem__, N, longest=None)
    per_mission = [[] for _ in range(B)]                                                  # (partner, first, last, inside, row of the minimum, d^2)
    for g in range(len(go) - 1):
        members = [b for b in range(int(go[g]), int(go[g + 1])) if included[b]]
        if len(members) < 2:
            continue
        k = np.arange(int(max(S[b] + N[b] for b in members)))
        P = np.stack([_at(pos[b], k, S[b]) for b in members])                            # (n, H, 3): where everybody stands at clock row k
        for a, i in enumerate(members):
            dx, dy, dz = (P[a, :, c][None, :] - P[:, :, c] for c in range(3))            # (n, H): partners first, rows ascending
            d2 = (dx * dx + dy * dy) + dz * dz
            inside = d2 < r2
            inside[a] = False                                                             # nobody is their own partner
            for c in np.flatnonzero(inside.any(axis=1)):
                hit = np.flatnonzero(inside[c])
                low = int(np.argmin(d2[c]))                                               # the first minimum: the lowest row
                per_mission[i].append((members[c], hit[0], hit[-1], len(hit), low, d2[c, low]))
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in per_mission])]).astype(np.int64)
    flat = [e for p in per_mission for e in p]
    pair_i = np.array([e[:5] for e in flat], dtype=np.int32).reshape(-1, nat.CONF_ROWS).T.copy()
    pair_d = np.sqrt(np.array([e[5] for e in flat], dtype=np.float64))
    return offsets, pair_d, pair_i


def conflict_pairs(cl) -> dict:
    """A conflict list (`Engine.conflicts` -> ConflictList, or anything with its fields; tensors on any device or arrays) -> the unique
    pairs i < j on the host, in ascending (i, j): dict of (n,) arrays `i`, `j`, `first_row`, `last_row`, `rows_inside`, `min_row`,
    `min_distance`.  The distance is bit-symmetric, so both directions of a pair must be listed and carry the same record: a list
    in which they do not is a ValueError."""
    off = _host_i64(cl.offsets)
    owner = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))
    partner = _host_i64(cl.partner)
    fields = {"first_row": _host_i64(cl.first_row), "last_row": _host_i64(cl.last_row), "rows_inside": _host_i64(cl.rows_inside),
              "min_row": _host_i64(cl.min_row), "min_distance": _host(cl.min_distance).reshape(-1)}
    if len(partner) != len(owner) or any(len(v) != len(owner) for v in fields.values()):
        raise ValueError("a conflict list holds offsets[-1] entries in every field")
    fwd, bwd = np.flatnonzero(owner < partner), np.flatnonzero(owner > partner)
    if len(fwd) + len(bwd) != len(owner):
        raise ValueError("a mission lists itself")
    fwd = fwd[np.lexsort((partner[fwd], owner[fwd]))]
    bwd = bwd[np.lexsort((owner[bwd], partner[bwd]))]
    if len(fwd) != len(bwd) or not (np.array_equal(owner[fwd], partner[bwd]) and np.array_equal(partner[fwd], owner[bwd])):
        raise ValueError("a pair is listed in one direction only")
    for name, v in fields.items():
        if not np.array_equal(v[fwd], v[bwd]):
            raise ValueError(f"the two directions of a pair disagree in {name}")
    return {"i": owner[fwd], "j": partner[fwd], **{name: v[fwd] for name, v in fields.items()}}


def separation_ok(sep, group_sizes=None) -> dict:
    """A separation audit (`Engine.separation` -> SeparationAudit, or anything with `min_distance`, `conflicts` and `compared`; tensors
    on any device or arrays) -> dict of (B,) bool host arrays: `clear` (nobody comes inside the radius: conflicts == 0), `complete`
    (the mission was compared with every other mission of its group: compared == size - 1; needs `group_sizes`, the size of each
    mission's group, (B,) or one number -- without it `complete` is all False) and `ok` (both).  A mission whose minimum distance is NaN
    -- an excluded one: no rows, or a singular plan -- fails all three: a plan that was not checked never looks clear."""
    dist = _host(sep.min_distance).reshape(-1)
    conflicts = _host(sep.conflicts).reshape(-1)
    compared = _host(sep.compared).reshape(-1)
    finite = ~np.isnan(dist)
    clear = finite & (conflicts == 0)
    if group_sizes is None:
        complete = np.zeros(len(dist), dtype=bool)
    else:
        sizes = np.broadcast_to(_host(group_sizes).reshape(-1), dist.shape) if np.size(group_sizes) == 1 else \
            _host(group_sizes).reshape(-1)
        if len(sizes) != len(dist):
            raise ValueError("one group size per mission (or one number)")
        complete = finite & (compared == sizes - 1)
    return {"clear": clear, "complete": complete, "ok": clear & complete}


def separation_from_log(log, radius, group_offsets=None):
    """The separation the fleet FLEW, recomputed from a state log -- the SPECIFICATION of `uavac_flown_separation_dev`
    (csrc/flown_separation.hip), which is tested against it bit for bit.  NumPy on the host.
    `log` (K, >= 3, B): the positions in rows 0-2 of every tick, as `Fleet.rollout(K, state_log=True)` returns them (a view at another
    pitch is fine: only columns 0 .. B - 1 exist here); `group_offsets` (G + 1,) or None = one group.

    The clock is the tick k = 0 .. K - 1.  For vehicle i and a partner j != i of its group: d^2 = (dx * dx + dy * dy) + dz * dz with
    separately rounded products and sums, r^2 = radius * radius, inside means d^2 < r^2 strictly.  A pair-tick is VALID iff its d^2 is not
    NaN.  The minimum is the lexicographic one of (d^2, tick, partner index) over the valid pair-ticks, one sqrt at the end.
    -> (sep (B,) f64, isep (SEP_ROWS, B) i32): minimum distance; partner, tick of the minimum, conflicts (partners with a valid pair-tick
    inside the radius), first tick with a partner inside (-1: none), compared (partners with at least one valid pair-tick).  No valid
    pair-tick at all -- a group of one, a vehicle that is NaN throughout --: +inf and -1 / -1 / 0 / -1 / 0."""
    log = _host(log)
    if log.ndim != 3 or log.shape[0] < 1 or log.shape[1] < 3 or log.shape[2] < 1:
        raise ValueError("log must have shape (K, >= 3, B) with K >= 1 and B >= 1")
    K, B = log.shape[0], log.shape[2]
    radius = _radius(radius)
    go = _group_offsets(group_offsets, B)
    r2 = radius * radius
    sep = np.full(B, np.inf)
    isep = np.zeros((nat.SEP_ROWS, B), dtype=np.int32)
    isep[[SEP_PARTNER, SEP_ROW, SEP_FIRST_CONFLICT]] = -1
    for g in range(len(go) - 1):
        g0, g1 = int(go[g]), int(go[g + 1])
        if g1 - g0 < 2:
            continue
        P = np.ascontiguousarray(log[:, 0:3, g0:g1])                                       # (K, 3, n): ticks first, partners ascending
        for a in range(g1 - g0):
            others = np.delete(np.arange(g1 - g0), a)
            with np.errstate(invalid="ignore", over="ignore"):
                dx, dy, dz = (P[:, c, a][:, None] - P[:, c, others] for c in range(3))     # (K, n - 1)
                d2 = (dx * dx + dy * dy) + dz * dz
            valid = ~np.isnan(d2)
            if not valid.any():
                continue
            b = g0 + a
            flat = int(np.argmin(np.where(valid, d2, np.inf)))                             # the first minimum: lowest tick, then lowest partner
            tick, j = divmod(flat, len(others))
            if valid[tick, j]:
                sep[b] = np.sqrt(d2[tick, j])
                isep[SEP_PARTNER, b], isep[SEP_ROW, b] = g0 + others[j], tick
            inside = d2 < r2
            isep[SEP_CONFLICTS, b] = int(inside.any(axis=0).sum())
            hit = np.flatnonzero(inside.any(axis=1))
            isep[SEP_FIRST_CONFLICT, b] = hit[0] if len(hit) else -1
            isep[SEP_COMPARED, b] = int(valid.any(axis=0).sum())
    return sep, isep


def conflicts_from_log(log, radius, group_offsets=None):
    """The conflict list of a FLIGHT, recomputed from a state log -- the SPECIFICATION of `uavac_flown_conflict_offsets_dev` and
    `uavac_flown_conflicts_dev` (csrc/flown_conflicts.hip), which are tested against it bit for bit.  NumPy on the host; the log, the
    clock (the tick), the groups, the rounding and the validity rule exactly as in `separation_from_log`: d^2 = (dx * dx + dy * dy) +
    dz * dz with separately rounded products and sums, inside means d^2 < r^2 strictly, a pair-tick is VALID iff its d^2 is not NaN.
    Vehicle i lists every vehicle j != i of its group that has a valid pair-tick inside the radius, in ascending j; a vehicle whose log
    is NaN throughout lists nothing and is listed by nobody, and a NaN tick in the middle of an incursion is not inside.
    -> (offsets (B + 1,) i64, pair_d (E,) f64, pair_i (CONF_ROWS, E) i32), the shape of `conflicts_from_rows`: the entries of vehicle i
    are [offsets[i], offsets[i + 1]); per entry the pair's minimum distance over its valid pair-ticks (the minimum of the squares, one
    sqrt), and the partner, the first and the last tick inside, the number of ticks inside, the tick of the minimum (the lowest one on
    a tie)."""
    log = _host(log)
    if log.ndim != 3 or log.shape[0] < 1 or log.shape[1] < 3 or log.shape[2] < 1:
        raise ValueError("log must have shape (K, >= 3, B) with K >= 1 and B >= 1")
    B = log.shape[2]
    radius = _radius(radius)
    go = _group_offsets(group_offsets, B)
    r2 = radius * radius
    per_vehicle = [[] for _ in range(B)]                                                  # (partner, first, last, inside, tick of the minimum, d^2)
    for g in range(len(go) - 1):
        g0, g1 = int(go[g]), int(go[g + 1])
        if g1 - g0 < 2:
            continue
        P = np.ascontiguousarray(log[:, 0:3, g0:g1])                                       # (K, 3, n): ticks first, partners ascending
        for a in range(g1 - g0):
            with np.errstate(invalid="ignore", over="ignore"):
                dx, dy, dz = (P[:, c, a][:, None] - P[:, c, :] for c in range(3))          # (K, n)
                d2 = (dx * dx + dy * dy) + dz * dz
                inside = d2 < r2                                                           # (a NaN is never below anything)
            inside[:, a] = False                                                           # nobody is their own partner
            for c in np.flatnonzero(inside.any(axis=0)):
                hit = np.flatnonzero(inside[:, c])
                low = int(np.argmin(np.where(np.isnan(d2[:, c]), np.inf, d2[:, c])))       # the first minimum over the valid ticks
                per_vehicle[g0 + a].append((g0 + c, hit[0], hit[-1], len(hit), low, d2[low, c]))
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in per_vehicle])]).astype(np.int64)
    flat = [e for p in per_vehicle for e in p]
    pair_i = np.array([e[:5] for e in flat], dtype=np.int32).reshape(-1, nat.CONF_ROWS).T.copy()
    pair_d = np.sqrt(np.array([e[5] for e in flat], dtype=np.float64))
    return offsets, pair_d, pair_i


def _pairs_of(cl) -> dict:
    """a conflict list or the dict `conflict_pairs` made of one -> that dict"""
    return cl if isinstance(cl, dict) else conflict_pairs(cl)


def conflict_diff(planned, flown, inner_per_outer: int = 1) -> dict:
    """Did tracking error create this conflict?  Two conflict lists over the same batch -- `planned` from `Engine.conflicts` (clock rows),
    `flown` from `Engine.flown_conflicts` (ticks); each a ConflictList or the dict `conflict_pairs` gives -- compared by their unique
    pairs i < j on the host.  -> dict of
      `both`          (n, 2) i64: the pairs in both lists, ascending, with `flown_first_tick` (n,) the flown list's first tick inside and
                      `planned_first_tick` (n,) the planned list's first row x `inner_per_outer` (the tick at which that row is due),
      `only_planned`  (n, 2): planned conflicts the flight did not have,
      `only_flown`    (n, 2): conflicts the plan did not have -- tracking error (or a plan other than the one flown) produced them."""
    F = int(inner_per_outer)
    if F < 1:
        raise ValueError("inner_per_outer must be >= 1")
    p, f = _pairs_of(planned), _pairs_of(flown)
    pk = {(int(i), int(j)): int(r) for i, j, r in zip(p["i"], p["j"], p["first_row"])}
    fk = {(int(i), int(j)): int(r) for i, j, r in zip(f["i"], f["j"], f["first_row"])}
    both = sorted(set(pk) & set(fk))

    def pairs(keys):
        return np.array(sorted(keys), dtype=np.int64).reshape(-1, 2)
    return {"both": pairs(both), "flown_first_tick": np.array([fk[k] for k in both], dtype=np.int64),
            "planned_first_tick": np.array([pk[k] * F for k in both], dtype=np.int64),
            "only_planned": pairs(set(pk) - set(fk)), "only_flown": pairs(set(fk) - set(pk))}


def audit_from_log(log, cuboids=None):
    """What the vehicles DID against the flight limits and the cuboids, recomputed from a state log -- the SPECIFICATION of
    `uavac_flown_audit_dev` (csrc/flown_audit.hip), which is tested against it bit for bit.  NumPy on the host.
    `log` (K, 13, B): x y z | q0 q1 q2 q3 | vx vy vz | p q r per tick, as `Fleet.rollout(K, state_log=True)` returns it (a view at
    another pitch is fine: only columns 0 .. B - 1 exist here); `cuboids` (n, 6) xmin xmax ymin ymax zmin zmax, or None = none.

    A tick of a vehicle is VALID iff its 13 values are finite; everything below is over a vehicle's valid ticks.  Products and sums are
    separately rounded, a maximum is taken of the squares, one sqrt comes last.
    -> dict of host arrays: `audit` (FLOWN_AUDIT_ROWS, B) f64 -- 0 the valid ticks, 1 sqrt(max(vx vx + vy vy)), 2 max(-vz), 3 max(vz),
    4 sqrt(max((vx vx + vy vy) + vz vz)), 5 max |2 (q1 q3 + q0 q2)|, 6 max |2 (q2 q3 - q0 q1)|, 7 sqrt(max((p p + q q) + r r)) --,
    `first_bad` (B,) i32 the first invalid tick (-1: none), and per cuboid (n, B): `hit_ticks` i32 the valid ticks inside it (inclusive
    test), `first_hit` i32 the first of them (-1: none), `clearance` f64 = sqrt of the smallest d2 = (ex ex + ey ey) + ez ez with
    ex = where(px < xmin, xmin - px, where(px > xmax, px - xmax, 0)), ..., and `clearance_tick` i32 the FIRST tick at which it is
    attained.  A vehicle without a valid tick: 0 ticks, NaN peaks, first_bad 0, no hits, first_hit -1, clearance NaN, tick -1."""
    log = _host(log)
    if log.ndim != 3 or log.shape[0] < 1 or log.shape[1] != nat.STATE_LOG_ROWS or log.shape[2] < 1:
        raise ValueError(f"log must have shape (K, {nat.STATE_LOG_ROWS}, B) with K >= 1 and B >= 1")
    K, B = log.shape[0], log.shape[2]
    cub = np.zeros((0, 6)) if cuboids is None else _host(cuboids)
    if cub.size % 6 or (cub.ndim == 2 and cub.shape[1] != 6):
        raise ValueError("cuboids must be (n, 6): xmin xmax ymin ymax zmin zmax")
    cub = cub.reshape(-1, 6)
    n = len(cub)
    if n > nat.AUDIT_MAX_CUBOIDS:
        raise ValueError(f"{n} cuboids; at most {nat.AUDIT_MAX_CUBOIDS} per audit")
    valid = np.isfinite(log).all(axis=1)                                                   # (K, B)
    px, py, pz, q0, q1, q2, q3, vx, vy, vz, p, q, r = (log[:, i, :] for i in range(nat.STATE_LOG_ROWS))
    with np.errstate(invalid="ignore", over="ignore"):
        vxy2 = vx * vx + vy * vy
        per_tick = (vxy2, -vz, vz, vxy2 + vz * vz, np.abs(2.0 * (q1 * q3 + q0 * q2)), np.abs(2.0 * (q2 * q3 - q0 * q1)),
                    (p * p + q * q) + r * r)
    any_valid = valid.any(axis=0)
    audit = np.full((nat.FLOWN_AUDIT_ROWS, B), np.nan)
    audit[0] = valid.sum(axis=0)
    for row, (values, root) in enumerate(zip(per_tick, (True, False, False, True, False, False, True)), start=1):
        peak = np.where(valid, values, -np.inf).max(axis=0)
        plus_zero = (valid & (values == 0.0) & ~np.signbit(values)).any(axis=0)            # the maximum of -0.0 and +0.0 is +0.0
        peak = np.where((peak == 0.0) & plus_zero, 0.0, peak)
        with np.errstate(invalid="ignore"):
            audit[row] = np.where(any_valid, np.sqrt(peak) if root else peak, np.nan)
    bad = ~valid
    first_bad = np.where(bad.any(axis=0), bad.argmax(axis=0), -1).astype(np.int32)
    hit_ticks = np.zeros((n, B), dtype=np.int32)
    first_hit = np.full((n, B), -1, dtype=np.int32)
    clearance = np.full((n, B), np.nan)
    clearance_tick = np.full((n, B), -1, dtype=np.int32)
    for c, (x0, x1, y0, y1, z0, z1) in enumerate(cub):
        with np.errstate(invalid="ignore", over="ignore"):
            inside = valid & (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1) & (pz >= z0) & (pz <= z1)
            ex = np.where(px < x0, x0 - px, np.where(px > x1, px - x1, 0.0))
            ey = np.where(py < y0, y0 - py, np.where(py > y1, py - y1, 0.0))
            ez = np.where(pz < z0, z0 - pz, np.where(pz > z1, pz - z1, 0.0))
            d2 = (ex * ex + ey * ey) + ez * ez
        hit_ticks[c] = inside.sum(axis=0)
        first_hit[c] = np.where(inside.any(axis=0), inside.argmax(axis=0), -1)
        for b in np.flatnonzero(any_valid):
            ticks = np.flatnonzero(valid[:, b])
            at = ticks[int(np.argmin(d2[ticks, b]))]                                       # the first minimum: the lowest tick
            clearance[c, b], clearance_tick[c, b] = np.sqrt(d2[at, b]), at
    return {"audit": audit, "first_bad": first_bad, "hit_ticks": hit_ticks, "first_hit": first_hit, "clearance": clearance,
            "clearance_tick": clearance_tick}


def flight_feasibility(audit, K, vehicle=None, slack: float = 0.0) -> dict:
    """A flight audit (`Engine.flown_audit` -> FlightAudit, or anything with its fields; tensors on any device or arrays) of a log of
    `K` ticks against the limits `plan_feasibility` judges a plan by -> dict of (B,) bool host arrays:
    complete (every tick is valid: ticks == K), speed_ok (speed_xy <= max_speed_xy + slack), ascent_ok (ascent <= max_ascent + slack),
    descent_ok (descent <= max_descent + slack), tilt_ok (bank_x and bank_y <= max_tilt + slack), clear (no valid tick inside any
    cuboid; all true when none was given), flown_ok (complete, the three limits and clear).  `tilt_ok` is reported but is not part of
    `flown_ok`: the control law clips the attitude COMMAND, not the attitude.  A NaN peak -- a vehicle without a valid tick -- fails
    every test, `clear` included.  `vehicle`: a `Vehicle` (or anything with the four limits); None = `uavac_vehicle_default`."""
    V = nat.Vehicle.default() if vehicle is None else vehicle
    slack = float(slack)
    ticks, speed_xy, ascent, descent = (_host(getattr(audit, f)).reshape(-1) for f in ("ticks", "speed_xy", "ascent", "descent"))
    bank_x, bank_y = _host(audit.bank_x).reshape(-1), _host(audit.bank_y).reshape(-1)
    with np.errstate(invalid="ignore"):
        complete = ticks == float(int(K))
        speed_ok = speed_xy <= float(V.max_speed_xy) + slack
        ascent_ok = ascent <= float(V.max_ascent) + slack
        descent_ok = descent <= float(V.max_descent) + slack
        tilt_ok = (bank_x <= float(V.max_tilt) + slack) & (bank_y <= float(V.max_tilt) + slack)
    clear = ~(np.isnan(speed_xy) | np.isnan(ascent) | np.isnan(descent))
    hits = getattr(audit, "hit_ticks", None)
    if hits is not None:
        hits = _host(hits, np.int64)
        if hits.size:
            clear = clear & (hits.reshape(-1, len(ticks)) == 0).all(axis=0)
    return {"complete": complete, "speed_ok": speed_ok, "ascent_ok": ascent_ok, "descent_ok": descent_ok, "tilt_ok": tilt_ok,
            "clear": clear, "flown_ok": complete & speed_ok & ascent_ok & descent_ok & clear}


DEMAND_ROWS_TOTAL, DEMAND_THRUST_MAX, DEMAND_THRUST_MIN, DEMAND_BANK_X, DEMAND_BANK_Y, DEMAND_BODY_RATE = range(nat.DEMAND_ROWS)
DEMAND_INVERTED, DEMAND_FIRST_INVERTED = range(nat.IDEMAND_ROWS)                                # idemand rows (include/uavac.h)


def demand_from_rows(rows, jerk, row_offsets, g, cuboids=None):
    """What a plan asks of the vehicle, recomputed from SAMPLED rows and jerk -- the SPECIFICATION of `uavac_minsnap_demand_dev`
    (csrc/minsnap_demand.hip), which is tested against it bit for bit.  NumPy on the host.
    `rows` (N, 11): x y z | vx vy vz | ax ay az | yaw | spline, missions back to back, as the sampler writes them; `jerk` (N, 3) as
    `Engine.sample_derivatives` gives it; `row_offsets` (B + 1,); `g` the gravitational acceleration (`vehicle.g`), finite and > 0;
    `cuboids` (n, 6) xmin xmax ymin ymax zmin zmax, or None = none.

    Per row, every product, sum, quotient and fmax one rounded operation, in this order (NED: hover has fz = g):
        fz = g - az;  n2 = (ax ax + ay ay) + fz fz;  bx2 = n2 > 0 ? (ax ax) / n2 : 0, by2 likewise with ay
        jj = (jx jx + jy jy) + jz jz;  jf = (jx ax + jy ay) - jz fz;  w2 = n2 > 0 ? fmax(jj - (jf jf) / n2, 0) / n2 : 0
        inverted = fz <= 0;  per cuboid ex, ey, ez and d2 = (ex ex + ey ey) + ez ez exactly as `audit_from_log` defines them
    n2 is the specific thrust a perfectly tracked row needs, squared; bx2 and by2 the squares of the bank command the control law would
    form (csrc/control_law.h: acx / acc_z before its clamp to max_tilt); w2 the square of the roll / pitch rate the curve demands (the
    jerk across the thrust direction over the thrust; no yaw rate).  A maximum or minimum is taken of the SQUARES (fmax / fmin: a NaN
    that overflow makes of finite samples is dropped) and one sqrt comes last; on a tie the lowest row wins.
    -> dict of host arrays: `demand` (DEMAND_ROWS, B) f64 -- 0 the row total, 1 sqrt(max n2), 2 sqrt(min n2), 3 sqrt(max bx2), 4
    sqrt(max by2), 5 sqrt(max w2) --, `idemand` (IDEMAND_ROWS, B) i32 -- 0 the inverted rows, 1 the mission-local index of the first one
    (-1: none) --, and per cuboid (n, B): `clearance` f64 = sqrt(min d2) (0 inside or on a face) and `clearance_row` i32 the FIRST row
    that attains it.  A mission with a non-finite position, velocity, acceleration or jerk, and one without rows: NaN in rows 1-5,
    clearance NaN, every index -1, 0 inverted rows -- the plan audit's rule: a singular plan never looks feasible."""
    rows, jerk = _host(rows), _host(jerk)
    ro = _host_i64(row_offsets)
    B = len(ro) - 1
    if rows.ndim != 2 or rows.shape[1] != nat.TRAJ_COLS or jerk.shape != (rows.shape[0], 3):
        raise ValueError(f"rows must be (N, {nat.TRAJ_COLS}) and jerk (N, 3)")
    if B < 1 or ro[0] != 0 or ro[-1] != len(rows) or (np.diff(ro) < 0).any():
        raise ValueError("row_offsets must ascend from 0 to the number of rows")
    g = float(g)
    if not (np.isfinite(g) and g > 0.0):
        raise ValueError("g must be finite and > 0")
    cub = np.zeros((0, 6)) if cuboids is None else _host(cuboids)
    if cub.size % 6 or (cub.ndim == 2 and cub.shape[1] != 6):
        raise ValueError("cuboids must be (n, 6): xmin xmax ymin ymax zmin zmax")
    cub = cub.reshape(-1, 6)
    n = len(cub)
    if n > nat.AUDIT_MAX_CUBOIDS:
        raise ValueError(f"{n} cuboids; at most {nat.AUDIT_MAX_CUBOIDS} per call")
    px, py, pz = rows[:, 0], rows[:, 1], rows[:, 2]
    ax, ay, az = rows[:, 6], rows[:, 7], rows[:, 8]
    jx, jy, jz = jerk[:, 0], jerk[:, 1], jerk[:, 2]
    with np.errstate(all="ignore"):
        fz = g - az
        xx, yy = ax * ax, ay * ay
        n2 = (xx + yy) + fz * fz
        some = n2 > 0.0
        over = np.where(some, n2, 1.0)
        bx2, by2 = np.where(some, xx / over, 0.0), np.where(some, yy / over, 0.0)
        jj = (jx * jx + jy * jy) + jz * jz
        jf = (jx * ax + jy * ay) - jz * fz
        w2 = np.where(some, np.fmax(jj - (jf * jf) / over, 0.0) / over, 0.0)
        inverted = fz <= 0.0
        d2 = np.empty((n, len(rows)))
        for c, (x0, x1, y0, y1, z0, z1) in enumerate(cub):
            ex = np.where(px < x0, x0 - px, np.where(px > x1, px - x1, 0.0))
            ey = np.where(py < y0, y0 - py, np.where(py > y1, py - y1, 0.0))
            ez = np.where(pz < z0, z0 - pz, np.where(pz > z1, pz - z1, 0.0))
            d2[c] = (ex * ex + ey * ey) + ez * ez
    finite = np.isfinite(rows[:, 0:9]).all(axis=1) & np.isfinite(jerk).all(axis=1)
    demand = np.full((nat.DEMAND_ROWS, B), np.nan)
    idemand = np.zeros((nat.IDEMAND_ROWS, B), dtype=np.int32)
    idemand[DEMAND_FIRST_INVERTED] = -1
    clearance = np.full((n, B), np.nan)
    clearance_row = np.full((n, B), -1, dtype=np.int32)
    demand[DEMAND_ROWS_TOTAL] = np.diff(ro)
    for b in range(B):
        s = slice(int(ro[b]), int(ro[b + 1]))
        if s.start == s.stop or not finite[s].all():
            continue
        with np.errstate(invalid="ignore"):
            demand[1:, b] = np.sqrt([np.fmax.reduce(n2[s]), np.fmin.reduce(n2[s]), np.fmax.reduce(bx2[s]), np.fmax.reduce(by2[s]),
                                     np.fmax.reduce(w2[s])])
        upside = np.flatnonzero(inverted[s])
        idemand[:, b] = (len(upside), upside[0] if len(upside) else -1)
        for c in range(n):
            at = int(np.argmin(d2[c, s]))                                                  # the first minimum: the lowest row
            clearance[c, b], clearance_row[c, b] = np.sqrt(d2[c, s][at]), at
    return {"demand": demand, "idemand": idemand, "clearance": clearance, "clearance_row": clearance_row}


_DEMAND_FIELDS = ("rows", "thrust_max", "thrust_min", "bank_x", "bank_y", "body_rate")


def _demand_columns(demand) -> dict:
    """A PlanDemand (or anything with its fields; tensors on any device or arrays), or the dict `demand_from_rows` gives -> its columns
    as host arrays under PlanDemand's names."""
    if isinstance(demand, dict):
        block, iblock = _host(demand["demand"]), _host(demand["idemand"], np.int64)
        if block.ndim != 2 or block.shape[0] != nat.DEMAND_ROWS or iblock.shape != (nat.IDEMAND_ROWS, block.shape[1]):
            raise ValueError(f"a demand block is [{nat.DEMAND_ROWS}][B] and its integer block [{nat.IDEMAND_ROWS}][B]")
        out = dict(zip(_DEMAND_FIELDS, block))
        out.update(inverted_rows=iblock[DEMAND_INVERTED], first_inverted=iblock[DEMAND_FIRST_INVERTED],
                   clearance=_host(demand["clearance"]), clearance_row=_host(demand["clearance_row"], np.int64))
    else:
        out = {f: _host(getattr(demand, f)).reshape(-1) for f in _DEMAND_FIELDS}
        out.update(inverted_rows=_host(demand.inverted_rows, np.int64).reshape(-1),
                   first_inverted=_host(demand.first_inverted, np.int64).reshape(-1), clearance=_host(demand.clearance),
                   clearance_row=_host(demand.clearance_row, np.int64))
    B = len(out["rows"])
    out["clearance"] = out["clearance"].reshape(-1, B)
    out["clearance_row"] = out["clearance_row"].reshape(-1, B)
    return out


def demand_feasibility(demand, vehicle=None, slack: float = 0.0, min_clearance: float = 0.0) -> dict:
    """A plan demand (`Engine.demand` -> PlanDemand, anything with its fields, or the dict `demand_from_rows` gives; tensors on any
    device or arrays) against what the vehicle can give -> dict of (B,) bool host arrays:
    thrust_ok (mass thrust_max <= 4 max_thrust + slack and mass thrust_min >= 4 min_thrust - slack: four rotors, newtons), tilt_ok
    (bank_x and bank_y <= max_tilt + slack: the bank command the control law clips, csrc/control_law.h), upright (no row asks for
    thrust downward), clear (every clearance > min_clearance, strictly: at 0 a sample is inside a cuboid or on a face; all true when no
    cuboid was given), demand_ok (all four).  A NaN -- a mission with a non-finite sample or without rows -- fails every test, `upright`
    and `clear` included.  `vehicle`: a `Vehicle` (or anything with mass, min_thrust, max_thrust and max_tilt); None =
    `uavac_vehicle_default`.  `plan_feasibility` judges the other four limits."""
    V = nat.Vehicle.default() if vehicle is None else vehicle
    slack, min_clearance = float(slack), float(min_clearance)
    d = _demand_columns(demand)
    mass = float(V.mass)
    with np.errstate(invalid="ignore"):
        thrust_ok = (mass * d["thrust_max"] <= 4.0 * float(V.max_thrust) + slack) & \
                    (mass * d["thrust_min"] >= 4.0 * float(V.min_thrust) - slack)
        tilt_ok = (d["bank_x"] <= float(V.max_tilt) + slack) & (d["bank_y"] <= float(V.max_tilt) + slack)
        finite = ~(np.isnan(d["thrust_max"]) | np.isnan(d["thrust_min"]) | np.isnan(d["bank_x"]) | np.isnan(d["bank_y"]))
        upright = finite & (d["inverted_rows"] == 0)
        clear = finite & (d["clearance"] > min_clearance).all(axis=0)
    return {"thrust_ok": thrust_ok, "tilt_ok": tilt_ok, "upright": upright, "clear": clear,
            "demand_ok": thrust_ok & tilt_ok & upright & clear}


def audit_gap(demand, flight) -> dict:
    """Did tracking error eat the clearance, or was it planned that tight?  A plan demand (`Engine.demand`, or the dict of
    `demand_from_rows`) beside the flight audit of the same missions and cuboids (`Engine.flown_audit` -> FlightAudit, anything with
    bank_x, bank_y and clearance, or the dict of `audit_from_log`), on the host -> dict of
      `bank_excess`         (2, B) f64: flown bank - demanded bank, about x and about y (the flight banked more than a perfect track needs),
      `clearance_lost`      (n, B) f64: planned - flown clearance per cuboid (positive: the flight passed nearer than the plan),
      `hit_in_flight_only`  (n, B) bool: flown clearance 0 while the planned one is > 0.
    A NaN on either side gives NaN, and False in `hit_in_flight_only`.  Different batch sizes or cuboid counts are a ValueError."""
    d = _demand_columns(demand)
    B = len(d["rows"])
    if isinstance(flight, dict):
        block = _host(flight["audit"])
        f_bank, f_clear = np.stack([block[5], block[6]]), _host(flight["clearance"])
    else:
        f_bank, f_clear = np.stack([_host(flight.bank_x).reshape(-1), _host(flight.bank_y).reshape(-1)]), _host(flight.clearance)
    if f_bank.shape != (2, B):
        raise ValueError(f"the demand holds {B} missions, the flight audit {f_bank.shape[-1]} vehicles")
    f_clear = f_clear.reshape(-1, B)
    if f_clear.shape != d["clearance"].shape:
        raise ValueError(f"the demand holds {len(d['clearance'])} cuboids, the flight audit {len(f_clear)}")
    with np.errstate(invalid="ignore"):
        return {"bank_excess": f_bank - np.stack([d["bank_x"], d["bank_y"]]), "clearance_lost": d["clearance"] - f_clear,
                "hit_in_flight_only": (f_clear == 0.0) & (d["clearance"] > 0.0)}


def delay_rows(rows, row_offsets, start_rows, first_yaw):
    """The delay transform on SAMPLED rows -- the rule `uavac_minsnap_delay_dev` (csrc/minsnap_delay.hip) is tested against: the rows the
    sampler writes for the delayed plan.  NumPy on the host.
    `rows` (N, 11), missions back to back; `row_offsets` (B + 1,); `start_rows` (B,), clamped to 0 .. 2^29; `first_yaw` (B,): each
    mission's first heading (`plan.first_yaw`, `Engine.first_yaw`).
    Mission b becomes S_b HOLD rows followed by its own rows.  A hold row holds the position of the mission's row 0 (which is c0 of its
    first segment exactly), zero velocity and zero acceleration, the yaw first_yaw[b] and spline id 0 -- NOT row 0 repeated: a solved
    mission's row 0 carries velocities of rounding size.  The mission's own rows keep every bit; with S_b > 0 their spline ids move up
    by one.  A mission without rows cannot be delayed from rows (ValueError).
    -> (rows' (N + sum S, 11) f64, row_offsets' (B + 1,) i64)."""
    rows = _host(rows)
    ro = _host_i64(row_offsets)
    B = len(ro) - 1
    S = np.clip(_host_i64(start_rows), 0, _MAX_CLOCK)
    fy = _host(first_yaw).reshape(-1)
    if len(S) != B or len(fy) != B:
        raise ValueError("one start row and one first heading per mission")
    out_ro = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(np.diff(ro) + S, out=out_ro[1:])
    out = np.zeros((int(out_ro[-1]), rows.shape[1]), dtype=np.float64)
    for b in range(B):
        own = rows[ro[b]:ro[b + 1]]
        at = int(out_ro[b])
        if S[b] > 0:
            if len(own) == 0:
                raise ValueError(f"mission {b} has no rows: its hold position is not among the rows")
            out[at:at + S[b], 0:3] = own[0, 0:3]
            out[at:at + S[b], 9] = fy[b]
        out[at + S[b]:int(out_ro[b + 1])] = own
        if S[b] > 0:
            out[at + S[b]:int(out_ro[b + 1]), 10] += 1.0
    return out, out_ro


STAG_START, STAG_STEPS, STAG_EARLIER = range(nat.STAGGER_ROWS)                                   # istag rows (include/uavac.h)


def stagger_from_rows(rows, row_offsets, radius, group_offsets=None, start_rows=None, step=1, max_steps=255, max_group=None):
    """Prioritised deconfliction by start delay, decided on SAMPLED rows -- the SPECIFICATION of `uavac_minsnap_stagger_dev`
    (csrc/minsnap_stagger.hip), which is tested against it exactly.  NumPy on the host.
    `rows`, `row_offsets`, `radius`, `group_offsets` as `separation_from_rows` takes them, and the clock, the excluded missions and
    the arithmetic are the same: mission b with start s stands at its own row clamp(k - s, 0, N_b - 1); d^2 = (dx * dx + dy * dy) +
    dz * dz; r^2 = radius * radius; inside means d^2 < r^2 strictly.  `start_rows` (B,) or None = all 0: the BASE starts S_b, clamped
    to 0 .. 2^29.

    Per group the included missions in ascending batch index -- the priority: the lowest index is never delayed.  Mission i examines
    the candidates q = 0, 1, ..., max_steps in that order, candidate q with start s = S_i + q * step; it is clear iff for every
    included mission j < i of the group at its granted start T_j and every clock row k in [0, max(s + N_i, T_j + N_j)) the two are
    not inside the radius (past that row both hold their last rows: any longer horizon gives the same answer).  The first clear
    candidate is granted: T_i = s, steps = q; if none is clear the mission is unresolved: steps = -1, T_i = S_i, and it remains a
    partner for every later mission.  An excluded mission, and every mission of a group of more than STAGGER_MAX_GROUP, is not
    examined: its clamped base start, steps = -2, earlier = 0; nobody is checked against an excluded mission.
    `max_group`: a number sets that limit instead -- the SPECIFICATION of `uavac_minsnap_stagger_wide_dev` with `group_cap` = max_group
    (the rule itself has no size limit); None = STAGGER_MAX_GROUP.
    -> istag (STAGGER_ROWS, B) i32: the granted start row; steps; earlier (how many missions it was checked against)."""
    rows = _host(rows)
    ro = _host_i64(row_offsets)
    B = len(ro) - 1
    radius, step, max_steps = float(radius), int(step), int(max_steps)
    radius = _radius(radius)
    if step < 1 or not (0 <= max_steps <= nat.STAGGER_MAX_STEPS) or step * max_steps > _MAX_CLOCK:
        raise ValueError(f"step must be >= 1, max_steps in 0 .. {nat.STAGGER_MAX_STEPS}, step * max_steps at most 2^29")
    go = _group_offsets(group_offsets, B)
    S = _start_rows(start_rows, B)
    N = np.diff(ro)
    pos = [rows[ro[b]:ro[b + 1], 0:3] for b in range(B)]
    # the candidate is a start row: the mission's own rows from S_i + q * step on, up to the horizon of that candidate
    steps, earlier, _ = _prioritised_search(N, _included(pos.__getitem__, N), go, _max_group(max_group, nat.STAGGER_MAX_GROUP), max_steps, lambda i, q: pos[i],
                                            lambda i, q: int(S[i]) + q * step, radius * radius)
    istag = np.zeros((nat.STAGGER_ROWS, B), dtype=np.int32)
    istag[STAG_START], istag[STAG_STEPS], istag[STAG_EARLIER] = S + np.maximum(steps, 0) * step, steps, earlier
    return istag


def _traffic_side(traffic_rows, traffic_row_offsets, group_offsets, traffic_group_offsets, traffic_start_rows, go, upper=_MAX_CLOCK,
                  longest=_MAX_CLOCK):
    """The TRAFFIC of the `*_against_rows` rules, a second plan on sampled rows: `traffic_rows` (Nt, >= 3), `traffic_row_offsets`
    (Bt + 1,) -- Bt may be 0 --, `traffic_start_rows` (Bt,) or None = all 0, clamped like the plan's, `traffic_group_offsets` (G + 1,)
    ascending from 0 to Bt: group g of the plan meets group g of the traffic and nobody else's, so both sides give offsets, with the
    same G, or neither does (one group each); anything else is a ValueError.
    -> (pos: list of (N_j, 3), N (Bt,), S (Bt,), offsets (G + 1,), included (Bt,) bool)."""
    rows = _host(traffic_rows)
    rows = rows if rows.ndim == 2 else rows.reshape(-1, 3)                                # (no traffic at all: an empty array of any shape)
    ro = _host_i64(traffic_row_offsets)
    Bt = len(ro) - 1
    if Bt < 0:
        raise ValueError("traffic_row_offsets hold at least one entry")
    if (group_offsets is None) != (traffic_group_offsets is None):
        raise ValueError("group_offsets and traffic_group_offsets go together: both or none")
    tgo = _group_offsets(traffic_group_offsets, Bt)
    if len(tgo) != len(go):
        raise ValueError(f"the plan has {len(go) - 1} groups, the traffic {len(tgo) - 1}")
    S = _start_rows(traffic_start_rows, Bt, upper)
    N = np.diff(ro)
    pos = [rows[ro[b]:ro[b + 1], 0:3] for b in range(Bt)]
    return pos, N, S, tgo, _included(pos.__getitem__, N, longest)


def separation_against_rows(rows, row_offsets, traffic_rows, traffic_row_offsets, radius, group_offsets=None, traffic_group_offsets=None,
                            start_rows=None, traffic_start_rows=None):
    """The CROSS audit recomputed from sampled rows -- the SPECIFICATION of `uavac_minsnap_separation_against_dev`
    (csrc/minsnap_separation_against.hip), which is tested against it bit for bit.  NumPy on the host.
    `rows`, `row_offsets`, `radius`, `group_offsets`, `start_rows` as `separation_from_rows` takes them: the PLAN.  `traffic_rows`,
    `traffic_row_offsets`, `traffic_group_offsets`, `traffic_start_rows`: the TRAFFIC, a second plan on the same dt (`_traffic_side`:
    group g of the plan meets group g of the traffic; offsets on both sides or on neither).

    Every mission of the plan is compared with every included traffic mission of its group, and with nobody else: never with another
    mission of the plan.  The clock is `separation_from_rows`': a mission on either side stands at its own row clamp(k - S, 0, N - 1),
    and k runs below the horizon H_g = max(S + N) over the included missions of BOTH sides of the group.  Excluded missions (no rows,
    or a position that is not finite) as there: excluded traffic is nobody's partner and is not counted, an excluded plan mission
    reports NaN / -1 / -1 / 0 / -1 / 0.  A plan mission whose group has no included traffic reports +inf / -1 / -1 / 0 / -1 / 0.
    Arithmetic and ties as there: d^2 = (dx * dx + dy * dy) + dz * dz, the lexicographic minimum of (d^2, clock row, partner), one
    sqrt last, inside means d^2 < r^2 strictly.
    -> (sep (B,) f64, isep (SEP_ROWS, B) i32) with the layout of `separation_from_rows`: partner = the TRAFFIC batch index; the clock
    row of the minimum; conflicts = the traffic missions that come inside the radius; the first clock row with one inside; compared =
    the included traffic missions of the group."""
    rows = _host(rows)
    ro = _host_i64(row_offsets)
    B = len(ro) - 1
    radius = _radius(radius)
    go = _group_offsets(group_offsets, B)
    S = _start_rows(start_rows, B, upper=None)
    r2 = radius * radius
    N = np.diff(ro)
    pos = [rows[ro[b]:ro[b + 1], 0:3] for b in range(B)]
    included = _included(pos.__getitem__, N, longest=None)
    tpos, tN, tS, tgo, tinc = _traffic_side(traffic_rows, traffic_row_offsets, group_offsets, traffic_group_offsets, traffic_start_rows, go,
                                            upper=None, longest=None)
    sep = np.full(B, np.nan)
    isep = np.zeros((nat.SEP_ROWS, B), dtype=np.int32)
    isep[[SEP_PARTNER, SEP_ROW, SEP_FIRST_CONFLICT]] = -1
    for g in range(len(go) - 1):
        members = [b for b in range(int(go[g]), int(go[g + 1])) if included[b]]
        partners = [j for j in range(int(tgo[g]), int(tgo[g + 1])) if tinc[j]]
        if not members:
            continue
        if not partners:
            sep[members] = np.inf
            continue
        k = np.arange(int(max(max(S[b] + N[b] for b in members), max(tS[j] + tN[j] for j in partners))))
        T = np.stack([_at(tpos[j], k, tS[j]) for j in partners])                         # (n, H, 3): where the traffic stands at clock row k
        for b in members:
            own = _at(pos[b], k, S[b])
            dx, dy, dz = (own[:, c][:, None] - T[:, :, c].T for c in range(3))            # (H, n): rows first, partners ascending
            d2 = (dx * dx + dy * dy) + dz * dz
            row, j = divmod(int(np.argmin(d2)), len(partners))                           # the first minimum: lowest row, then lowest partner
            sep[b] = np.sqrt(d2[row, j])
            isep[SEP_PARTNER, b], isep[SEP_ROW, b], isep[SEP_COMPARED, b] = partners[j], row, len(partners)
            inside = d2 < r2
            isep[SEP_CONFLICTS, b] = int(inside.any(axis=0).sum())
            hit_rows = np.flatnonzero(inside.any(axis=1))
            isep[SEP_FIRST_CONFLICT, b] = hit_rows[0] if len(hit_rows) else -1
    return sep, isep


def conflicts_against_rows(rows, row_offsets, traffic_rows, traffic_row_offsets, radius, group_offsets=None, traffic_group_offsets=None,
                           start_rows=None, traffic_start_rows=None):
    """The CROSS conflict list recomputed from sampled rows -- the SPECIFICATION of `uavac_minsnap_conflict_against_offsets_dev` and
    `uavac_minsnap_conflicts_against_dev` (csrc/minsnap_conflicts_against.hip), which are tested against it bit for bit.  NumPy on
    the host; inputs, clock, groups, excluded missions, horizon and rounding exactly as in `separation_against_rows`: group g of the
    plan meets group g of the traffic, H_g covers both sides, each mission stands at clamp(k - S, 0, N - 1), d^2 = (dx * dx + dy * dy)
    + dz * dz, inside is strict.
    Mission i of the plan lists every included traffic mission j of its group with d^2(i, j, k) < r^2 at some clock row k below H_g,
    in ascending j.  Missions of the plan are never compared with each other; an excluded plan mission lists nothing, excluded
    traffic is listed by nobody, a group without included traffic lists nothing.
    -> (offsets (B + 1,) i64, pair_d (E,) f64, pair_i (CONF_ROWS, E) i32) with the layout of `conflicts_from_rows`: per entry the
    partner (the TRAFFIC batch index), the first and the last clock row inside, the number of rows inside, the clock row of the
    pair's minimum (the lowest one on a tie), and the minimum distance (the minimum of the squares, one sqrt)."""
    rows = _host(rows)
    ro = _host_i64(row_offsets)
    B = len(ro) - 1
    radius = _radius(radius)
    go = _group_offsets(group_offsets, B)
    S = _start_rows(start_rows, B, upper=None)
    r2 = radius * radius
    N = np.diff(ro)
    pos = [rows[ro[b]:ro[b + 1], 0:3] for b in range(B)]
    included = _included(pos.__getitem__, N, longest=None)
    tpos, tN, tS, tgo, tinc = _traffic_side(traffic_rows, traffic_row_offsets, group_offsets, traffic_group_offsets, traffic_start_rows, go,
                                            upper=None, longest=None)
    per_mission = [[] for _ in range(B)]                                                  # (partner, first, last, inside, row of the minimum, d^2)
    for g in range(len(go) - 1):
        members = [b for b in range(int(go[g]), int(go[g + 1])) if included[b]]
        partners = [j for j in range(int(tgo[g]), int(tgo[g + 1])) if tinc[j]]
        if not members or not partners:
            continue
        k = np.arange(int(max(max(S[b] + N[b] for b in members), max(tS[j] + tN[j] for j in partners))))
        T = np.stack([_at(tpos[j], k, tS[j]) for j in partners])                         # (n, H, 3): where the traffic stands at clock row k
        for i in members:
            own = _at(pos[i], k, S[i])
            dx, dy, dz = (own[:, c][None, :] - T[:, :, c] for c in range(3))              # (n, H): partners first, rows ascending
            d2 = (dx * dx + dy * dy) + dz * dz
            inside = d2 < r2
            for c in np.flatnonzero(inside.any(axis=1)):
                hit = np.flatnonzero(inside[c])
                low = int(np.argmin(d2[c]))                                               # the first minimum: the lowest row
                per_mission[i].append((partners[c], hit[0], hit[-1], len(hit), low, d2[c, low]))
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in per_mission])]).astype(np.int64)
    flat = [e for p in per_mission for e in p]
    pair_i = np.array([e[:5] for e in flat], dtype=np.int32).reshape(-1, nat.CONF_ROWS).T.copy()
    pair_d = np.sqrt(np.array([e[5] for e in flat], dtype=np.float64))
    return offsets, pair_d, pair_i


def conflicts_transposed(cl, n_partners):
    """The CSR transpose of a conflict list between two sides, on the host: the list seen from the owners' side (`cl`: the tuple
    `conflicts_against_rows` returns, or an `Engine.conflicts_against` -> ConflictList, or anything with its fields; tensors on any
    device or arrays) -> the list seen from the partners' side, as the same tuple (offsets (n_partners + 1,) i64, pair_d (E,) f64,
    pair_i (CONF_ROWS, E) i32): per partner the owners that list it, in ascending index, with the same five values.  The distance is
    bit-symmetric, so the transpose of `plan against traffic` is `traffic against plan` with the sides and their groups swapped, bit
    for bit: "which arrivals does committed mission j have to expect", without a second device call.  The cross-side counterpart of
    `conflict_pairs`.  A list whose slices do not sum to its entries, or with a partner outside 0 .. n_partners - 1, is a ValueError."""
    if not hasattr(cl, "offsets"):
        off, dist, block = _host_i64(cl[0]), _host(cl[1]).reshape(-1), _host(cl[2], np.int64)
        if block.ndim != 2 or block.shape[0] != nat.CONF_ROWS:
            raise ValueError("pair_i holds CONF_ROWS rows")
    else:
        off, dist = _host_i64(cl.offsets), _host(cl.min_distance).reshape(-1)
        block = np.stack([_host_i64(v).reshape(-1) for v in (cl.partner, cl.first_row, cl.last_row, cl.rows_inside, cl.min_row)])
    n_partners = int(n_partners)
    E = len(dist)
    if len(off) < 1 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != E or block.shape[1] != E:
        raise ValueError("a conflict list holds offsets[-1] entries in every field, in slices that ascend from 0")
    partner = block[0]
    if n_partners < 0 or (E and (partner.min() < 0 or partner.max() >= n_partners)):
        raise ValueError("a partner lies outside 0 .. n_partners - 1")
    owner = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))
    order = np.lexsort((owner, partner))                                                  # by partner, then by owner: both ascend
    offsets = np.concatenate([[0], np.cumsum(np.bincount(partner, minlength=n_partners))]).astype(np.int64)
    pair_i = np.empty((nat.CONF_ROWS, E), dtype=np.int32)
    pair_i[0] = owner[order]
    pair_i[1:] = block[1:, order]
    return offsets, dist[order].astype(np.float64), pair_i


def stagger_against_rows(rows, row_offsets, traffic_rows, traffic_row_offsets, radius, group_offsets=None, traffic_group_offsets=None,
                         start_rows=None, traffic_start_rows=None, step=1, max_steps=255, max_group=None):
    """`stagger_from_rows` against committed TRAFFIC that never moves -- the SPECIFICATION of `uavac_minsnap_stagger_against_dev`
    (csrc/minsnap_stagger_against.hip), which is tested against it exactly.  NumPy on the host.
    The plan's arguments, the clock, the excluded missions, the arithmetic and the rule are `stagger_from_rows`', with `max_group` =
    the call's `group_cap` (None: no limit but the batch -- the call is always block-wise; the limit counts the plan's missions of a
    group only).  The traffic's are `separation_against_rows`': a second plan on the same dt whose group g meets the plan's group g.
    A traffic mission stands as planned at its start row `traffic_start_rows[j]` (clamped to 0 .. 2^29): it has no candidates, is never
    examined and never written; an excluded one is nobody's partner and is not counted.
    ONE MORE CLAUSE IN "CLEAR": candidate q of mission i is clear iff it is outside the radius of every included mission j < i of its
    group at its granted start AND of every included traffic mission of its group at that mission's start, at every clock row below
    the horizon, which covers the traffic's ends too.  `earlier` counts the included traffic of the group plus the included plan
    missions before it, and the first included mission of a group is examined whenever its group has included traffic.  A group
    without included traffic gives exactly `stagger_from_rows(..., max_group=max_group)`.
    -> istag (STAGGER_ROWS, B) i32, as `stagger_from_rows`."""
    rows = _host(rows)
    ro = _host_i64(row_offsets)
    B = len(ro) - 1
    radius, step, max_steps = _radius(float(radius)), int(step), int(max_steps)
    if step < 1 or not (0 <= max_steps <= nat.STAGGER_MAX_STEPS) or step * max_steps > _MAX_CLOCK:
        raise ValueError(f"step must be >= 1, max_steps in 0 .. {nat.STAGGER_MAX_STEPS}, step * max_steps at most 2^29")
    go = _group_offsets(group_offsets, B)
    S = _start_rows(start_rows, B)
    N = np.diff(ro)
    pos = [rows[ro[b]:ro[b + 1], 0:3] for b in range(B)]
    tpos, tN, tS, tgo, tinc = _traffic_side(traffic_rows, traffic_row_offsets, group_offsets, traffic_group_offsets, traffic_start_rows, go)
    steps, earlier, _ = _prioritised_search(
        np.concatenate([N, tN]), _included(pos.__getitem__, N), go, _max_group(max_group, max(B, 1)), max_steps,
        lambda i, q: pos[i] if i < B else tpos[i - B], lambda i, q: int(S[i]) + q * step if i < B else int(tS[i - B]), radius * radius,
        committed=lambda g: [(B + j, 0) for j in range(int(tgo[g]), int(tgo[g + 1])) if tinc[j]])
    istag = np.zeros((nat.STAGGER_ROWS, B), dtype=np.int32)
    istag[STAG_START], istag[STAG_STEPS], istag[STAG_EARLIER] = S + np.maximum(steps, 0) * step, steps, earlier
    return istag


def stagger_ok(istag) -> dict:
    """A stagger result (`Engine.stagger` -> StaggerResult, anything with `steps`, or the [STAGGER_ROWS][B] block itself; tensors on
    any device or arrays) -> dict of (B,) bool host arrays: `resolved` (steps >= 0: a start was granted) and `examined` (steps !=
    -2).  A mission that was not examined -- an excluded one, or one of an oversized group -- never looks resolved."""
    if hasattr(istag, "steps"):
        steps = _host(istag.steps).reshape(-1)
    else:
        block = _host(istag)
        if block.ndim != 2 or block.shape[0] != nat.STAGGER_ROWS:
            raise ValueError(f"a stagger block is [{nat.STAGGER_ROWS}][B], got {block.shape}")
        steps = block[STAG_STEPS]
    return {"resolved": steps >= 0, "examined": steps != -2}


LAYER_LAYER, LAYER_STEPS, LAYER_EARLIER = range(nat.LAYER_ROWS)                                  # ilayer rows (include/uavac.h)
LAYER_BLOCKED = nat.LAYER_OBS_ROWS - 1                                                           # ... and the row the search with obstacles adds


def shift_coeffs(coeffs, seg_offsets_or_m, offsets):
    """The offset transform on coefficients -- the rule `uavac_minsnap_shift_dev` (csrc/minsnap_layer.hip) is tested against bit for
    bit.  NumPy on the host, elementwise.
    `coeffs`: anything that reshapes to (S, 8, 3) -- a Plan's (B, 8 m, 3) or a RaggedBatch's (S, 8, 3).  `seg_offsets_or_m`: the ragged
    batch's segment offsets (B + 1,), or an int m = segments per mission of a uniform batch.  `offsets` (B, 3).
    Every segment of mission b gets c0'[a] = c0[a] + offsets[b][a] (one rounded sum); c1 .. c7 keep every bit, and a mission whose three
    offsets are all +-0 is not touched at all (a -0.0 stays -0.0).  Non-finite offsets pass through.
    -> a new array of the shape of `coeffs`."""
    co = np.array(_host(coeffs))
    out = co.reshape(-1, 8, 3)
    off = _host(offsets).reshape(-1, 3)
    B = len(off)
    if np.ndim(seg_offsets_or_m) == 0:
        m = int(seg_offsets_or_m)
        if m < 1 or B * m != len(out):
            raise ValueError(f"{len(out)} segments are not {B} missions of {m}")
        so = np.arange(B + 1, dtype=np.int64) * m
    else:
        so = _host_i64(seg_offsets_or_m)
        if len(so) != B + 1 or so[0] != 0 or so[-1] != len(out) or (np.diff(so) < 0).any():
            raise ValueError("seg_offsets must ascend from 0 to the number of segments, one entry per mission and one more")
    for b in range(B):
        if (off[b] == 0.0).all():
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            out[so[b]:so[b + 1], 0, :] = out[so[b]:so[b + 1], 0, :] + off[b]
    return co


def layer_from_rows(rows_at, row_offsets, radius, group_offsets=None, start_rows=None, max_steps=63, max_group=None):
    """Prioritised deconfliction by offset layers, decided on SAMPLED rows -- the SPECIFICATION of `uavac_minsnap_layer_dev`
    (csrc/minsnap_layer.hip), which is tested against it exactly.  NumPy on the host.
    `rows_at(q)` -> the (N, >= 3) rows of the WHOLE batch with every mission on layer q, i.e. of the plan with fl(q * delta) added to
    c0 of every segment (`Engine.sample_rows(Engine.shift(plan, q * delta))`); a callable, so that the caller can sample lazily and
    memoise -- it is asked for the layers 0 .. max_steps at most, layer 0 first.  `row_offsets`, `radius`, `group_offsets` as
    `stagger_from_rows` takes them, and the clock, the excluded missions (judged on layer 0) and the arithmetic are the same.
    `start_rows` (B,) or None = all 0: FIXED starts S_b, clamped to 0 .. 2^29; nobody is delayed.

    Per group the included missions in ascending batch index -- the priority: the lowest index is never moved.  Mission i examines
    the layers q = 0, 1, ..., max_steps in that order; its candidate q reads rows_at(q), partner j reads rows_at(L_j), its GRANTED
    layer.  A candidate is clear iff for every included mission j < i of the group and every clock row k in [0, max(S_i + N_i, S_j +
    N_j)) the two are not inside the radius.  The first clear candidate is granted: L_i = steps = q; if none is clear the mission is
    unresolved: steps = -1, L_i = 0, and it remains a partner for every later mission.  An excluded mission, and every mission of a
    group of more than LAYER_MAX_GROUP, is not examined: layer 0, steps = -2, earlier = 0; nobody is checked against an excluded one.
    `max_group`: a number sets that limit instead (`uavac_minsnap_layer_wide_dev` without cuboids, `group_cap` = max_group); None =
    LAYER_MAX_GROUP.
    -> ilayer (LAYER_ROWS, B) i32: the granted layer; steps; earlier (how many missions it was checked against)."""
    return _layer_search(rows_at, row_offsets, radius, (), group_offsets, start_rows, max_steps, max_group)[:nat.LAYER_ROWS]


def layer_obstacles_from_rows(rows_at, row_offsets, radius, cuboids, group_offsets=None, start_rows=None, max_steps=63, max_group=None):
    """`layer_from_rows` with obstacles -- the SPECIFICATION of `uavac_minsnap_layer_obs_dev` (csrc/minsnap_layer_obs.hip), which is
    tested against it exactly.  NumPy on the host.  `rows_at`, `row_offsets`, `radius`, `group_offsets`, `start_rows`, `max_steps` as
    `layer_from_rows` takes them, and the clock, the excluded missions (judged on layer 0), the clamped starts, `LAYER_MAX_GROUP` and
    the distance arithmetic are the same.  `cuboids` (n, 6): xmin xmax ymin ymax zmin zmax, 0 <= n <= AUDIT_MAX_CUBOIDS.  `max_group`: a
    number sets the group limit instead -- the SPECIFICATION of `uavac_minsnap_layer_wide_dev` with `group_cap` = max_group.

    The differences, and only these.  Candidate q of mission i is BLOCKED when any of the mission's own rows
    rows_at(q)[ro[i]:ro[i + 1], 0:3] lies inside any cuboid by the audit's inclusive test (x >= xmin and x <= xmax and ...: a NaN bound
    or an inverted box contains nothing); those rows cover its whole shared clock, since before its start it holds row 0 and after its
    end row N - 1.  The cuboid test comes first: a blocked candidate is never compared with partners.  EVERY included mission is
    examined, the first of its group too (earlier = 0, no partners): it gets the lowest layer that no cuboid blocks, so "the lowest
    index is never moved" becomes "is moved only by a cuboid".  A mission for which no layer 0 .. max_steps is both unblocked and clear
    is unresolved: steps = -1, layer 0, and it remains a partner for later missions.
    -> ilayer (LAYER_OBS_ROWS, B) i32: rows 0-2 as `layer_from_rows`; row 3 `blocked` = how many of the candidates q = 0 .. steps - 1
    (0 .. max_steps when unresolved) a cuboid refused, 0 for a mission that was not examined.  With n = 0 rows 0-2 equal
    `layer_from_rows` exactly and row 3 is zero."""
    return _layer_search(rows_at, row_offsets, radius, cuboids, group_offsets, start_rows, max_steps, max_group)


def layer_against_rows(rows_at, row_offsets, traffic_rows, traffic_row_offsets, radius, cuboids=None, group_offsets=None,
                       traffic_group_offsets=None, start_rows=None, traffic_start_rows=None, max_steps=63, max_group=None):
    """`layer_obstacles_from_rows` against committed TRAFFIC that never moves -- the SPECIFICATION of
    `uavac_minsnap_layer_against_dev` (csrc/minsnap_layer_against.hip), which is tested against it exactly.  NumPy on the host.
    `rows_at`, `row_offsets`, `radius`, `cuboids` (None or zero rows: no obstacles), `group_offsets`, `start_rows`, `max_steps` as
    `layer_obstacles_from_rows` takes them, and the rule is that one's -- the cuboid policy: every included mission is examined, a
    blocked candidate is refused before anybody is compared --, with `max_group` = the call's `group_cap` (None: no limit but the
    batch).  The traffic's arguments are `stagger_against_rows`'; a traffic mission is compared AS IT IS, on no layer, at its start
    row (a caller who has layered the traffic passes the rows of the shifted plan), has no candidates and is never examined.
    One more clause in "clear": the candidate is also outside the radius of every included traffic mission of its group, up to a
    horizon that covers the traffic's ends too; `earlier` counts the included traffic of the group plus the included plan missions
    before it.  A group without included traffic gives exactly `layer_obstacles_from_rows(..., max_group=max_group)`.
    -> ilayer (LAYER_OBS_ROWS, B) i32, as `layer_obstacles_from_rows`."""
    B = len(_host_i64(row_offsets)) - 1
    return _layer_search(rows_at, row_offsets, radius, () if cuboids is None else cuboids, group_offsets, start_rows, max_steps,
                         max(B, 1) if max_group is None else max_group,
                         traffic=(traffic_rows, traffic_row_offsets, traffic_group_offsets, traffic_start_rows))


def _layer_search(rows_at, row_offsets, radius, cuboids, group_offsets, start_rows, max_steps, max_group=None, traffic=None):
    """Both layer rules -> ilayer (LAYER_OBS_ROWS, B) i32.  Without cuboids nothing is ever blocked and rows 0-2 are `layer_from_rows`.
    `traffic`: (rows, row_offsets, group_offsets, start_rows) of `layer_against_rows`."""
    ro = _host_i64(row_offsets)
    B = len(ro) - 1
    radius, max_steps = float(radius), int(max_steps)
    if not callable(rows_at):
        raise ValueError("rows_at must be a callable: layer -> rows")
    radius = _radius(radius)
    if not (0 <= max_steps <= nat.LAYER_MAX_STEPS):
        raise ValueError(f"max_steps must be in 0 .. {nat.LAYER_MAX_STEPS}")
    cub = _host(cuboids)
    if cub.size and (cub.ndim != 2 or cub.shape[1] != 6):
        raise ValueError("cuboids must be (n, 6): xmin xmax ymin ymax zmin zmax")
    cub = cub.reshape(-1, 6)
    if len(cub) > nat.AUDIT_MAX_CUBOIDS:
        raise ValueError(f"{len(cub)} cuboids; at most {nat.AUDIT_MAX_CUBOIDS}")
    go = _group_offsets(group_offsets, B)
    S = _start_rows(start_rows, B)
    N = np.diff(ro)

    committed = None
    if traffic is not None:                                                           # (keys B .. B + Bt - 1: as planned, at their own starts)
        tpos, tN, tS, tgo, tinc = _traffic_side(traffic[0], traffic[1], group_offsets, traffic[2], traffic[3], go)
        N, S = np.concatenate([N, tN]), np.concatenate([S, tS])

        def committed(g):
            return [(B + j, 0) for j in range(int(tgo[g]), int(tgo[g + 1])) if tinc[j]]

    def pos(b, q):                                                                    # the candidate is a layer: the mission's rows of rows_at(q)
        if b >= B:
            return tpos[b - B]
        return _host(rows_at(q))[ro[b]:ro[b + 1], 0:3]

    def is_blocked(b, q):
        p = pos(b, q)
        with np.errstate(invalid="ignore"):
            for x in cub:
                if ((p[:, 0] >= x[0]) & (p[:, 0] <= x[1]) & (p[:, 1] >= x[2]) & (p[:, 1] <= x[3]) & (p[:, 2] >= x[4]) & (p[:, 2] <= x[5])).any():
                    return True
        return False

    steps, earlier, blocked = _prioritised_search(N, _included(lambda b: pos(b, 0), N[:B]), go, _max_group(max_group, nat.LAYER_MAX_GROUP), max_steps, pos,
                                                  lambda b, q: int(S[b]), radius * radius, is_blocked if len(cub) else None, committed)
    ilayer = np.zeros((nat.LAYER_OBS_ROWS, B), dtype=np.int32)
    ilayer[LAYER_LAYER], ilayer[LAYER_STEPS], ilayer[LAYER_EARLIER], ilayer[LAYER_BLOCKED] = np.maximum(steps, 0), steps, earlier, blocked
    return ilayer


def _layer_block(result):
    block = _host(result)
    if block.ndim != 2 or block.shape[0] not in (nat.LAYER_ROWS, nat.LAYER_OBS_ROWS):
        raise ValueError(f"a layer block is [{nat.LAYER_ROWS}][B] (with obstacles [{nat.LAYER_OBS_ROWS}][B]), got {block.shape}")
    return block


def layer_ok(result) -> dict:
    """A layer result (`Engine.layer` -> LayerResult, anything with `steps`, or the [LAYER_ROWS][B] block itself -- with obstacles the
    [LAYER_OBS_ROWS][B] one; tensors on any device or arrays) -> dict of (B,) bool host arrays: `resolved` (steps >= 0: a layer was
    granted, layer 0 included) and `examined` (steps != -2).  A mission that was not examined -- an excluded one, or one of an oversized
    group -- never looks resolved."""
    if hasattr(result, "steps"):
        steps = _host(result.steps).reshape(-1)
    else:
        steps = _layer_block(result)[LAYER_STEPS]
    return {"resolved": steps >= 0, "examined": steps != -2}


def blocked_out(result, max_steps: int):
    """The missions for which EVERY layer 0 .. `max_steps` hits a cuboid: steps == -1 and blocked == max_steps + 1, from the result of
    a layer search with obstacles (`Engine.layer(..., obstacles=)` -> LayerResult, anything with `steps` and `blocked`, or the
    [LAYER_OBS_ROWS][B] block; `max_steps` as the search was given it) -> (B,) bool host array.  "Too crowded" (unresolved with fewer
    blocked layers) may yield to more layers or another delta; a blocked-out mission needs a new plan around the obstacle."""
    if hasattr(result, "steps"):
        if getattr(result, "blocked", None) is None:
            raise ValueError("a layer result without `blocked`: the search was run without obstacles")
        steps, blocked = (_host(v).reshape(-1) for v in (result.steps, result.blocked))
    else:
        block = _layer_block(result)
        if block.shape[0] != nat.LAYER_OBS_ROWS:
            raise ValueError(f"a layer block with obstacles is [{nat.LAYER_OBS_ROWS}][B], got {block.shape}")
        steps, blocked = block[LAYER_STEPS], block[LAYER_BLOCKED]
    return (steps == -1) & (blocked == int(max_steps) + 1)


def take_parts(coeffs, times, seg_rows, seg_offsets_or_m, index):
    """A gather of missions on a plan's parts -- the construction `uavac_minsnap_take_dev` (csrc/minsnap_take.hip) is tested against bit
    for bit.  NumPy on the host; nothing is computed.
    `coeffs`: anything that reshapes to (S, 8, 3); `times` (S values, or None) and `seg_rows` (S values) per segment back to back;
    `seg_offsets_or_m`: the ragged batch's segment offsets (B + 1,), or an int m = segments per mission of a uniform batch.  `index`
    (n,) integers in 0 .. B - 1: duplicates and any order are allowed, n may exceed B.
    Mission i of the result is mission index[i] of the input, every bit of it.
    -> (coeffs (S', 8, 3), times (S',) or None, seg_rows (S',) i32, seg_offsets (n + 1,) i64)."""
    co = _host(coeffs).reshape(-1, 8, 3)
    sr = _host(seg_rows, np.int32).reshape(-1)
    tm = None if times is None else _host(times).reshape(-1)
    if np.ndim(seg_offsets_or_m) == 0:
        m = int(seg_offsets_or_m)
        if m < 1 or len(co) % m:
            raise ValueError(f"{len(co)} segments are not missions of {m}")
        so = np.arange(len(co) // m + 1, dtype=np.int64) * m
    else:
        so = _host_i64(seg_offsets_or_m)
        if len(so) < 2 or so[0] != 0 or so[-1] != len(co) or (np.diff(so) < 0).any():
            raise ValueError("seg_offsets must ascend from 0 to the number of segments, one entry per mission and one more")
    B = len(so) - 1
    if len(sr) != len(co) or (tm is not None and len(tm) != len(co)):
        raise ValueError("one row count (and one duration) per segment")
    idx = _host_i64(index)
    if len(idx) < 1:
        raise ValueError("an empty selection")
    if (idx < 0).any() or (idx >= B).any():
        raise ValueError(f"index must be in 0 .. {B - 1}")
    seg = np.concatenate([np.arange(so[b], so[b + 1], dtype=np.int64) for b in idx])
    out_so = np.concatenate([[0], np.cumsum(np.diff(so)[idx])]).astype(np.int64)
    return co[seg].copy(), None if tm is None else tm[seg].copy(), sr[seg].copy(), out_so


def take_rows(rows, row_offsets, index):
    """The sampled rows of selected missions back to back: what the sampler writes for `Engine.take(plan, index)` when `rows` are the
    plan's -- every row keeps all of its columns, the spline ids included.  `index` as `take_parts` takes it.
    -> (rows (N', cols), row_offsets (n + 1,) i64)."""
    rows = _host(rows)
    ro = _host_i64(row_offsets)
    B = len(ro) - 1
    idx = _host_i64(index)
    if len(idx) < 1:
        raise ValueError("an empty selection")
    if (idx < 0).any() or (idx >= B).any():
        raise ValueError(f"index must be in 0 .. {B - 1}")
    out = np.concatenate([rows[ro[b]:ro[b + 1]] for b in idx])
    return out, np.concatenate([[0], np.cumsum(np.diff(ro)[idx])]).astype(np.int64)


def priority_order(priority, group_offsets=None):
    """Priorities into a within-group order -- the SPECIFICATION of `uavac_fleet_order_dev` (csrc/minsnap_take.hip), which is tested
    against it exactly.  NumPy on the host.
    `priority` (B,) f64.  `group_offsets` (G + 1,) or None = one group of all B; every entry is clamped as the fleet's kernels clamp
    it -- group g holds [g0, g1) with g0 = clamp(go[g], 0, B) and g1 = clamp(go[g + 1], g0, B) -- so offsets that do not reach from 0
    to B leave a head or a tail that no group holds.
    Within each group the missions are sorted by the total order "a before b" iff p_a is a number and p_b is NaN, or p_a < p_b, or
    (p_a == p_b or both are NaN) and a < b: a LOWER priority goes first, -0.0 ties with +0.0, NaN comes after +inf, ties go to the lower
    batch index.
    -> (order, rank), (B,) i32 each: order[g0 + k] is the mission in slot k of its group, rank its inverse (rank[order[s]] = s); a
    mission that no group holds keeps its place, order[b] = rank[b] = b."""
    p = _host(priority).reshape(-1)
    B = len(p)
    go = np.array([0, B], dtype=np.int64) if group_offsets is None else _host_i64(group_offsets)
    if len(go) < 2:
        raise ValueError("group offsets hold at least two entries")
    order = np.arange(B, dtype=np.int32)
    nan = np.isnan(p)
    key = np.where(nan, np.inf, p)                                                    # (a NaN sorts behind +inf through the second key)
    for g in range(len(go) - 1):
        g0 = int(min(max(go[g], 0), B))
        g1 = int(min(max(go[g + 1], g0), B))
        ids = np.arange(g0, g1)
        # lexsort: the last key is the primary one; -0.0 == +0.0 for it, and it is stable, so ties go to the lower index
        order[g0:g1] = ids[np.lexsort((ids, nan[ids], key[ids]))]
    rank = np.empty(B, dtype=np.int32)
    rank[order] = np.arange(B, dtype=np.int32)
    return order, rank


def envelope_from_rows(rows, row_offsets, rows_reach=None):
    """Every mission's swept box on SAMPLED rows -- the SPECIFICATION of `uavac_minsnap_envelope_dev` (csrc/minsnap_envelope.hip),
    which is tested against it as numbers.  NumPy on the host.
    `rows` (N, >= 3) and `row_offsets` (B + 1,) as `separation_from_rows` takes them.  `rows_reach` (N, >= 3) or None: the rows of the
    same plan with an offset added to c0 of every segment (`Engine.shift(plan, reach)`: the same row counts); the box is then the hull
    of both.
    -> (lo, hi), (B, 3) f64 each: the minimum and the maximum of the mission's positions per axis.  A mission without rows, or with a
    position that is not finite on either side, gets NaN in all six."""
    rows = _host(rows)
    ro = _host_i64(row_offsets)
    B = len(ro) - 1
    sides = [rows[:, 0:3]] if rows_reach is None else [rows[:, 0:3], _host(rows_reach)[:, 0:3]]
    if any(len(p) != len(sides[0]) for p in sides):
        raise ValueError("rows_reach holds one row per row of rows")
    lo, hi = np.full((B, 3), np.nan), np.full((B, 3), np.nan)
    for b in range(B):
        p = np.concatenate([s[ro[b]:ro[b + 1]] for s in sides])
        if len(p) and np.isfinite(p).all():
            lo[b], hi[b] = p.min(axis=0), p.max(axis=0)
    return lo, hi


def airspaces_from_envelopes(lo, hi, radius, group_offsets=None, rounds=None, labels=None):
    """Independent airspaces from swept boxes -- the SPECIFICATION of `uavac_fleet_airspaces_dev` (csrc/fleet_airspaces.hip), which is
    tested against it exactly, the round count included.  NumPy on the host.
    `lo`, `hi` (B, 3): the boxes (`envelope_from_rows`).  `group_offsets` (G + 1,) or None = one group of all B, every entry clamped
    as `priority_order` clamps it; a mission that no group holds is linked to nobody.
    THE LINK.  Missions i != j of the same group are linked iff on all three axes lo_i - hi_j < radius and lo_j - hi_i < radius (each
    difference one rounded subtraction, the comparison strict): two boxes that are `radius` apart on some axis are not linked, and
    neither is a box that holds a NaN, to anybody.
    ONE ROUND, on whole arrays: m[i] = min(lab[i], min of lab[j] over the linked j); lab'[i] = m[m[i]] (the pointer jump).  The first
    round starts from lab[i] = i, or from `labels` (B,) when they are given (a resumed call).  At most `rounds` rounds are run (None:
    as many as it takes); the first round that changes nothing is the last one run.
    -> (labels (B,) i32, the number of rounds that changed a label, converged: the last round run changed nothing).  Once converged,
    labels[b] is the lowest batch index of b's connected component; before that the labels describe a FINER partition than the
    components and must not be used for anything but a resumed call."""
    lo, hi = _host(lo).reshape(-1, 3), _host(hi).reshape(-1, 3)
    B = len(lo)
    if len(hi) != B:
        raise ValueError("one lo and one hi per mission")
    radius = _radius(radius)
    if rounds is not None and int(rounds) < 1:
        raise ValueError("rounds must be >= 1")
    go = np.array([0, B], dtype=np.int64) if group_offsets is None else _host_i64(group_offsets)
    if len(go) < 2:
        raise ValueError("group offsets hold at least two entries")
    lab = np.arange(B, dtype=np.int64) if labels is None else np.clip(_host_i64(labels), 0, max(B - 1, 0))
    if len(lab) != B:
        raise ValueError("one label per mission")
    linked = []                                                                       # per group: (g0, g1, the (g, g) link matrix)
    for g in range(len(go) - 1):
        g0 = int(min(max(go[g], 0), B))
        g1 = int(min(max(go[g + 1], g0), B))
        if g1 - g0 < 2:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            gap = lo[g0:g1, None, :] - hi[None, g0:g1, :]                             # gap[i, j] = lo_i - hi_j
            link = (gap < radius).all(axis=2)
        link = link & link.T
        np.fill_diagonal(link, False)
        linked.append((g0, g1, link))
    changed, converged = 0, False
    while rounds is None or changed < int(rounds):
        m = lab.copy()
        for g0, g1, link in linked:
            m[g0:g1] = np.minimum(m[g0:g1], np.where(link, lab[None, g0:g1], B).min(axis=1))
        new = m[m]
        if np.array_equal(new, lab):
            converged = True
            break
        lab, changed = new, changed + 1
    return lab.astype(np.int32), changed, converged


def airspace_order(labels, group_offsets=None):
    """Missions sorted by airspace within each caller group: `priority_order(labels, group_offsets)` -- stable, so the missions of an
    airspace keep their relative order -- and the boundaries where the label changes.  What `Engine.airspaces` computes on the device
    (`uavac_fleet_order_dev` with the labels as priorities, exact in float64).
    -> (order, rank, airspace_offsets): order and rank (B,) i32 as `priority_order` gives them; airspace_offsets (A + 1,) i64 ascending
    from 0 to B, airspace a holds the slots [airspace_offsets[a], airspace_offsets[a + 1]) of `order`."""
    lab = _host_i64(labels)
    order, rank = priority_order(lab.astype(np.float64), group_offsets)
    sorted_lab = lab[order]
    starts = np.flatnonzero(np.concatenate([[True], sorted_lab[1:] != sorted_lab[:-1]])) if len(lab) else np.zeros(0, dtype=np.int64)
    return order, rank, np.concatenate([starts, [len(lab)]]).astype(np.int64)
