"""One tick of the fused rollout from ARBITRARY states against the long-double C oracle (oracle_rollout_ld).

Every other rollout test starts from uavac_state_init (rest, unit quaternion, cursor 0) and stays in the benign interior of
csrc/control_law.h.  Here ~4 000 hand-placed lanes each isolate one branch of the reformulated control law -- the large-rotation
and off-unit branches of free_body_step, both copies of the inv_n2 selection, every range of floored_mod, the cross-multiplied
choice of allocate at its ties, fast_sqrt at 0, the corners of euler_trig, small and negative R22, the ground branch -- and one
tick from there is compared lane by lane, output by output.

THE BOUND.  t = the long-double result, r = the fp64 oracle's, g = the kernel's:
        |g - t| <= M max(|r - t|, U 2^-53 kappa max(1, |t|), rotor floor),    M = U = 16; kappa = 1 and the rotor floor is immaterial
but for the lanes of CONDITIONING and ROTOR FLOOR below.
The fp64 oracle's own distance from the long-double result is the error scale of the lane (it carries the conditioning of R22 -> 0,
cos phi -> 0, ...); the floor is U ulps of the output's magnitude.  M: the kernel's primitives claim <= 2 ulp where the oracle's
are correctly rounded (x4), and a handful of re-associated operations lie between input and output (x4).  Both constants come
from the reference side -- tests/test_oracle_c.py shows that margin 1 suffices for the fp64 oracle -- never from the kernel.

CONDITIONING.  The floor above misses one thing the kernel and the fp64 oracle share but do not share lane by lane: the outer loop
divides by R22 (altitude, roll_pitch) and by cos phi (yaw_rate), and multiplies by cos theta = sqrt(1 - st^2).  R22 and the cn of
cos phi are 1 - 2 (x^2 + y^2): their ABSOLUTE rounding error is a few 2^-53 whatever their size, so their relative error -- and that
of every quotient -- is a few 2^-53 / |R22| resp. / |cos phi|; d(cos theta) = d(st^2) / (2 cos theta) is 2^-53 / cos theta.  |r - t|
carries exactly these factors, but it is ONE draw of that error: in a few lanes the oracle's roundings cancel by luck and 16 |r - t|
falls below what any other correct fp64 evaluation gives (first seen on the NumPy restatement below, before any kernel ran: lane
"pose/phi~+-pi/2", pqr_cmd[2] = -145 158.8, 2.8 x the unconditioned bound).  So the floor of a lane whose tick runs the outer loop is
multiplied by  kappa = max(1, 1/|R22|) max(1, 1/|cos phi|) max(1, 1/cos theta)  of its input attitude (pose_conditioning; cos theta
only while st is not clamped: clamped, it is exactly 0).  kappa is 1 within rounding for a level vehicle and on inner-only ticks.

ROTOR FLOOR.  omega_cmd = sqrt(f / kf), and f = clip(col + sc mf) is a sum that CANCELS for the rotor that limits the moment scale:
sc = (min_thrust - col) / mf there, so col + sc mf = min_thrust up to the rounding of sc mf, an absolute error d <= U 2^-53
max(1, max_thrust) in f.  With min_thrust = 0 (uavac_check_vehicle admits it) that residue is either clipped to 0 or is a positive
1e-16 whose square root is 1e-8: the reference shows 0 in some lanes and 1e-8 in others, by the luck of one rounding, and so does any
correct fp64 evaluation (first seen on the kernel: vehicle "free-2ms-F10-min0", omega_cmd 1.3e-8 where t = r = 0, i.e. a rotor
force of 1.7e-16 N).  |sqrt(a) - sqrt(b)| <= |a - b| / max(sqrt(b), sqrt|a - b|), so omega_cmd gets the absolute floor
e_omc = (d / kf) / max(|t|, sqrt(d / kf)) -- 8e-15 at hover (4 x the ulp floor there: f carries the ulps of max_thrust, not omega's) and sqrt(d / kf) = 9e-8 only where the
command is 0 -- and what follows it inherits it through the tick's own arithmetic (rotor_floor): omega the lag's share resp e_omc, the total
thrust and the torques 8 kf |omega| resp e_omc, velocity dt / m of that, position dt of that, rates dt max(arm, kappa) / min(I) of it,
attitude dt / 2 of that.  For a vehicle with min_thrust > 0 everything downstream of omega_cmd lies below the ulp floor.  Over K = F + 1 ticks
(test_across_an_outer_tick) the residue does not stay in the rotors: the vehicle integrates it, the outer tick inside the flight
reads the perturbed velocity, and the body-rate loop hands the commands back to the rotors (seen on the kernel, same vehicle:
thrust_cmd and pqr_cmd 3e-10 off after 11 ticks in the lanes with a rotor commanded to 0; a first-order worst-case bound on that loop
came out at 1e-2 rad/s, no check at all).  Like a tumbling vehicle, such a lane is not compared over K ticks: the reference's own
omega_cmd selects the lanes, none below a quarter of the hover speed in any tick (rotors_well_conditioned; every lane of the
vehicles with min_thrust = 0.1).  The one-tick tests compare every lane.

EXCLUSIONS.  A discontinuous decision that the long-double oracle takes with a margin under 1e-9 (yaw wrap at +-pi, the sign of
R22 in altitude, ground r > 0, the take-off height; oracle_tick_margins_ld) is not compared in value: such a lane must be
finite and inside the actuator limits.  At most 0.5 % of the lanes, asserted.

euler_trig's h == 0 needs sn == 0 and cn == 0 exactly.  For a UNIT quaternion cn = R22, and R22 == 0 makes altitude divide by
zero (the reference too): no finite output.  A stored quaternion off the unit sphere reaches it with finite outputs:
q = (a, 1/2, 1/2, -a), a != +-1/2 a binary fraction -- sn = 2 (a/2 - a/2) and cn = 1 - 2 (1/4 + 1/4) are exactly 0 while
R22 = 1 - 1 / |q|^2 != 0.  Family "pose/h0" holds sixteen of them.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M_BOUND, U_FLOOR = 16.0, 16.0
MARGIN = 1e-9
TWO_PI = 2.0 * np.pi                         # == kTwoPi of control_law.h (2 * the fp64 pi)

# one vehicle per launch: (name, dt, F, ground, min_thrust)
CONFIGS = (("free-1ms-F10", 0.001, 10, 0, 0.1), ("ground-2ms-F10", 0.002, 10, 1, 0.1), ("free-1ms-F1", 0.001, 1, 0, 0.1),
           ("free-2ms-F10-min0", 0.002, 10, 0, 0.0))


def vehicle_params(dt, F, ground, min_thrust):
    from oracle.control_oracle import Vehicle as PyVehicle
    p = PyVehicle()
    v = {n: getattr(p, n) for n in ("g", "mass", "arm", "kf", "kappa", "max_thrust", "tau_rise", "tau_fall", "max_ascent", "max_descent",
                                    "max_speed_xy", "max_horiz_accel", "max_tilt", "kp_xy", "kd_xy", "kp_z", "kd_z", "ki_z", "kp_roll",
                                    "kp_pitch", "kp_yaw", "kp_p", "kp_q", "kp_r", "ground_z", "ground_clearance")}
    v.update(dt=dt, dt_outer=dt * F, inertia=tuple(p.inertia), min_thrust=min_thrust, inner_per_outer=F, ground=ground,
             ground_timeconst=0.02)
    return v


def make_vehicle(cls, v):
    V = cls.default()
    for n, val in v.items():
        if n == "inertia":
            V.inertia[:] = val
        else:
            setattr(V, n, val)
    return V


# ------------------------------------------------------------------------------------------ quaternions
def _unit(x):
    return x / np.linalg.norm(x)


def q_axis(axis, angle):
    axis = _unit(np.asarray(axis, float))
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def q_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def q_euler(phi, theta, psi):                # ZYX, the convention of quad.py:189-213
    return q_mul(q_mul(q_axis([0, 0, 1], psi), q_axis([0, 1, 0], theta)), q_axis([1, 0, 0], phi))


def _psi_of(q):
    return np.arctan2(2 * (q[0] * q[3] + q[1] * q[2]), 1 - 2 * (q[2] * q[2] + q[3] * q[3]))


# ------------------------------------------------------------------------------------------ the families
@functools.lru_cache(maxsize=None)
def build(name):
    """-> dict(state (30, B), istate (4, B), traj (N, 11), row_offsets (B+1,), vehicle (dict), labels [B])"""
    cfg = {c[0]: c for c in CONFIGS}[name]
    _, dt, F, ground, min_thrust = cfg
    v = vehicle_params(dt, F, ground, min_thrust)
    rng = np.random.default_rng(abs(hash_name(name)))
    fmin, fmax, kf, mass, g = v["min_thrust"], v["max_thrust"], v["kf"], v["mass"], v["g"]
    I = np.array(v["inertia"])
    kp = np.array([v["kp_p"], v["kp_q"], v["kp_r"]])
    hover = np.sqrt(mass * g / (4 * kf))
    thr_w = 2.0 * np.sqrt(1e-3) / dt                       # |w| at which free_body_step leaves the Taylor series
    lanes = []

    def rvec(scale=1.0):
        return rng.standard_normal(3) * scale

    def rdir():
        return _unit(rng.standard_normal(3))

    def lane(label, phase=None, **kw):
        p = np.array([rng.uniform(0, 20), rng.uniform(0, 12), -rng.uniform(1, 5)])
        d = dict(p=p, q=q_mul(q_axis([0, 0, 1], rng.uniform(-3, 3)), q_axis(np.append(rng.standard_normal(2), 0), rng.uniform(0, 0.3))),
                 v=rvec(), w=rvec(), om=hover * (1 + 0.1 * rng.standard_normal(4)), omc=np.full(4, hover), integ=rng.uniform(-1, 1),
                 thrust=mass * g * rng.uniform(0.8, 1.2), pqr=rvec(), gbits=0, idx=None, nrows=5, rows=None)
        d.update(kw)
        n = d["nrows"]
        if d["rows"] is None:
            rows = np.zeros((n, 11))
            rows[:, 0:3] = d["p"] + rng.standard_normal((n, 3))
            rows[:, 3:9] = rng.standard_normal((n, 6))
            rows[:, 9] = rng.uniform(-3, 3, n)
            d["rows"] = rows
        if d["idx"] is None:
            d["idx"] = int(rng.integers(0, n))
        if "tg" in kw:                                     # overrides of the row under the cursor: {column: value}
            for c, val in kw["tg"].items():
                d["rows"][d["idx"], c] = val
        base = F * int(rng.integers(0, 50))
        if phase == "outer" or F == 1:
            d["inner"] = base
        elif phase == "inner":
            d["inner"] = base + int(rng.integers(1, F))
        elif isinstance(phase, int):
            d["inner"] = base + phase
        else:
            d["inner"] = base + int(rng.integers(0, F))
        d["label"] = label
        lanes.append(d)
        return d

    def still(**kw):                                       # w = 0, pqr_cmd free, all rotors equal: the moment is I kp pqr_cmd
        kw.setdefault("om", np.full(4, hover))
        return dict(w=np.zeros(3), **kw)

    N = 16
    families = cfg_families(name)

    if "norm" in families:
        for s in (1.0, 1 + 1e-13, 1 - 1e-13, 1 + 1e-11, 1 - 1e-11, 1 + 4e-7, 1 - 4e-7, 1 + 6e-7, 1 - 6e-7, 0.98, 1.02, 0.5, 2.0):
            for _ in range(N):
                q = _unit(rng.standard_normal(4)) if rng.random() < 0.5 else q_axis(rdir(), rng.uniform(0, 1.0))
                lane(f"norm/{s - 1:+.0e}" if abs(s - 1) < 1e-3 else f"norm/x{s}", q=q * s)

    if "pose" in families:
        for _ in range(N):
            lane("pose/level", q=q_axis([0, 0, 1], rng.uniform(-3, 3)))
            lane("pose/tilt", q=q_mul(q_axis([0, 0, 1], rng.uniform(-3, 3)), q_axis(np.append(rng.standard_normal(2), 0), rng.uniform(0.3, 1.2))))
            lane("pose/inverted", q=q_mul(q_axis([0, 0, 1], rng.uniform(-3, 3)), q_axis(np.append(rng.standard_normal(2), 0), np.pi - rng.uniform(0, 0.2))))
        for r22 in (1e-3, -1e-3, 1e-2, -1e-2):
            for _ in range(N):
                lane(f"pose/R22={r22:+.0e}", phase="outer",
                     q=q_mul(q_axis([0, 0, 1], rng.uniform(-3, 3)), q_axis(np.append(rng.standard_normal(2), 0), np.arccos(r22))))
        for sgn in (1, -1):
            for k in range(N):
                # a STORED quaternion off the unit sphere reaches the asin clamp (2 (q0 q2 - q3 q1) = |q|^2 sin theta >= 1) and
                # cos_theta -> 0 at a healthy R22 = cos phi cos theta of the normalised attitude ...
                th = sgn * rng.uniform(0.9, 1.2)
                qe = q_euler(rng.uniform(-0.5, 0.5), th, rng.uniform(-3, 3))
                lane("pose/asin-clamp", phase="outer", q=qe * np.sqrt(rng.uniform(1.01, 1.5) / np.sin(abs(th))))
                lane("pose/cos-theta~0", phase="outer", q=qe * np.sqrt((1 - 1e-9 * rng.uniform(0.1, 1)) / np.sin(abs(th))))
                lane("pose/phi~+-pi/2", phase="outer", q=q_euler(sgn * (np.pi / 2 - rng.choice([1e-3, -1e-3, 1e-2, -1e-2])), rng.uniform(-0.5, 0.5), rng.uniform(-3, 3)))
            # ... a UNIT one at theta = +-pi/2 (exactly, and within 1e-9) has R22 = 0 to rounding: altitude's division decides
            # its sign by a hair, the lane is excluded from the value comparison -- one of each, the exclusion cap allows no more
            lane("pose/theta=+-pi/2", phase="outer", q=np.array([np.sqrt(0.5), 0, sgn * np.sqrt(0.5), 0]))
            lane("pose/theta~+-pi/2", phase="outer", q=q_euler(rng.uniform(-0.5, 0.5), sgn * (np.pi / 2 - 1e-9 * rng.uniform(0.1, 1)), rng.uniform(-3, 3)))
        for a in (0.125, 0.25, 0.375, 0.625, 0.75, 1.0, 1.25, 1.5):
            lane("pose/h0", phase="outer", q=np.array([a, 0.5, 0.5, -a]))
            lane("pose/h0", phase="outer", q=np.array([-a, -0.5, 0.5, -a]))

    if "rate" in families:
        for wn in (0.0, 1e-9, 1.0, 40.0, 120.0, 400.0):
            for _ in range(N):
                lane(f"rate/{wn:g}", w=wn * rdir())
            for ax in range(3):
                for _ in range(6):
                    lane(f"rate/{wn:g}/axis", w=wn * np.eye(3)[ax] * rng.choice([-1, 1]))
        # either side of the threshold: a single-axis spin with pqr_cmd == w and equal rotors on an inner-only tick has no moment,
        # no gyroscopic term and no rotor torque, so |w| after the step is |w| before it, exactly
        for side in (1 - 1e-6, 1 + 1e-6):
            for k in range(2 * N):
                w = thr_w * side * np.eye(3)[k % 3] * (-1) ** (k // 3)
                lane(f"rate/thr*{side - 1:+.0e}", phase="inner" if F > 1 else None, w=w, pqr=w.copy(), om=np.full(4, hover * rng.uniform(0.7, 1.3)))

    if "rotor" in families:
        c_mid = 2 * (fmin + fmax)
        for thrust, tname in ((-2.0, "-2"), (4 * fmin, "4min"), (c_mid, "mid"), (4 * fmax, "4max"), (100.0, "100")):
            col = min(max(thrust, 4 * fmin), 4 * fmax) / 4
            eq = np.sqrt(col / kf)
            for rel in ("above", "below", "equal", "zero"):
                for _ in range(N // 2):
                    om = {"above": eq * rng.uniform(1.05, 2.0, 4), "below": eq * rng.uniform(0.1, 0.95, 4), "equal": np.full(4, eq),
                          "zero": np.zeros(4)}[rel]
                    lane(f"rotor/{tname}/{rel}", phase="inner", **still(thrust=thrust, pqr=np.zeros(3), om=om))

    if "alloc" in families:
        sat = lambda ax, head: head * 4 * (v["arm"] if ax < 2 else v["kappa"]) / (I[ax] * kp[ax])   # noqa: E731  pqr_cmd at which the limit is 1
        for _ in range(N):
            lane("alloc/zero", phase="inner", **still(pqr=np.zeros(3)))
        for ax in range(3):
            for _ in range(N):
                cmd = np.zeros(3); cmd[ax] = rng.uniform(0.05, 0.8) * sat(ax, 1.0) * rng.choice([-1, 1])
                lane(f"alloc/axis{ax}", phase="inner", **still(pqr=cmd))
        for side, thrust in (("top", 4 * fmax - rng.uniform(0.01, 1.0, N)), ("bottom", 4 * fmin + rng.uniform(0.01, 1.0, N))):
            for t in thrust:
                lane(f"alloc/sat-{side}", phase="inner", **still(thrust=float(t), pqr=rvec(20.0)))
        for t in (4 * fmin, 4 * fmax):
            for _ in range(N):
                lane("alloc/col-at-limit", phase="inner", **still(thrust=t, pqr=rvec(5.0)))
        for _ in range(N):
            lane("alloc/x1e3", phase="inner", **still(pqr=rvec(1e3 * sat(0, 2.0))))
        # the cross-multiplication tie: col exactly mid-range (up == dn in fp64) and a pure roll command (mpos == mneg)
        # (with min_thrust = 0.1 no fp64 col has equal head-room on both sides: the tie lanes live in the min_thrust = 0 vehicle)
        col = tie_collective(fmin, fmax)
        for _ in range(2 * N if col is not None else 0):
            cmd = np.array([rng.uniform(0.2, 3.0) * sat(0, 1.0) * rng.choice([-1, 1]), 0.0, 0.0])
            lane("alloc/tie", phase="inner", **still(thrust=4 * col, pqr=cmd))
        # na == nb: the largest |mf| equals the head-room exactly (searched among the neighbouring doubles of the command)
        for _ in range(N):
            thrust, pc = na_eq_nb_lane(v, rng)
            lane("alloc/na==nb", phase="inner", **still(thrust=thrust, pqr=np.array([pc, 0.0, 0.0])))

    if "outer" in families:
        for val in (10.0, -10.0, 10.5, -10.5):
            for _ in range(N):
                lane(f"outer/integ{val:+g}", phase="outer", integ=val)
        for val in (-v["max_ascent"], v["max_descent"], -v["max_ascent"] - 1.5, v["max_descent"] + 1.5):
            for _ in range(N):
                lane(f"outer/vz{val:+g}", phase="outer", tg={5: val})
        for sp, sname in ((0.5, "below"), (1.0, "at"), (1.7, "above")):
            for k in range(N):
                ax = k % 2
                vel = [0.0, 0.0]; vel[ax] = sp * v["max_speed_xy"] * (-1) ** (k // 2)
                if sname != "at":
                    vel[1 - ax] = 0.3 * rng.standard_normal()
                lane(f"outer/speed-{sname}", phase="outer", tg={3: vel[0], 4: vel[1]})
        for _ in range(N):
            pl = lane("outer/accel-sat", phase="outer")
            pl["rows"][pl["idx"], 0:2] = pl["p"][0:2] + 100.0 * _unit(rng.standard_normal(2))
        for ax in (0, 1):
            for sgn in (1.0, -1.0):
                for _ in range(N):
                    pl = lane(f"outer/tilt{'xy'[ax]}{sgn:+.0f}", phase="outer", q=q_axis([0, 0, 1], rng.uniform(-3, 3)), v=np.zeros(3))
                    pl["rows"][pl["idx"], 3:9] = 0.0
                    pl["rows"][pl["idx"], 0:3] = pl["p"]
                    pl["rows"][pl["idx"], ax] += sgn * 2.0          # kp_xy * 2 m = 32 m/s^2 -> clipped to 12 -> 12 / (c/m) > 0.7
        for lo, hi, yname in ((-TWO_PI, 0.0, "(-2pi,0)"), (0.0, TWO_PI, "[0,2pi)"), (TWO_PI, 2 * TWO_PI, "[2pi,4pi)"), (2 * TWO_PI, 30.0, ">=4pi"),
                              (-30.0, -TWO_PI, "<=-2pi")):
            for _ in range(N):
                lane(f"outer/yaw{yname}", phase="outer", tg={9: rng.uniform(lo + 1e-3, hi - 1e-3)})
        for val in (0.0, TWO_PI, -TWO_PI, 2 * TWO_PI, -2 * TWO_PI):
            for _ in range(N):
                lane(f"outer/yaw={val / np.pi:+.0f}pi", phase="outer", tg={9: val})
        for sgn in (1.0, -1.0):
            for off in (1e-6, -1e-6):
                for _ in range(N // 2):
                    pl = lane("outer/yaw-wrap", phase="outer")
                    pl["rows"][pl["idx"], 9] = _psi_of(pl["q"]) + sgn * np.pi + off

    if "ground" in families:
        zc = v["ground_z"] - v["ground_clearance"]
        # at rest on the plane, rotors stopped: 1e-6 either side of r = 0 (exactly on it the decision r > 0 has no margin and the lane
        # is excluded from the value comparison: two of those, the exclusion cap allows no more)
        for k in range(N + 2):
            r0 = 0.0 if k >= N else 1e-6 * (-1) ** k
            lane("ground/resting", p=np.array([rng.uniform(0, 20), rng.uniform(0, 12), zc + r0]), v=np.zeros(3), w=np.zeros(3), om=np.zeros(4),
                 q=np.array([1.0, 0, 0, 0]))
        for _ in range(N):
            lane("ground/clear", p=np.array([rng.uniform(0, 20), rng.uniform(0, 12), -rng.uniform(2, 6)]), gbits=2)
        for depth in (1e-6, 1e-3, 1e-2):
            for vz in (-0.5, 0.5):
                for rot in (0.0, 1.0, 1.9):                # stopped, hover, hard: vz_free on either side of vz_ref
                    for _ in range(4):
                        lane(f"ground/pressed{depth:g}", p=np.array([rng.uniform(0, 20), rng.uniform(0, 12), zc + depth]),
                             v=np.array([0.1 * rng.standard_normal(), 0.1 * rng.standard_normal(), vz * rng.uniform(0.2, 1)]),
                             om=np.full(4, rot * hover), omc=np.full(4, rot * hover), gbits=1)
        for depth in (-1e-6, -1e-3):
            for _ in range(N):
                lane(f"ground/above{-depth:g}", p=np.array([rng.uniform(0, 20), rng.uniform(0, 12), zc + depth]), v=rvec(0.01), gbits=0)
        for off in (1e-3, -1e-3, 1e-6, -1e-6):
            for _ in range(N):
                lane(f"ground/takeoff{off:+g}", p=np.array([rng.uniform(0, 20), rng.uniform(0, 12), v["ground_z"] - 0.1 - off]),
                     v=rvec(0.001), gbits=0)
        for _ in range(N):
            lane("ground/hit-after-takeoff", p=np.array([rng.uniform(0, 20), rng.uniform(0, 12), zc + rng.uniform(1e-3, 1e-2)]), v=rvec(0.05), gbits=2)

    if "sched" in families:
        for n, idx, sname in ((9, 0, "first"), (9, 4, "mid"), (9, 7, "penultimate"), (9, 8, "last"), (1, 0, "one-row")):
            for _ in range(N):
                lane(f"sched/{sname}", phase="outer", nrows=n, idx=idx)
        for ph in range(F):
            for _ in range(N):
                lane(f"sched/phase{ph}", phase=ph)

    while len(lanes) % 64 != 37:                           # never a whole number of 64-lane tiles
        lane("filler")

    B = len(lanes)
    state = np.zeros((30, B))
    istate = np.zeros((4, B), dtype=np.int32)
    offs = np.zeros(B + 1, dtype=np.int64)
    for b, d in enumerate(lanes):
        state[0:3, b], state[3:7, b], state[7:10, b], state[10:13, b] = d["p"], d["q"], d["v"], d["w"]
        state[13:17, b], state[17:21, b] = d["om"], d["omc"]
        state[21, b], state[22, b], state[23:26, b] = d["integ"], d["thrust"], d["pqr"]
        istate[:, b] = (d["idx"], d["inner"], 0, d["gbits"])
        offs[b + 1] = offs[b] + len(d["rows"])
    traj = np.concatenate([d["rows"] for d in lanes])
    assert np.isfinite(state).all() and np.isfinite(traj).all() and B % 64 != 0
    for a in (state, istate, offs, traj):
        a.setflags(write=False)
    return dict(name=name, state=state, istate=istate, traj=traj, row_offsets=offs, vehicle=v, labels=[d["label"] for d in lanes], B=B)


def hash_name(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31)


def cfg_families(name):
    return {"free-1ms-F10": ("norm", "pose", "rate", "rotor", "alloc", "outer", "sched"),
            "ground-2ms-F10": ("ground", "norm", "rate", "sched"),
            "free-1ms-F1": ("outer", "pose", "rate"),
            "free-2ms-F10-min0": ("rotor", "alloc", "rate")}[name]


def tie_collective(fmin, fmax):
    """A collective thrust per rotor with fmax - col == col - fmin exactly in fp64, next to the middle of the range, or None."""
    col = 0.5 * (fmin + fmax)
    for k in range(-64, 65):
        c = col
        for _ in range(abs(k)):
            c = np.nextafter(c, np.inf if k > 0 else -np.inf)
        if 4 * c * 0.25 == c and fmax - c == c - fmin:
            return float(c)
    return None


def na_eq_nb_lane(v, rng):
    """(thrust, roll-rate command) whose largest |mf| equals the head-room dn = col - min_thrust exactly (allocate's na == nb), with
    allocate's own operations (control_law.h: Mx = ikp pc, pb = Mx inv_arm, mf = pb / 4): draw the command, put col at
    mf + min_thrust, keep the draw when the subtraction gives mf back exactly."""
    ikp, inv_arm = v["inertia"][0] * v["kp_p"], 1.0 / v["arm"]
    for _ in range(1000):
        pc = float(rng.uniform(0.05, 0.5))
        mf = ((ikp * pc) * inv_arm) * 0.25
        col = mf + v["min_thrust"]
        thrust = 4.0 * col
        if thrust * 0.25 == col and col - v["min_thrust"] == mf and col - v["min_thrust"] < v["max_thrust"] - col:
            return thrust, pc * float(rng.choice([-1, 1]))
    raise AssertionError("no fp64 lane with mf == dn")


# ------------------------------------------------------------------------------------------ control_law.h restated in NumPy
def _floored_mod(a, b, mutate):
    ident = np.abs(a) < b
    sub = ~ident & (a >= b) & (a < 2.0 * b)
    r = np.where(ident, a, np.where(sub, a - b, np.fmod(a, b)))
    fix = (r != 0.0) & (r < 0.0)
    if mutate != "no_fixup":
        r = np.where(fix, r + b, r)
    return r, dict(ident=ident, sub=sub, fmod=~ident & ~sub, fix=fix)


def numpy_tick(fam, mutate=None):
    """One tick of every lane of `fam` with the formulas and the branch predicates of csrc/control_law.h (plain fp64, no fused
    multiply-adds) -> (state (26, B), cmd (12, B), istate (4, B), branches: dict of per-lane booleans / values).  `mutate` flips one
    thing: "s3_sign", "sin_times_wn", "rsqrt_e", "pos_wins", "no_fixup" (the mutation check of this file's tests)."""
    v, st, ist = fam["vehicle"], fam["state"], fam["istate"]
    B = fam["B"]
    offs = fam["row_offsets"]
    nrows = np.diff(offs)
    tg = fam["traj"][offs[:-1] + np.clip(ist[0], 0, nrows - 1)].T
    px, py, pz, q0, q1, q2, q3, vx, vy, vz, wp, wq, wr = (st[i].copy() for i in range(13))
    om, omc = st[13:17].copy(), st[17:21].copy()
    integ, thrust, pc, qc, rc = (st[i].copy() for i in (21, 22, 23, 24, 25))
    idx, inner, gbits = ist[0].copy(), ist[1].copy(), ist[3].copy()
    F, dt = v["inner_per_outer"], v["dt"]
    outer = (inner % F == 0) & (nrows > 0)
    fmin, fmax = v["min_thrust"], v["max_thrust"]
    c_min, c_max = 4.0 * fmin, 4.0 * fmax
    br = {"outer": outer}
    with np.errstate(all="ignore"):
        inv_n = 1.0 / np.sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3)
        a0, a1, a2, a3 = q0 * inv_n, q1 * inv_n, q2 * inv_n, q3 * inv_n
        R00, R01, R02 = 1.0 - 2.0 * (a2 * a2 + a3 * a3), 2.0 * (a1 * a2 - a0 * a3), 2.0 * (a1 * a3 + a0 * a2)
        R10, R11, R12 = 2.0 * (a1 * a2 + a0 * a3), 1.0 - 2.0 * (a1 * a1 + a3 * a3), 2.0 * (a2 * a3 - a0 * a1)
        R22 = 1.0 - 2.0 * (a1 * a1 + a2 * a2)
        zd = np.clip(tg[5], -v["max_ascent"], v["max_descent"])
        ez, ezd = tg[2] - pz, zd - vz
        integ_raw = integ + ez * v["dt_outer"]
        integ_o = np.clip(integ_raw, -10.0, 10.0)
        acc_z = (v["kp_z"] * ez + v["ki_z"] * integ_o + v["kd_z"] * ezd + tg[8] - v["g"]) / R22
        thrust_o = np.clip(-v["mass"] * acc_z, c_min, c_max)
        vm = np.sqrt(tg[3] * tg[3] + tg[4] * tg[4])
        spd = vm > v["max_speed_xy"]
        sc = np.where(spd, v["max_speed_xy"] / vm, 1.0)
        acx = v["kp_xy"] * (tg[0] - px) + v["kd_xy"] * (tg[3] * sc - vx) + tg[6]
        acy = v["kp_xy"] * (tg[1] - py) + v["kd_xy"] * (tg[4] * sc - vy) + tg[7]
        am = np.sqrt(acx * acx + acy * acy)
        asat = am > v["max_horiz_accel"]
        sc = np.where(asat, v["max_horiz_accel"] / am, 1.0)
        acx, acy = acx * sc, acy * sc
        inv_accz = -v["mass"] / thrust_o
        bx_raw, by_raw = acx * inv_accz, acy * inv_accz
        bxc, byc = np.clip(bx_raw, -v["max_tilt"], v["max_tilt"]), np.clip(by_raw, -v["max_tilt"], v["max_tilt"])
        bdx, bdy = v["kp_roll"] * (bxc - R02), v["kp_pitch"] * (byc - R12)
        pc_o, qc_o = (R10 * bdx - R00 * bdy) * (1.0 / R22), (R11 * bdx - R01 * bdy) * (1.0 / R22)
        sn, cn = 2.0 * (q0 * q1 + q2 * q3), 1.0 - 2.0 * (q1 * q1 + q2 * q2)
        h = np.sqrt(sn * sn + cn * cn)
        sphi, cphi = np.where(h > 0.0, sn / h, 0.0), np.where(h > 0.0, cn / h, 1.0)
        st_raw = 2.0 * (q0 * q2 - q3 * q1)
        st_ = np.clip(st_raw, -1.0, 1.0)
        cth = np.sqrt(np.maximum(1.0 - st_ * st_, 0.0))
        psi = np.arctan2(2.0 * (q0 * q3 + q1 * q2), 1.0 - 2.0 * (q2 * q2 + q3 * q3))
        pd, m1 = _floored_mod(tg[9], TWO_PI, mutate)
        wrap_arg = pd - psi + np.pi
        ye, m2 = _floored_mod(wrap_arg, TWO_PI, mutate)
        ye = ye - np.pi
        rc_o = (v["kp_yaw"] * ye * cth - qc_o * sphi) / cphi
        br.update(R22=R22, integ_raw=integ_raw, tzd=tg[5], vm=vm, spd=spd, asat=asat, bx_raw=bx_raw, by_raw=by_raw, h=h, st_raw=st_raw, cth=cth,
                  cphi=cphi, yaw=tg[9], mod1=m1, mod2=m2, wrap_margin=np.minimum(ye + np.pi, np.pi - ye))
        integ, thrust = np.where(outer, integ_o, integ), np.where(outer, thrust_o, thrust)
        pc, qc, rc = np.where(outer, pc_o, pc), np.where(outer, qc_o, qc), np.where(outer, rc_o, rc)
        idx = np.where(outer, np.minimum(idx + 1, nrows - 1), idx)
        # inner loop
        I = v["inertia"]
        ikp = (I[0] * v["kp_p"], I[1] * v["kp_q"], I[2] * v["kp_r"])
        Iwx, Iwy, Iwz = I[0] * wp, I[1] * wq, I[2] * wr
        Mx = ikp[0] * (pc - wp) + (wq * Iwz - wr * Iwy)
        My = ikp[1] * (qc - wq) + (wr * Iwx - wp * Iwz)
        Mz = ikp[2] * (rc - wr) + (wp * Iwy - wq * Iwx)
        col = np.clip(thrust, c_min, c_max) * 0.25
        up, dn = fmax - col, col - fmin
        pb, qb, rb = Mx * (1.0 / v["arm"]), My * (1.0 / v["arm"]), -Mz * (1.0 / v["kappa"])
        mf = np.stack([(pb + qb + rb) * 0.25, (-pb + qb - rb) * 0.25, (-pb - qb + rb) * 0.25, (pb - qb - rb) * 0.25])
        mpos, mneg = mf.max(axis=0), -mf.min(axis=0)
        lhs, rhs = up * mneg, dn * mpos
        pos_wins = lhs < rhs
        if mutate == "pos_wins":
            pos_wins = ~pos_wins
        na, nb = np.where(pos_wins, up, dn), np.where(pos_wins, mpos, mneg)
        scale = np.where(na < nb, na / nb, 1.0)
        f = np.clip(scale * mf + col, fmin, fmax)
        omc = np.sqrt(np.maximum(f * (1.0 / v["kf"]), 2.2250738585072014e-308))
        rise = omc > om
        resp = np.where(rise, 1.0 - np.exp(-dt / v["tau_rise"]), 1.0 - np.exp(-dt / v["tau_fall"]))
        om_in = om
        om = om + resp * (omc - om)
        br.update(up=up, dn=dn, mpos=mpos, mneg=mneg, lhs=lhs, rhs=rhs, na=na, nb=nb, mf=mf, f=f, rise=rise, om_in=om_in, omc=omc)
        cmd = np.stack([thrust, pc, qc, rc, *omc, *om])
        # vehicle
        qn2 = q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3
        window = np.abs(qn2 - 1.0) < 1.0e-12
        inv_n2 = np.where(window, 1.0, 1.0 / qn2)
        fr = v["kf"] * om * om
        T = fr[0] + fr[1] + fr[2] + fr[3]
        tx, ty = v["arm"] * (fr[0] + fr[3] - fr[1] - fr[2]), v["arm"] * (fr[0] + fr[1] - fr[2] - fr[3])
        tz = v["kappa"] * (-fr[0] + fr[1] - fr[2] + fr[3])
        s2 = 2.0 * inv_n2
        bzx, bzy, bzz = (q1 * q3 + q0 * q2) * s2, (q2 * q3 - q0 * q1) * s2, 1.0 - s2 * (q1 * q1 + q2 * q2)
        tm = T * (1.0 / v["mass"]) * dt
        vx, vy = vx - tm * bzx, vy - tm * bzy
        vz_free = dt * v["g"] + (vz - tm * bzz)
        zc = v["ground_z"] - v["ground_clearance"]
        if v["ground"]:
            tc = v["ground_timeconst"]
            r_in = pz - zc
            vz_ref = vz + dt * -((2.0 / tc) * vz + (1.0 / (tc * tc)) * r_in)
            use_ref = (r_in > 0.0) & (vz_ref < vz_free)
            vz = np.where(use_ref, vz_ref, vz_free)
            br.update(r_in=r_in, use_ref=use_ref)
        else:
            vz = vz_free
        cx, cy, cz = wq * Iwz - wr * Iwy, wr * Iwx - wp * Iwz, wp * Iwy - wq * Iwx
        wp, wq, wr = wp + dt * ((tx - cx) / I[0]), wq + dt * ((ty - cy) / I[1]), wr + dt * ((tz - cz) / I[2])
        px, py, pz = px + dt * vx, py + dt * vy, pz + dt * vz
        w2 = wp * wp + (wq * wq + wr * wr)
        h2 = 0.25 * dt * dt * w2
        large = h2 >= 1.0e-3
        s3 = 1.0 / 6 if mutate == "s3_sign" else -1.0 / 6
        ch_s = 1.0 + h2 * (-0.5 + h2 * (1.0 / 24 + h2 * (-1.0 / 720 + h2 * (1.0 / 40320))))
        sh_s = 0.5 * dt * (1.0 + h2 * (s3 + h2 * (1.0 / 120 + h2 * (-1.0 / 5040 + h2 * (1.0 / 362880)))))
        wn = np.sqrt(w2)
        hh = 0.5 * dt * wn
        sh_l = np.sin(hh) * wn if mutate == "sin_times_wn" else np.sin(hh) / wn
        ch, sh = np.where(large, np.cos(hh), ch_s), np.where(large, sh_l, sh_s)
        d1, d2, d3 = sh * wp, sh * wq, sh * wr
        n0 = q0 * ch - (q1 * d1 + (q2 * d2 + q3 * d3))
        n1 = q0 * d1 + (q1 * ch + (q2 * d3 - q3 * d2))
        n2 = q0 * d2 + (q2 * ch + (q3 * d1 - q1 * d3))
        n3 = q0 * d3 + (q3 * ch + (q1 * d2 - q2 * d1))
        e = (n0 * n0 + (n1 * n1 + (n2 * n2 + n3 * n3))) - 1.0
        rsq = np.abs(e) > 1.0e-6
        inv = np.where(rsq, 1.0 / np.sqrt(e if mutate == "rsqrt_e" else e + 1.0), 1.0 + e * (-0.5 + e * 0.375))
        q0, q1, q2, q3 = n0 * inv, n1 * inv, n2 * inv, n3 * inv
        br.update(window=window, large=large, h2=h2, e=e, rsq=rsq, qn2=qn2)
        if v["ground"]:
            gbits = np.where(v["ground_z"] - pz >= 0.1, gbits | 2, gbits)
            touch = pz - zc > 0.0
            gbits = np.where(touch, gbits | 1, gbits & ~1)
            gbits = np.where(touch & ((gbits & 2) != 0), gbits | 4, gbits)
            br.update(touch=touch, r_out=pz - zc, takeoff_margin=v["ground_z"] - pz - 0.1)
    new = np.stack([px, py, pz, q0, q1, q2, q3, vx, vy, vz, wp, wq, wr, *om, *omc, integ, thrust, pc, qc, rc])
    return new, cmd, np.stack([idx, inner + 1, ist[2], gbits]).astype(np.int32), br


def census(fams):
    """-> {mask name: lanes over all configurations that take that branch}, every predicate restated from control_law.h."""
    out = {}

    def add(name, m):
        out[name] = out.get(name, 0) + int(np.count_nonzero(m))

    for fam in fams:
        _, _, _, b = numpy_tick(fam)
        v, o = fam["vehicle"], b["outer"]
        F = v["inner_per_outer"]
        inner_only = ~o
        off_unit = ~b["window"]
        add("free_body/taylor", ~b["large"]); add("free_body/large-rotation", b["large"])
        thr = np.abs(b["h2"] / 1e-3 - 1) < 1e-5
        add("free_body/just-below-threshold", thr & ~b["large"]); add("free_body/just-above-threshold", thr & b["large"])
        add("renorm/series-off-unit", off_unit & ~b["rsq"]); add("renorm/rsqrt", b["rsq"])
        add("renorm/just-below-e_small", ~b["rsq"] & (np.abs(b["e"]) > 5e-7)); add("renorm/just-above-e_small", b["rsq"] & (np.abs(b["e"]) < 2e-6))
        add("inv_n2/exactly-one-off-unit", b["window"] & (b["qn2"] != 1.0) & (np.abs(b["qn2"] - 1) > 1e-13)); add("inv_n2/reciprocal", off_unit)
        add("inv_n2/reciprocal-near-window", off_unit & (np.abs(b["qn2"] - 1) < 1e-10))
        y, m1, m2 = b["yaw"], b["mod1"], b["mod2"]
        add("floored_mod/(-2pi,0)", o & m1["ident"] & (y < 0)); add("floored_mod/[0,2pi)", o & m1["ident"] & (y >= 0))
        add("floored_mod/[2pi,4pi)", o & m1["sub"]); add("floored_mod/fmod>=4pi", o & m1["fmod"] & (y > 0))
        add("floored_mod/fmod<=-2pi", o & m1["fmod"] & (y < 0)); add("floored_mod/fix-up", o & m1["fix"])
        add("floored_mod/fmod-with-fix-up", o & m1["fmod"] & m1["fix"])
        add("floored_mod/a==0", o & (y == 0)); add("floored_mod/a==+-2pi", o & (np.abs(y) == TWO_PI)); add("floored_mod/a==+-4pi", o & (np.abs(y) == 2 * TWO_PI))
        add("yaw/wrap-sub", o & m2["sub"])          # (pd in [0, 2 pi) and psi in [-pi, pi]: pd - psi + pi >= 0, the second fix-up cannot fire)
        add("yaw/within-2e-6-of-wrap", o & (b["wrap_margin"] < 2e-6) & (b["wrap_margin"] > 1e-7))
        has = b["mpos"] > 0
        add("allocate/pos-wins", inner_only & has & (b["lhs"] < b["rhs"])); add("allocate/neg-wins", inner_only & has & (b["lhs"] > b["rhs"]))
        add("allocate/cross-tie", inner_only & has & (b["lhs"] == b["rhs"]) & (b["up"] == b["dn"]) & (b["mpos"] == b["mneg"]))
        add("allocate/na==nb", inner_only & has & (b["na"] == b["nb"])); add("allocate/scaled", inner_only & (b["na"] < b["nb"]))
        add("allocate/unscaled", inner_only & has & (b["na"] > b["nb"])); add("allocate/all-mf-zero", inner_only & (b["mf"] == 0).all(axis=0))
        add("allocate/col-at-min", inner_only & (b["dn"] == 0)); add("allocate/col-at-max", inner_only & (b["up"] == 0))
        add("allocate/1e3x", inner_only & (b["nb"] > 500 * b["na"]) & (b["na"] > 0))
        add("motors/rise", inner_only & b["rise"].all(axis=0)); add("motors/fall", inner_only & (b["omc"] < b["om_in"]).all(axis=0))
        add("motors/tie", inner_only & (b["omc"] == b["om_in"]).all(axis=0)); add("motors/f==0", inner_only & (b["f"] == 0).all(axis=0))
        add("motors/omega==0", inner_only & (b["om_in"] == 0).all(axis=0))
        add("euler/h==0", o & (b["h"] == 0)); add("euler/asin-clamp", o & (np.abs(b["st_raw"]) >= 1)); add("euler/cos-theta<1e-6", o & (b["cth"] < 1e-6))
        add("euler/cos-phi-small", o & (np.abs(b["cphi"]) < 2e-2) & (b["h"] > 0))
        add("R22/small", o & (np.abs(b["R22"]) < 1.5e-2)); add("R22/negative", o & (b["R22"] < 0))
        add("outer/integ-clamp-hi", o & (b["integ_raw"] > 10)); add("outer/integ-clamp-lo", o & (b["integ_raw"] < -10))
        add("outer/ascent-clamp", o & (b["tzd"] < -v["max_ascent"])); add("outer/descent-clamp", o & (b["tzd"] > v["max_descent"]))
        add("outer/ascent-at", o & (b["tzd"] == -v["max_ascent"])); add("outer/descent-at", o & (b["tzd"] == v["max_descent"]))
        add("outer/speed-sat", o & b["spd"]); add("outer/speed-at", o & (b["vm"] == v["max_speed_xy"])); add("outer/accel-sat", o & b["asat"])
        add("outer/tilt-x+", o & (b["bx_raw"] > v["max_tilt"])); add("outer/tilt-x-", o & (b["bx_raw"] < -v["max_tilt"]))
        add("outer/tilt-y+", o & (b["by_raw"] > v["max_tilt"])); add("outer/tilt-y-", o & (b["by_raw"] < -v["max_tilt"]))
        if v["ground"]:
            ist = fam["istate"]
            add("ground/resting", (np.abs(b["r_in"]) < 2e-6) & (fam["state"][13:17] == 0).all(axis=0)); add("ground/pressed-ref", b["use_ref"]); add("ground/pressed-free", (b["r_in"] > 0) & ~b["use_ref"])
            add("ground/clear", b["r_in"] < -1); add("ground/takeoff-just-above", (b["takeoff_margin"] >= 0) & (b["takeoff_margin"] < 2e-3) & (ist[3] & 2 == 0))
            add("ground/takeoff-just-below", (b["takeoff_margin"] < 0) & (b["takeoff_margin"] > -2e-3))
            add("ground/contact-after-takeoff", b["touch"] & (ist[3] & 2 != 0))
        nrows = np.diff(fam["row_offsets"])
        add("sched/cursor-0", o & (fam["istate"][0] == 0) & (nrows > 1)); add("sched/cursor-last", o & (fam["istate"][0] == nrows - 1) & (nrows > 1))
        add("sched/cursor-penultimate", o & (fam["istate"][0] == nrows - 2)); add("sched/one-row", o & (nrows == 1))
        if F == 10:
            for ph in range(F):
                add(f"sched/phase-{ph}", fam["istate"][1] % F == ph)
    return out


# ------------------------------------------------------------------------------------------ the references and the bound
@functools.lru_cache(maxsize=None)
def reference(name, K=1):
    """Both oracles, K ticks from every lane of build(name) -> dict: t_* (long double), r_* (fp64): state (26, B), slog (K, 13, B),
    clog (K, 12, B), istate (4, B); margins (5, B) of the first tick.  Computed once per session, read-only."""
    from oracle import c_oracle as cc
    fam = build(name)
    B, offs = fam["B"], fam["row_offsets"]
    V = make_vehicle(cc.Vehicle, fam["vehicle"])
    out = {k: np.empty(s, d) for k, s, d in (("t_state", (26, B), float), ("r_state", (26, B), float), ("t_slog", (K, 13, B), float),
                                             ("r_slog", (K, 13, B), float), ("t_clog", (K, 12, B), float), ("r_clog", (K, 12, B), float),
                                             ("t_istate", (4, B), np.int32), ("r_istate", (4, B), np.int32), ("margins", (5, B), float))}
    for b in range(B):
        rows = np.ascontiguousarray(fam["traj"][offs[b]:offs[b + 1]])
        s0, i0 = np.ascontiguousarray(fam["state"][:26, b]), np.ascontiguousarray(fam["istate"][:, b])
        out["margins"][:, b] = cc.tick_margins_ld(rows, s0, i0, V)
        for tag, fn in (("t", cc.rollout_ld), ("r", cc.rollout)):
            s, i = s0.copy(), i0.copy()
            sl, cl = fn(rows, s, i, K, V)
            out[f"{tag}_state"][:, b], out[f"{tag}_istate"][:, b] = s, i
            out[f"{tag}_slog"][:, :, b], out[f"{tag}_clog"][:, :, b] = sl, cl
    for a in out.values():
        a.setflags(write=False)
    return out


def excluded(name):
    """Lanes whose long-double tick takes a discontinuous decision with a margin under 1e-9."""
    return (reference(name)["margins"] < MARGIN).any(axis=0)


def bound(t, r, margin=M_BOUND, kappa=1.0, extra=0.0):
    return margin * np.maximum(np.maximum(np.abs(r - t), U_FLOOR * 2.0 ** -53 * kappa * np.maximum(1.0, np.abs(t))), extra)


def rotor_floor(v, t_omc, t_om, ticks=1):
    """The floor of ROTOR FLOOR in the module docstring -> (state (26, B), state log (13, B), command log (12, B)) absolute terms, from
    the long-double omega_cmd t_omc (..., 4, B) and omega t_om (..., 4, B) of the tick(s); over `ticks` ticks the vehicle integrates it."""
    K = ticks
    d = U_FLOOR * 2.0 ** -53 * max(1.0, v["max_thrust"]) / v["kf"]
    lead = tuple(range(t_omc.ndim - 1))
    e_omc = (d / np.maximum(np.abs(t_omc), np.sqrt(d))).max(axis=lead)
    e_om = min(1.0, K * (1.0 - np.exp(-v["dt"] / min(v["tau_rise"], v["tau_fall"])))) * e_omc      # the lag contracts
    e_T = 4 * 2 * v["kf"] * np.abs(t_om).max(axis=lead) * e_om
    e_v = K * v["dt"] * e_T / v["mass"]
    e_w = K * v["dt"] * max(v["arm"], v["kappa"]) * e_T / min(v["inertia"])
    B = t_omc.shape[-1]
    st, cl = np.zeros((26, B)), np.zeros((12, B))
    st[0:3], st[3:7], st[7:10], st[10:13] = K * v["dt"] * e_v, K * 0.5 * v["dt"] * e_w, e_v, e_w
    st[13:17], st[17:21] = e_om, e_omc
    cl[4:8], cl[8:12] = e_omc, e_om
    return st, st[:13].copy(), cl


def rotors_well_conditioned(v, t_omc):
    """Lanes whose reference never commands a rotor below a quarter of the hover speed in the ticks t_omc (K, 4, B): there the rotor
    floor stays within 4x its hover size (for a vehicle with min_thrust >= m g / 64 that is every lane)."""
    return (np.abs(t_omc) >= 0.25 * np.sqrt(v["mass"] * v["g"] / (4 * v["kf"]))).all(axis=(0, 1))


def pose_conditioning(q):
    """kappa of the module docstring for the attitudes q (4, ...): how much the outer loop amplifies one rounding error of its divisors."""
    with np.errstate(all="ignore"):
        n2 = (q * q).sum(axis=0)
        R22 = 1.0 - 2.0 * (q[1] * q[1] + q[2] * q[2]) / n2
        sn, cn = 2.0 * (q[0] * q[1] + q[2] * q[3]), 1.0 - 2.0 * (q[1] * q[1] + q[2] * q[2])
        h = np.sqrt(sn * sn + cn * cn)
        cphi = np.where(h > 0.0, np.abs(cn) / h, 1.0)
        st = 2.0 * (q[0] * q[2] - q[3] * q[1])
        cth = np.where(np.abs(st) < 1.0, np.sqrt(np.abs(1.0 - st * st)), 1.0)       # (clamped: cos_theta is exactly 0, nothing to amplify)
        k = np.maximum(1.0, 1.0 / np.abs(R22)) * np.maximum(1.0, 1.0 / cphi) * np.maximum(1.0, 1.0 / cth)
    return np.where(np.isfinite(k), k, 1.0)


def conditioning(fam):
    """Per lane: pose_conditioning of the attitude on a tick that runs the outer loop, 1 on an inner-only tick."""
    nrows = np.diff(fam["row_offsets"])
    outer = (fam["istate"][1] % fam["vehicle"]["inner_per_outer"] == 0) & (nrows > 0)
    return np.where(outer, pose_conditioning(fam["state"][3:7]), 1.0)


GROUPS = (("position", slice(0, 3)), ("attitude", slice(3, 7)), ("velocity", slice(7, 10)), ("rates", slice(10, 13)),
          ("rotors", slice(13, 21)), ("commands", slice(21, 26)))


def worst_ratios(fam, g, t, r):
    """{family: {output group: worst |g - t| / bound}} over the 26 state rows (excluded lanes left out by the caller)."""
    with np.errstate(all="ignore"):
        ratio = np.abs(g - t) / bound(t, r, kappa=conditioning(fam), extra=rotor_floor(fam["vehicle"], t[17:21], t[13:17])[0])
    heads = np.array([lab.split("/")[0] for lab in fam["labels"]])
    return {h: {gname: float(np.nanmax(ratio[sl][:, heads == h])) for gname, sl in GROUPS} for h in sorted(set(heads))}


def assert_within_bound(what, fam, g, t, r, keep, margin=M_BOUND, kappa=None, extra=0.0):
    """|g - t| <= margin max(|r - t|, U kappa ulp, extra) for every kept lane and output; the message names the worst lanes."""
    assert np.isfinite(t[..., keep]).all() and np.isfinite(r[..., keep]).all(), f"{what}: the reference is not finite"
    kappa = conditioning(fam) if kappa is None else kappa
    bad = ~(np.abs(g - t) <= bound(t, r, margin, kappa, extra)) & keep
    if bad.any():
        idx = np.argwhere(bad)
        ratio = np.abs(g - t) / bound(t, r, margin, kappa, extra)
        worst = sorted(idx.tolist(), key=lambda i: -np.nan_to_num(ratio[tuple(i)], nan=np.inf))[:12]
        lines = [f"{fam['labels'][i[-1]]} lane {i[-1]} out {i[:-1]}: g={g[tuple(i)]!r} t={t[tuple(i)]!r} r={r[tuple(i)]!r} x{ratio[tuple(i)]:.3g}" for i in worst]
        raise AssertionError(f"{what} [{fam['name']}]: {len(idx)} values of {len(set(idx[:, -1].tolist()))} lanes beyond the bound\n" + "\n".join(lines))


def assert_actuators_sane(fam, state, clog, lanes):
    v = fam["vehicle"]
    assert np.isfinite(state[:, lanes]).all() and np.isfinite(clog[..., lanes]).all()
    lo, hi = np.sqrt(v["min_thrust"] / v["kf"]), np.sqrt(v["max_thrust"] / v["kf"])
    omc = state[17:21, lanes]
    assert (omc >= lo * (1 - 1e-12) - 1e-150).all() and (omc <= hi * (1 + 1e-12)).all()
    th = state[22, lanes]
    assert (th >= 4 * v["min_thrust"]).all() and (th <= 4 * v["max_thrust"]).all()


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    return Engine("cuda:0")


@pytest.fixture(scope="module")
def need_ld():
    from oracle import c_oracle as cc
    if cc.lib().oracle_ldbl_mant_dig() < 64:
        pytest.skip("long double is no wider than double here")


def _P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


class Launcher:
    """Fresh device copies of one family's (state, istate) and every form of the tick on them."""

    def __init__(self, eng, fam):
        import torch
        from uav_ac import _native as nat
        self.eng, self.fam, self.torch, self.nat = eng, fam, torch, nat
        self.V = make_vehicle(nat.Vehicle, fam["vehicle"])
        self.rows = torch.as_tensor(fam["traj"].copy(), device=eng.device)
        self.offs = torch.as_tensor(fam["row_offsets"].copy(), device=eng.device)
        self.B = fam["B"]
        eng._bind_stream()

    def fresh(self, lanes=slice(None)):
        st = self.torch.as_tensor(self.fam["state"][:, lanes].copy(), device=self.eng.device)
        ist = self.torch.as_tensor(self.fam["istate"][:, lanes].copy(), device=self.eng.device)
        return st, ist

    def rollout(self, K=1, slog=True, clog=True, score=False, pitch=0, lanes=slice(None), state=None):
        torch, eng = self.torch, self.eng
        st, ist = state if state is not None else self.fresh(lanes)
        B = st.shape[1]
        b0 = 0 if lanes == slice(None) else lanes.start
        offs = self.offs[b0:b0 + B + 1].contiguous()
        P = pitch or B
        # NaN-filled logs: a column the kernel must write and did not shows up
        sl = torch.full((K, 13, P), float("nan"), dtype=torch.float64, device=eng.device) if slog else None
        cl = torch.full((K, 12, P), float("nan"), dtype=torch.float64, device=eng.device) if clog else None
        if pitch:
            eng.ctx.set_option("log_pitch", pitch)
        try:
            if score:
                sc = torch.zeros((self.nat.SCORE_ROWS, B), dtype=torch.float64, device=eng.device)
                eng.ctx.call("uavac_control_rollout_scored_dev", C.byref(self.V), _P(self.rows), _P(offs), _P(st), _P(ist), B, K, _P(sl), None, None, 0, _P(sc))
            else:
                eng.ctx.call("uavac_control_rollout_dev", C.byref(self.V), _P(self.rows), _P(offs), _P(st), _P(ist), B, K, _P(sl), _P(cl), None, 0)
        finally:
            if pitch:
                eng.ctx.set_option("log_pitch", 0)
        return st, ist, (None if sl is None else sl[:, :, :B]), (None if cl is None else cl[:, :, :B])

    def step(self):
        st, ist = self.fresh()
        self.eng.ctx.call("uavac_control_step_dev", C.byref(self.V), _P(self.rows), _P(self.offs), _P(st), _P(ist), self.B)
        return st, ist

    def split_tick(self):
        st, ist = self.fresh()
        self.eng.ctx.call("uavac_controller_tick_dev", C.byref(self.V), _P(self.rows), _P(self.offs), _P(st), _P(ist), self.B)
        self.eng.ctx.call("uavac_dynamics_step_dev", C.byref(self.V), _P(st), _P(ist), self.B, None, 0)
        return st, ist


@functools.lru_cache(maxsize=None)
def _gpu_tick(eng, name):
    """One tick with both logs from every lane of the family, on the host: (state (30, B), istate (4, B), slog (1, 13, B), clog)."""
    st, ist, sl, cl = Launcher(eng, build(name)).rollout(1)
    return tuple(x.cpu().numpy() for x in (st, ist, sl, cl))


NAMES = [c[0] for c in CONFIGS]


@pytest.mark.parametrize("name", NAMES)
def test_one_tick_equals_the_long_double_oracle(eng, need_ld, name):
    """State rows 0-25, the 13 state-log rows, the 12 command-log rows within the bound of the module docstring, istate equal,
    lane by lane; excluded lanes (at most 0.5 %) finite and inside the actuator limits.  Observed worst |g - t| / bound per family
    and output group: profiles/one_tick_parity.json (UAVAC_ONE_TICK_PROFILE=<file> rewrites this configuration's entry)."""
    fam, ref = build(name), reference(name)
    st, ist, sl, cl = _gpu_tick(eng, name)
    ex = excluded(name)
    keep = ~ex
    assert ex.mean() <= 0.005, (name, int(ex.sum()))
    prof = os.environ.get("UAVAC_ONE_TICK_PROFILE")
    if prof:
        data = json.load(open(prof)) if os.path.exists(prof) else {}
        data[name] = {"lanes": fam["B"], "excluded": int(ex.sum()),
                      "worst_ratio": _ratios_kept(fam, st[:26], ref, keep)}
        json.dump(data, open(prof, "w"), indent=1, sort_keys=True)
    assert_actuators_sane(fam, st, cl, ex)
    x_st, x_sl, x_cl = rotor_floor(fam["vehicle"], ref["t_state"][17:21], ref["t_state"][13:17])
    assert_within_bound("state", fam, st[:26], ref["t_state"], ref["r_state"], keep, extra=x_st)
    assert_within_bound("state log", fam, sl, ref["t_slog"], ref["r_slog"], keep, extra=x_sl)
    assert_within_bound("command log", fam, cl, ref["t_clog"], ref["r_clog"], keep, extra=x_cl)
    assert np.array_equal(sl[0], st[0:13]) and np.array_equal(cl[0, 0], st[22]) and np.array_equal(cl[0, 8:12], st[13:17])
    assert np.array_equal(ist[:, keep], ref["t_istate"][:, keep]), np.flatnonzero((ist != ref["t_istate"]).any(axis=0) & keep)[:8]
    assert np.array_equal(ist[0:3], ref["t_istate"][0:3])


def _ratios_kept(fam, g, ref, keep):
    g = np.where(keep, g, ref["t_state"])                   # an excluded lane contributes ratio 0
    return worst_ratios(fam, g, ref["t_state"], ref["r_state"])


@pytest.mark.parametrize("name", NAMES)
def test_every_form_of_the_tick_gives_the_same_bits(eng, name):
    """From the same arbitrary states: no log, either log alone, the scored twin, uavac_control_step_dev, the split tick
    (controller tick + dynamics step: the second copy of the inv_n2 selection), a pitched log, and the batch cut into two
    launches of different B, all equal the both-logs launch bit for bit."""
    import torch
    fam = build(name)
    L = Launcher(eng, fam)
    B = fam["B"]
    st0, ist0, sl0, cl0 = L.rollout(1)

    def same(what, st, ist, sl=None, cl=None, rows=30):
        assert torch.equal(st[:rows].view(torch.int64), st0[:rows].view(torch.int64)), (name, what, "state")
        assert torch.equal(ist, ist0), (name, what, "istate")
        assert sl is None or torch.equal(sl.view(torch.int64), sl0.view(torch.int64)), (name, what, "state log")
        assert cl is None or torch.equal(cl.view(torch.int64), cl0.view(torch.int64)), (name, what, "command log")

    same("no log", *L.rollout(1, slog=False, clog=False))
    same("state log", *L.rollout(1, clog=False))
    same("command log", *L.rollout(1, slog=False))
    same("scored", *L.rollout(1, clog=False, score=True))
    same("control_step", *L.step())
    same("split tick", *L.split_tick())
    pitch = (B + 15) // 16 * 16 + 16
    same("pitched log", *L.rollout(1, pitch=pitch))
    cut = B // 3 + 1
    a, b = L.rollout(1, lanes=slice(0, cut)), L.rollout(1, lanes=slice(cut, B))
    same("two launches", torch.cat([a[0], b[0]], dim=1), torch.cat([a[1], b[1]], dim=1), torch.cat([a[2], b[2]], dim=2), torch.cat([a[3], b[3]], dim=2))


@pytest.mark.parametrize("name", [n for n in NAMES if "F10" in n])
def test_across_an_outer_tick(eng, need_ld, name):
    """K = F + 1 in one launch == launches of 1 + F bit for bit, and equals the long-double oracle within the bound for the lanes
    whose oracle rates stay below 40 rad/s (tests/test_gpu_fuzz.py's rule: a vehicle that has not tumbled away) and whose oracle rotor commands stay
    away from 0 (ROTOR FLOOR in the module docstring)."""
    import torch
    fam = build(name)
    K = fam["vehicle"]["inner_per_outer"] + 1
    L = Launcher(eng, fam)
    st, ist, sl, cl = L.rollout(K)
    s1, i1, sl1, cl1 = L.rollout(1)
    s2, i2, sl2, cl2 = L.rollout(K - 1, state=(s1, i1))
    assert torch.equal(st[:26].view(torch.int64), s2[:26].view(torch.int64)) and torch.equal(ist, i2)
    assert torch.equal(sl.view(torch.int64), torch.cat([sl1, sl2]).view(torch.int64))
    assert torch.equal(cl.view(torch.int64), torch.cat([cl1, cl2]).view(torch.int64))
    ref = reference(name, K)
    tame = np.isfinite(ref["r_slog"]).all(axis=(0, 1)) & np.isfinite(ref["t_slog"]).all(axis=(0, 1))
    tame &= (np.abs(np.where(np.isfinite(ref["r_slog"][:, 10:13]), ref["r_slog"][:, 10:13], np.inf)).max(axis=(0, 1)) < 40.0)
    tame &= np.abs(fam["state"][10:13]).max(axis=0) < 40.0
    tame &= ~excluded(name) & ~_decides_by_a_hair_later(fam, ref)
    # ... and whose reference commands no rotor to (nearly) zero on the way: the sqrt at 0 of ROTOR FLOOR is an ill-conditioned value
    # that K ticks and the outer loop inside them amplify, like a tumble (only the min_thrust = 0 vehicle has such lanes)
    tame &= rotors_well_conditioned(fam["vehicle"], ref["t_clog"][:, 4:8])
    assert tame.sum() >= 64                                  # more than a tile of lanes is compared
    g = st.cpu().numpy()
    # the outer loop runs somewhere inside the K ticks: the worst conditioning among the start and the reference's logged attitudes
    kappa = np.maximum(pose_conditioning(fam["state"][3:7]), pose_conditioning(ref["t_slog"][:, 3:7].transpose(1, 0, 2)).max(axis=0))
    x_st, x_sl, x_cl = rotor_floor(fam["vehicle"], ref["t_clog"][:, 4:8], ref["t_clog"][:, 8:12], ticks=K)
    assert_within_bound("state after F + 1 ticks", fam, g[:26], ref["t_state"], ref["r_state"], tame, kappa=kappa, extra=x_st)
    assert_within_bound("state log", fam, sl.cpu().numpy(), ref["t_slog"], ref["r_slog"], tame, kappa=kappa, extra=x_sl)
    assert_within_bound("command log", fam, cl.cpu().numpy(), ref["t_clog"], ref["r_clog"], tame, kappa=kappa, extra=x_cl)
    assert np.array_equal(ist.cpu().numpy()[:, tame], ref["t_istate"][:, tame])


def _decides_by_a_hair_later(fam, ref):
    """Lanes whose ground decisions (r > 0, the take-off height) fall within 1e-9 in one of the later ticks of the K-tick reference."""
    v = fam["vehicle"]
    if not v["ground"]:
        return np.zeros(fam["B"], bool)
    z = ref["t_slog"][:, 2]
    zc = v["ground_z"] - v["ground_clearance"]
    return ((np.abs(z - zc) < MARGIN) | (np.abs(v["ground_z"] - z - 0.1) < MARGIN)).any(axis=0)


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform-m6", "ragged"])
def test_plan_fed_tick_from_arbitrary_states(eng, need_ld, ragged):
    """256 planned missions, random in-range cursors, the body / rotor / attitude / scheduling families (ragged batch: with the
    ground plane and its family too) on the vehicles, carried yaw scan invalidated (state row 26 = -1, as Fleet does after a
    replan): plan-fed by scan, by dense yaw column and through the ragged entry point, and row-fed on the sampled rows, all bit
    for bit the same tick; that tick equals the long-double oracle on the sampled rows within the bound."""
    import torch
    from uav_ac import _native as nat
    from oracle import c_oracle as cc
    from oracle import minsnap_oracle as mo
    name = "ground-2ms-F10" if ragged else "free-1ms-F10"
    fam = build(name)
    v = dict(fam["vehicle"])
    B, m, F = 256, 6, v["inner_per_outer"]
    pdt = v["dt"] * F
    rng = np.random.default_rng(77 + ragged)
    wps = mo.synthetic_missions(B, m)
    if ragged:
        counts = rng.integers(1, m + 1, B)
        plan = eng.plan_ragged([wps[b, :counts[b] + 1] for b in range(B)], 2.0, pdt)
        seg_offsets, max_m = plan.seg_offsets, plan.max_m
    else:
        plan = eng.plan(wps, 2.0, pdt, dense_yaw=True)
        seg_offsets, max_m = torch.arange(B + 1, dtype=torch.int64, device=eng.device) * m, m
    heads = np.array([lab.split("/")[0] for lab in fam["labels"]])
    pick = rng.permutation(np.flatnonzero(np.isin(heads, ("rate", "rotor", "norm", "pose", "ground", "sched"))))[:B]
    assert len(pick) == B
    ro = plan.row_offsets.cpu().numpy()
    nrows = np.diff(ro)
    state0 = fam["state"][:, pick].copy()
    istate0 = fam["istate"][:, pick].copy()
    istate0[0] = rng.integers(0, nrows)
    istate0[0, :8] = nrows[:8] - 1
    istate0[0, 8:16] = 0
    state0[26] = -1.0
    V = make_vehicle(nat.Vehicle, v)
    eng._bind_stream()

    def run(form):
        st, ist = torch.as_tensor(state0, device=eng.device), torch.as_tensor(istate0, device=eng.device)
        sl = torch.full((1, 13, B), float("nan"), dtype=torch.float64, device=eng.device)
        cl = torch.full((1, 12, B), float("nan"), dtype=torch.float64, device=eng.device)
        tail = (_P(st), _P(ist), B, 1, _P(sl), _P(cl), None, 0)
        if form == "rows":
            eng.ctx.call("uavac_control_rollout_dev", C.byref(V), _P(plan.traj), _P(plan.row_offsets), *tail)
        elif form == "ragged":
            eng.ctx.call("uavac_control_rollout_plan_ragged_dev", C.byref(V), _P(plan.coeffs), _P(plan.seg_rows), _P(seg_offsets), _P(plan.row_offsets),
                         _P(plan.first_yaw), int(max_m), pdt, *tail)
        else:
            eng.ctx.call("uavac_control_rollout_plan_dev", C.byref(V), _P(plan.coeffs), _P(plan.seg_rows), _P(plan.row_offsets),
                         _P(plan.yaw) if form == "dense" else None, _P(plan.first_yaw), m, pdt, *tail)
        return st, ist, sl, cl

    base = run("rows")
    for form in (("ragged",) if ragged else ("scan", "dense", "ragged")):
        got = run(form)
        for what, a, b in zip(("state", "istate", "state log", "command log"), got, base):
            a, b = (a[:26], b[:26]) if what == "state" else (a, b)
            assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b), (form, what)
    rows = plan.traj.cpu().numpy()
    Vc = make_vehicle(cc.Vehicle, v)
    t, r, ti = np.empty((26, B)), np.empty((26, B)), np.empty((4, B), np.int32)
    ex = np.zeros(B, bool)
    for b in range(B):
        mission = np.ascontiguousarray(rows[ro[b]:ro[b + 1]])
        s0, i0 = np.ascontiguousarray(state0[:26, b]), np.ascontiguousarray(istate0[:, b])
        ex[b] = (cc.tick_margins_ld(mission, s0, i0, Vc) < MARGIN).any()
        for out, fn in ((t, cc.rollout_ld), (r, cc.rollout)):
            s, i = s0.copy(), i0.copy()
            fn(mission, s, i, 1, Vc, log_state=False, log_cmd=False)
            out[:, b] = s
            ti[:, b] = i
    assert ex.mean() <= 0.005
    sub = dict(fam, labels=[fam["labels"][i] for i in pick])
    kappa = np.where(istate0[1] % F == 0, pose_conditioning(state0[3:7]), 1.0)
    assert_within_bound("plan-fed state", sub, base[0].cpu().numpy()[:26], t, r, ~ex, kappa=kappa, extra=rotor_floor(v, t[17:21], t[13:17])[0])
    assert np.array_equal(base[1].cpu().numpy()[:, ~ex], ti[:, ~ex])
