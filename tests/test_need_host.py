"""Retiming to the tilt and thrust limits, the parts that need no GPU: `scoring.need_from_rows` -- the NumPy specification of
`uavac_minsnap_need_dev` -- on hand-made one-row missions whose answers are exact and on the C oracle's rows; the extended rule
`scoring.retime_factors(..., need=...)` with its `binding`; and the plumbing: the library exports the three entry points and the ctypes
table and constants say what include/uavac.h says.

Slowing a mission by k leaves its curve in place and divides its accelerations by u = k^2.  The expected values below are written out
with Python floats (IEEE double, one operation at a time) from the closed forms, not taken from the function:
    tilt        u >= (tau az + sqrt(q)) / (tau g),  q = max(ax^2 - tau^2 h, ay^2 - tau^2 h, 0) > 0, h = ax^2 + ay^2
    upright     u >= az / g
    thrust max  u >= (sqrt((g az)^2 + |a|^2 D) - g az) / D,  D = Fmax^2 - g^2
    thrust min  u >= (g az + sqrt((g az)^2 - |a|^2 E)) / E,  E = g^2 - Fmin^2, where az > 0 and the root exists
and need = sqrt(max(u, 0)).

The oracle sets: the CPU measurement the feature was specified from.  "fast" is the default vehicle with the four flight limits at
10 / 10 / 10 / 12, so that they are not the bottleneck; "weak" is the same with max_thrust = 1.6 N per rotor.
"""
import ctypes as C
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import REPO

G, TAU = 9.81, 0.7
FMAX, FMIN = (4.0 * 4.5) / 0.5, (4.0 * 0.1) / 0.5           # the laboratory vehicle: 36 and 0.8 m/s^2
D, E = FMAX * FMAX - G * G, G * G - FMIN * FMIN
NAN = float("nan")
MARGIN = 1e-3


def vehicle(fast=False, max_thrust=None, **more):
    from uav_ac import _native as nat
    V = nat.Vehicle.default()
    if fast:
        V.max_speed_xy, V.max_ascent, V.max_descent, V.max_horiz_accel = 10.0, 10.0, 10.0, 12.0
    if max_thrust is not None:
        V.max_thrust = max_thrust
    for k, v in more.items():
        setattr(V, k, v)
    return V


def _rows(accels):
    rows = np.zeros((len(accels), 11))
    rows[:, 6:9] = accels
    return rows


def _one(a, V=None):
    from uav_ac.scoring import need_from_rows
    need = need_from_rows(_rows([a]), [0, 1], V)
    assert need.shape == (4, 1)
    return need[:, 0]


# ------------------------------------------------------------------------------------------------ hand-made rows, exact answers
def test_the_laboratory_vehicle_and_its_limits():
    from uav_ac.scoring import demand_limits
    V = vehicle()
    assert (V.g, V.max_tilt, V.mass, V.max_thrust, V.min_thrust) == (G, TAU, 0.5, 4.5, 0.1)
    assert demand_limits() == demand_limits(V) == (G, TAU, FMAX, FMIN)
    for bad in (dict(g=0.0), dict(g=NAN), dict(max_tilt=0.0), dict(max_tilt=math.inf), dict(max_thrust=1.0), dict(max_thrust=math.inf),
                dict(max_thrust=G * 0.5 / 4.0), dict(min_thrust=-0.1), dict(min_thrust=G * 0.5 / 4.0), dict(min_thrust=NAN)):
        with pytest.raises(ValueError):
            demand_limits(vehicle(**bad))


def test_hover_needs_nothing():
    need = _one((0, 0, 0))
    assert need.tolist() == [0.0, 0.0, 0.0, 0.0] and not np.signbit(need).any()


def test_a_horizontal_g_at_tilt_0_7():
    # ax = g, ay = az = 0: q = g g - tau^2 g g, u = sqrt(q) / (tau g) = sqrt(1 - tau^2) / tau, about 1.02: a bank command of sqrt(1 / 2)
    xx = G * G
    q = xx - (TAU * TAU) * xx
    u = (TAU * 0.0 + math.sqrt(q)) / (TAU * G)
    need = _one((G, 0, 0))
    assert need[0] == math.sqrt(u) and abs(u - math.sqrt(1.0 - TAU * TAU) / TAU) < 1e-12 and u > 1.0
    assert need[1] == 0.0 and need[3] == 0.0
    assert need[2] == math.sqrt((math.sqrt(0.0 + xx * D) - 0.0) / D)      # thrust g sqrt(2) of 36: far from binding
    assert need[2] < 1.0
    swapped = _one((0, -G, 0))
    assert swapped.tolist() == need.tolist()


def test_free_fall_sits_at_one_and_the_least_thrust_covers_it():
    # a = (0, 0, g): upright u = 1 exactly; thrust min d = (g g)^2 - g g E, u = (g g + sqrt(d)) / E = g / (g - Fmin) up to rounding
    need = _one((0, 0, G))
    gz = G * G
    d = gz * gz - (0.0 + G * G) * E
    assert need[1] == 1.0
    assert need[3] == math.sqrt((gz + math.sqrt(d)) / E)
    assert abs(need[3] - math.sqrt(G / (G - FMIN))) < 1e-12 and need[3] > 1.0
    assert need[0] == 0.0
    # the known edge: with min_thrust = 0 nothing asks for a slowdown, although the row counts as inverted
    zero = _one((0, 0, G), vehicle(min_thrust=0.0))
    assert zero[1] == 1.0 and zero[3] == 1.0 and zero.max() == 1.0


def test_a_row_that_pushes_down_binds_upright_alone():
    # az = 2 g, thrust downward of g.  With Fmin > 0 the least thrust would ask for more (u = az / (g - Fmin)); with Fmin = 0 its
    # condition is empty and its closed form collapses onto the upright bound: d = (g az)^2 - az^2 g^2 = 0 exactly (doubling is exact)
    az = 2.0 * G
    need = _one((0, 0, az), vehicle(min_thrust=0.0))
    assert need[1] == math.sqrt(az / G) == math.sqrt(2.0)
    assert need[0] == 0.0 and need[2] < 1.0
    assert need[3] == need[1]
    assert int(np.argmax(need)) == 1                                        # the first of equals, as `binding` counts
    lab = _one((0, 0, az))
    assert lab[1] == math.sqrt(2.0) and lab[3] > lab[1] and abs(lab[3] - math.sqrt(az / (G - FMIN))) < 1e-12


def test_a_pure_climb_binds_the_largest_thrust():
    az = -30.0                                                             # NED: 30 m/s^2 upward, thrust 39.81 of 36
    need = _one((0, 0, az))
    gz = G * az
    u = (math.sqrt(gz * gz + (0.0 + az * az) * D) - gz) / D
    assert need[2] == math.sqrt(u) and need[2] > 1.0
    assert abs(u - 30.0 / (FMAX - G)) < 1e-12                              # g + 30 / u = Fmax
    assert need[0] == 0.0 and need[1] == 0.0 and need[3] == 0.0


def test_maxima_run_over_a_missions_rows_and_missions_do_not_mix():
    from uav_ac.scoring import need_from_rows
    rows = _rows([(0, 0, 0), (G, 0, 0), (0, 0, G),                        # mission 0: hover, a bank, free fall
                  (0, 0, -30.0), (0, 0, 0)])                               # mission 1: a climb, hover
    need = need_from_rows(rows, [0, 3, 5], None)
    assert need[:, 0].tolist() == [_one((G, 0, 0))[0], 1.0, max(_one((G, 0, 0))[2], _one((0, 0, G))[2]), _one((0, 0, G))[3]]
    assert need[:, 1].tolist() == [0.0, 0.0, _one((0, 0, -30.0))[2], 0.0]


def test_a_non_finite_row_and_a_mission_without_rows_report_nan():
    from uav_ac.scoring import need_from_rows, retime_factors
    for col in (1, 4, 8):                                                   # a position, a velocity, an acceleration
        rows = _rows([(0, 0, 0), (G, 0, 0), (0, 0, 0), (0, 0, 0), (G, 0, 0)])
        rows[1, col] = NAN if col != 4 else math.inf
        need = need_from_rows(rows, [0, 2, 2, 4, 5], None)                  # mission 0 holds the bad row, mission 1 has no rows
        assert np.isnan(need[:, :2]).all()
        assert need[:, 2].tolist() == [0.0, 0.0, 0.0, 0.0] and need[0, 3] == _one((G, 0, 0))[0]
        block = np.ones((8, 4))
        out = retime_factors(block, None, MARGIN, need=need)
        assert np.isnan(out["factors"][:2]).all() and out["binding"][:2].tolist() == [-1, -1] and out["n_nan"] == 2
    rows = _rows([(0, 0, 0)] * 3)
    rows[1, 9] = NAN                                                         # the yaw column is no part of it
    assert not np.isnan(need_from_rows(rows, [0, 3], None)).any()
    with pytest.raises(ValueError):
        need_from_rows(rows, [0, 2], None)
    with pytest.raises(ValueError):
        need_from_rows(rows[:, :9], [0, 3], None)


# ------------------------------------------------------------------------------------------------ the extended rule
def crafted():
    """An audit block and a need block, B = 12, and the expected (factor, binding).  Limits of the default vehicle: 3, 3, 2, 12."""
    cases = [
        # speed_xy, ascent, descent, accel_xy | tilt, upright, thrust_max, thrust_min | factor (None = NaN), binding
        ((2.0, 1.0, 1.0, 5.0), (0.5, 0.2, 0.6, 0.0), 1.0, 0),                                   # all inside: speed_xy 2/3 is nearest
        ((2.0, 1.0, 1.0, 5.0), (1.25, 0.2, 0.6, 0.0), 1.25 / (1.0 - MARGIN), 4),                # each need binding alone
        ((2.0, 1.0, 1.0, 5.0), (0.5, 1.5, 0.6, 0.0), 1.5 / (1.0 - MARGIN), 5),
        ((2.0, 1.0, 1.0, 5.0), (0.5, 0.2, 1.1, 0.0), 1.1 / (1.0 - MARGIN), 6),
        ((2.0, 1.0, 1.0, 5.0), (0.5, 0.2, 0.6, 1.01), 1.01 / (1.0 - MARGIN), 7),
        ((4.5, 1.0, 1.0, 5.0), (1.25, 0.2, 0.6, 0.0), (4.5 / 3.0) / (1.0 - MARGIN), 0),         # the audit's term is the larger one
        ((4.5, 4.5, 3.0, 5.0), (1.5, 1.5, 1.5, 1.5), 1.5 / (1.0 - MARGIN), 0),                  # seven terms tie at 1.5: the first
        ((2.0, 1.0, 1.0, 5.0), (0.5, 1.25, 1.25, 0.0), 1.25 / (1.0 - MARGIN), 5),               # a tie among the needs
        ((2.0, 1.0, 3.0, 5.0), (0.5, 1.5, 0.6, 1.5), 1.5 / (1.0 - MARGIN), 2),                  # descent 3/2 ties with two needs
        ((3.0, 1.0, 1.0, 5.0), (1.0, 0.2, 0.6, 0.0), 1.0, 0),                                   # exactly at the limits: not slowed
        ((2.0, 1.0, 1.0, 5.0), (NAN, NAN, NAN, NAN), None, -1),                                 # NaN in the need block alone
        ((2.0, NAN, 1.0, 5.0), (0.5, 0.2, 0.6, 0.0), None, -1),                                 # ... in the audit block alone
    ]
    B = len(cases)
    audit = np.full((8, B), 0.25)
    audit[1:5] = np.array([c[0] for c in cases]).T
    need = np.array([c[1] for c in cases]).T
    factors = np.array([NAN if c[2] is None else c[2] for c in cases])
    return audit, need, factors, np.array([c[3] for c in cases], dtype=np.int32)


def test_without_a_need_block_the_rule_is_todays():
    from uav_ac.scoring import retime_factors
    audit, _, _, _ = crafted()
    v = 1.0 + 0.1 * np.arange(audit.shape[1])
    out = retime_factors(audit, None, MARGIN, v)
    assert "binding" not in out and set(out) == {"factors", "retimed", "nan", "n_retimed", "n_nan", "velocities"}
    limits = (3.0, 3.0, 2.0, 12.0)
    for b in range(audit.shape[1]):
        s, a, d, x = audit[1:5, b]
        if any(math.isnan(t) for t in (s, a, d, x)):
            assert math.isnan(out["factors"][b]) and out["velocities"][b] == v[b]
            continue
        r = max(s / limits[0], a / limits[1], d / limits[2], math.sqrt(x / limits[3]))
        k = r / (1.0 - MARGIN) if r > 1.0 else 1.0
        assert out["factors"][b] == k and out["velocities"][b] == (v[b] / k if r > 1.0 else v[b]), b
    assert out["n_retimed"] == 3 and out["n_nan"] == 1


def test_the_extended_rule_and_binding_takes_the_first_maximum_on_ties():
    from uav_ac.scoring import BINDING_NAMES, retime_factors
    assert BINDING_NAMES == ("speed_xy", "ascent", "descent", "accel_xy", "tilt", "upright", "thrust_max", "thrust_min")
    audit, need, factors, binding = crafted()
    v = 1.0 + 0.1 * np.arange(len(factors))
    out = retime_factors(audit, None, MARGIN, v, need=need)
    assert np.array_equal(out["factors"], factors, equal_nan=True)
    assert out["binding"].dtype == np.int32 and out["binding"].tolist() == binding.tolist()
    slowed = factors > 1.0
    assert out["retimed"].tolist() == slowed.tolist() and out["n_retimed"] == int(slowed.sum()) == 8 and out["n_nan"] == 2
    assert np.array_equal(out["velocities"][slowed], v[slowed] / factors[slowed])
    assert np.array_equal(out["velocities"][~slowed].view(np.int64), v[~slowed].view(np.int64))     # untouched: the same bits
    # a PlanNeed-like record goes in as well; a block of another size does not
    again = retime_factors(audit, None, MARGIN, v, need=SimpleNamespace(block=need))
    assert np.array_equal(again["factors"], factors, equal_nan=True) and again["binding"].tolist() == binding.tolist()
    with pytest.raises(ValueError):
        retime_factors(audit, None, MARGIN, v, need=need[:, :-1])


# ------------------------------------------------------------------------------------------------ the oracle's rows
_SETS = {}


def oracle_set(m, B, velocity):
    """Per mission set, computed once and left unchanged: the C oracle's rows and jerk, and the audit block NumPy makes of the rows."""
    if (m, B, velocity) not in _SETS:
        from oracle import c_oracle as cc
        from oracle import minsnap_oracle as mo
        wps = mo.synthetic_missions(B, m)
        ref = cc.plan_threads(wps, velocity, 0.01, derivs=True)
        rows, ro = ref["rows"], ref["row_offsets"]
        audit = np.zeros((8, B))
        for b in range(B):
            r = rows[ro[b]:ro[b + 1]]
            audit[0, b] = len(r)
            audit[1, b] = np.sqrt(r[:, 3] * r[:, 3] + r[:, 4] * r[:, 4]).max()
            audit[2, b], audit[3, b] = (-r[:, 5]).max(), r[:, 5].max()
            audit[4, b] = np.sqrt(r[:, 6] * r[:, 6] + r[:, 7] * r[:, 7]).max()
        _SETS[(m, B, velocity)] = dict(wps=wps, ref=ref, audit=audit)
    return _SETS[(m, B, velocity)]


def judged(rows, jerk, ro, V):
    from uav_ac.scoring import demand_feasibility, demand_from_rows, need_from_rows
    f = demand_feasibility(demand_from_rows(rows, jerk, ro, float(V.g)), V)
    return need_from_rows(rows, ro, V), f


# (m, B, velocity, weak) -> missions the demand judges infeasible as planned, and among the missions the extended rule slows down how
# many each term binds.  At 3 m/s the fast vehicle's four limits slow 1, 0 and 4 missions of the three sets and leave 23, 25 and 7
# infeasible; at 6 m/s they slow all 37 and 32 stay bound by the tilt; the weak vehicle is bound by thrust_max in 36 and by tilt in 1.
TABLE = [
    ((8, 37, 3.0, False), 23, {"tilt": 23}),
    ((1, 48, 3.0, False), 25, {"tilt": 25}),
    ((2, 48, 3.0, False), 7, {"tilt": 7, "accel_xy": 3}),
    ((8, 37, 6.0, False), 37, {"tilt": 32, "accel_xy": 5}),
    ((8, 37, 3.0, True), 37, {"thrust_max": 36, "tilt": 1}),
]


@pytest.mark.parametrize("key, infeasible, binds", TABLE)
def test_need_above_one_is_exactly_what_the_demand_judges_infeasible(key, infeasible, binds):
    from uav_ac.scoring import BINDING_NAMES, retime_factors
    m, B, velocity, weak = key
    k = oracle_set(m, B, velocity)
    ref = k["ref"]
    for V in (vehicle(fast=True, max_thrust=1.6 if weak else None), vehicle(max_thrust=1.6 if weak else None)):
        need, f = judged(ref["rows"], ref["jerk"], ref["row_offsets"], V)
        bad = ~(f["thrust_ok"] & f["tilt_ok"] & f["upright"])
        assert np.array_equal(need.max(axis=0) > 1.0, bad)                  # the flight limits play no part in either
        assert int(bad.sum()) == infeasible
    V = vehicle(fast=True, max_thrust=1.6 if weak else None)
    need, _ = judged(ref["rows"], ref["jerk"], ref["row_offsets"], V)
    out = retime_factors(k["audit"], V, MARGIN, need=need)
    names = [BINDING_NAMES[i] for i in out["binding"][out["retimed"]]]
    print(f"{key}: {infeasible} of {B} infeasible, {out['n_retimed']} slowed, binding {dict((n, names.count(n)) for n in set(names))}")
    assert {n: names.count(n) for n in set(names)} == binds
    four = retime_factors(k["audit"], V, MARGIN)
    assert (out["factors"] >= four["factors"]).all()
    assert np.array_equal(out["factors"][out["binding"] < 4], four["factors"][out["binding"] < 4])


def test_the_laboratory_vehicle_at_3_m_s_is_bound_by_its_flight_limits_alone():
    from uav_ac.scoring import need_from_rows, retime_factors
    k = oracle_set(8, 37, 3.0)
    need = need_from_rows(k["ref"]["rows"], k["ref"]["row_offsets"], None)
    v = np.full(37, 3.0)
    four, ext = retime_factors(k["audit"], None, MARGIN, v), retime_factors(k["audit"], None, MARGIN, v, need=need)
    assert four["n_retimed"] == 37 and (ext["binding"] < 4).all()
    assert np.array_equal(four["factors"].view(np.int64), ext["factors"].view(np.int64))
    assert np.array_equal(four["velocities"].view(np.int64), ext["velocities"].view(np.int64))


def test_replanning_at_the_retimed_speed_makes_the_mission_feasible():
    from oracle import c_oracle as cc
    from uav_ac.scoring import retime_factors
    k = oracle_set(8, 37, 3.0)
    V = vehicle(fast=True)
    ref = k["ref"]
    need, f = judged(ref["rows"], ref["jerk"], ref["row_offsets"], V)
    out = retime_factors(k["audit"], V, MARGIN, need=need)
    picked = np.flatnonzero(out["retimed"])[[0, 7, 15, 22]]
    assert not f["tilt_ok"][picked].any()
    for b in picked:
        again = cc.plan_threads(k["wps"][b:b + 1], 3.0 / out["factors"][b], 0.01, derivs=True)
        n, g = judged(again["rows"], again["jerk"], again["row_offsets"], V)
        print(f"mission {b}: factor {out['factors'][b]:.6f}, afterwards at {n.max():.6f} of its binding limit")
        assert g["tilt_ok"][0] and g["thrust_ok"][0] and g["upright"][0]
        assert 0.998 < n.max() <= 1.0                                       # one pass: just inside (margin 1e-3 in k, 2e-3 in u)


# ------------------------------------------------------------------------------------------------ the plumbing
def test_entry_points_header_table_and_constants_agree():
    from uav_ac import _native as nat
    from uav_ac import plans
    lib = nat.lib()
    with open(os.path.join(REPO, "include", "uavac.h")) as fh:
        header = fh.read()
    assert re.findall(r"^#define UAVAC_NEED_ROWS (\d+)$", header, flags=re.M) == [str(nat.NEED_ROWS)] and nat.NEED_ROWS == 4
    counts = {"uavac_minsnap_need_dev": 9, "uavac_minsnap_retime_demand_factors_dev": 11, "uavac_minsnap_retime_demand_dev": 23}
    for name, n in counts.items():
        assert hasattr(lib, name) and name in nat.exported_symbols()
        proto = re.search(rf"^int {name}\(([^;]*)\);", header, flags=re.M).group(1)
        kinds = []
        for param in proto.split(","):
            pointer = "*" in param or "[" in param                          # (limits[4] and demand_limits[4] are host arrays)
            kinds.append(C.c_void_p if pointer else {"int": C.c_int, "double": C.c_double}[param.split()[0]])
        res, args = nat._SIGNATURES[name]
        assert res is C.c_int and args == kinds and len(args) == n, name
    # the loop is uavac_minsnap_retime_dev with demand_limits, need and binding added
    old = re.search(r"^int uavac_minsnap_retime_dev\(([^;]*)\);", header, flags=re.M).group(1)
    new = re.search(r"^int uavac_minsnap_retime_demand_dev\(([^;]*)\);", header, flags=re.M).group(1)
    names = [[p.split()[-1].lstrip("*") for p in proto.split(",")] for proto in (old, new)]
    assert [n for n in names[1] if n not in names[0]] == ["demand_limits[4]", "need", "binding"]
    assert [n for n in names[1] if n in names[0]] == names[0]
    assert [f for f in plans.PlanNeed.__dataclass_fields__] == ["tilt", "upright", "thrust_max", "thrust_min", "block"]
    fields = [f for f in plans.RetimeResult.__dataclass_fields__]
    assert fields[-2:] == ["need", "binding"] and fields[:6] == ["plan", "velocities", "factors", "passes", "converged", "audit"]
    r = plans.RetimeResult(None, None, None, 0, None, None)
    assert r.need is None and r.binding is None
    # no context: refused before anything else, like every entry point
    assert lib.uavac_minsnap_need_dev(None, None, None, None, 1, 1, 0.01, None, None) == nat.EINVAL
    assert lib.uavac_minsnap_retime_demand_factors_dev(None, None, None, 1, None, None, 0.0, None, None, None, None) == nat.EINVAL
