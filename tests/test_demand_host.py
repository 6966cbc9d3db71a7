"""Plan demand, host side: `scoring.demand_from_rows` -- the NumPy specification of `uavac_minsnap_demand_dev` -- on hand-made rows
whose answers are exact, on every position of a sample relative to a cuboid, and on the C oracle's rows; the judges
`scoring.demand_feasibility` and `scoring.audit_gap` on synthetic inputs; and the plumbing: the library exports the entry point and the
ctypes table and constants say what include/uavac.h says."""
import ctypes as C
import itertools
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import REPO

G = 9.81
NAN = float("nan")
CUBS = np.array([[6.0, 14.0, 2.0, 9.0, -4.0, -2.8], [10.0, 12.0, 5.0, 7.0, -10.0, 0.0], [3.7, 4.3, 4.0, 10.0, -3.4, -2.8]])


def _rows(samples):
    """[(p, a, j)] with 3-tuples -> rows (N, 11) with zero velocity, yaw and spline id, and jerk (N, 3)."""
    rows, jerk = np.zeros((len(samples), 11)), np.zeros((len(samples), 3))
    for i, (p, a, j) in enumerate(samples):
        rows[i, 0:3], rows[i, 6:9], jerk[i] = p, a, j
    return rows, jerk


def _one(p=(0, 0, 0), a=(0, 0, 0), j=(0, 0, 0), cuboids=None):
    """the demand of a mission of one row -> (demand (6,), idemand (2,), clearance (n,), clearance_row (n,))"""
    from uav_ac.scoring import demand_from_rows
    d = demand_from_rows(*_rows([(p, a, j)]), [0, 1], G, cuboids)
    return d["demand"][:, 0], d["idemand"][:, 0], d["clearance"][:, 0], d["clearance_row"][:, 0]


# ------------------------------------------------------------------------------------------------ hand-made rows, exact answers
def test_hover_demands_g_no_bank_and_no_rate():
    d, i, c, r = _one()
    assert d.tolist() == [1.0, G, G, 0.0, 0.0, 0.0] and i.tolist() == [0, -1]
    assert not np.signbit(d[3:]).any()                                       # +0.0, not -0.0
    assert c.shape == r.shape == (0,)


def test_a_horizontal_g_banks_to_the_square_root_of_one_half():
    d, i, _, _ = _one(a=(G, 0, 0))
    assert d[3] == math.sqrt(0.5) and d[4] == 0.0                           # g g / (g g + g g) is 1 / 2 exactly
    assert d[1] == d[2] == math.sqrt(G * G + G * G) and i.tolist() == [0, -1]
    d, _, _, _ = _one(a=(0, -G, 0))
    assert d[4] == math.sqrt(0.5) and d[3] == 0.0


def test_free_fall_has_no_thrust_no_bank_and_counts_as_inverted():
    d, i, _, _ = _one(a=(0, 0, G), j=(1, 2, 3))
    assert d.tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0] and i.tolist() == [1, 0]      # n2 = 0: nothing is divided by it
    d, i, _, _ = _one(a=(1.0, 0, 2 * G))                                     # thrust downward, and the bank is still |ax| / |a - g e3|
    assert i.tolist() == [1, 0] and d[3] == math.sqrt((1.0 * 1.0) / (1.0 * 1.0 + G * G))


def test_jerk_across_the_thrust_is_a_rate_and_jerk_along_it_is_none():
    d, _, _, _ = _one(j=(1, 0, 0))
    assert d[5] == math.sqrt(1.0 / (G * G))
    d, _, _, _ = _one(j=(0, 0, 2))                                           # hover: the thrust points along -z
    assert d[5] == 0.0 and not np.signbit(d[5])
    d, _, _, _ = _one(a=(3.0, 0, G - 4.0), j=(-1.5, 0, 2.0))                 # thrust direction (3, 0, -4); the jerk is -1/2 of it
    assert d[1] == 5.0 and d[3] == math.sqrt(9.0 / 25.0) and d[5] == 0.0
    d, _, _, _ = _one(a=(3.0, 0, G - 4.0), j=(4.0, 0, 3.0))                  # ... and one across it: |j| / |f| = 5 / 5
    assert d[5] == 1.0


def test_maxima_and_minima_run_over_a_missions_rows_and_missions_do_not_mix():
    from uav_ac.scoring import demand_from_rows
    z = (0, 0, 0)
    rows, jerk = _rows([(z, z, z), (z, (G, 0, 0), (1, 0, 0)), (z, (0, 0, G), z),      # mission 0: hover, a bank, free fall
                        (z, (0, 0, 2 * G), z), (z, (0, 0, -G), z)])                      # mission 1: thrust downward, then 2 g upward
    d = demand_from_rows(rows, jerk, [0, 3, 5], G)
    assert d["demand"][:, 0].tolist() == [3.0, math.sqrt(G * G + G * G), 0.0, math.sqrt(0.5), 0.0, math.sqrt(0.5 / (G * G + G * G))]
    assert d["idemand"][:, 0].tolist() == [1, 2]
    assert d["demand"][:, 1].tolist() == [2.0, G + G, G, 0.0, 0.0, 0.0] and d["idemand"][:, 1].tolist() == [1, 0]


# ------------------------------------------------------------------------------------------------ cuboids
UNIT = np.array([[0.0, 1.0, 0.0, 1.0, 0.0, 1.0]])


@pytest.mark.parametrize("off", list(itertools.product((-1, 0, 1), repeat=3)))
def test_distance_to_a_cuboid_from_every_side_edge_and_corner(off):
    # 1 beyond the face on every axis with a non-zero offset: 6 faces, 12 edges, 8 corners, and the inside
    p = tuple(0.5 + 1.5 * o for o in off)
    _, _, c, r = _one(p=p, cuboids=UNIT)
    assert c[0] == math.sqrt(float(sum(o != 0 for o in off))) and r[0] == 0


def test_on_a_face_counts_as_inside_and_a_tie_takes_the_lowest_row():
    from uav_ac.scoring import demand_from_rows
    z = (0, 0, 0)
    assert _one(p=(1.0, 0.5, 0.5), cuboids=UNIT)[2][0] == 0.0
    assert _one(p=(0.25, 0.0, 1.0), cuboids=UNIT)[2][0] == 0.0
    rows, jerk = _rows([((3, 0.5, 0.5), z, z), ((2, 0.5, 0.5), z, z), ((0.5, 0.5, -1), z, z), ((0.5, 2, 0.5), z, z),
                        ((0.5, 0.5, 0.5), z, z), ((0.2, 0.2, 0.2), z, z)])
    d = demand_from_rows(rows, jerk, [0, 4, 6], G, np.concatenate([UNIT, UNIT + 10.0]))
    assert d["clearance"][0].tolist() == [1.0, 0.0] and d["clearance_row"][0].tolist() == [1, 0]      # rows 1, 2 and 3 tie; rows 0 and 1 tie
    assert d["clearance_row"][1].tolist() == [0, 0] and d["clearance"][1, 1] == math.sqrt((9.5 * 9.5 + 9.5 * 9.5) + 9.5 * 9.5)
    # a cuboid with a NaN bound or infinitely far away: what the comparisons give, and still the lowest row
    odd = np.array([[NAN, 1.0, 0.0, 1.0, 0.0, 1.0], [math.inf, math.inf, 0.0, 1.0, 0.0, 1.0]])
    d = demand_from_rows(rows, jerk, [0, 4, 6], G, odd)
    assert d["clearance"][0].tolist() == [1.0, 0.0] and d["clearance_row"][0].tolist() == [1, 0]
    assert d["clearance"][1].tolist() == [math.inf, math.inf] and d["clearance_row"][1].tolist() == [0, 0]


def test_a_non_finite_row_and_a_mission_without_rows_are_excluded():
    from uav_ac.scoring import demand_from_rows, demand_feasibility
    z = (0, 0, 0)
    for where in ("p", "v", "a", "j"):
        rows, jerk = _rows([(z, z, z), ((0.5, 0.5, 0.5), (0, 0, 2 * G), z), (z, z, z), (z, z, z), (z, (G, 0, 0), z)])
        if where == "v":
            rows[1, 4] = math.inf
        else:
            {"p": rows[:, 0:3], "a": rows[:, 6:9], "j": jerk}[where][1, 2] = NAN
        d = demand_from_rows(rows, jerk, [0, 2, 2, 4, 5], G, UNIT)           # mission 0 holds the bad row, mission 1 has no rows
        assert d["demand"][0].tolist() == [2.0, 0.0, 2.0, 1.0]
        for b in (0, 1):
            assert np.isnan(d["demand"][1:, b]).all() and d["idemand"][:, b].tolist() == [0, -1]
            assert np.isnan(d["clearance"][0, b]) and d["clearance_row"][0, b] == -1
        assert d["demand"][1:, 2].tolist() == [G, G, 0.0, 0.0, 0.0] and d["clearance_row"][0].tolist() == [-1, -1, 0, 0]
        assert d["demand"][3, 3] == math.sqrt(0.5)
        for key, v in demand_feasibility(d).items():
            assert v.tolist()[:2] == [False, False], key
    rows, jerk = _rows([(z, z, z)] * 5)
    rows[1, 9] = NAN                                                           # the yaw column is no part of the demand
    assert not np.isnan(demand_from_rows(rows, jerk, [0, 2, 4, 5], G)["demand"]).any()
    with pytest.raises(ValueError):
        demand_from_rows(rows, jerk[:-1], [0, 5], G)
    with pytest.raises(ValueError):
        demand_from_rows(rows, jerk, [0, 4], G)
    for g in (0.0, -G, NAN, math.inf):
        with pytest.raises(ValueError):
            demand_from_rows(rows, jerk, [0, 5], g)
    with pytest.raises(ValueError):
        demand_from_rows(rows, jerk, [0, 5], G, np.zeros((17, 6)))


# ------------------------------------------------------------------------------------------------ the oracle's rows
def _oracle_demand(m, B, velocity):
    from oracle import c_oracle as cc
    from oracle import minsnap_oracle as mo
    from uav_ac.scoring import demand_from_rows
    ref = cc.plan_threads(mo.synthetic_missions(B, m), velocity, 0.01, derivs=True)
    return ref, demand_from_rows(ref["rows"], ref["jerk"], ref["row_offsets"], G, CUBS)


def test_the_tilt_bound_binds_where_the_acceleration_bound_does_not():
    import torch
    from uav_ac.scoring import demand_feasibility, plan_feasibility
    ref, d = _oracle_demand(8, 37, 3.0)
    f = demand_feasibility(d)
    rows, ro = ref["rows"], ref["row_offsets"]
    accel_xy = np.array([np.sqrt(rows[ro[b]:ro[b + 1], 6] ** 2 + rows[ro[b]:ro[b + 1], 7] ** 2).max() for b in range(37)])
    zero = torch.zeros(37, dtype=torch.float64)
    accel_ok = plan_feasibility(SimpleNamespace(speed_xy=zero, ascent=zero, descent=zero, accel_xy=torch.as_tensor(accel_xy)))["accel_ok"].numpy()
    missed = int((~f["tilt_ok"] & accel_ok).sum())
    print(f"(8, 37) at 3 m/s: {int((~f['tilt_ok']).sum())} missions demand more than max_tilt, {missed} of them pass accel_ok; "
          f"peak bank {d['demand'][3:5].max():.3f}, least thrust {d['demand'][2].min():.2f} m/s^2")
    assert missed >= 1                                                        # (the NumPy oracle gives 22 of 23)
    assert f["upright"].all() and f["thrust_ok"].all() and d["idemand"][0].sum() == 0
    assert (d["clearance"] == 0.0).any() and not f["clear"].all() and f["clear"].any()
    assert (f["demand_ok"] == (f["thrust_ok"] & f["tilt_ok"] & f["upright"] & f["clear"])).all()


def test_a_fast_plan_asks_for_thrust_downward():
    _, d = _oracle_demand(8, 37, 6.0)
    from uav_ac.scoring import demand_feasibility
    inverted, first = d["idemand"]
    print(f"(8, 37) at 6 m/s: {int(inverted.sum())} inverted rows in {int((inverted > 0).sum())} missions")
    assert inverted.sum() > 0
    assert ((inverted > 0) == (first >= 0)).all()
    assert (demand_feasibility(d)["upright"] == (inverted == 0)).all()


# ------------------------------------------------------------------------------------------------ the judges
def _up(x):
    return math.nextafter(x, math.inf)


def _down(x):
    return math.nextafter(x, -math.inf)


def _demand(thrust_max, thrust_min, bank_x, bank_y, inverted=None, clearance=None, as_tensors=False):
    B = len(thrust_max)
    inverted = [0] * B if inverted is None else inverted
    clearance = np.zeros((0, B)) if clearance is None else np.asarray(clearance, dtype=np.float64).reshape(-1, B)
    f = dict(rows=np.full(B, 10.0), thrust_max=np.array(thrust_max), thrust_min=np.array(thrust_min), bank_x=np.array(bank_x),
             bank_y=np.array(bank_y), body_rate=np.zeros(B), inverted_rows=np.array(inverted, dtype=np.int32),
             first_inverted=np.where(np.array(inverted) > 0, 0, -1).astype(np.int32), clearance=clearance,
             clearance_row=np.zeros(clearance.shape, dtype=np.int32))
    if as_tensors:
        import torch
        f = {k: torch.as_tensor(v) for k, v in f.items()}
    return SimpleNamespace(**f)


def test_demand_feasibility_limits_slack_nan_and_vehicle():
    from uav_ac import _native as nat
    from uav_ac.scoring import demand_feasibility
    V = nat.Vehicle.default()
    assert (V.mass, V.min_thrust, V.max_thrust, V.max_tilt) == (0.5, 0.1, 4.5, 0.7)      # the laboratory vehicle: 0.8 .. 36 m/s^2
    hi, lo, tilt = 36.0, 0.8, 0.7
    # 0: everything at its limit; 1-4: one quantity one ulp outside; 5: NaN; 6: well inside; 7: an inverted row
    d = _demand([hi, _up(hi), hi, hi, hi, NAN, 10.0, 10.0], [lo, lo, _down(lo), lo, lo, NAN, 9.0, 0.9],
                [tilt, tilt, tilt, _up(tilt), tilt, NAN, 0.1, 0.1], [tilt, tilt, tilt, tilt, _up(tilt), NAN, 0.1, 0.1],
                inverted=[0, 0, 0, 0, 0, 0, 0, 3])
    for form in (d, _demand(d.thrust_max, d.thrust_min, d.bank_x, d.bank_y, d.inverted_rows.tolist(), as_tensors=True)):
        f = demand_feasibility(form)
        assert set(f) == {"thrust_ok", "tilt_ok", "upright", "clear", "demand_ok"}
        assert all(v.dtype == bool and v.shape == (8,) for v in f.values())
        assert f["thrust_ok"].tolist() == [True, False, False, True, True, False, True, True]
        assert f["tilt_ok"].tolist() == [True, True, True, False, False, False, True, True]
        assert f["upright"].tolist() == [True] * 5 + [False, True, False]
        assert f["clear"].tolist() == [True] * 5 + [False, True, True]           # no cuboid given; NaN fails every test
        assert f["demand_ok"].tolist() == [True, False, False, False, False, False, True, False]
    g = demand_feasibility(d, vehicle=V)
    assert all(f[k].tolist() == g[k].tolist() for k in f)
    assert demand_feasibility(d, slack=1e-9)["demand_ok"].tolist() == [True] * 5 + [False, True, False]
    assert demand_feasibility(d, slack=-0.05)["demand_ok"].tolist() == [False] * 6 + [True, False]
    W = SimpleNamespace(mass=1.0, min_thrust=0.0, max_thrust=2.0, max_tilt=0.05)  # anything that carries the four fields will do
    w = demand_feasibility(d, vehicle=W)
    assert w["thrust_ok"].tolist() == [False] * 8 and not w["tilt_ok"].any()


def test_demand_feasibility_clear_is_strict_and_takes_a_margin():
    from uav_ac.scoring import demand_feasibility
    ok = ([10.0] * 4, [9.0] * 4, [0.1] * 4, [0.1] * 4)
    d = _demand(*ok, clearance=[[1.0, 0.0, 0.5, NAN], [2.0, 3.0, 5e-324, 1.0]])
    assert demand_feasibility(d)["clear"].tolist() == [True, False, True, False]
    assert demand_feasibility(d, min_clearance=0.5)["clear"].tolist() == [True, False, False, False]
    assert demand_feasibility(d, min_clearance=0.5)["demand_ok"].tolist() == [True, False, False, False]
    nan = _demand([NAN, 10.0], [NAN, 9.0], [NAN, 0.1], [NAN, 0.1], clearance=[[NAN, 1.0]])
    assert demand_feasibility(nan)["clear"].tolist() == [False, True]


def test_audit_gap_sets_a_plan_beside_its_flight():
    from uav_ac.scoring import audit_gap
    d = _demand([10.0] * 3, [9.0] * 3, [0.5, 0.75, NAN], [0.25, 0.5, NAN], clearance=[[1.0, 0.5, NAN], [0.0, 2.0, NAN]])
    flight = SimpleNamespace(bank_x=np.array([0.75, 0.5, 0.1]), bank_y=np.array([0.25, 1.0, 0.1]),
                             clearance=np.array([[0.25, 0.0, 0.0], [0.0, 2.5, 1.0]]))
    gap = audit_gap(d, flight)
    assert set(gap) == {"bank_excess", "clearance_lost", "hit_in_flight_only"}
    assert np.array_equal(gap["bank_excess"], [[0.25, -0.25, NAN], [0.0, 0.5, NAN]], equal_nan=True)
    assert np.array_equal(gap["clearance_lost"], [[0.75, 0.5, NAN], [0.0, -0.5, NAN]], equal_nan=True)
    assert gap["hit_in_flight_only"].tolist() == [[False, True, False], [False, False, False]]      # planned inside too: not "only"
    # the dict forms of both specifications
    block = np.zeros((8, 3))
    block[5], block[6] = flight.bank_x, flight.bank_y
    as_dict = {"demand": np.stack([d.rows, d.thrust_max, d.thrust_min, d.bank_x, d.bank_y, d.body_rate]),
               "idemand": np.stack([d.inverted_rows, d.first_inverted]), "clearance": d.clearance, "clearance_row": d.clearance_row}
    again = audit_gap(as_dict, {"audit": block, "clearance": flight.clearance})
    assert all(np.array_equal(gap[k], again[k], equal_nan=True) for k in gap)
    none = audit_gap(_demand([10.0], [9.0], [0.5], [0.25]), SimpleNamespace(bank_x=[0.5], bank_y=[0.5], clearance=np.zeros((0, 1))))
    assert none["clearance_lost"].shape == none["hit_in_flight_only"].shape == (0, 1) and none["bank_excess"].tolist() == [[0.0], [0.25]]
    with pytest.raises(ValueError):
        audit_gap(d, SimpleNamespace(bank_x=np.zeros(2), bank_y=np.zeros(2), clearance=np.zeros((2, 2))))
    with pytest.raises(ValueError):
        audit_gap(d, SimpleNamespace(bank_x=np.zeros(3), bank_y=np.zeros(3), clearance=np.zeros((1, 3))))


# ------------------------------------------------------------------------------------------------ the plumbing
def test_demand_entry_point_header_table_and_constants_agree():
    from uav_ac import _native as nat
    from uav_ac import plans
    lib = nat.lib()
    name = "uavac_minsnap_demand_dev"
    assert hasattr(lib, name) and name in nat.exported_symbols()
    with open(os.path.join(REPO, "include", "uavac.h")) as fh:
        header = fh.read()
    defines = dict(re.findall(r"^#define (UAVAC_I?DEMAND_ROWS) (\d+)$", header, flags=re.M))
    assert defines == {"UAVAC_DEMAND_ROWS": str(nat.DEMAND_ROWS), "UAVAC_IDEMAND_ROWS": str(nat.IDEMAND_ROWS)}
    assert (nat.DEMAND_ROWS, nat.IDEMAND_ROWS) == (6, 2)
    proto = re.search(rf"^int {name}\(([^;]*)\);", header, flags=re.M).group(1)
    kinds = []
    for param in proto.split(","):
        kinds.append(C.c_void_p if "*" in param else {"int": C.c_int, "double": C.c_double}[param.split()[0]])
    res, args = nat._SIGNATURES[name]
    assert res is C.c_int and args == kinds and len(args) == 14
    fields = [f for f in plans.PlanDemand.__dataclass_fields__]
    assert fields == ["rows", "thrust_max", "thrust_min", "bank_x", "bank_y", "body_rate", "inverted_rows", "first_inverted", "clearance",
                      "clearance_row", "block"]
    # no context: refused before anything else, like every entry point
    assert getattr(lib, name)(None, None, None, None, 1, 1, 0.01, G, None, 0, None, None, None, None) == nat.EINVAL
