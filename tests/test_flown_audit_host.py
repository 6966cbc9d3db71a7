"""The plan audit of a flight, the part that needs no GPU: the entry point is exported and declared as the header declares it, a NULL
context is refused, the build keeps the two kernels inside their budget, and the rule itself -- `uav_ac.scoring.audit_from_log`, the
NumPy statement the kernel is tested against bit for bit (tests/test_gpu_flown_audit.py) -- gives the answers that hand-made logs have by
inspection; `uav_ac.scoring.flight_feasibility` turns them into verdicts.

The hand-made logs stand on a binary grid (steps of 0.125), so every square and every sum below is exact."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import REPO

KINDS = {"int": C.c_int, "double": C.c_double, "int64_t": C.c_int64}
NAN = np.nan
IDENTITY = (1.0, 0.0, 0.0, 0.0)
FIELDS = ("ticks", "speed_xy", "ascent", "descent", "speed", "bank_x", "bank_y", "body_rate")


def log_of(*vehicles):
    """Vehicles given as lists of ticks, a tick a dict of the rows that differ from rest at the origin with identity attitude
    (pos, quat, vel, rate) -> a state log (K, 13, B)."""
    K = len(vehicles[0])
    log = np.zeros((K, 13, len(vehicles)))
    log[:, 3, :] = 1.0
    for b, ticks in enumerate(vehicles):
        assert len(ticks) == K
        for k, t in enumerate(ticks):
            for name, rows in (("pos", slice(0, 3)), ("quat", slice(3, 7)), ("vel", slice(7, 10)), ("rate", slice(10, 13))):
                if name in t:
                    log[k, rows, b] = t[name]
    return log


def test_entry_point_is_exported_and_declared_like_the_header():
    from uav_ac import _native as nat
    name = "uavac_flown_audit_dev"
    assert name in nat.exported_symbols() and nat.FLOWN_AUDIT_ROWS == 8 and nat.FLOWN_AUDIT_MAX_SPLIT == 64
    fn = getattr(nat.lib(), name)
    restype, argtypes = nat._SIGNATURES[name]
    raw = open(os.path.join(REPO, "include", "uavac.h")).read()
    assert re.search(r"#define\s+UAVAC_FLOWN_AUDIT_ROWS\s+8\b", raw) and re.search(r"#define\s+UAVAC_FLOWN_AUDIT_MAX_SPLIT\s+64\b", raw)
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    args = re.search(rf"int\s+{name}\s*\(([^)]*)\)\s*;", text).group(1)
    params = [" ".join(a.split()) for a in args.split(",")]
    kinds = [C.c_void_p if "*" in a else KINDS[a.split()[0]] for a in params]
    assert restype is C.c_int and len(argtypes) == 13 and kinds == list(argtypes), params
    # a NULL context is refused before anything else is looked at (pure host code: no GPU needed)
    assert fn(None, None, 1, 1, 1, None, 0, None, None, None, None, None, None) == nat.EINVAL


def test_the_build_keeps_the_flown_audit_kernels_in_registers():
    from uav_ac import _buildcheck
    counts = _buildcheck.check_flown_audit_kernels()
    if counts is None:
        pytest.skip("no object files here (a library that was built elsewhere)")
    assert len(counts) == 2 and max(counts.values()) <= 128
    assert any("flown_audit_kernel" in k for k in counts) and any("flown_audit_merge_kernel" in k for k in counts)


def test_known_peaks_over_the_valid_ticks():
    from uav_ac.scoring import audit_from_log
    h = 0.5                                                  # quaternion (h, h, h, h): a unit quaternion on the grid
    a = [{"vel": (0.75, 1.0, -0.5), "rate": (0.25, 0.5, 0.5)},                          # |v_xy| 1.25, climbing at 0.5, |w| 0.75
         {"vel": (-3.0, 4.0, 12.0), "quat": (h, h, h, h)},                              # |v_xy| 5, sinking at 12, |v| 13; R13 = 1, R23 = 0
         {"vel": (0.0, 0.0, -2.0), "quat": (h, -h, h, h), "rate": (-2.0, 1.0, 2.0)}]    # climbing at 2; R13 = 0, R23 = 1; |w| 3
    rest = [{}, {"vel": (0.0, 0.0, -0.0)}, {}]               # vz = +0.0, -0.0, +0.0
    out = audit_from_log(log_of(a, rest))
    assert out["audit"].dtype == np.float64 and out["audit"].shape == (8, 2) and out["first_bad"].dtype == np.int32
    assert out["audit"][:, 0].tolist() == [3.0, 5.0, 2.0, 12.0, 13.0, 1.0, 1.0, 3.0]
    assert out["audit"][:, 1].tolist() == [3.0] + [0.0] * 7 and out["first_bad"].tolist() == [-1, -1]
    # a vehicle at rest: the maximum of -0.0 and +0.0 is +0.0, whatever the order of the ticks
    assert not np.signbit(out["audit"][1:, 1]).any()
    # n = 0: the per-cuboid outputs are there and empty
    for key, dtype in (("hit_ticks", np.int32), ("first_hit", np.int32), ("clearance", np.float64), ("clearance_tick", np.int32)):
        assert out[key].shape == (0, 2) and out[key].dtype == dtype
    empty = audit_from_log(log_of(a, rest), np.zeros((0, 6)))
    assert all(np.array_equal(empty[k], out[k], equal_nan=True) for k in out)


def test_hits_on_a_face_and_clearance_to_face_edge_and_corner_with_ties_to_the_lower_tick():
    from uav_ac.scoring import audit_from_log
    box = [[1.0, 2.0, 1.0, 2.0, -2.0, -1.0]]
    face = [{"pos": (0.5, 1.5, -1.5)}, {"pos": (0.25, 1.5, -1.5)}, {"pos": (2.75, 1.25, -1.25)}, {"pos": (0.5, 1.5, -1.5)}]      # 0.5, 0.75, 0.75, 0.5 off a face
    edge = [{"pos": (0.625, 0.5, -1.5)}, {"pos": (2.375, 2.5, -1.5)}, {"pos": (5, 5, 5)}, {"pos": (2.375, 0.5, -1.5)}]          # (0.375, 0.5): 0.625, three times
    corner = [{"pos": (5, 5, 5)}, {"pos": (2.25, 2.75, -0.5)}, {"pos": (0.75, 0.25, -2.5)}, {"pos": (5, 5, 5)}]                 # (0.25, 0.75, 0.5): sqrt(0.875), twice
    on_face = [{"pos": (3, 3, 3)}, {"pos": (1.0, 1.5, -1.5)}, {"pos": (1.5, 1.5, -1.5)}, {"pos": (2.0, 2.0, -1.0)}]             # on a face, inside, on a corner
    out = audit_from_log(log_of(face, edge, corner, on_face), box)
    assert out["clearance"][0].tolist() == [0.5, 0.625, np.sqrt(0.875), 0.0]
    assert out["clearance_tick"][0].tolist() == [0, 0, 1, 1]           # equal clearances: the lower tick
    assert out["hit_ticks"][0].tolist() == [0, 0, 0, 3] and out["first_hit"][0].tolist() == [-1, -1, -1, 1]
    assert out["audit"][0].tolist() == [4.0] * 4
    # two cuboids are judged apart, and one that holds nobody has no hit and a positive clearance
    two = audit_from_log(log_of(face, on_face), box + [[10.0, 11.0, 10.0, 11.0, 10.0, 11.0]])
    assert two["hit_ticks"].tolist() == [[0, 3], [0, 0]] and two["first_hit"].tolist() == [[-1, 1], [-1, -1]]
    assert (two["clearance"][1] > 0).all() and two["clearance_tick"][1].tolist() == [2, 0]
    # a NaN bound gives 0 on its axis, an inverted one what the two comparisons give: defined results, no hit
    odd = audit_from_log(log_of(face), [[NAN, 2.0, 1.0, 2.0, -2.0, -1.0], [2.0, 1.0, 1.0, 2.0, -2.0, -1.0]])
    assert odd["hit_ticks"].tolist() == [[0], [0]] and odd["clearance"][0].tolist() == [0.0] and odd["clearance_tick"][0].tolist() == [0]
    assert odd["clearance"][1].tolist() == [1.5] and odd["clearance_tick"][1].tolist() == [0]      # x < xmin = 2 at ticks 0, 1, 3: 1.5, 1.75, 1.5; at tick 2 x > xmax = 1 by 1.75


def test_invalid_ticks_are_counted_reported_and_ignored():
    from uav_ac.scoring import audit_from_log
    box = [[1.0, 2.0, 1.0, 2.0, -2.0, -1.0]]
    fast_inside = {"pos": (1.5, 1.5, -1.5), "vel": (8.0, 0.0, 0.0)}
    some = [{"vel": (1.0, 0.0, 0.0)}, dict(fast_inside, rate=(NAN, 0.0, 0.0)), {"pos": (0.5, 1.5, -1.5)}, dict(fast_inside, vel=(NAN, 0, 0))]
    inf_q3 = [{"vel": (2.0, 0.0, 0.0)}, dict(fast_inside, quat=(1.0, 0.0, 0.0, np.inf)), {}, {}]      # q3 is in no peak: the tick is invalid all the same
    never = [{"pos": (NAN, NAN, NAN)}] * 4
    out = audit_from_log(log_of(some, inf_q3, never), box)
    assert out["audit"][0].tolist() == [2.0, 3.0, 0.0] and out["first_bad"].tolist() == [1, 1, 0]
    assert out["audit"][1, :2].tolist() == [1.0, 2.0]                  # the fast ticks were invalid: ignored
    assert out["hit_ticks"][0].tolist() == [0, 0, 0] and out["first_hit"][0].tolist() == [-1, -1, -1]
    assert out["clearance"][0, 0] == 0.5 and out["clearance_tick"][0, 0] == 2 and out["clearance_tick"][0, 1] == 0
    # the vehicle that is NaN throughout: the no-valid-tick record
    assert np.isnan(out["audit"][1:, 2]).all() and np.isnan(out["clearance"][0, 2]) and out["clearance_tick"][0, 2] == -1


def test_malformed_input_raises():
    from uav_ac.scoring import audit_from_log
    log = log_of([{}], [{}])
    for bad in (log[0], log[:, :12], log[:0], np.zeros((2, 14, 3))):
        with pytest.raises(ValueError):
            audit_from_log(bad)
    for cub in (np.zeros((2, 5)), np.zeros(7), np.zeros((17, 6))):
        with pytest.raises(ValueError):
            audit_from_log(log, cub)


def test_flight_feasibility_verdicts():
    from uav_ac.scoring import flight_feasibility
    V = SimpleNamespace(max_speed_xy=5.0, max_ascent=3.0, max_descent=2.0, max_tilt=0.5)
    #                  clean  fast   climbs sinks  tilted short  hit    NaN
    a = SimpleNamespace(
        ticks=np.array([10.0, 10.0, 10.0, 10.0, 10.0, 9.0, 10.0, 0.0]),
        speed_xy=np.array([5.0, 5.125, 1.0, 1.0, 1.0, 1.0, 1.0, NAN]),
        ascent=np.array([3.0, 1.0, 3.5, 1.0, 1.0, 1.0, 1.0, NAN]),
        descent=np.array([2.0, 1.0, 1.0, 2.25, 1.0, 1.0, 1.0, NAN]),
        bank_x=np.array([0.5, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, NAN]),
        bank_y=np.array([0.25, 0.1, 0.1, 0.1, 0.75, 0.1, 0.1, NAN]),
        hit_ticks=np.array([[0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 4, 0]], dtype=np.int32))
    v = flight_feasibility(a, 10, V)
    assert set(v) == {"complete", "speed_ok", "ascent_ok", "descent_ok", "tilt_ok", "clear", "flown_ok"}
    assert all(x.dtype == bool and x.shape == (8,) for x in v.values())
    assert v["complete"].tolist() == [True, True, True, True, True, False, True, False]
    assert v["speed_ok"].tolist() == [True, False, True, True, True, True, True, False]
    assert v["ascent_ok"].tolist() == [True, True, False, True, True, True, True, False]
    assert v["descent_ok"].tolist() == [True, True, True, False, True, True, True, False]
    assert v["tilt_ok"].tolist() == [True, True, True, True, False, True, True, False]
    assert v["clear"].tolist() == [True, True, True, True, True, True, False, False]
    assert v["flown_ok"].tolist() == [True, False, False, False, True, False, False, False]      # tilt is reported, not judged
    # slack widens the three limits and the tilt; without cuboids everybody with numbers is clear
    a.hit_ticks = np.zeros((0, 8), dtype=np.int32)
    w = flight_feasibility(a, 10, V, slack=0.25)
    assert w["speed_ok"].tolist()[:2] == [True, True] and w["descent_ok"][3] and w["tilt_ok"][4] and not w["ascent_ok"][2]
    assert w["clear"].tolist() == [True] * 7 + [False] and w["flown_ok"].tolist() == [True, True, False, True, True, False, True, False]
