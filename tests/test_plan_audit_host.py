"""Plan audit, host side: the library exports `uavac_minsnap_audit_dev`, the ctypes table declares it as include/uavac.h does,
and `scoring.plan_feasibility` judges hand-made audits the way its docstring says (pure torch, CPU tensors here)."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest


def test_audit_entry_point_is_exported_and_declared_with_twelve_arguments():
    from uav_ac import _native as nat
    lib = nat.lib()
    assert hasattr(lib, "uavac_minsnap_audit_dev")
    assert "uavac_minsnap_audit_dev" in nat.exported_symbols()
    res, args = nat._SIGNATURES["uavac_minsnap_audit_dev"]
    P = C.c_void_p
    assert res is C.c_int
    assert args == [P, P, P, P, C.c_int, C.c_int, C.c_double, P, C.c_int, P, P, P] and len(args) == 12
    assert (nat.AUDIT_ROWS, nat.AUDIT_MAX_CUBOIDS) == (8, 16)
    # no context: refused before anything else, like every entry point
    assert lib.uavac_minsnap_audit_dev(None, None, None, None, 1, 1, 0.01, None, 0, None, None, None) == nat.EINVAL


def _audit(speed_xy, ascent, descent, accel_xy, hit_rows=None):
    import torch
    t = lambda v: torch.tensor(v, dtype=torch.float64)      # noqa: E731
    B = len(speed_xy)
    hits = torch.zeros((0, B), dtype=torch.int32) if hit_rows is None else torch.tensor(hit_rows, dtype=torch.int32).reshape(-1, B)
    return SimpleNamespace(speed_xy=t(speed_xy), ascent=t(ascent), descent=t(descent), accel_xy=t(accel_xy), hit_rows=hits)


def _up(x):
    return math.nextafter(x, math.inf)


def test_plan_feasibility_limits_slack_nan_and_vehicle():
    from uav_ac import _native as nat
    from uav_ac.scoring import plan_feasibility
    V = nat.Vehicle.default()
    sp, asc, desc, acc = V.max_speed_xy, V.max_ascent, V.max_descent, V.max_horiz_accel
    assert (asc, desc, sp, acc) == (3.0, 2.0, 3.0, 12.0)          # the laboratory vehicle
    nan = float("nan")
    # mission 0: everything exactly at its limit; 1-4: one quantity one ulp above; 5: NaN peaks; 6: well inside
    a = _audit([sp, _up(sp), sp, sp, sp, nan, 1.0], [asc, asc, _up(asc), asc, asc, nan, 1.0],
               [desc, desc, desc, _up(desc), desc, nan, 1.0], [acc, acc, acc, acc, _up(acc), nan, 1.0])
    f = plan_feasibility(a)
    assert set(f) == {"speed_ok", "ascent_ok", "descent_ok", "accel_ok", "clear", "feasible"}
    assert all(v.dtype.is_floating_point is False and tuple(v.shape) == (7,) for v in f.values())
    assert f["speed_ok"].tolist() == [True, False, True, True, True, False, True]
    assert f["ascent_ok"].tolist() == [True, True, False, True, True, False, True]
    assert f["descent_ok"].tolist() == [True, True, True, False, True, False, True]
    assert f["accel_ok"].tolist() == [True, True, True, True, False, False, True]
    assert f["clear"].tolist() == [True, True, True, True, True, False, True]          # no cuboid given; NaN fails every test
    assert f["feasible"].tolist() == [True, False, False, False, False, False, True]
    # vehicle=None is the default vehicle
    g = plan_feasibility(a, vehicle=V)
    assert all(f[k].tolist() == g[k].tolist() for k in f)
    # slack moves every limit: one ulp above passes with any positive slack that survives the addition, NaN still fails
    s = plan_feasibility(a, slack=1e-9)
    assert s["feasible"].tolist() == [True, True, True, True, True, False, True]
    s = plan_feasibility(a, slack=-0.5)                            # a margin asked for: at the limit is no longer enough
    assert s["feasible"].tolist() == [False, False, False, False, False, False, True]
    # a vehicle with other limits
    W = V.copy()
    W.max_speed_xy, W.max_ascent, W.max_descent, W.max_horiz_accel = 0.5, 5.0, 5.0, 20.0
    w = plan_feasibility(a, vehicle=W)
    assert w["speed_ok"].tolist() == [False] * 7
    assert w["ascent_ok"].tolist() == w["descent_ok"].tolist() == w["accel_ok"].tolist() == [True] * 5 + [False, True]
    assert not w["feasible"].any()
    # anything that carries the four limits will do
    X = SimpleNamespace(max_speed_xy=10.0, max_ascent=10.0, max_descent=10.0, max_horiz_accel=100.0)
    assert plan_feasibility(a, vehicle=X)["feasible"].tolist() == [True] * 5 + [False, True]


def test_plan_feasibility_clear_with_and_without_cuboids():
    import torch
    from uav_ac.scoring import plan_feasibility
    nan = float("nan")
    peaks = ([1.0, 1.0, 1.0, nan], [1.0] * 3 + [nan], [1.0] * 3 + [nan], [1.0] * 3 + [nan])
    none = plan_feasibility(_audit(*peaks))
    assert none["clear"].tolist() == [True, True, True, False]
    # two cuboids: mission 0 misses both, 1 is inside the first for 3 samples, 2 inside the second for 1; the NaN mission has no hits
    hits = plan_feasibility(_audit(*peaks, hit_rows=[[0, 3, 0, 0], [0, 0, 1, 0]]))
    assert hits["clear"].tolist() == [True, False, False, False]
    assert hits["feasible"].tolist() == [True, False, False, False]
    assert hits["speed_ok"].tolist() == [True, True, True, False]
    # a PlanAudit-shaped object without the field at all
    bare = _audit(*peaks)
    del bare.hit_rows
    assert plan_feasibility(bare)["clear"].tolist() == [True, True, True, False]
    assert all(v.dtype == torch.bool for v in hits.values())
