"""Retiming plans to the flight limits, the parts that need no GPU: the rule (`uav_ac.scoring.retime_factors`, the specification the
kernel of csrc/minsnap_retime.hip is tested against in tests/test_gpu_retime.py), the loop it rests on replayed with the NumPy
oracle, and the C ABI's new symbols.

The rule, per mission, every step one rounded IEEE operation:
    r = max(speed_xy / L0, ascent / L1, descent / L2, sqrt(accel_xy / L3));  NaN peak -> NaN;  r <= 1 -> 1.0;  else r / (1 - margin)
The expected factors below are written out with Python floats (IEEE double, one operation at a time), not taken from the function.
"""
import math
import os
import re

import numpy as np
import pytest

from conftest import REPO

MARGIN = 1e-3
LIMITS = (3.0, 3.0, 2.0, 12.0)          # max_speed_xy, max_ascent, max_descent, max_horiz_accel of uavac_vehicle_default
NAN = float("nan")

# (speed_xy, ascent, descent, accel_xy) and the factor the rule gives; None = NaN
CRAFTED = [
    ((2.0, 1.0, 1.0, 5.0), 1.0),                                         # all under the limits
    ((4.5, 1.0, 1.0, 5.0), (4.5 / 3.0) / (1.0 - MARGIN)),                # each of the four limits binding alone
    ((2.0, 3.3, 1.0, 5.0), (3.3 / 3.0) / (1.0 - MARGIN)),
    ((2.0, 1.0, 2.9, 5.0), (2.9 / 2.0) / (1.0 - MARGIN)),
    ((2.0, 1.0, 1.0, 27.0), math.sqrt(27.0 / 12.0) / (1.0 - MARGIN)),
    ((3.0, 1.0, 1.0, 5.0), 1.0),                                         # a peak exactly at its limit: not slowed down
    ((2.0, 3.0, 2.0, 12.0), 1.0),                                        # ... three of them at once
    ((2.0, -0.7, 2.5, 5.0), (2.5 / 2.0) / (1.0 - MARGIN)),               # a negative ascent peak (a mission that only descends)
    ((2.0, -0.7, 1.0, 5.0), 1.0),
    ((NAN, NAN, NAN, NAN), None),                                        # what the audit writes for a singular plan
    ((4.5, NAN, 1.0, 5.0), None),                                        # one NaN among the four is enough
    ((3.6, 1.0, 3.0, 30.0), math.sqrt(30.0 / 12.0) / (1.0 - MARGIN)),    # several over: the largest ratio decides (1.2, 1.5, 1.58)
    ((3.0000000000000004, 1.0, 1.0, 5.0), (3.0000000000000004 / 3.0) / (1.0 - MARGIN)),      # one ulp over
]


def crafted_block(B=None):
    """The crafted audit block [8][B] (tiled to B columns when B is given), the expected factors and a set of velocities."""
    n = len(CRAFTED)
    B = n if B is None else B
    idx = np.arange(B) % n
    peaks = np.array([c[0] for c in CRAFTED]).T                         # (4, n)
    want = np.array([NAN if c[1] is None else c[1] for c in CRAFTED])
    block = np.empty((8, B))
    block[0] = 100.0 + np.arange(B)                                      # row totals: not read
    block[1:5] = peaks[:, idx]
    block[5:8] = 0.25                                                    # accel_up, accel_down, speed: not read
    velocities = 0.5 + 0.013 * np.arange(B) + (np.arange(B) % 7) / 3.0   # no two alike
    return block, want[idx], velocities


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def test_retime_factors_on_the_crafted_block():
    from types import SimpleNamespace
    from uav_ac.scoring import retime_factors
    block, want, vel = crafted_block()
    got = retime_factors(block, margin=MARGIN, velocities=vel)
    assert np.array_equal(np.isnan(got["factors"]), np.isnan(want))
    ok = ~np.isnan(want)
    assert same_bits(got["factors"][ok], want[ok]), (got["factors"], want)
    assert got["nan"].tolist() == np.isnan(want).tolist() and got["n_nan"] == 2
    assert got["retimed"].tolist() == [bool(w > 1.0) for w in want] and got["n_retimed"] == 7
    # velocities: untouched bit for bit unless retimed, one division otherwise
    keep = ~got["retimed"]
    assert same_bits(got["velocities"][keep], vel[keep])
    assert same_bits(got["velocities"][~keep], np.array([v / k for v, k in zip(vel[~keep], want[~keep])]))
    # the same from an object with the audit's fields, from torch tensors, and for an explicit vehicle
    import torch
    obj = SimpleNamespace(speed_xy=torch.as_tensor(block[1]), ascent=torch.as_tensor(block[2]), descent=torch.as_tensor(block[3]),
                          accel_xy=torch.as_tensor(block[4]))
    veh = SimpleNamespace(max_speed_xy=LIMITS[0], max_ascent=LIMITS[1], max_descent=LIMITS[2], max_horiz_accel=LIMITS[3])
    for a, v in ((obj, None), (torch.as_tensor(block), veh)):
        assert same_bits(retime_factors(a, v, MARGIN)["factors"], got["factors"])
    # other limits, no margin: k == r
    wide = SimpleNamespace(max_speed_xy=9.0, max_ascent=9.0, max_descent=9.0, max_horiz_accel=36.0)
    f = retime_factors(block, wide, 0.0)["factors"]
    assert np.all(f[ok] == 1.0) and np.isnan(f[~ok]).all()
    tight = SimpleNamespace(max_speed_xy=1.0, max_ascent=3.0, max_descent=2.0, max_horiz_accel=12.0)
    assert retime_factors(block, tight, 0.0)["factors"][0] == 2.0
    for bad in (dict(margin=1.0), dict(margin=-1e-9), dict(margin=NAN),
                dict(vehicle=SimpleNamespace(max_speed_xy=0.0, max_ascent=3.0, max_descent=2.0, max_horiz_accel=12.0)),
                dict(vehicle=SimpleNamespace(max_speed_xy=3.0, max_ascent=3.0, max_descent=math.inf, max_horiz_accel=12.0))):
        with pytest.raises(ValueError):
            retime_factors(block, **bad)
    with pytest.raises(ValueError):
        retime_factors(np.zeros((7, 4)))


def oracle_peaks(wp, velocity, dt):
    """The audit's four peaks of one mission from the NumPy oracle's own solve and sampler."""
    from oracle import minsnap_oracle as mo
    coeffs, times, _, _ = mo.solve_coefficients(wp, velocity, method="solve")
    _, v, a, _ = mo.sample(coeffs, times, dt)
    return (np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]).max(), (-v[:, 2]).max(), v[:, 2].max(),
            np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]).max())


@pytest.mark.parametrize("m", [2, 8])
def test_one_pass_of_the_rule_makes_every_oracle_mission_feasible(m):
    """The loop of uavac_minsnap_retime_dev with the NumPy oracle in the place of the device chain: 48 bench missions at the
    bench's 3 m/s all exceed a limit of the default vehicle; planned again at velocity / k they are all inside, after ONE pass."""
    from oracle import minsnap_oracle as mo
    from uav_ac.scoring import retime_factors
    B, v0, dt = 48, 3.0, 0.01
    wps = mo.synthetic_missions(B, m)

    def audit_block(vel):
        block = np.zeros((8, B))
        for b in range(B):
            block[1:5, b] = oracle_peaks(wps[b], vel[b], dt)
        return block

    lim = np.array(LIMITS)[:, None]
    before = audit_block(np.full(B, v0))
    excess = np.max(np.concatenate([before[1:4] / lim[:3], np.sqrt(before[4:5] / lim[3:])]), axis=0)
    assert (excess > 1.0).all()                                          # every mission is infeasible as planned
    first = retime_factors(before, margin=MARGIN, velocities=np.full(B, v0))
    assert first["n_retimed"] == B and first["n_nan"] == 0
    assert same_bits(first["factors"], excess / (1.0 - MARGIN))
    after = audit_block(first["velocities"])
    ratio = np.max(after[1:5] / lim, axis=0)
    print(f"m={m}: worst excess before {excess.min():.3f} .. {excess.max():.3f}; worst peak / limit after one pass "
          f"{ratio.min():.5f} .. {ratio.max():.5f}")
    assert (after[1:5] <= lim).all()                                     # feasible with no slack
    second = retime_factors(after, margin=MARGIN, velocities=first["velocities"])
    assert second["n_retimed"] == 0 and (second["factors"] == 1.0).all()
    assert same_bits(second["velocities"], first["velocities"])


NEW_SYMBOLS = ("uavac_minsnap_row_counts_v_dev", "uavac_minsnap_row_counts_ragged_v_dev", "uavac_minsnap_plan_v_dev",
               "uavac_minsnap_retime_factors_dev", "uavac_minsnap_retime_dev")


def test_the_new_entry_points_are_declared_exported_and_prototyped():
    from uav_ac import _native as nat
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "uavac.h")).read(), flags=re.S)
    lib = nat.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in nat.exported_symbols()
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == text.split(name + "(")[1].split(")")[0].count(",") + 1, name
    assert lib.uavac_version() == nat.VERSION == 310
    # nothing runs without a context: the entry points refuse a NULL one before they look at anything else
    assert lib.uavac_minsnap_retime_factors_dev(None, None, 1, None, 0.0, None, None, None) == nat.EINVAL
    assert lib.uavac_minsnap_plan_v_dev(None, None, 1, 1, None, 0.01, None, None, None, None, None, None, 0, None, None) == nat.EINVAL
