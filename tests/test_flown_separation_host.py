"""The separation the fleet flew, the part that needs no GPU: the entry point is exported and declared as the header declares it, a NULL
context is refused, the build keeps the kernels inside their budgets, and the rule itself -- `uav_ac.scoring.separation_from_log`, the
NumPy statement the kernel is tested against bit for bit (tests/test_gpu_flown_separation.py) -- gives the answers that hand-made logs
have by inspection.

The hand-made logs stand on a binary grid (steps of 0.125), so every d^2 below is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO

KINDS = {"int": C.c_int, "double": C.c_double, "int64_t": C.c_int64}
NONE = [np.inf, -1, -1, 0, -1, 0]


def log_of(*tracks, rows=13):
    """Vehicles given as (K, 3) position lists -> a state log (K, 13, B): positions in rows 0-2, the other rows junk that is never read."""
    K = len(tracks[0])
    log = np.full((K, rows, len(tracks)), 1e300)
    for b, t in enumerate(tracks):
        log[:, 0:3, b] = np.asarray(t, dtype=np.float64).reshape(K, 3)
    return log


def record(sep, isep, b):
    return [float(sep[b])] + isep[:, b].tolist()


def test_entry_point_is_exported_and_declared_like_the_header():
    from uav_ac import _native as nat
    name = "uavac_flown_separation_dev"
    assert name in nat.exported_symbols() and nat.STATE_LOG_ROWS == 13
    fn = getattr(nat.lib(), name)
    restype, argtypes = nat._SIGNATURES[name]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "uavac.h")).read(), flags=re.S)
    args = re.search(rf"int\s+{name}\s*\(([^)]*)\)\s*;", text).group(1)
    params = [" ".join(a.split()) for a in args.split(",")]
    kinds = [C.c_void_p if "*" in a else KINDS[a.split()[0]] for a in params]
    assert restype is C.c_int and len(argtypes) == 10 and kinds == list(argtypes), params
    # a NULL context is refused before anything else is looked at (pure host code: no GPU needed)
    assert fn(None, None, 1, 1, 1, None, 0, 0.5, None, None) == nat.EINVAL


def test_the_build_keeps_the_flown_separation_kernels_in_registers():
    from uav_ac import _buildcheck
    counts = _buildcheck.check_flown_separation_kernels()
    if counts is None:
        pytest.skip("no object files here (a library that was built elsewhere)")
    assert len(counts) == 2 and max(counts.values()) <= 168
    assert any("flown_separation_kernel" in k for k in counts) and any("flown_merge_kernel" in k for k in counts)
    # the move of the shared reduction into one header left the plan audit's kernels inside their budget too
    assert max(_buildcheck.check_separation_kernels().values()) <= 168


def test_ties_between_ticks_go_to_the_lower_tick_and_between_partners_to_the_lower_partner():
    from uav_ac.scoring import separation_from_log
    still = [[0, 0, 0]] * 4
    on_x = [[1, 0, 0], [0.5, 0, 0], [0.5, 0, 0], [1, 0, 0]]          # 0.5 from the origin at ticks 1 and 2
    on_y = [[0, 0.5, 0], [0, 1, 0], [0, 1, 0], [0, 0.5, 0]]          # 0.5 from the origin at ticks 0 and 3
    log = log_of(still, on_x, on_y)
    sep, isep = separation_from_log(log, 0.75)
    assert sep.dtype == np.float64 and isep.dtype == np.int32 and isep.shape == (5, 3)
    assert record(sep, isep, 0) == [0.5, 2, 0, 2, 0, 2]      # 0.25 four times: the lowest tick wins, and there partner 2 stands
    assert record(sep, isep, 1) == [0.5, 0, 1, 1, 1, 2]      # the origin at tick 1; vehicle 2 stays sqrt(1.25) away
    assert record(sep, isep, 2) == [0.5, 0, 0, 1, 0, 2]
    # inside means strictly inside: at radius 0.5 nobody is
    sep, isep = separation_from_log(log, 0.5)
    assert isep[2].tolist() == [0, 0, 0] and isep[3].tolist() == [-1, -1, -1] and sep.tolist() == [0.5, 0.5, 0.5]
    # two partners equally near at the same tick: the lower index
    log = log_of([[0, 0, 0]] * 2, [[0.5, 0, 0]] * 2, [[0, 0.5, 0]] * 2, [[0, 0, -0.5]] * 2)
    sep, isep = separation_from_log(log, 0.625)
    assert record(sep, isep, 0) == [0.5, 1, 0, 3, 0, 3]
    assert record(sep, isep, 1) == [0.5, 0, 0, 1, 0, 3] and record(sep, isep, 3) == [0.5, 0, 0, 1, 0, 3]
    # one tick is a log too, and rows past the positions are never read
    sep1, isep1 = separation_from_log(log[:1, :3], 0.625)
    assert np.array_equal(sep1, sep) and np.array_equal(isep1, isep)


def test_a_vehicle_whose_log_holds_nan_is_visible_in_compared():
    from uav_ac.scoring import separation_from_log
    nan = np.nan
    a = [[0, 0, 0], [0, 0, 0], [0, 0, 0]]
    b = [[0.125, nan, 0], [1, 0, 0], [0.25, 0, 0]]           # one coordinate NaN at tick 0 (where it would have been nearest)
    c = [[nan, nan, nan]] * 3                                # NaN throughout
    d = [[0, 2, 0], [0, 2, 0], [nan, 2, 0]]
    sep, isep = separation_from_log(log_of(a, b, c, d), 0.5)
    assert record(sep, isep, 0) == [0.25, 1, 2, 1, 2, 2]     # compared with b and d, not with c
    assert record(sep, isep, 1) == [0.25, 0, 2, 1, 2, 2]     # b and d: only tick 1 is valid between them
    assert record(sep, isep, 2) == NONE                      # no valid pair-tick at all
    assert record(sep, isep, 3)[1:] == [0, 0, 0, -1, 2] and sep[3] == 2.0
    # separation_ok applies unchanged: the NaN vehicle is not ok, and its neighbours are not complete
    from types import SimpleNamespace
    from uav_ac.scoring import separation_ok
    v = separation_ok(SimpleNamespace(min_distance=sep, conflicts=isep[2], compared=isep[4]), 4)
    assert v["complete"].tolist() == [False] * 4 and v["clear"].tolist() == [False, False, True, True]


def test_groups_are_audited_apart_and_a_group_of_one_has_nobody():
    from uav_ac.scoring import separation_from_log
    rng = np.random.default_rng(3)
    tracks = [rng.integers(0, 16, (5, 3)) * 0.125 for _ in range(6)]
    log = log_of(*tracks)
    sep, isep = separation_from_log(log, 0.5, [0, 3, 4, 4, 6])        # sizes 3, 1, 0, 2
    assert record(sep, isep, 3) == NONE
    assert set(isep[0, 0:3].tolist()) <= {0, 1, 2} and set(isep[0, 4:6].tolist()) == {4, 5} and isep[4].tolist() == [2, 2, 2, 0, 1, 1]
    # a group audited alone gives the same numbers with the partner indices shifted; so does a view of a wider log
    wide = np.concatenate([log, np.zeros((5, 13, 2))], axis=2)
    for lo, hi in ((0, 3), (4, 6)):
        s, i = separation_from_log(log[:, :, lo:hi], 0.5)
        assert np.array_equal(s, sep[lo:hi]) and np.array_equal(i[1:], isep[1:, lo:hi]) and np.array_equal(i[0] + lo, isep[0, lo:hi])
    s, i = separation_from_log(wide[:, :, :6], 0.5, [0, 3, 4, 4, 6])
    assert np.array_equal(s, sep) and np.array_equal(i, isep)
    # the same vehicles in one airspace: everybody is compared with the five others
    _, one = separation_from_log(log, 0.5)
    assert one[4].tolist() == [5] * 6


def test_malformed_input_raises():
    from uav_ac.scoring import separation_from_log
    log = log_of([[0, 0, 0]], [[1, 0, 0]], [[2, 0, 0]])
    for go in ([0, 2, 1, 3], [1, 3], [0, 2], [0]):
        with pytest.raises(ValueError):
            separation_from_log(log, 0.5, go)
    for radius in (-1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            separation_from_log(log, radius)
    for bad in (log[0], log[:, :2], log[:0]):
        with pytest.raises(ValueError):
            separation_from_log(bad, 0.5)
