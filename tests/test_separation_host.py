"""Separation audit, the part that needs no GPU: the entry point is exported and declared as the header declares it, a NULL context
is refused, and the rule itself -- `uav_ac.scoring.separation_from_rows`, the NumPy statement the kernel is tested against bit for
bit (tests/test_gpu_separation.py) -- gives the answers that hand-made rows have by inspection; `scoring.separation_ok` on hand-made
blocks."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import REPO


def rows_of(*paths):
    """Missions given as (N_b, 3) position lists -> (rows (N, 11), row_offsets (B + 1,)): the sampler's layout, positions in 0-2."""
    ro = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    rows = np.zeros((int(ro[-1]), 11))
    for b, p in enumerate(paths):
        rows[ro[b]:ro[b + 1], 0:3] = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    return rows, ro


def line(p0, p1, n):
    return np.linspace(np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64), n)


def test_entry_point_is_exported_and_declared_like_the_header():
    from uav_ac import _native as nat
    assert nat.SEP_ROWS == 5
    assert "uavac_minsnap_separation_dev" in nat.exported_symbols()
    fn = nat.lib().uavac_minsnap_separation_dev
    restype, argtypes = nat._SIGNATURES["uavac_minsnap_separation_dev"]
    assert restype is C.c_int and len(argtypes) == 13
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "uavac.h")).read(), flags=re.S)
    args = re.search(r"int\s+uavac_minsnap_separation_dev\s*\(([^)]*)\)\s*;", text).group(1)
    params = [" ".join(a.split()) for a in args.split(",")]
    assert len(params) == 13
    kinds = [C.c_void_p if "*" in a else {"int": C.c_int, "double": C.c_double}[a.split()[0]] for a in params]
    assert kinds == list(argtypes), params
    assert re.search(r"#define\s+UAVAC_SEP_ROWS\s+5\b", text)
    assert int(re.search(r"#define\s+UAVAC_SEP_MAX_SPLIT\s+(\d+)", text).group(1)) == nat.SEP_MAX_SPLIT
    # a NULL context is refused before anything else is looked at (pure host code: no GPU needed)
    assert fn(None, None, None, None, 1, 1, 0.01, None, 0, None, 0.5, None, None) == nat.EINVAL


def test_two_straight_lines_crossing():
    from uav_ac.scoring import separation_from_rows
    # both pass (5, 5, -3): A along x at row 50, B along y at row 50 -> distance 0 there; 0.1 m per row each
    a, b = line([0, 5, -3], [10, 5, -3], 101), line([5, 0, -3], [5, 10, -3], 101)
    sep, isep = separation_from_rows(*rows_of(a, b), radius=0.5)
    assert sep.tolist() == [0.0, 0.0]
    assert isep[0].tolist() == [1, 0] and isep[1].tolist() == [50, 50] and isep[4].tolist() == [1, 1]
    # d(k) = sqrt(2) * 0.1 * |k - 50| < 0.5  <=>  |k - 50| <= 3: first inside at row 47
    assert isep[2].tolist() == [1, 1] and isep[3].tolist() == [47, 47]
    _, zero = separation_from_rows(*rows_of(a, b), radius=0.0)
    assert zero[2].tolist() == [0, 0] and zero[3].tolist() == [-1, -1]       # distance 0 is not < 0


def test_a_parked_vehicle_and_a_passing_one():
    from uav_ac.scoring import separation_from_rows
    parked = [[4.0, 0.25, -3.0]]                              # one row: holds it for the whole horizon
    passing = line([0, 0, -3], [8, 0, -3], 81)                # 0.1 m per row along y = 0: nearest at row 40, 0.25 m off
    sep, isep = separation_from_rows(*rows_of(parked, passing), radius=0.5)
    assert sep.tolist() == [0.25, 0.25] and isep[0].tolist() == [1, 0] and isep[1].tolist() == [40, 40]
    # inside while 0.0625 + dx^2 < 0.25 <=> |dx| < 0.433: rows 36 .. 44
    assert isep[2].tolist() == [1, 1] and isep[3].tolist() == [36, 36] and isep[4].tolist() == [1, 1]
    # the test is strict: at a radius of exactly the closest approach nobody is inside
    _, strict = separation_from_rows(*rows_of(parked, passing), radius=0.25)
    assert strict[2].tolist() == [0, 0] and strict[3].tolist() == [-1, -1]


def test_a_staggered_start_removes_the_conflict():
    from uav_ac.scoring import separation_from_rows
    a, b = line([0, 5, -3], [10, 5, -3], 101), line([5, 0, -3], [5, 10, -3], 101)
    rows, ro = rows_of(a, b)
    sep, isep = separation_from_rows(rows, ro, 0.5, start_rows=[0, 40])
    # B waits at (5, 0) until row 40; A passes x = 5 at row 50, 5 m away from B's y = 1.0 there
    assert isep[2].tolist() == [0, 0] and isep[3].tolist() == [-1, -1]
    # A ends at (10, 5) at row 100 and holds; B reaches (5, 10) at row 140: horizon 141.  nearest: minimise (0.1k - 5)^2 + (0.1(k-40) - 5)^2
    # for k <= 100 -> k = 70: distance sqrt(4 + 4)
    assert isep[1].tolist() == [70, 70] and np.allclose(sep, np.sqrt(8.0), rtol=0, atol=1e-12)
    # a negative start row counts as 0
    again = separation_from_rows(rows, ro, 0.5, start_rows=[-7, 40])
    assert np.array_equal(again[0], sep) and np.array_equal(again[1], isep)


def test_a_duplicate_reports_distance_zero_and_the_lowest_partner():
    from uav_ac.scoring import separation_from_rows
    a = line([0, 0, -3], [3, 0, -3], 31)
    far = line([0, 9, -3], [3, 9, -3], 31)
    sep, isep = separation_from_rows(*rows_of(far, a, a.copy(), a.copy()), radius=0.5)
    assert sep.tolist() == [9.0, 0.0, 0.0, 0.0]
    assert isep[0].tolist() == [1, 2, 1, 1]                   # the LOWEST partner among equals (and never oneself)
    assert isep[1].tolist() == [0, 0, 0, 0]                   # ... at the lowest row
    assert isep[2].tolist() == [0, 2, 2, 2] and isep[3].tolist() == [-1, 0, 0, 0] and isep[4].tolist() == [3, 3, 3, 3]


def test_a_tie_across_rows_goes_to_the_lowest_row():
    from uav_ac.scoring import separation_from_rows
    # A stands still; B passes through two points at the same distance 1.0 (rows 2 and 6), farther everywhere else
    a = [[0.0, 0.0, 0.0]] * 9
    b = [[3, 0, 0], [2, 0, 0], [1, 0, 0], [0, 2, 0], [0, 3, 0], [0, 2, 0], [0, 1, 0], [0, 2, 0], [0, 3, 0]]
    sep, isep = separation_from_rows(*rows_of(a, b), radius=1.0)
    assert sep.tolist() == [1.0, 1.0] and isep[1].tolist() == [2, 2]
    assert isep[2].tolist() == [0, 0]                         # 1.0 is not < 1.0


def test_groups_of_one_empty_groups_and_separate_airspaces():
    from uav_ac.scoring import separation_from_rows
    a = line([0, 0, -3], [3, 0, -3], 31)
    rows, ro = rows_of(a, a + [0, 0.1, 0], a + [0, 0.2, 0], a + [0, 0.3, 0])
    sep, isep = separation_from_rows(rows, ro, 0.5, group_offsets=[0, 1, 1, 3, 4])     # sizes 1, 0, 2, 1
    assert sep[0] == np.inf and sep[3] == np.inf and np.allclose(sep[1:3], 0.1, rtol=0, atol=1e-15)
    assert isep[0].tolist() == [-1, 2, 1, -1] and isep[1].tolist() == [-1, 0, 0, -1]
    assert isep[2].tolist() == [0, 1, 1, 0] and isep[3].tolist() == [-1, 0, 0, -1] and isep[4].tolist() == [0, 1, 1, 0]
    # one airspace: everybody sees the neighbours
    _, one = separation_from_rows(rows, ro, 0.25)
    assert one[2].tolist() == [2, 3, 3, 2] and one[4].tolist() == [3, 3, 3, 3]       # within 0.25 m: the next two lines, not the third
    with pytest.raises(ValueError):
        separation_from_rows(rows, ro, 0.5, group_offsets=[0, 3, 2, 4])
    with pytest.raises(ValueError):
        separation_from_rows(rows, ro, -1.0)


def test_an_excluded_mission_and_what_its_neighbours_report():
    from uav_ac.scoring import separation_from_rows
    a = line([0, 0, -3], [3, 0, -3], 31)
    broken = a + [0, 0.05, 0]
    broken[:] = np.nan                                        # what a singular solve samples to
    rows, ro = rows_of(a, broken, a + [0, 0.3, 0], np.zeros((0, 3)))                   # ... and one mission without rows
    sep, isep = separation_from_rows(rows, ro, 0.5)
    assert np.isnan(sep[[1, 3]]).all() and np.allclose(sep[[0, 2]], 0.3, rtol=0, atol=1e-15)
    assert isep[:, 1].tolist() == [-1, -1, 0, -1, 0] and isep[:, 3].tolist() == [-1, -1, 0, -1, 0]
    assert isep[:, 0].tolist() == [2, 0, 1, 0, 1] and isep[:, 2].tolist() == [0, 0, 1, 0, 1]      # compared 1 of 3: the gap is visible


def test_separation_ok_on_hand_made_blocks():
    from uav_ac.scoring import separation_ok
    sep = SimpleNamespace(min_distance=np.array([2.0, 0.3, np.nan, np.inf, 1.5]), conflicts=np.array([0, 1, 0, 0, 0]),
                          compared=np.array([4, 4, 0, 0, 3]))
    v = separation_ok(sep, group_sizes=5)
    assert v["clear"].tolist() == [True, False, False, True, True]
    assert v["complete"].tolist() == [True, True, False, False, False]
    assert v["ok"].tolist() == [True, False, False, False, False]
    per = separation_ok(sep, group_sizes=np.array([5, 5, 5, 1, 4]))
    assert per["complete"].tolist() == [True, True, False, True, True] and per["ok"].tolist() == [True, False, False, True, True]
    none = separation_ok(sep)                                 # without the sizes nothing can be called complete
    assert not none["complete"].any() and not none["ok"].any() and none["clear"].tolist() == v["clear"].tolist()
    with pytest.raises(ValueError):
        separation_ok(sep, group_sizes=[5, 5])


def test_the_build_keeps_the_separation_kernels_in_registers():
    from uav_ac import _buildcheck
    counts = _buildcheck.check_separation_kernels()
    if counts is None:
        pytest.skip("no object files here (a library that was built elsewhere)")
    assert len(counts) == 3 and max(counts.values()) <= 168
