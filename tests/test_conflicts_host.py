"""Conflict list, the part that needs no GPU: the two entry points are exported and declared as the header declares them, a NULL context
is refused, and the rule itself -- `uav_ac.scoring.conflicts_from_rows`, the NumPy statement the kernels are tested against bit for bit
(tests/test_gpu_conflicts.py) -- gives the answers that hand-made rows have by inspection and agrees with `separation_from_rows`;
`scoring.conflict_pairs` on good and on doctored lists."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import REPO

PARTNER, FIRST, LAST, INSIDE, MIN_ROW = range(5)


def rows_of(*paths):
    """Missions given as (N_b, 3) position lists -> (rows (N, 11), row_offsets (B + 1,)): the sampler's layout, positions in 0-2."""
    ro = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    rows = np.zeros((int(ro[-1]), 11))
    for b, p in enumerate(paths):
        rows[ro[b]:ro[b + 1], 0:3] = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    return rows, ro


def line(p0, p1, n):
    return np.linspace(np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64), n)


def as_list(offsets, pair_d, pair_i):
    return SimpleNamespace(offsets=offsets, partner=pair_i[0], first_row=pair_i[1], last_row=pair_i[2], rows_inside=pair_i[3],
                           min_row=pair_i[4], min_distance=pair_d)


def test_entry_points_are_exported_and_declared_like_the_header():
    from uav_ac import _native as nat
    assert nat.CONF_ROWS == 5
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "uavac.h")).read(), flags=re.S)
    assert re.search(r"#define\s+UAVAC_CONF_ROWS\s+5\b", text)
    for name, n in (("uavac_minsnap_conflict_offsets_dev", 12), ("uavac_minsnap_conflicts_dev", 15)):
        assert name in nat.exported_symbols()
        restype, argtypes = nat._SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == n
        args = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", text).group(1)
        params = [" ".join(a.split()) for a in args.split(",")]
        assert len(params) == n
        kinds = [C.c_void_p if "*" in a else {"int": C.c_int, "double": C.c_double, "int64_t": C.c_int64}[a.split()[0]] for a in params]
        assert kinds == list(argtypes), params
    # a NULL context is refused before anything else is looked at (pure host code: no GPU needed)
    lib = nat.lib()
    assert lib.uavac_minsnap_conflict_offsets_dev(None, None, None, None, 1, 1, 0.01, None, 0, None, 0.5, None) == nat.EINVAL
    assert lib.uavac_minsnap_conflicts_dev(None, None, None, None, 1, 1, 0.01, None, 0, None, 0.5, None, 0, None, None) == nat.EINVAL


def test_two_straight_lines_crossing():
    from uav_ac.scoring import conflicts_from_rows
    # both pass (5, 5, -3) at row 50, 0.1 m per row each: d(k) = sqrt(2) * 0.1 * |k - 50| < 0.5  <=>  |k - 50| <= 3
    a, b = line([0, 5, -3], [10, 5, -3], 101), line([5, 0, -3], [5, 10, -3], 101)
    off, d, i = conflicts_from_rows(*rows_of(a, b), radius=0.5)
    assert off.dtype == np.int64 and d.dtype == np.float64 and i.dtype == np.int32 and i.shape == (5, 2)
    assert off.tolist() == [0, 1, 2] and d.tolist() == [0.0, 0.0]
    assert i[PARTNER].tolist() == [1, 0] and i[FIRST].tolist() == [47, 47] and i[LAST].tolist() == [53, 53]
    assert i[INSIDE].tolist() == [7, 7] and i[MIN_ROW].tolist() == [50, 50]
    # radius 0: distance 0 is not < 0 -- nothing is listed, and the empty arrays keep their shapes
    off, d, i = conflicts_from_rows(*rows_of(a, b), radius=0.0)
    assert off.tolist() == [0, 0, 0] and d.shape == (0,) and i.shape == (5, 0)


def test_a_parked_vehicle_and_a_passing_one():
    from uav_ac.scoring import conflicts_from_rows
    parked = [[4.0, 0.25, -3.0]]                              # one row: holds it for the whole horizon
    passing = line([0, 0, -3], [8, 0, -3], 81)                # 0.1 m per row along y = 0: nearest at row 40, 0.25 m off
    off, d, i = conflicts_from_rows(*rows_of(parked, passing), radius=0.5)
    # inside while 0.0625 + dx^2 < 0.25 <=> |dx| < 0.433: rows 36 .. 44
    assert off.tolist() == [0, 1, 2] and d.tolist() == [0.25, 0.25] and i[PARTNER].tolist() == [1, 0]
    assert i[FIRST].tolist() == [36, 36] and i[LAST].tolist() == [44, 44] and i[INSIDE].tolist() == [9, 9] and i[MIN_ROW].tolist() == [40, 40]
    # the test is strict: at a radius of exactly the closest approach nobody is inside
    assert conflicts_from_rows(*rows_of(parked, passing), radius=0.25)[0].tolist() == [0, 0, 0]


def test_passing_twice_leaves_a_gap():
    from uav_ac.scoring import conflicts_from_rows
    parked = [[4.0, 0.25, -3.0]]
    out = line([0, 0, -3], [8, 0, -3], 81)
    there_and_back = np.concatenate([out, out[-2::-1]])       # 161 rows: past the parked one at row 40 and again at row 120
    off, d, i = conflicts_from_rows(*rows_of(parked, there_and_back), radius=0.5)
    assert off.tolist() == [0, 1, 2] and d.tolist() == [0.25, 0.25]
    assert i[FIRST].tolist() == [36, 36] and i[LAST].tolist() == [124, 124] and i[INSIDE].tolist() == [18, 18]
    assert (i[INSIDE] < i[LAST] - i[FIRST] + 1).all()
    assert i[MIN_ROW].tolist() == [40, 40]                    # the same distance at rows 40 and 120: the lowest row


def test_start_rows_move_an_incursion():
    from uav_ac.scoring import conflicts_from_rows
    a, b = line([0, 5, -3], [10, 5, -3], 101), line([5, 0, -3], [5, 10, -3], 101)
    rows, ro = rows_of(a, b)
    # B waits 40 rows: when A passes x = 5, B is 4 m short of the crossing -- nobody inside any more
    assert conflicts_from_rows(rows, ro, 0.5, start_rows=[0, 40])[0].tolist() == [0, 0, 0]
    # both wait the same 25 rows: the incursion moves with them; a negative start counts as 0
    off, d, i = conflicts_from_rows(rows, ro, 0.5, start_rows=[25, 25])
    assert i[FIRST].tolist() == [72, 72] and i[LAST].tolist() == [78, 78] and i[INSIDE].tolist() == [7, 7] and i[MIN_ROW].tolist() == [75, 75]
    again = conflicts_from_rows(rows, ro, 0.5, start_rows=[-3, 0])
    for got, want in zip(again, conflicts_from_rows(rows, ro, 0.5)):
        assert np.array_equal(got, want)
    # two missions that wait on the same first waypoint are inside from row 0 on, and stay inside after their ends if they end together
    c = line([0, 5, -3], [0, 9, -3], 41)
    off, d, i = conflicts_from_rows(*rows_of(a, c), radius=0.5, start_rows=[10, 30])
    # A leaves at row 10, 0.1 m per row: inside while 0.1 (k - 10) < 0.5 <=> k <= 14
    assert i[FIRST].tolist() == [0, 0] and i[LAST].tolist() == [14, 14] and i[INSIDE].tolist() == [15, 15] and d.tolist() == [0.0, 0.0]
    assert i[MIN_ROW].tolist() == [0, 0]


def test_groups_are_never_compared_and_partners_ascend():
    from uav_ac.scoring import conflicts_from_rows
    a = line([0, 0, -3], [3, 0, -3], 31)
    rows, ro = rows_of(a, a + [0, 0.1, 0], a + [0, 0.2, 0], a + [0, 0.3, 0])
    off, d, i = conflicts_from_rows(rows, ro, 0.5, group_offsets=[0, 1, 1, 3, 4])       # sizes 1, 0, 2, 1: a group of one lists nothing
    assert off.tolist() == [0, 0, 1, 2, 2] and i[PARTNER].tolist() == [2, 1] and np.allclose(d, 0.1, rtol=0, atol=1e-15)
    assert i[FIRST].tolist() == [0, 0] and i[LAST].tolist() == [30, 30] and i[INSIDE].tolist() == [31, 31]
    # one airspace, within 0.25 m: the next two lines, not the third -- partners in ascending batch index
    off, d, i = conflicts_from_rows(rows, ro, 0.25)
    assert off.tolist() == [0, 2, 5, 8, 10]
    assert i[PARTNER].tolist() == [1, 2, 0, 2, 3, 0, 1, 3, 1, 2]
    with pytest.raises(ValueError):
        conflicts_from_rows(rows, ro, 0.5, group_offsets=[0, 3, 2, 4])
    with pytest.raises(ValueError):
        conflicts_from_rows(rows, ro, -1.0)


def test_an_excluded_mission_lists_nothing_and_is_listed_by_nobody():
    from uav_ac.scoring import conflicts_from_rows
    a = line([0, 0, -3], [3, 0, -3], 31)
    broken = a + [0, 0.05, 0]
    broken[:] = np.nan                                        # what a singular solve samples to
    rows, ro = rows_of(a, broken, a + [0, 0.3, 0], np.zeros((0, 3)))                   # ... and one mission without rows
    off, d, i = conflicts_from_rows(rows, ro, 0.5)
    assert off.tolist() == [0, 1, 1, 2, 2] and i[PARTNER].tolist() == [2, 0] and np.allclose(d, 0.3, rtol=0, atol=1e-15)


def _random_rows(seed, B=9):
    rng = np.random.default_rng(seed)
    paths = []
    for b in range(B):
        n = int(rng.integers(20, 60))
        p0, p1 = rng.uniform(0, 3, 3), rng.uniform(0, 3, 3)
        paths.append(line(p0, p1, n) + rng.normal(0, 0.01, (n, 3)))
    return rows_of(*paths)


@pytest.mark.parametrize("seed", range(4))
def test_the_list_agrees_with_the_audit(seed):
    from uav_ac.scoring import conflict_pairs, conflicts_from_rows, separation_from_rows
    rows, ro = _random_rows(seed)
    B = len(ro) - 1
    for go, st in ((None, None), ([0, 4, 4, 5, B], (np.arange(B) % 3) * 7)):
        sep, isep = separation_from_rows(rows, ro, 0.8, go, st)
        off, d, i = conflicts_from_rows(rows, ro, 0.8, go, st)
        assert np.array_equal(np.diff(off), isep[2]) and off[0] == 0
        assert isep[2].sum() > 0
        for b in range(B):
            e = slice(off[b], off[b + 1])
            assert (np.diff(i[PARTNER, e]) > 0).all()
            if isep[2, b] == 0:
                assert isep[3, b] == -1
                continue
            assert i[FIRST, e].min() == isep[3, b]
            assert min(zip(d[e], i[MIN_ROW, e], i[PARTNER, e])) == (sep[b], isep[1, b], isep[0, b])
        pairs = conflict_pairs(as_list(off, d, i))             # both directions carry the same record
        assert 2 * len(pairs["i"]) == off[-1] and (pairs["i"] < pairs["j"]).all()


def test_conflict_pairs_and_a_doctored_list():
    from uav_ac.scoring import conflict_pairs, conflicts_from_rows
    a = line([0, 0, -3], [3, 0, -3], 31)
    rows, ro = rows_of(a, a + [0, 0.1, 0], a + [0, 0.2, 0], a + [0, 0.3, 0])
    off, d, i = conflicts_from_rows(rows, ro, 0.25)
    pairs = conflict_pairs(as_list(off, d, i))
    assert pairs["i"].tolist() == [0, 0, 1, 1, 2] and pairs["j"].tolist() == [1, 2, 2, 3, 3]
    assert pairs["first_row"].tolist() == [0] * 5 and pairs["rows_inside"].tolist() == [31] * 5
    assert np.allclose(pairs["min_distance"], [0.1, 0.2, 0.1, 0.2, 0.1], rtol=0, atol=1e-15)
    empty = conflict_pairs(as_list(np.zeros(5, dtype=np.int64), d[:0], i[:, :0]))
    assert all(len(v) == 0 for v in empty.values())
    for row in (FIRST, LAST, INSIDE, MIN_ROW):                # one direction of a pair says something else
        bad = i.copy()
        bad[row, 3] += 1
        with pytest.raises(ValueError):
            conflict_pairs(as_list(off, d, bad))
    worse = d.copy()
    worse[0] = np.nextafter(worse[0], 1.0)
    with pytest.raises(ValueError):
        conflict_pairs(as_list(off, worse, i))
    one_way = i.copy()
    one_way[PARTNER, 0] = 3                                   # 0 lists 3, 3 does not list 0
    with pytest.raises(ValueError):
        conflict_pairs(as_list(off, d, one_way))
    with pytest.raises(ValueError):
        conflict_pairs(as_list(off, d[:-1], i))


def test_the_build_keeps_the_conflict_kernels_inside_their_budgets():
    from uav_ac import _buildcheck
    counts = _buildcheck.check_conflict_kernels()
    if counts is None:
        pytest.skip("no object files here (a library that was built elsewhere)")
    assert len(counts) == 5
    tiled = [v for n, v in counts.items() if "discover" in n or "measure" in n]        # the 48 KB tile: three waves per SIMD
    plain = [v for n, v in counts.items() if not ("discover" in n or "measure" in n)]
    assert len(tiled) == 2 and max(tiled) <= 168 and len(plain) == 3 and max(plain) <= 64
