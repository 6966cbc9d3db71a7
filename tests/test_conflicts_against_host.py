"""The cross conflict list on the host: the rule `conflicts_against_rows` of uav_ac/scoring.py -- the specification of
`uavac_minsnap_conflict_against_offsets_dev` and `uavac_minsnap_conflicts_against_dev` --, the host-side CSR transpose
`conflicts_transposed`, the two prototypes and the build's budget row for the new object file.  Nothing here needs a GPU.

The rule is checked against an INDEPENDENT derivation from a rule that the GPU tests pin: the per-group interleaved concatenation
[traffic_g, plan_g] run through `conflicts_from_rows`, of whose entries those with a traffic partner are kept; and against the cross
audit `separation_against_rows`, whose three guarantees it has to meet.  The fixture is tests/test_against_host.py's: 18 traffic and
30 plan missions, radius 1.0, one group per side or GO / TGO.  Every comparison is equality, on integers and on the bytes of doubles."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO
from test_against_host import GO, RADIUS, TGO, interleave, keep, missions, offsets_after

PARTNER, FIRST, LAST, INSIDE, MIN_ROW = range(5)
ONE = (np.array([0, 30]), np.array([0, 18]))
_MEMO = {}


def rule(grouped, radius=RADIUS):
    """`conflicts_against_rows` on the module's fixture, computed once per (groups, radius)"""
    if (grouped, radius) not in _MEMO:
        from uav_ac.scoring import conflicts_against_rows
        traffic, plan = missions()
        groups = dict(group_offsets=GO, traffic_group_offsets=TGO) if grouped else {}
        _MEMO[(grouped, radius)] = conflicts_against_rows(plan[0], plan[1], traffic[0], traffic[1], radius, start_rows=plan[2],
                                                          traffic_start_rows=traffic[2], **groups)
    return _MEMO[(grouped, radius)]


def identical(got, want):
    """offsets, the five integer rows and the distances' bytes"""
    return (got[0].dtype == want[0].dtype == np.int64 and np.array_equal(got[0], want[0]) and got[2].dtype == want[2].dtype == np.int32
            and got[2].shape == want[2].shape and np.array_equal(got[2], want[2]) and got[1].dtype == want[1].dtype == np.float64
            and got[1].tobytes() == want[1].tobytes())


def entries(cl, i):
    """the entries of owner i as a list of (partner, first, last, inside, min row, the distance's bytes)"""
    off, d, p = cl
    return [tuple(int(v) for v in p[:, e]) + (d[e].tobytes(),) for e in range(off[i], off[i + 1])]


# ------------------------------------------------------------------------------------------------ 1: the cross pairs of the plain list
@pytest.mark.parametrize("grouped", (False, True), ids=("one group", "two groups"))
def test_the_cross_list_is_the_cross_entries_of_the_list_of_the_concatenation(grouped):
    from uav_ac.scoring import conflicts_from_rows
    traffic, plan = missions()
    go, tgo = (GO, TGO) if grouped else ONE
    rows, ro, st, off, t_at, p_at = interleave(traffic, plan, tgo, go)
    traffic_of = {int(c): j for j, c in enumerate(t_at)}
    g_of = np.searchsorted(go, np.arange(len(p_at)), side="right") - 1
    for radius in (1.0e3, RADIUS):                           # every pair listed; then the conflicting pairs alone
        got = rule(grouped, radius)
        assert got[0].dtype == np.int64 and got[1].dtype == np.float64 and got[2].dtype == np.int32
        assert got[0].shape == (len(p_at) + 1,) and got[2].shape == (5, got[0][-1]) and got[1].shape == (got[0][-1],) and got[0][0] == 0
        whole = conflicts_from_rows(rows, ro, radius, off, st)
        for i, c in enumerate(p_at):
            cross = [(traffic_of[e[0]],) + e[1:] for e in entries(whole, c) if e[0] in traffic_of]
            mine = entries(got, i)
            assert mine == cross, (radius, i)
            assert [e[0] for e in mine] == sorted(e[0] for e in mine)                  # ascending traffic index
        if radius > RADIUS:
            assert np.diff(got[0]).tolist() == [int(tgo[g + 1] - tgo[g]) for g in g_of]
            for i, g in enumerate(g_of):
                assert got[2][PARTNER, got[0][i]:got[0][i + 1]].tolist() == list(range(tgo[g], tgo[g + 1]))
            assert (got[2][FIRST] == 0).all()
        else:
            n = np.diff(got[0])
            assert 5 < (n > 0).sum() < len(p_at), "the fixture's true radius separates nobody, or everybody"
            if not grouped:                                  # what the fixture is here for: several partners, and a pair that parts and meets again
                assert (n >= 2).any() and (got[2][INSIDE] < got[2][LAST] - got[2][FIRST] + 1).any()


# ------------------------------------------------------------------------------------------------ 2: the cross audit's guarantees
@pytest.mark.parametrize("grouped", (False, True), ids=("one group", "two groups"))
def test_the_guarantees_against_the_cross_audit(grouped):
    from uav_ac.scoring import separation_against_rows
    traffic, plan = missions()
    groups = dict(group_offsets=GO, traffic_group_offsets=TGO) if grouped else {}
    sep, isep = separation_against_rows(plan[0], plan[1], traffic[0], traffic[1], RADIUS, start_rows=plan[2], traffic_start_rows=traffic[2],
                                        **groups)
    off, d, p = rule(grouped)
    assert np.array_equal(np.diff(off), isep[2]) and isep[2].sum() > 0
    for i in range(len(sep)):
        e = slice(off[i], off[i + 1])
        if off[i] == off[i + 1]:
            assert isep[3, i] == -1
            continue
        assert p[FIRST, e].min() == isep[3, i]
        least = min(zip(d[e], p[MIN_ROW, e], p[PARTNER, e]))
        assert (np.float64(least[0]).tobytes(), least[1], least[2]) == (sep[i].tobytes(), isep[1, i], isep[0, i]), i


# ------------------------------------------------------------------------------------------------ 3: the transpose
@pytest.mark.parametrize("grouped", (False, True), ids=("one group", "two groups"))
def test_the_transpose_is_the_list_with_the_sides_swapped(grouped):
    from uav_ac.scoring import conflicts_against_rows, conflicts_transposed
    traffic, plan = missions()
    groups = dict(group_offsets=TGO, traffic_group_offsets=GO) if grouped else {}
    swapped = conflicts_against_rows(traffic[0], traffic[1], plan[0], plan[1], RADIUS, start_rows=traffic[2], traffic_start_rows=plan[2],
                                     **groups)
    cl = rule(grouped)
    assert cl[0][-1] > 0
    assert identical(conflicts_transposed(cl, 18), swapped)
    assert identical(conflicts_transposed(swapped, 30), cl)                           # ... and back


def test_the_transpose_takes_a_list_by_its_fields_and_refuses_a_broken_one():
    import collections
    from uav_ac.scoring import conflicts_transposed
    off, d, p = rule(False)
    Fields = collections.namedtuple("Fields", "offsets partner first_row last_row rows_inside min_row min_distance")
    assert identical(conflicts_transposed(Fields(off, *p, d), 18), conflicts_transposed((off, d, p), 18))
    empty = conflicts_transposed((np.zeros(4, dtype=np.int64), np.zeros(0), np.zeros((5, 0), dtype=np.int32)), 7)
    assert empty[0].tolist() == [0] * 8 and empty[1].shape == (0,) and empty[2].shape == (5, 0)
    short = off.copy()
    short[-1] -= 1
    for bad in ((short, d, p), (off, d[:-1], p), (off, d, p[:, :-1]), (off[::-1].copy(), d, p)):
        with pytest.raises(ValueError):                      # slices that do not sum to the entries
            conflicts_transposed(bad, 18)
    with pytest.raises(ValueError):                          # a partner the other side does not have
        conflicts_transposed((off, d, p), int(p[PARTNER].max()))


# ------------------------------------------------------------------------------------------------ 4: excluded and empty
def test_excluded_missions_and_groups_without_traffic():
    from uav_ac.scoring import conflicts_against_rows
    traffic, plan = missions()
    base = rule(True)
    n = np.diff(base[0])
    # an excluded plan mission (a position that is not finite; no rows at all) lists nothing, everybody else what they listed
    busy = int(n.argmax())
    assert n[busy] > 0
    prows = plan[0].copy()
    prows[plan[1][busy], 1] = np.nan
    got = conflicts_against_rows(prows, plan[1], traffic[0], traffic[1], RADIUS, GO, TGO, plan[2], traffic[2])
    assert got[0][busy] == got[0][busy + 1]
    assert all(entries(got, i) == entries(base, i) for i in range(30) if i != busy)
    others = [i for i in range(30) if i != busy]
    less = keep(plan, others)
    ro = np.insert(less[1], busy + 1, less[1][busy])                                  # the mission stays in the batch, without rows
    got = conflicts_against_rows(less[0], ro, traffic[0], traffic[1], RADIUS, GO, TGO, plan[2], traffic[2])
    assert got[0][busy] == got[0][busy + 1] and all(entries(got, i) == entries(base, i) for i in others)
    # an excluded traffic mission is listed by nobody; everybody else's entries are unchanged
    loud = int(np.bincount(base[2][PARTNER]).argmax())
    trows = traffic[0].copy()
    trows[traffic[1][loud]:traffic[1][loud + 1]] = np.nan
    got = conflicts_against_rows(plan[0], plan[1], trows, traffic[1], RADIUS, GO, TGO, plan[2], traffic[2])
    assert not (got[2][PARTNER] == loud).any() and (base[2][PARTNER] == loud).any()
    assert all(entries(got, i) == [e for e in entries(base, i) if e[0] != loud] for i in range(30))
    # ... and so they are, up to renumbering, when it is not in the batch at all (excluded traffic does not count for the horizon)
    which = np.array([j for j in range(18) if j != loud])
    t_less = keep(traffic, which)
    got2 = conflicts_against_rows(plan[0], plan[1], t_less[0], t_less[1], RADIUS, GO, offsets_after(TGO, which), plan[2], t_less[2])
    renumbered = got[2].copy()
    renumbered[PARTNER] -= renumbered[PARTNER] > loud
    assert identical(got2, (got[0], got[1], renumbered))
    # group 0 loses its traffic and lists nothing; group 1 is what it was, with the partners renumbered
    t1 = keep(traffic, np.arange(TGO[1], TGO[2]))
    got = conflicts_against_rows(plan[0], plan[1], t1[0], t1[1], RADIUS, GO, [0, 0, len(t1[2])], plan[2], t1[2])
    e0 = int(base[0][GO[1]])
    assert e0 > 0 and (got[0][:GO[1] + 1] == 0).all()
    shifted = base[2][:, e0:].copy()
    shifted[PARTNER] -= TGO[1]
    assert identical(got, (np.concatenate([np.zeros(GO[1], dtype=np.int64), base[0][GO[1]:] - e0]), base[1][e0:], shifted))
    # no traffic at all
    got = conflicts_against_rows(plan[0], plan[1], np.zeros((0, 3)), [0], RADIUS, GO, [0, 0, 0], plan[2], None)
    assert got[0].tolist() == [0] * 31 and got[1].shape == (0,) and got[2].shape == (5, 0) and got[2].dtype == np.int32
    for bad in (dict(group_offsets=GO), dict(traffic_group_offsets=TGO), dict(group_offsets=GO, traffic_group_offsets=[0, 18])):
        with pytest.raises(ValueError):
            conflicts_against_rows(plan[0], plan[1], traffic[0], traffic[1], RADIUS, **bad)


# ------------------------------------------------------------------------------------------------ 5: the ABI and the build
@pytest.mark.parametrize("name, plain, count", (("uavac_minsnap_conflict_against_offsets_dev", "uavac_minsnap_conflict_offsets_dev", 19),
                                                ("uavac_minsnap_conflicts_against_dev", "uavac_minsnap_conflicts_dev", 22)))
def test_entry_points_are_exported_and_declared_like_the_header(name, plain, count):
    from uav_ac import _native as nat
    assert name in nat.exported_symbols()
    fn = getattr(nat.lib(), name)
    restype, argtypes = nat._SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == count
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "uavac.h")).read(), flags=re.S)
    params = [" ".join(a.split()) for a in re.search(rf"int\s+{name}\s*\(([^)]*)\)\s*;", text).group(1).split(",")]
    kinds = [C.c_void_p if "*" in a else {"int": C.c_int, "double": C.c_double, "int64_t": C.c_int64}[a.split()[0]] for a in params]
    assert kinds == list(argtypes), params
    # the plan-side call, with the traffic's seven arguments put in behind G -- where the cross audit has them
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names[9:16] == ["t_coeffs", "t_seg_rows", "t_seg_offsets", "Bt", "mt", "t_group_offsets", "t_start_rows"]
    audit = [" ".join(a.split()).split()[-1].lstrip("*")
             for a in re.search(r"int\s+uavac_minsnap_separation_against_dev\s*\(([^)]*)\)\s*;", text).group(1).split(",")]
    assert names[:18] == audit[:18] and names[16:18] == ["start_rows", "radius"]
    assert names[18:] == ["pair_offsets", "capacity", "pair_d", "pair_i"][:count - 18]
    before = nat._SIGNATURES[plain][1]
    assert list(argtypes) == list(before[:9]) + [C.c_void_p] * 3 + [C.c_int] * 2 + [C.c_void_p] * 2 + list(before[9:])
    # a NULL context is refused before anything else is looked at (pure host code: no GPU needed)
    args = [None if t is C.c_void_p else (0.5 if t is C.c_double else 1) for t in argtypes]
    assert fn(*args) == nat.EINVAL


def test_the_build_budgets_the_new_object_file():
    from uav_ac import _buildcheck as bc
    rows = [r for r in bc.BUDGETS if r.obj == "minsnap_conflicts_against.o"]
    assert len(rows) == 1
    row = rows[0]
    assert row.kernels == ("conflict_against_prepass_kernel", "conflict_against_discover_kernel", "conflict_count_kernel",
                           "conflict_list_kernel", "conflict_against_measure_kernel")
    assert row.limit is bc.FROM_LDS and row.scratch_free and not row.extra and not row.at_least
    assert [r.key for r in bc.BUDGETS].count(row.key) == 1
    # the rows of the cross audit and of the plan-side list are what they were
    assert next(r for r in bc.BUDGETS if r.key == "separation_against_kernels").kernels == (
        "against_prepass_kernel", "separation_against_kernel", "against_merge_kernel")
    assert next(r for r in bc.BUDGETS if r.key == "conflict_kernels").kernels == (
        "conflict_prepass_kernel", "conflict_discover_kernel", "conflict_count_kernel", "conflict_list_kernel", "conflict_measure_kernel")
    counts = bc.check_cross_conflict_kernels()
    if counts is None:
        pytest.skip("no object files here (a library that was built elsewhere)")
    assert len(counts) == 5 and max(counts.values()) <= 168
    small = [v for k, v in counts.items() if "discover" not in k and "measure" not in k]
    assert len(small) == 3 and max(small) <= 64             # eight waves per SIMD without the tile
