"""Deconfliction against committed traffic that never moves, on the host: the three rules `separation_against_rows`,
`stagger_against_rows` and `layer_against_rows` of uav_ac/scoring.py -- the specification of `uavac_minsnap_separation_against_dev`,
`uavac_minsnap_stagger_against_dev` and `uavac_minsnap_layer_against_dev` --, the prototypes and the build's budgets for the three new
object files.  Nothing here needs a GPU.

Each rule is checked against an INDEPENDENT derivation from a rule that the GPU tests pin: the per-group interleaved concatenation
[traffic_g, plan_g] run through `conflicts_from_rows`, `stagger_from_rows` or `layer_obstacles_from_rows`.  Rows: the oracle's
(`oracle.minsnap_oracle.plan`) for `synthetic_missions(48, 3)` at 3 m/s and dt = 0.02; the first 18 are the traffic, the other 30 the
plan; radius 1.0, at which about half of the 48 are in somebody's way."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO

DT, VEL, RADIUS = 0.02, 3.0, 1.0
N_ALL, N_TRAFFIC = 48, 18
GO, TGO = np.array([0, 12, 30]), np.array([0, 10, 18])       # two groups on each side
CUBOIDS = np.array([[11.13, 12.37, 6.21, 7.43, -20.0, 20.0], [3.17, 21.29, 1.61, 15.83, -4.613, -4.087]])
DZ = 0.25

_MEMO = {}


def missions():
    """(the traffic's rows, row offsets, start rows; the plan's), computed once"""
    if "missions" not in _MEMO:
        from oracle import minsnap_oracle as mo
        parts = [mo.plan(w, VEL, DT, "solve")[:, :3] for w in mo.synthetic_missions(N_ALL, 3)]
        starts = (np.arange(N_ALL) % 5) * 7
        _MEMO["missions"] = (join(parts[:N_TRAFFIC]) + (starts[:N_TRAFFIC],), join(parts[N_TRAFFIC:]) + (starts[N_TRAFFIC:],))
    return _MEMO["missions"]


def join(parts):
    return np.concatenate(parts), np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)


def split(rows, ro):
    return [rows[ro[b]:ro[b + 1]] for b in range(len(ro) - 1)]


def interleave(traffic, plan, tgo, go):
    """The concatenation [traffic_g, plan_g] per group of two sides given as (rows, row offsets, start rows) -> (rows, row offsets,
    start rows, group offsets, where each traffic mission went, where each plan mission went)."""
    tparts, pparts = split(*traffic[:2]), split(*plan[:2])
    parts, starts, off, t_at, p_at = [], [], [0], np.zeros(len(tparts), dtype=int), np.zeros(len(pparts), dtype=int)
    for g in range(len(go) - 1):
        for j in range(tgo[g], tgo[g + 1]):
            t_at[j] = len(parts)
            parts.append(tparts[j]), starts.append(traffic[2][j])
        for i in range(go[g], go[g + 1]):
            p_at[i] = len(parts)
            parts.append(pparts[i]), starts.append(plan[2][i])
        off.append(len(parts))
    rows, ro = join(parts)
    return rows, ro, np.array(starts), np.array(off), t_at, p_at


def keep(side, which):
    """the missions `which` (indices) of a side"""
    parts = split(*side[:2])
    rows, ro = join([parts[b] for b in which])
    return rows, ro, np.asarray(side[2])[which]


def offsets_after(go, which):
    """group offsets of a side once only the missions `which` (ascending indices) are kept"""
    return np.array([int((np.asarray(which) < o).sum()) for o in go])


# ------------------------------------------------------------------------------------------------ 1: the cross audit
@pytest.mark.parametrize("grouped", (False, True))
def test_the_cross_audit_is_the_cross_pairs_of_the_conflict_list(grouped):
    from uav_ac.scoring import conflicts_from_rows, separation_against_rows
    traffic, plan = missions()
    go, tgo = (GO, TGO) if grouped else (np.array([0, 30]), np.array([0, 18]))
    rows, ro, st, off, t_at, p_at = interleave(traffic, plan, tgo, go)
    traffic_of = {int(c): j for j, c in enumerate(t_at)}
    groups = dict(group_offsets=go, traffic_group_offsets=tgo) if grouped else {}
    for radius in (1.0e3, RADIUS):                           # every pair listed; then the conflicting pairs alone
        sep, isep = separation_against_rows(plan[0], plan[1], traffic[0], traffic[1], radius, start_rows=plan[2], traffic_start_rows=traffic[2],
                                            **groups)
        offsets, pair_d, pair_i = conflicts_from_rows(rows, ro, radius, off, st)
        seen = 0
        for i, c in enumerate(p_at):
            cross = [(pair_d[e], int(pair_i[4, e]), traffic_of[int(pair_i[0, e])], int(pair_i[1, e]))
                     for e in range(offsets[c], offsets[c + 1]) if int(pair_i[0, e]) in traffic_of]
            assert isep[2, i] == len(cross), (radius, i)
            assert isep[3, i] == (min(e[3] for e in cross) if cross else -1), (radius, i)
            if cross:
                d, row, partner, _ = min(cross)
                assert (sep[i].tobytes(), isep[1, i], isep[0, i]) == (np.float64(d).tobytes(), row, partner), (radius, i)
                seen += 1
        g_of = np.searchsorted(go, np.arange(len(p_at)), side="right") - 1
        assert isep[4].tolist() == [int(tgo[g + 1] - tgo[g]) for g in g_of]
        if radius > RADIUS:
            assert seen == len(p_at) and (isep[2] == isep[4]).all() and (isep[3] == 0).all()
        else:
            assert 5 < seen < len(p_at), "the fixture's true radius separates nobody, or everybody"


def test_the_cross_audit_without_traffic_and_with_excluded_missions():
    from uav_ac.scoring import separation_against_rows
    traffic, plan = missions()
    base = separation_against_rows(plan[0], plan[1], traffic[0], traffic[1], RADIUS, GO, TGO, plan[2], traffic[2])
    # group 0 loses its traffic: +inf / -1 / -1 / 0 / -1 / 0; group 1 is what it was, with the partners renumbered
    t1 = keep(traffic, np.arange(TGO[1], TGO[2]))
    sep, isep = separation_against_rows(plan[0], plan[1], t1[0], t1[1], RADIUS, GO, [0, 0, len(t1[2])], plan[2], t1[2])
    assert np.isposinf(sep[:GO[1]]).all() and (isep[:, :GO[1]] == np.array([-1, -1, 0, -1, 0])[:, None]).all()
    assert sep[GO[1]:].tobytes() == base[0][GO[1]:].tobytes() and np.array_equal(isep[1:, GO[1]:], base[1][1:, GO[1]:])
    assert np.array_equal(isep[0, GO[1]:], base[1][0, GO[1]:] - TGO[1])
    # an excluded traffic mission is nobody's partner and is not counted; an excluded plan mission reports NaN
    trows, prows = traffic[0].copy(), plan[0].copy()
    loud = int(np.bincount(base[1][0][base[1][0] >= 0]).argmax())                    # the traffic mission that is most often the closest
    trows[traffic[1][loud]:traffic[1][loud + 1]] = np.nan
    prows[plan[1][3], 1] = np.inf
    sep, isep = separation_against_rows(prows, plan[1], trows, traffic[1], RADIUS, GO, TGO, plan[2], traffic[2])
    assert np.isnan(sep[3]) and isep[:, 3].tolist() == [-1, -1, 0, -1, 0] and not (isep[0] == loud).any()
    g_loud = 0 if loud < TGO[1] else 1
    want = base[1][4].copy()
    want[GO[g_loud]:GO[g_loud + 1]] -= 1
    want[3] = 0
    assert isep[4].tolist() == want.tolist()
    for bad in (dict(group_offsets=GO), dict(traffic_group_offsets=TGO), dict(group_offsets=GO, traffic_group_offsets=[0, 18])):
        with pytest.raises(ValueError):
            separation_against_rows(plan[0], plan[1], traffic[0], traffic[1], RADIUS, **bad)


# ------------------------------------------------------------------------------------------------ 2: stagger
def clear_traffic():
    """the traffic's missions that `stagger_from_rows` resolves, at their granted starts: pairwise clear -> (the side, its group offsets)"""
    if "clear" not in _MEMO:
        from uav_ac.scoring import stagger_from_rows
        traffic, _ = missions()
        istag = stagger_from_rows(traffic[0], traffic[1], RADIUS, TGO, traffic[2], 1, 100)
        ok = np.flatnonzero(istag[1] >= 0)
        assert (istag[1] > 0).any() and 10 < len(ok)
        side = keep(traffic, ok)
        _MEMO["clear"] = ((side[0], side[1], istag[0][ok]), offsets_after(TGO, ok))
    return _MEMO["clear"]


def test_stagger_against_clear_traffic_is_the_rule_on_the_concatenation():
    from uav_ac.scoring import stagger_against_rows, stagger_from_rows
    _, plan = missions()
    traffic, tgo = clear_traffic()
    rows, ro, st, off, t_at, p_at = interleave(traffic, plan, tgo, GO)
    whole = stagger_from_rows(rows, ro, RADIUS, off, st, 1, 100)
    assert (whole[1, t_at] == 0).all() and np.array_equal(whole[0, t_at], traffic[2])       # clear traffic stays where it is
    got = stagger_against_rows(plan[0], plan[1], traffic[0], traffic[1], RADIUS, GO, tgo, plan[2], traffic[2], 1, 100)
    assert np.array_equal(got, whole[:, p_at])
    alone = stagger_from_rows(plan[0], plan[1], RADIUS, GO, plan[2], 1, 100)
    assert (got[:2] != alone[:2]).any() and (got[1] > 0).any() and (got[1] == -1).any()
    assert got[2, 0] == tgo[1] and np.array_equal(got[2], alone[2] + np.repeat(np.diff(tgo), np.diff(GO)))      # earlier counts the traffic
    # the first mission of a group is examined when its group has traffic: against its own twin it cannot stay where it is
    twin = keep(plan, [0])
    first = stagger_against_rows(plan[0], plan[1], twin[0], twin[1], RADIUS, GO, [0, 1, 1], plan[2], twin[2], 1, 100)
    assert first[1, 0] != 0 and first[2, 0] == 1 and np.array_equal(first[:, GO[1]:], alone[:, GO[1]:])
    # one group on each side
    rows, ro, st, off, t_at, p_at = interleave(traffic, plan, [0, tgo[-1]], [0, GO[-1]])
    assert np.array_equal(stagger_against_rows(plan[0], plan[1], traffic[0], traffic[1], RADIUS, None, None, plan[2], traffic[2], 1, 100),
                          stagger_from_rows(rows, ro, RADIUS, None, st, 1, 100)[:, p_at])


def test_stagger_without_traffic_is_the_plain_rule():
    from uav_ac.scoring import stagger_against_rows, stagger_from_rows
    traffic, plan = missions()
    alone = stagger_from_rows(plan[0], plan[1], RADIUS, GO, plan[2], 2, 50)
    nobody = (np.zeros((0, 3)), np.array([0]))
    assert np.array_equal(stagger_against_rows(plan[0], plan[1], *nobody, RADIUS, GO, [0, 0, 0], plan[2], None, 2, 50), alone)
    assert np.array_equal(stagger_against_rows(plan[0], plan[1], *nobody, RADIUS, None, None, plan[2], None, 2, 50),
                          stagger_from_rows(plan[0], plan[1], RADIUS, None, plan[2], 2, 50))
    # group 0's traffic is all excluded: the group answers as the plain rule; group 1 has traffic and does not
    trows = traffic[0].copy()
    trows[:traffic[1][TGO[1]], 2] = np.nan
    got = stagger_against_rows(plan[0], plan[1], trows, traffic[1], RADIUS, GO, TGO, plan[2], traffic[2], 2, 50)
    assert np.array_equal(got[:, :GO[1]], alone[:, :GO[1]]) and (got[:, GO[1]:] != alone[:, GO[1]:]).any()
    # the group limit counts the plan's missions of a group
    capped = stagger_against_rows(plan[0], plan[1], traffic[0], traffic[1], RADIUS, GO, TGO, plan[2], traffic[2], 2, 50, max_group=12)
    assert (capped[1, GO[1]:] == -2).all() and (capped[2, GO[1]:] == 0).all() and (capped[1, :GO[1]] != -2).all()


# ------------------------------------------------------------------------------------------------ 3: layer
def lifted(rows):
    memo = {}

    def rows_at(q):
        if q not in memo:
            memo[q] = rows.copy()
            memo[q][:, 2] -= q * DZ
        return memo[q]
    return rows_at


@pytest.mark.parametrize("cuboids", (None, CUBOIDS), ids=("no cuboids", "cuboids"))
def test_layer_against_clear_traffic_is_the_rule_on_the_concatenation(cuboids):
    from uav_ac.scoring import layer_against_rows, layer_obstacles_from_rows
    raw, plan = missions()
    cub = np.zeros((0, 6)) if cuboids is None else cuboids
    first = layer_obstacles_from_rows(lifted(raw[0]), raw[1], RADIUS, cub, TGO, raw[2], 20)
    ok = np.flatnonzero(first[1] >= 0)
    assert (first[1] > 0).any() and len(ok) > 10
    parts = split(raw[0], raw[1])
    trows, tro = join([parts[b] - np.array([0.0, 0.0, first[0, b] * DZ]) for b in ok])       # the traffic on its granted layers
    traffic, tgo = (trows, tro, raw[2][ok]), offsets_after(TGO, ok)
    rows, ro, st, off, t_at, p_at = interleave(traffic, plan, tgo, GO)
    whole = layer_obstacles_from_rows(lifted(rows), ro, RADIUS, cub, off, st, 20)
    assert (whole[1, t_at] == 0).all()                       # clear traffic stays on its layer
    got = layer_against_rows(lifted(plan[0]), plan[1], traffic[0], traffic[1], RADIUS, cuboids, GO, tgo, plan[2], traffic[2], 20)
    assert np.array_equal(got, whole[:, p_at])
    alone = layer_obstacles_from_rows(lifted(plan[0]), plan[1], RADIUS, cub, GO, plan[2], 20)
    assert (got[:2] != alone[:2]).any() and (got[1] > 0).any()
    assert np.array_equal(got[2], alone[2] + np.repeat(np.diff(tgo), np.diff(GO)))
    assert (got[3] > 0).any() if cuboids is not None else not got[3].any()
    # without traffic, and with a group whose traffic is all excluded: the plain rule
    assert np.array_equal(layer_against_rows(lifted(plan[0]), plan[1], np.zeros((0, 3)), [0], RADIUS, cuboids, GO, [0, 0, 0], plan[2], None, 20),
                          alone)
    gone = traffic[0].copy()
    gone[:traffic[1][tgo[1]], 0] = np.nan
    half = layer_against_rows(lifted(plan[0]), plan[1], gone, traffic[1], RADIUS, cuboids, GO, tgo, plan[2], traffic[2], 20)
    assert np.array_equal(half[:, :GO[1]], alone[:, :GO[1]]) and np.array_equal(half[:, GO[1]:], got[:, GO[1]:])


# ------------------------------------------------------------------------------------------------ 4: traffic that conflicts with itself
def test_traffic_that_conflicts_with_itself_is_not_moved_and_the_answers_differ():
    """Its own fixture: of `synthetic_missions(64, 3)` the even missions are committed, the odd ones arrive, one group on each side.
    (Where a delayed committed mission changes a newcomer's answer depends on the geometry: with the module's 18 + 30 the re-run moves
    two committed missions and the 30 answers happen to stay; here it moves four and changes two.)"""
    from oracle import minsnap_oracle as mo
    from uav_ac.scoring import separation_against_rows, separation_from_rows, stagger_against_rows, stagger_from_rows
    parts = [mo.plan(w, VEL, DT, "solve")[:, :3] for w in mo.synthetic_missions(64, 3)]
    starts = (np.arange(64) % 5) * 7
    traffic, plan = (join(parts[0::2]) + (starts[0::2],), join(parts[1::2]) + (starts[1::2],))
    assert separation_from_rows(traffic[0], traffic[1], RADIUS, None, traffic[2])[1][2].sum() > 0      # the traffic is in its own way
    rows, ro, st, off, t_at, p_at = interleave(traffic, plan, [0, 32], [0, 32])
    whole = stagger_from_rows(rows, ro, RADIUS, off, st, 1, 100)
    assert (whole[1, t_at] > 0).any(), "the re-run of everybody moves no committed mission: the fixture shows nothing"
    got = stagger_against_rows(plan[0], plan[1], traffic[0], traffic[1], RADIUS, None, None, plan[2], traffic[2], 1, 100)
    assert (got[:2] != whole[:2, p_at]).any()                # the point of the feature: the committed missions stood still
    assert np.array_equal(got[2], whole[2, p_at])            # (both count the same missions before each newcomer)
    # and every resolved newcomer is clear of the traffic where the traffic IS
    _, isep = separation_against_rows(plan[0], plan[1], traffic[0], traffic[1], RADIUS, None, None, got[0], traffic[2])
    assert (isep[2][got[1] >= 0] == 0).all() and (got[1] >= 0).any()


# ------------------------------------------------------------------------------------------------ the ABI and the build
@pytest.mark.parametrize("name, wide, count", (("uavac_minsnap_separation_against_dev", "uavac_minsnap_separation_dev", 20),
                                               ("uavac_minsnap_stagger_against_dev", "uavac_minsnap_stagger_wide_dev", 22),
                                               ("uavac_minsnap_layer_against_dev", "uavac_minsnap_layer_wide_dev", 27)))
def test_entry_points_are_exported_and_declared_like_the_header(name, wide, count):
    from uav_ac import _native as nat
    assert name in nat.exported_symbols()
    fn = getattr(nat.lib(), name)
    restype, argtypes = nat._SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == count
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "uavac.h")).read(), flags=re.S)
    params = [" ".join(a.split()) for a in re.search(rf"int\s+{name}\s*\(([^)]*)\)\s*;", text).group(1).split(",")]
    kinds = [C.c_void_p if "*" in a else {"int": C.c_int, "double": C.c_double}[a.split()[0]] for a in params]
    assert kinds == list(argtypes), params
    # the call without traffic, with the traffic's seven arguments put in behind G
    assert [p.split()[-1].lstrip("*") for p in params[9:16]] == ["t_coeffs", "t_seg_rows", "t_seg_offsets", "Bt", "mt", "t_group_offsets", "t_start_rows"]
    plain = nat._SIGNATURES[wide][1]
    assert list(argtypes) == list(plain[:9]) + [C.c_void_p] * 3 + [C.c_int] * 2 + [C.c_void_p] * 2 + list(plain[9:])
    # a NULL context is refused before anything else is looked at (pure host code: no GPU needed)
    args = [None if t is C.c_void_p else (0.5 if t is C.c_double else 1) for t in argtypes]
    assert fn(*args) == nat.EINVAL


def test_the_build_budgets_the_three_new_object_files():
    from uav_ac import _buildcheck as bc
    rows = {r.key: r for r in bc.BUDGETS if r.key.endswith("_against_kernels")}
    assert {k: r.obj for k, r in rows.items()} == {"stagger_against_kernels": "minsnap_stagger_against.o",
                                                    "layer_against_kernels": "minsnap_layer_against.o",
                                                    "separation_against_kernels": "minsnap_separation_against.o"}
    assert all(r.limit is bc.FROM_LDS and r.scratch_free and not r.extra and not r.at_least for r in rows.values())
    for noun in ("stagger", "layer"):
        assert rows[f"{noun}_against_kernels"].kernels == (f"{noun}_prepass_kernel", "traffic_prepass_kernel", "traffic_carry_kernel",
                                                           f"against_{noun}_seed_kernel", f"wide_{noun}_seed_kernel", f"wide_{noun}_kernel")
    # the rows of the objects without traffic are what they were
    assert next(r for r in bc.BUDGETS if r.key == "stagger_wide_kernels").kernels == ("stagger_prepass_kernel", "wide_stagger_seed_kernel", "wide_stagger_kernel")
    assert next(r for r in bc.BUDGETS if r.key == "separation_kernels").kernels == ("separation_prepass_kernel", "minsnap_separation_kernel", "separation_merge_kernel")
    for check, n in ((bc.check_stagger_against_kernels, 6), (bc.check_layer_against_kernels, 6), (bc.check_separation_against_kernels, 3)):
        counts = check()
        if counts is None:
            pytest.skip("no object files here (a library that was built elsewhere)")
        assert len(counts) == n and max(counts.values()) <= 168
