"""Start delays that clear the separation audit, the part that needs no GPU: the entry point is exported and declared as the header
declares it, a NULL context is refused, the build keeps the kernels inside their budgets, and the rule itself --
`uav_ac.scoring.stagger_from_rows`, the NumPy statement the kernel is tested against exactly (tests/test_gpu_stagger.py) -- gives the
answers that hand-made rows have by inspection; `scoring.stagger_ok` on hand-made blocks.

The hand-made paths advance 0.125 m per row on a binary grid, so every d^2 below is exact: two perpendicular paths that cross at the
same own row and are q rows apart on the clock come as close as d^2 = 0.0078125 q^2 (q even) or 0.0078125 (q^2 + 1) (q odd)."""
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


def line(p0, p1, n=81):
    return np.linspace(np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64), n)


ALONG_X = line([0, 5, -3], [10, 5, -3])                      # both pass (5, 5, -3) at their own row 40
ALONG_Y = line([5, 0, -3], [5, 10, -3])


def test_entry_point_is_exported_and_declared_like_the_header():
    from uav_ac import _native as nat
    assert (nat.STAGGER_ROWS, nat.STAGGER_MAX_STEPS, nat.STAGGER_MAX_GROUP) == (3, 1023, 256)
    assert "uavac_minsnap_stagger_dev" in nat.exported_symbols()
    fn = nat.lib().uavac_minsnap_stagger_dev
    restype, argtypes = nat._SIGNATURES["uavac_minsnap_stagger_dev"]
    assert restype is C.c_int and len(argtypes) == 14
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "uavac.h")).read(), flags=re.S)
    args = re.search(r"int\s+uavac_minsnap_stagger_dev\s*\(([^)]*)\)\s*;", text).group(1)
    params = [" ".join(a.split()) for a in args.split(",")]
    assert len(params) == 14
    kinds = [C.c_void_p if "*" in a else {"int": C.c_int, "double": C.c_double}[a.split()[0]] for a in params]
    assert kinds == list(argtypes), params
    for name, value in (("ROWS", nat.STAGGER_ROWS), ("MAX_STEPS", nat.STAGGER_MAX_STEPS), ("MAX_GROUP", nat.STAGGER_MAX_GROUP)):
        assert int(re.search(rf"#define\s+UAVAC_STAGGER_{name}\s+(\d+)", text).group(1)) == value
    # a NULL context is refused before anything else is looked at (pure host code: no GPU needed)
    assert fn(None, None, None, None, 1, 1, 0.01, None, 0, None, 0.5, 1, 255, None) == nat.EINVAL


def test_the_build_keeps_the_stagger_kernels_in_registers():
    from uav_ac import _buildcheck
    counts = _buildcheck.check_stagger_kernels()
    if counts is None:
        pytest.skip("no object files here (a library that was built elsewhere)")
    assert len(counts) == 2 and max(counts.values()) <= 168
    assert any("minsnap_stagger_kernel" in k for k in counts) and any("stagger_prepass_kernel" in k for k in counts)


def test_groups_as_the_fleet_calls_take_them():
    """`Engine._groups`, behind separation, stagger, layer and flown_separation: None, a group size, offsets; the refusals and their words."""
    import torch
    from uav_ac.engine import Engine
    eng = object.__new__(Engine)                             # (no context: the helper needs the device and torch only)
    eng._torch, eng.device = torch, torch.device("cpu")
    assert eng._groups(None, 10) == (None, 0) and eng._groups(None, 256, 256) == (None, 0)
    for groups, want in ((4, [0, 4, 8, 10]), (np.int64(5), [0, 5, 10]), (16, [0, 10]), ([0, 3, 10], [0, 3, 10]),
                         (np.array([0, 10]), [0, 10]), (torch.tensor([0, 1, 10], dtype=torch.int32), [0, 1, 10])):
        for limit in (None, 10):
            go, G = eng._groups(groups, 10, limit)
            assert go.dtype == torch.int64 and go.tolist() == want and G == len(want) - 1
    for call, words in ((lambda: eng._groups(0, 10), "a group size must be >= 1"),
                        (lambda: eng._groups(-3, 10, 256), "a group size must be >= 1"),
                        (lambda: eng._groups([0], 10), "group offsets hold at least two entries"),
                        (lambda: eng._groups(None, 257, 256), "one group of 257 missions; at most 256 per group"),
                        (lambda: eng._groups(300, 600, 256), "a group of 300 missions; at most 256 per group"),
                        (lambda: eng._groups(torch.tensor([0, 1, 300]), 300, 256), "a group of 299 missions; at most 256 per group")):
        with pytest.raises(ValueError) as err:
            call()
        assert str(err.value) == words
    assert eng._groups([0, 300], 300)[1] == 1                # (no limit: the separation audits take a group of any size)


def test_two_crossing_paths_the_second_gets_the_smallest_clearing_delay():
    from uav_ac.scoring import separation_from_rows, stagger_from_rows
    rows, ro = rows_of(ALONG_X, ALONG_Y)
    # r^2 = 0.25: q = 5 gives 0.0078125 * 26 = 0.203 (inside), q = 6 gives 0.0078125 * 36 = 0.281 (clear)
    istag = stagger_from_rows(rows, ro, 0.5)
    assert istag.dtype == np.int32 and istag.shape == (3, 2)
    assert istag[0].tolist() == [0, 6] and istag[1].tolist() == [0, 6] and istag[2].tolist() == [0, 1]
    _, before = separation_from_rows(rows, ro, 0.5)
    _, after = separation_from_rows(rows, ro, 0.5, start_rows=istag[0])
    assert before[2].tolist() == [1, 1] and after[2].tolist() == [0, 0]
    _, one_less = separation_from_rows(rows, ro, 0.5, start_rows=[0, 5])
    assert one_less[2].tolist() == [1, 1]                    # the delay is the smallest one
    # the priority is the batch index: the other order delays the other mission
    swapped = stagger_from_rows(*rows_of(ALONG_Y, ALONG_X), 0.5)
    assert swapped[0].tolist() == [0, 6] and swapped[1].tolist() == [0, 6]
    # base starts shift the answer: the second mission is already five rows late, one more is enough ... and six late needs nothing
    assert stagger_from_rows(rows, ro, 0.5, start_rows=[0, 5])[:2].tolist() == [[0, 6], [0, 1]]
    assert stagger_from_rows(rows, ro, 0.5, start_rows=[0, 6])[:2].tolist() == [[0, 6], [0, 0]]
    assert stagger_from_rows(rows, ro, 0.5, start_rows=[3, 0])[:2].tolist() == [[3, 9], [0, 9]]
    # radius 0 delays nobody: distance 0 is not < 0
    zero = stagger_from_rows(rows, ro, 0.0)
    assert zero[0].tolist() == [0, 0] and zero[1].tolist() == [0, 0] and zero[2].tolist() == [0, 1]


def test_step_grants_multiples_only_and_max_steps_bounds_the_search():
    from uav_ac.scoring import stagger_from_rows
    rows, ro = rows_of(ALONG_X, ALONG_Y)
    by4 = stagger_from_rows(rows, ro, 0.5, step=4)           # candidates 0, 4 (0.125: inside), 8 (0.5: clear)
    assert by4[0].tolist() == [0, 8] and by4[1].tolist() == [0, 2]
    by5 = stagger_from_rows(rows, ro, 0.5, start_rows=[0, 1], step=5)                  # 1 + 5 q: 1, 6
    assert by5[0].tolist() == [0, 6] and by5[1].tolist() == [0, 1]
    # max_steps = 0 grants nothing: only q = 0 is examined
    none = stagger_from_rows(rows, ro, 0.5, max_steps=0)
    assert none[0].tolist() == [0, 0] and none[1].tolist() == [0, -1] and none[2].tolist() == [0, 1]
    short = stagger_from_rows(rows, ro, 0.5, max_steps=5)
    assert short[0].tolist() == [0, 0] and short[1].tolist() == [0, -1]
    exact = stagger_from_rows(rows, ro, 0.5, max_steps=6)
    assert exact[0].tolist() == [0, 6] and exact[1].tolist() == [0, 6]
    # an unresolved mission keeps its BASE start
    kept = stagger_from_rows(rows, ro, 0.5, start_rows=[0, 2], max_steps=2)
    assert kept[0].tolist() == [0, 2] and kept[1].tolist() == [0, -1]
    for bad in (dict(step=0), dict(max_steps=-1), dict(max_steps=1024), dict(step=2 ** 20, max_steps=1023)):
        with pytest.raises(ValueError):
            stagger_from_rows(rows, ro, 0.5, **bad)


def test_a_head_on_pair_is_unresolved_and_still_blocks_a_third_mission():
    from uav_ac.scoring import stagger_from_rows
    a = line([0, 0, -3], [10, 0, -3])
    b = line([10, 0, -3], [0, 0, -3])                        # starts where `a` ends and flies towards it: waiting does not help
    # `c` crosses their line at x = 2.5 at its own row 40; with base start 20 that is clock row 60, when `b` is there (`a` was at row 20)
    c = line([2.5, -5, -3], [2.5, 5, -3])
    rows, ro = rows_of(a, b, c)
    istag = stagger_from_rows(rows, ro, 0.5, start_rows=[0, 0, 20])
    assert istag[0].tolist() == [0, 0, 26] and istag[1].tolist() == [0, -1, 6] and istag[2].tolist() == [0, 1, 2]
    # without `b` nothing is in its way
    alone = stagger_from_rows(*rows_of(a, c), 0.5, start_rows=[0, 20])
    assert alone[0].tolist() == [0, 20] and alone[1].tolist() == [0, 0]


def test_a_shared_first_waypoint_cannot_be_resolved_by_waiting():
    from uav_ac.scoring import stagger_from_rows
    a, b = line([0, 0, -3], [10, 0, -3]), line([0, 0, -3], [0, 10, -3])
    istag = stagger_from_rows(*rows_of(a, b), 0.5, max_steps=40)
    assert istag[0].tolist() == [0, 0] and istag[1].tolist() == [0, -1]
    # ... nor a shared last one
    a, b = line([0, 0, -3], [10, 0, -3]), line([10, 10, -3], [10, 0, -3])
    assert stagger_from_rows(*rows_of(a, b), 0.5, max_steps=40)[1].tolist() == [0, -1]


def test_groups_of_one_empty_groups_an_excluded_mission_and_a_negative_start():
    from uav_ac.scoring import stagger_from_rows
    rows, ro = rows_of(ALONG_X, ALONG_Y, ALONG_X, ALONG_Y)
    istag = stagger_from_rows(rows, ro, 0.5, group_offsets=[0, 1, 1, 3, 4])           # sizes 1, 0, 2, 1
    assert istag.tolist() == [[0, 0, 6, 0], [0, 0, 6, 0], [0, 0, 1, 0]]
    one = stagger_from_rows(rows, ro, 0.5)                   # one airspace: the copies of an earlier path can never be cleared
    assert one[1].tolist() == [0, 6, -1, -1] and one[0].tolist() == [0, 6, 0, 0] and one[2].tolist() == [0, 1, 2, 3]
    # an excluded mission is not examined, and the others' `earlier` is one lower
    broken = ALONG_X.copy()
    broken[:] = np.nan
    rows, ro = rows_of(ALONG_X, broken, ALONG_Y, np.zeros((0, 3)), ALONG_Y + [0.0, 0.0, 2.0])
    istag = stagger_from_rows(rows, ro, 0.5, start_rows=[0, 7, 0, 9, 0])
    assert istag[:, 1].tolist() == [7, -2, 0] and istag[:, 3].tolist() == [9, -2, 0]
    assert istag[:, 0].tolist() == [0, 0, 0] and istag[:, 2].tolist() == [6, 6, 1] and istag[:, 4].tolist() == [0, 0, 2]
    # a negative base start counts as 0
    rows, ro = rows_of(ALONG_X, ALONG_Y)
    assert stagger_from_rows(rows, ro, 0.5, start_rows=[-7, -1]).tolist() == stagger_from_rows(rows, ro, 0.5).tolist()
    assert stagger_from_rows(rows, ro, 0.5, start_rows=[-7, 2]).tolist() == [[0, 6], [0, 4], [0, 1]]
    # a group above the size limit is not examined at all; its neighbour is
    from uav_ac import _native as nat
    n = nat.STAGGER_MAX_GROUP + 1
    parked = [[[float(b), 0.0, 0.0]] for b in range(n)]
    rows, ro = rows_of(*parked, ALONG_X, ALONG_Y)
    big = stagger_from_rows(rows, ro, 0.5, group_offsets=[0, n, n + 2], start_rows=np.arange(n + 2))
    assert (big[1, :n] == -2).all() and (big[2, :n] == 0).all() and big[0, :n].tolist() == list(range(n))
    assert big[:, n:].tolist() == [[n, n + 6], [0, 5], [0, 1]]
    within = stagger_from_rows(rows[:n - 1], ro[:n], 0.5)
    assert (within[1] == 0).all() and within[2].tolist() == list(range(n - 1))


def test_malformed_offsets_and_a_bad_radius_raise():
    from uav_ac.scoring import stagger_from_rows
    rows, ro = rows_of(ALONG_X, ALONG_Y, ALONG_X)
    for go in ([0, 2, 1, 3], [1, 3], [0, 2], [0]):
        with pytest.raises(ValueError):
            stagger_from_rows(rows, ro, 0.5, group_offsets=go)
    for radius in (-1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            stagger_from_rows(rows, ro, radius)
    with pytest.raises(ValueError):
        stagger_from_rows(rows, ro, 0.5, start_rows=[0, 0])


def test_stagger_ok_on_hand_made_blocks():
    from uav_ac.scoring import stagger_ok
    block = np.array([[0, 6, 3, 9, 0], [0, 6, -1, -2, 255], [0, 1, 2, 0, 3]], dtype=np.int32)
    v = stagger_ok(block)
    assert set(v) == {"resolved", "examined"}
    assert v["resolved"].tolist() == [True, True, False, False, True]
    assert v["examined"].tolist() == [True, True, True, False, True]
    w = stagger_ok(SimpleNamespace(steps=block[1]))
    assert w["resolved"].tolist() == v["resolved"].tolist() and w["examined"].tolist() == v["examined"].tolist()
    assert not (v["resolved"] & ~v["examined"]).any()        # a mission that was not examined never looks resolved
    with pytest.raises(ValueError):
        stagger_ok(np.zeros((2, 5), dtype=np.int32))


def test_granted_starts_clear_the_audit_in_every_fully_resolved_group():
    """Property, on random straight legs through a small box (seeded): the audit with the granted starts finds nobody inside the
    radius in any group all of whose missions were resolved -- and the draw is such that delays were needed to get there."""
    from uav_ac.scoring import separation_from_rows, stagger_from_rows, stagger_ok
    rng = np.random.default_rng(20)
    B, size, radius = 40, 5, 0.75
    paths = []
    for b in range(B):
        p0, p1 = rng.uniform(0.0, 6.0, 3), rng.uniform(0.0, 6.0, 3)
        paths.append(line(p0, p1, int(rng.integers(30, 90))))
    rows, ro = rows_of(*paths)
    go = np.arange(0, B + 1, size)
    base = rng.integers(0, 25, B)
    istag = stagger_from_rows(rows, ro, radius, go, base, step=2, max_steps=100)
    ok = stagger_ok(istag)
    assert ok["examined"].all() and (istag[2] == np.arange(B) % size).all()
    assert ((istag[0] - base)[ok["resolved"]] == 2 * istag[1][ok["resolved"]]).all() and (istag[0] == base)[~ok["resolved"]].all()
    _, before = separation_from_rows(rows, ro, radius, go, base)
    _, after = separation_from_rows(rows, ro, radius, go, istag[0])
    whole = [g for g in range(B // size) if ok["resolved"][go[g]:go[g + 1]].all()]
    assert len(whole) >= 3
    for g in whole:
        assert (after[2, go[g]:go[g + 1]] == 0).all() and (after[3, go[g]:go[g + 1]] == -1).all(), g
    assert any((istag[1, go[g]:go[g + 1]] > 0).any() and (before[2, go[g]:go[g + 1]] > 0).any() for g in whole)
    # and between resolved missions of ANY group nobody is inside: audit the resolved ones alone
    keep = np.flatnonzero(ok["resolved"])
    sub_rows, sub_ro = rows_of(*[paths[b] for b in keep])
    sub_go = np.searchsorted(keep, go)
    _, sub = separation_from_rows(sub_rows, sub_ro, radius, sub_go, istag[0, keep])
    assert (sub[2] == 0).all()
