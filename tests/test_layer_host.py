"""Offset layers that clear the separation audit, and the offset plan transform -- the part that needs no GPU: the entry points are
exported and declared as the header declares them, a NULL context is refused, the build keeps the kernels inside their budgets, and the
rules themselves -- `uav_ac.scoring.layer_from_rows` and `shift_coeffs`, the NumPy statements the kernels are tested against exactly
(tests/test_gpu_layer.py) -- give the answers that hand-made rows have by inspection; `scoring.layer_ok` on hand-made blocks.

The hand-made paths advance 0.125 m per row on a binary grid and the layer steps are binary fractions, so every d^2 below is exact."""
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


def layered(rows, delta):
    """rows_at for hand-made rows: every mission on layer q is the rows with q * delta added to the position (exact on the grid)."""
    asked = []

    def rows_at(q):
        asked.append(q)
        out = rows.copy()
        if q:
            out[:, 0:3] = out[:, 0:3] + q * np.asarray(delta, dtype=np.float64)
        return out
    rows_at.asked = asked
    return rows_at


def line(p0, p1, n=81):
    return np.linspace(np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64), n)


ALONG_X = line([0, 5, -3], [10, 5, -3])                      # both pass (5, 5, -3) at their own row 40
ALONG_Y = line([5, 0, -3], [5, 10, -3])
UP = (0.0, 0.0, -0.25)


def signature_from_header(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "uavac.h")).read(), flags=re.S)
    args = re.search(rf"int\s+{name}\s*\(([^)]*)\)\s*;", text).group(1)
    params = [" ".join(a.split()) for a in args.split(",")]
    return [C.c_void_p if "*" in a else {"int": C.c_int, "double": C.c_double, "int64_t": C.c_int64}[a.split()[0]] for a in params], text


def test_entry_points_are_exported_and_declared_like_the_header():
    from uav_ac import _native as nat
    assert (nat.LAYER_ROWS, nat.LAYER_MAX_STEPS, nat.LAYER_MAX_GROUP) == (3, 1023, 256)
    for name, n_args in (("uavac_minsnap_layer_dev", 17), ("uavac_minsnap_shift_dev", 8)):
        assert name in nat.exported_symbols()
        getattr(nat.lib(), name)
        restype, argtypes = nat._SIGNATURES[name]
        kinds, text = signature_from_header(name)
        assert restype is C.c_int and len(argtypes) == n_args and kinds == list(argtypes), (name, kinds)
    for name, value in (("ROWS", nat.LAYER_ROWS), ("MAX_STEPS", nat.LAYER_MAX_STEPS), ("MAX_GROUP", nat.LAYER_MAX_GROUP)):
        assert int(re.search(rf"#define\s+UAVAC_LAYER_{name}\s+(\d+)", text).group(1)) == value
    assert nat.lib().uavac_version() == nat.VERSION == 310
    # a NULL context is refused before anything else is looked at (pure host code: no GPU needed)
    assert nat.lib().uavac_minsnap_layer_dev(None, None, None, None, 1, 1, 0.01, None, 0, None, 0.5, 0.0, 0.0, -0.5, 63, None, None) == nat.EINVAL
    assert nat.lib().uavac_minsnap_shift_dev(None, None, None, 1, 1, 1, None, None) == nat.EINVAL
    from uav_ac.fleet import Engine, LayerResult
    assert callable(Engine.layer) and callable(Engine.shift)
    assert [f for f in LayerResult.__dataclass_fields__] == ["layers", "steps", "earlier", "block", "offsets"]


def test_the_build_keeps_the_layer_kernels_in_registers():
    from uav_ac import _buildcheck
    counts = _buildcheck.check_layer_kernels()
    if counts is None:
        pytest.skip("no object files here (a library that was built elsewhere)")
    assert len(counts) == 3 and max(counts.values()) <= 168
    for k in ("minsnap_layer_kernel", "layer_prepass_kernel", "minsnap_shift_kernel"):
        assert any(k in n for n in counts), k
    lds = {k.name: k.group_segment_fixed_size for k in _buildcheck.check_budgets("layer_kernels") if "minsnap_layer_kernel" in k.name}
    assert len(lds) == 1 and 3 * max(lds.values()) <= _buildcheck.LDS_BYTES_PER_CU          # three workgroups per CU


def test_two_missions_on_one_line_are_not_resolved_by_waiting_but_by_layers():
    from uav_ac.scoring import layer_from_rows, separation_from_rows, stagger_from_rows
    a = line([0, 0, -3], [10, 0, -3])
    b = line([10, 0, -3], [0, 0, -3])                        # head on, along the same line
    rows, ro = rows_of(a, b)
    assert stagger_from_rows(rows, ro, 0.5, max_steps=200)[1].tolist() == [0, -1]
    for dz, want in ((0.25, 2), (0.125, 4), (0.375, 2), (0.5, 1), (1.0, 1)):          # ceil(r / |dz|): at exactly r nobody is inside
        rows_at = layered(rows, (0.0, 0.0, -dz))
        il = layer_from_rows(rows_at, ro, 0.5)
        assert il.dtype == np.int32 and il.shape == (3, 2)
        assert il.tolist() == [[0, want], [0, want], [0, 1]], (dz, il)
        assert rows_at.asked[0] == 0 and max(rows_at.asked) == want                   # no layer past the granted one is asked for
        # the audit on the shifted rows confirms it, and one layer less does not do
        moved = rows.copy()
        moved[ro[1]:, 2] -= want * dz
        assert separation_from_rows(moved, ro, 0.5)[1][2].tolist() == [0, 0]
        moved[ro[1]:, 2] += dz
        assert separation_from_rows(moved, ro, 0.5)[1][2].tolist() == [1, 1]
    # the lowest index is never moved, whatever the order
    swapped = layer_from_rows(layered(rows_of(b, a)[0], UP), ro, 0.5)
    assert swapped.tolist() == [[0, 2], [0, 2], [0, 1]]
    # a copy of an earlier mission, a shared first waypoint: the same
    il = layer_from_rows(layered(rows_of(a, a)[0], UP), ro, 0.5)
    assert il[0].tolist() == [0, 2]
    fan = rows_of(a, line([0, 0, -3], [0, 10, -3]), line([0, 0, -3], [-10, 0, -3]))
    il = layer_from_rows(layered(fan[0], UP), fan[1], 0.5)
    assert il.tolist() == [[0, 2, 4], [0, 2, 4], [0, 1, 2]]
    # a lateral delta is the same code
    il = layer_from_rows(layered(rows, (0.0, 0.25, 0.0)), ro, 0.5)
    assert il[0].tolist() == [0, 2]
    # fixed starts take part: `b` five rows late still meets `a` on the line
    assert layer_from_rows(layered(rows, UP), ro, 0.5, start_rows=[0, 5])[0].tolist() == [0, 2]
    # radius 0 moves nobody: distance 0 is not < 0
    assert layer_from_rows(layered(rows, UP), ro, 0.0).tolist() == [[0, 0], [0, 0], [0, 1]]


def test_max_steps_bounds_the_search_and_an_unresolved_mission_stays_a_partner():
    from uav_ac.scoring import layer_from_rows
    a = line([0, 0, -3], [10, 0, -3])
    b = line([10, 0, -3], [0, 0, -3])
    # `c` crosses their line at x = 2.5 at its own row 40; with start 24 that is clock row 64: `b` passed there at row 60 (`a` at row 20),
    # the closest approach to `b` is d^2 = 0.125 at row 62
    c = line([2.5, -5, -3], [2.5, 5, -3])
    rows, ro = rows_of(a, b, c)
    up = (0.0, 0.0, -0.4375)
    il = layer_from_rows(layered(rows, up), ro, 0.5, start_rows=[0, 0, 24], max_steps=1)
    # b: 0.4375 < 0.5 on layer 1: unresolved, stays on layer 0.  c: inside b on layer 0 (0.125 < 0.25), clear on layer 1 (0.125 + 0.19140625)
    assert il.tolist() == [[0, 0, 1], [0, -1, 1], [0, 1, 2]]
    # without `b` nothing is in its way
    alone = layer_from_rows(layered(rows_of(a, c)[0], up), rows_of(a, c)[1], 0.5, start_rows=[0, 24], max_steps=1)
    assert alone.tolist() == [[0, 0], [0, 0], [0, 1]]
    # with one more layer `b` is resolved, and `c` then has to clear `b` where `b` stands NOW: on layer 2
    il = layer_from_rows(layered(rows, up), ro, 0.5, start_rows=[0, 0, 24], max_steps=2)
    assert il.tolist() == [[0, 2, 0], [0, 2, 0], [0, 1, 2]]
    # max_steps = 0 examines layer 0 only
    none = layer_from_rows(layered(rows, up), ro, 0.5, start_rows=[0, 0, 24], max_steps=0)
    assert none.tolist() == [[0, 0, 0], [0, -1, -1], [0, 1, 2]]
    for bad in (dict(max_steps=-1), dict(max_steps=1024)):
        with pytest.raises(ValueError):
            layer_from_rows(layered(rows, up), ro, 0.5, **bad)


def test_an_all_zero_delta_is_legal():
    from uav_ac.scoring import layer_from_rows
    rows, ro = rows_of(ALONG_X, ALONG_Y, ALONG_X + [0.0, 0.0, 2.0])
    il = layer_from_rows(layered(rows, (0.0, 0.0, 0.0)), ro, 0.5, max_steps=5)
    assert il.tolist() == [[0, 0, 0], [0, -1, 0], [0, 1, 2]]


def test_groups_excluded_missions_negative_starts_and_oversized_groups():
    from uav_ac import _native as nat
    from uav_ac.scoring import layer_from_rows
    rows, ro = rows_of(ALONG_X, ALONG_Y, ALONG_X, ALONG_Y)
    il = layer_from_rows(layered(rows, UP), ro, 0.5, group_offsets=[0, 1, 1, 3, 4])   # sizes 1, 0, 2, 1
    assert il.tolist() == [[0, 0, 2, 0], [0, 0, 2, 0], [0, 0, 1, 0]]
    one = layer_from_rows(layered(rows, UP), ro, 0.5)        # one airspace: the copies go two layers above what they copy
    assert one.tolist() == [[0, 2, 4, 6], [0, 2, 4, 6], [0, 1, 2, 3]]
    # an excluded mission is not examined, and the others' `earlier` is one lower
    broken = ALONG_X.copy()
    broken[:] = np.nan
    rows, ro = rows_of(ALONG_X, broken, ALONG_Y, np.zeros((0, 3)), ALONG_Y + [0.0, 0.0, 2.0])
    il = layer_from_rows(layered(rows, UP), ro, 0.5, start_rows=[0, 7, 0, 9, 0])
    assert il[:, 1].tolist() == [0, -2, 0] and il[:, 3].tolist() == [0, -2, 0]
    assert il[:, 0].tolist() == [0, 0, 0] and il[:, 2].tolist() == [2, 2, 1] and il[:, 4].tolist() == [0, 0, 2]
    # a negative start counts as 0
    rows, ro = rows_of(ALONG_X, ALONG_Y)
    assert layer_from_rows(layered(rows, UP), ro, 0.5, start_rows=[-7, -1]).tolist() == layer_from_rows(layered(rows, UP), ro, 0.5).tolist()
    # six rows late the crossing is clear (tests/test_stagger_host.py): fixed starts decide
    assert layer_from_rows(layered(rows, UP), ro, 0.5, start_rows=[0, 6])[1].tolist() == [0, 0]
    assert layer_from_rows(layered(rows, UP), ro, 0.5, start_rows=[0, 5])[1].tolist() == [0, 1]      # 0.203125 + 0.0625 >= 0.25
    # a group above the size limit is not examined at all; its neighbour is
    n = nat.LAYER_MAX_GROUP + 1
    parked = [[[float(b), 0.0, 0.0]] for b in range(n)]
    rows, ro = rows_of(*parked, ALONG_X, ALONG_Y)
    big = layer_from_rows(layered(rows, UP), ro, 0.5, group_offsets=[0, n, n + 2])
    assert (big[1, :n] == -2).all() and (big[2, :n] == 0).all() and (big[0, :n] == 0).all()
    assert big[:, n:].tolist() == [[0, 2], [0, 2], [0, 1]]
    within = layer_from_rows(layered(rows[:n - 1], UP), ro[:n], 0.5)
    assert (within[1] == 0).all() and within[2].tolist() == list(range(n - 1))


def test_invalid_arguments_raise():
    from uav_ac.scoring import layer_from_rows, layer_ok, shift_coeffs
    rows, ro = rows_of(ALONG_X, ALONG_Y, ALONG_X)
    for go in ([0, 2, 1, 3], [1, 3], [0, 2], [0]):
        with pytest.raises(ValueError):
            layer_from_rows(layered(rows, UP), ro, 0.5, group_offsets=go)
    for radius in (-1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            layer_from_rows(layered(rows, UP), ro, radius)
    with pytest.raises(ValueError):
        layer_from_rows(layered(rows, UP), ro, 0.5, start_rows=[0, 0])
    with pytest.raises(ValueError):
        layer_from_rows(rows, ro, 0.5)                       # rows instead of a callable
    with pytest.raises(ValueError):
        layer_ok(np.zeros((2, 5), dtype=np.int32))
    co = np.zeros((6, 8, 3))
    for bad in ((4, np.zeros((2, 3))), ([0, 2, 5], np.zeros((2, 3))), ([0, 4, 2, 6], np.zeros((3, 3))), ([1, 3, 6], np.zeros((2, 3))),
                (0, np.zeros((2, 3)))):
        with pytest.raises(ValueError):
            shift_coeffs(co, *bad)


def test_shift_coeffs_moves_c0_only_and_leaves_unmoved_missions_alone():
    from uav_ac.scoring import shift_coeffs
    rng = np.random.default_rng(7)
    B, m = 5, 3
    co = rng.standard_normal((B, 8 * m, 3))
    co[1, 0, :] = [-0.0, 0.0, -0.0]
    co[2, 8, 1] = -0.0
    off = rng.standard_normal((B, 3))
    off[1] = [0.0, -0.0, 0.0]                                # not moved: every bit stays, the zeros keep their signs
    off[2] = [0.0, 0.0, -0.5]                                # moved: the sum is formed on every axis, -0.0 + 0.0 = +0.0
    off[4] = [np.nan, np.inf, 1.0]                           # passes through
    before = co.copy()
    out = shift_coeffs(co, m, off)
    assert out.shape == co.shape and np.array_equal(co.view(np.uint64), before.view(np.uint64))      # the input is left alone
    o4, c4 = out.reshape(B, m, 8, 3), before.reshape(B, m, 8, 3)
    assert np.array_equal(o4[:, :, 1:].view(np.uint64), c4[:, :, 1:].view(np.uint64))                # c1 .. c7 keep every bit
    assert np.array_equal(o4[1].view(np.uint64), c4[1].view(np.uint64))
    for b in (0, 2, 3):
        assert np.array_equal(o4[b, :, 0], c4[b, :, 0] + off[b])
    assert not np.signbit(o4[2, 1, 0, 1]) and np.signbit(c4[2, 1, 0, 1])
    assert np.isnan(o4[4, :, 0, 0]).all() and np.isinf(o4[4, :, 0, 1]).all() and np.array_equal(o4[4, :, 0, 2], c4[4, :, 0, 2] + 1.0)
    # ragged: the same numbers through segment offsets, whatever the shape given
    so = np.array([0, 1, 3, 3, 6])
    flat = rng.standard_normal((6, 8, 3))
    off = rng.standard_normal((4, 3))
    got = shift_coeffs(flat, so, off)
    want = flat.copy()
    for b in range(4):
        want[so[b]:so[b + 1], 0] += off[b]
    assert np.array_equal(got, want) and np.array_equal(shift_coeffs(flat.reshape(6, 24), so, off).reshape(6, 8, 3), want)


def test_layer_ok_on_hand_made_blocks():
    from uav_ac.scoring import layer_ok
    block = np.array([[0, 6, 0, 0, 63], [0, 6, -1, -2, 63], [0, 1, 2, 0, 3]], dtype=np.int32)
    v = layer_ok(block)
    assert set(v) == {"resolved", "examined"}
    assert v["resolved"].tolist() == [True, True, False, False, True]
    assert v["examined"].tolist() == [True, True, True, False, True]
    w = layer_ok(SimpleNamespace(steps=block[1]))
    assert w["resolved"].tolist() == v["resolved"].tolist() and w["examined"].tolist() == v["examined"].tolist()
    assert not (v["resolved"] & ~v["examined"]).any()        # a mission that was not examined never looks resolved


def test_granted_layers_clear_the_audit_in_every_fully_resolved_group():
    """Property, on random straight legs through a small box (seeded): the audit of the rows on their granted layers finds nobody
    inside the radius in any group all of whose missions were resolved -- and the draw is such that layers were needed to get there."""
    from uav_ac.scoring import layer_from_rows, layer_ok, separation_from_rows
    rng = np.random.default_rng(20)
    B, size, radius = 40, 5, 0.75
    paths = []
    for b in range(B):
        p0, p1 = rng.uniform(0.0, 6.0, 3), rng.uniform(0.0, 6.0, 3)
        paths.append(line(p0, p1, int(rng.integers(30, 90))))
    rows, ro = rows_of(*paths)
    go = np.arange(0, B + 1, size)
    start = rng.integers(0, 25, B)
    delta = np.array([0.0, 0.0, -0.3])
    il = layer_from_rows(layered(rows, delta), ro, radius, go, start, max_steps=3)
    ok = layer_ok(il)
    assert ok["examined"].all() and (il[2] == np.arange(B) % size).all()
    assert (il[0] == np.maximum(il[1], 0)).all() and (il[1] > 0).any() and (il[1] == -1).any()
    moved = rows.copy()
    for b in range(B):
        if il[0, b]:
            moved[ro[b]:ro[b + 1], 0:3] = rows[ro[b]:ro[b + 1], 0:3] + il[0, b] * delta
    _, before = separation_from_rows(rows, ro, radius, go, start)
    _, after = separation_from_rows(moved, ro, radius, go, start)
    whole = [g for g in range(B // size) if ok["resolved"][go[g]:go[g + 1]].all()]
    assert len(whole) >= 3
    for g in whole:
        assert (after[2, go[g]:go[g + 1]] == 0).all() and (after[3, go[g]:go[g + 1]] == -1).all(), g
    assert any((il[1, go[g]:go[g + 1]] > 0).any() and (before[2, go[g]:go[g + 1]] > 0).any() for g in whole)
    # and between resolved missions of ANY group nobody is inside: audit the resolved ones alone
    keep = np.flatnonzero(ok["resolved"])
    sub_rows, sub_ro = rows_of(*[moved[ro[b]:ro[b + 1], 0:3] for b in keep])
    _, sub = separation_from_rows(sub_rows, sub_ro, radius, np.searchsorted(keep, go), start[keep])
    assert (sub[2] == 0).all()
