"""Offset layers that keep out of cuboids -- the part that needs no GPU: the entry point is exported and declared as the header declares
it, a NULL context is refused, the build keeps the new kernels inside their budgets, and the rule itself --
`uav_ac.scoring.layer_obstacles_from_rows`, the NumPy statement the kernel is tested against exactly
(tests/test_gpu_layer_obstacles.py) -- gives `layer_from_rows` when there are no cuboids and, on three hand-made straight missions, the
answers that can be read off by eye; `scoring.blocked_out` and `layer_ok` on its blocks.

The hand-made paths advance 0.125 m per row on a binary grid and the layer steps are binary fractions, so every position below is
exact and a face can be put exactly on a sample."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import REPO

UP = (0.0, 0.0, -0.25)
# the cuboids of tests/test_gpu_layer_obstacles.py: the faces lie off the grid of the waypoints
CUBOIDS = np.array([[11.13, 12.37, 6.21, 7.43, -20.0, 20.0], [3.17, 21.29, 1.61, 15.83, -4.613, -4.087],
                    [22.31, 25.87, 11.19, 14.57, -9.011, -2.203], [1.09, 4.91, -1.27, 2.33, -5.897, -3.511]])


def rows_of(*paths):
    """Missions given as (N_b, 3) position lists -> (rows (N, 11), row_offsets (B + 1,)): the sampler's layout, positions in 0-2."""
    ro = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    rows = np.zeros((int(ro[-1]), 11))
    for b, p in enumerate(paths):
        rows[ro[b]:ro[b + 1], 0:3] = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    return rows, ro


def layered(rows, delta):
    """rows_at for given rows: every mission on layer q is the rows with q * delta added to the position; memoised."""
    memo = {}

    def rows_at(q):
        if q not in memo:
            memo[q] = rows[:, 0:3] + q * np.asarray(delta, dtype=np.float64) if q else rows[:, 0:3]
        return memo[q]
    return rows_at


def line(p0, p1, n=81):
    return np.linspace(np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64), n)


def signature_from_header(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "uavac.h")).read(), flags=re.S)
    args = re.search(rf"int\s+{name}\s*\(([^)]*)\)\s*;", text).group(1)
    params = [" ".join(a.split()) for a in args.split(",")]
    return [C.c_void_p if "*" in a else {"int": C.c_int, "double": C.c_double, "int64_t": C.c_int64}[a.split()[0]] for a in params], text


def test_the_entry_point_is_exported_and_declared_like_the_header():
    from uav_ac import _native as nat
    from uav_ac import scoring
    name = "uavac_minsnap_layer_obs_dev"
    assert name in nat.exported_symbols()
    getattr(nat.lib(), name)
    restype, argtypes = nat._SIGNATURES[name]
    kinds, text = signature_from_header(name)
    assert restype is C.c_int and len(argtypes) == 19 and kinds == list(argtypes), kinds
    # uavac_minsnap_layer_dev's arguments, with cuboids and n_cuboids between max_steps and the outputs
    plain = nat._SIGNATURES["uavac_minsnap_layer_dev"][1]
    assert list(argtypes) == list(plain[:15]) + [C.c_void_p, C.c_int] + list(plain[15:])
    assert int(re.search(r"#define\s+UAVAC_LAYER_OBS_ROWS\s+(\d+)", text).group(1)) == nat.LAYER_OBS_ROWS == 4
    assert scoring.LAYER_BLOCKED == 3 and (scoring.LAYER_LAYER, scoring.LAYER_STEPS, scoring.LAYER_EARLIER) == (0, 1, 2)
    # a NULL context is refused before anything else is looked at (pure host code: no GPU needed)
    assert nat.lib().uavac_minsnap_layer_obs_dev(None, None, None, None, 1, 1, 0.01, None, 0, None, 0.5, 0.0, 0.0, -0.5, 63, None, 0, None,
                                                 None) == nat.EINVAL
    from uav_ac.fleet import DeconflictResult, Engine, LayerResult
    assert callable(Engine.deconflict) and "obstacles" in Engine.layer.__code__.co_varnames
    assert [f for f in DeconflictResult.__dataclass_fields__] == ["plan", "stagger", "layer", "resolved"]
    # `blocked` is read from the block: None without obstacles, row 3 with them
    three, four = np.zeros((3, 5), dtype=np.int32), np.arange(20, dtype=np.int32).reshape(4, 5)
    assert LayerResult(*three, three, None).blocked is None and LayerResult(*four[:3], four, None).blocked.tolist() == four[3].tolist()


def test_the_build_keeps_the_new_kernels_in_their_budget_and_the_old_ones_where_they_were():
    from uav_ac import _buildcheck
    counts = _buildcheck.check_layer_obs_kernels()
    if counts is not None:                                   # (None: no object files here, a library that was built elsewhere)
        assert len(counts) == 2 and max(counts.values()) <= 168
        lds, old = ({k.name: k.group_segment_fixed_size for k in _buildcheck.check_budgets(key) if "minsnap_layer_kernel" in k.name}
                    for key in ("layer_obs_kernels", "layer_kernels"))
        assert len(lds) == 1 and 3 * max(lds.values()) <= _buildcheck.LDS_BYTES_PER_CU      # three workgroups per CU
        assert max(lds.values()) - max(old.values()) == 16 * 6 * 8 + 16                    # the cuboids and two words
        assert len(_buildcheck.check_layer_kernels()) == 3


def test_without_cuboids_the_rule_is_layer_from_rows():
    from oracle import c_oracle as cc
    from oracle import minsnap_oracle as mo
    from uav_ac.scoring import layer_from_rows, layer_obstacles_from_rows
    ref = cc.plan_threads(mo.synthetic_missions(96, 8), 3.0, 0.01)
    rows, ro = ref["rows"], ref["row_offsets"]
    rows_at = layered(rows, UP)
    go = np.arange(0, 97, 32)
    st = (np.arange(96) % 5) * 37
    for kw in (dict(group_offsets=go, max_steps=15), dict(group_offsets=go, start_rows=st, max_steps=3)):
        want = layer_from_rows(rows_at, ro, 0.5, **kw)
        for none in (np.zeros((0, 6)), [], None):
            got = layer_obstacles_from_rows(rows_at, ro, 0.5, none if none is not None else np.empty((0, 6)), **kw)
            assert got.dtype == np.int32 and got.shape == (4, 96)
            assert np.array_equal(got[:3], want) and (got[3] == 0).all()
        assert (want[1] > 0).any()
    # cuboids that contain nothing are no cuboids: a NaN bound, an inverted box
    nothing = np.array([[np.nan, 30.0, -30.0, 30.0, -30.0, 30.0], [30.0, -30.0, -30.0, 30.0, -30.0, 30.0]])
    got = layer_obstacles_from_rows(rows_at, ro, 0.5, nothing, group_offsets=go, max_steps=15)
    assert np.array_equal(got[:3], layer_from_rows(rows_at, ro, 0.5, group_offsets=go, max_steps=15)) and (got[3] == 0).all()
    # with the cuboids of the GPU test the rule moves the first of a group, blocks, and leaves missions unresolved
    got = layer_obstacles_from_rows(rows_at, ro, 0.5, CUBOIDS, group_offsets=go, max_steps=15)
    plain = layer_from_rows(rows_at, ro, 0.5, group_offsets=go, max_steps=15)
    print("blocked > 0:", int((got[3] > 0).sum()), "unresolved:", int((got[1] == -1).sum()), "first of group:", got[0, go[:-1]].tolist(),
          "differ:", int((got[0] != plain[0]).sum()))
    assert int((got[3] > 0).sum()) == 55 and int((got[1] == -1).sum()) == 16 and got[0, go[:-1]].tolist() == [8, 7, 7]
    assert int((got[0] != plain[0]).sum()) == 48 and (got[2] == plain[2]).all()


A = line([0, 0, -3], [10, 0, -3])                            # A and B head on along one line, both through the slab
B_ = line([10, 0, -3], [0, 0, -3])
C_ = line([20, -5, -3], [20, 5, -3])                         # far from both, through the pillar
SLAB = [4.0, 6.0, -1.0, 1.0, -3.55, -2.9]                    # contains the layers 0, 1, 2 of A and B (z = -3, -3.25, -3.5), not layer 3
PILLAR = [19.0, 21.0, -1.0, 1.0, -100.0, 100.0]              # contains every layer of C


def test_three_straight_missions_a_slab_and_a_pillar():
    from uav_ac.scoring import blocked_out, layer_from_rows, layer_obstacles_from_rows, layer_ok
    rows, ro = rows_of(A, B_, C_)
    rows_at = layered(rows, UP)
    # no cuboids: A stays, B goes two layers up (ceil(r / |dz|)), C stays
    assert layer_obstacles_from_rows(rows_at, ro, 0.5, [], max_steps=7).tolist() == [[0, 2, 0], [0, 2, 0], [0, 1, 2], [0, 0, 0]]
    il = layer_obstacles_from_rows(rows_at, ro, 0.5, [SLAB, PILLAR], max_steps=7)
    assert il.dtype == np.int32 and il.shape == (4, 3)
    # A: the first of its group, nobody to clear -- moved by the slab alone: layers 0-2 blocked, layer 3, earlier 0
    assert il[:, 0].tolist() == [3, 3, 0, 3]
    # B: layers 0-2 blocked (its layer 2 is ALSO 0.25 m from A on layer 3: blocked and in conflict counts as blocked), layers 3 and 4
    # inside A's radius (0 and 0.25 m), layer 5 at exactly 0.5 m: clear
    assert il[:, 1].tolist() == [5, 5, 1, 3]
    # C: every layer 0 .. 7 inside the pillar: unresolved, layer 0, blocked = max_steps + 1
    assert il[:, 2].tolist() == [0, -1, 2, 8]
    assert blocked_out(il, 7).tolist() == [False, False, True]
    ok = layer_ok(il)
    assert ok["resolved"].tolist() == [True, True, False] and ok["examined"].all()
    as_result = SimpleNamespace(steps=il[1], blocked=il[3])
    assert blocked_out(as_result, 7).tolist() == [False, False, True] and layer_ok(as_result)["resolved"].tolist() == [True, True, False]
    # the granted layers are outside every cuboid, and nobody resolved is inside anybody's radius
    for b in (0, 1):
        p = rows_at(int(il[0, b]))[ro[b]:ro[b + 1]]
        for x in (SLAB, PILLAR):
            assert not ((p[:, 0] >= x[0]) & (p[:, 0] <= x[1]) & (p[:, 1] >= x[2]) & (p[:, 1] <= x[3]) & (p[:, 2] >= x[4]) & (p[:, 2] <= x[5])).any()
    # the faces are inclusive: a slab that ENDS on layer 2 (z = -3.5 exactly) still blocks it, one a hair lower does not
    on_face = layer_obstacles_from_rows(rows_at, ro, 0.5, [[4.0, 6.0, -1.0, 1.0, -3.5, -2.9]], max_steps=7)
    assert on_face[:, 0].tolist() == [3, 3, 0, 3]
    below = layer_obstacles_from_rows(rows_at, ro, 0.5, [[4.0, 6.0, -1.0, 1.0, -3.4999, -2.9]], max_steps=7)
    assert below[:, 0].tolist() == [2, 2, 0, 2] and below[:, 1].tolist() == [4, 4, 1, 2]
    # too crowded is not blocked out: with max_steps = 4 B finds nothing (0-2 blocked, 3 and 4 in conflict), blocked stays 3
    few = layer_obstacles_from_rows(rows_at, ro, 0.5, [SLAB, PILLAR], max_steps=4)
    assert few[:, 1].tolist() == [0, -1, 1, 3] and few[:, 2].tolist() == [0, -1, 2, 5]
    assert blocked_out(few, 4).tolist() == [False, False, True]
    # groups: B and C in a group of their own -- B is then the first of its group and is moved by the slab alone
    il = layer_obstacles_from_rows(rows_at, ro, 0.5, [SLAB, PILLAR], group_offsets=[0, 1, 3], max_steps=7)
    assert il.tolist() == [[3, 3, 0], [3, 3, -1], [0, 0, 1], [3, 3, 8]]
    # fixed starts do not change what a cuboid blocks (a mission's rows cover its whole clock); the pair search sees them as before:
    # A has long landed at (10, 0) on layer 3 when B, which waits there, starts
    late = layer_obstacles_from_rows(rows_at, ro, 0.5, [SLAB, PILLAR], start_rows=[0, 500, 0], max_steps=7)
    assert late[:, 1].tolist() == [5, 5, 1, 3] and late[3].tolist() == [3, 3, 8]
    # an excluded mission and an oversized group are not examined: blocked 0
    broken = np.full((5, 3), np.nan)
    rows2, ro2 = rows_of(A, broken, B_)
    il = layer_obstacles_from_rows(layered(rows2, UP), ro2, 0.5, [SLAB], max_steps=7)
    assert il[:, 1].tolist() == [0, -2, 0, 0] and il[:, 0].tolist() == [3, 3, 0, 3] and il[:, 2].tolist() == [5, 5, 1, 3]
    assert not blocked_out(il, 7).any() and layer_ok(il)["examined"].tolist() == [True, False, True]
    assert layer_from_rows(layered(rows2, UP), ro2, 0.5, max_steps=7)[0].tolist() == [0, 0, 2]


def test_invalid_arguments_raise():
    from uav_ac import _native as nat
    from uav_ac.scoring import blocked_out, layer_obstacles_from_rows
    rows, ro = rows_of(A, B_, C_)
    rows_at = layered(rows, UP)
    for bad in (np.zeros((nat.AUDIT_MAX_CUBOIDS + 1, 6)), np.zeros((2, 5)), np.zeros(6), np.zeros((3, 4))):
        with pytest.raises(ValueError):
            layer_obstacles_from_rows(rows_at, ro, 0.5, bad)
    assert layer_obstacles_from_rows(rows_at, ro, 0.5, np.zeros((nat.AUDIT_MAX_CUBOIDS, 6))).shape == (4, 3)
    for go in ([0, 2, 1, 3], [1, 3], [0, 2], [0]):
        with pytest.raises(ValueError):
            layer_obstacles_from_rows(rows_at, ro, 0.5, [SLAB], group_offsets=go)
    for radius in (-1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            layer_obstacles_from_rows(rows_at, ro, radius, [SLAB])
    for kw in (dict(start_rows=[0, 0]), dict(max_steps=-1), dict(max_steps=nat.LAYER_MAX_STEPS + 1)):
        with pytest.raises(ValueError):
            layer_obstacles_from_rows(rows_at, ro, 0.5, [SLAB], **kw)
    with pytest.raises(ValueError):
        layer_obstacles_from_rows(rows, ro, 0.5, [SLAB])     # rows instead of a callable
    with pytest.raises(ValueError):
        blocked_out(np.zeros((3, 5), dtype=np.int32), 7)     # a block without the fourth row
    with pytest.raises(ValueError):
        blocked_out(SimpleNamespace(steps=np.zeros(3), blocked=None), 7)
