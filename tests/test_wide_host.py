"""The searches for groups of any size, on the host: `max_group=` of the three scoring rules -- the specification of
`uavac_minsnap_stagger_wide_dev` and `uavac_minsnap_layer_wide_dev` --, the prototypes, the build's budgets for the two new object
files, and `Engine._group_cap`.  The hand-made cases are tests/test_stagger_host.py's; nothing here needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO
from test_stagger_host import ALONG_X, ALONG_Y, rows_of

CUBOID = np.array([[4.5, 5.5, 4.5, 5.5, -3.5, -2.5]])       # around the crossing point of the pair


def rows_at_of(paths, dz=1.0):
    """rows_at for the layer rules: every mission q * dz higher (NED: z falls) on layer q"""
    rows, ro = rows_of(*paths)
    memo = {}

    def rows_at(q):
        if q not in memo:
            memo[q] = rows.copy()
            memo[q][:, 2] -= q * dz
        return memo[q]
    return rows_at, ro


def parked(n, x0=100.0):
    """n missions that stand still, 3 m apart, far from the crossing pair"""
    return [np.tile([x0 + 3.0 * b, 0.0, -3.0], (5, 1)) for b in range(n)]


# ------------------------------------------------------------------------------------------------ max_group
def test_none_is_the_narrow_limit_on_the_hand_made_cases():
    from uav_ac import _native as nat
    from uav_ac.scoring import layer_from_rows, layer_obstacles_from_rows, stagger_from_rows
    rows, ro = rows_of(ALONG_X, ALONG_Y)
    want = stagger_from_rows(rows, ro, 0.5)
    assert want[:2].tolist() == [[0, 6], [0, 6]]             # (tests/test_stagger_host.py)
    for max_group in (None, nat.STAGGER_MAX_GROUP, 2, 300):
        assert np.array_equal(stagger_from_rows(rows, ro, 0.5, max_group=max_group), want)
    assert stagger_from_rows(rows, ro, 0.5, max_group=1)[1].tolist() == [-2, -2]
    rows_at, ro = rows_at_of([ALONG_X, ALONG_Y])
    lay = layer_from_rows(rows_at, ro, 0.5)
    obs = layer_obstacles_from_rows(rows_at, ro, 0.5, CUBOID)
    assert lay[:2].tolist() == [[0, 1], [0, 1]] and obs.tolist() == [[1, 2], [1, 2], [0, 1], [1, 1]]
    for max_group in (None, nat.LAYER_MAX_GROUP, 2, 300):
        assert np.array_equal(layer_from_rows(rows_at, ro, 0.5, max_group=max_group), lay)
        assert np.array_equal(layer_obstacles_from_rows(rows_at, ro, 0.5, CUBOID, max_group=max_group), obs)
    assert layer_from_rows(rows_at, ro, 0.5, max_group=1)[1].tolist() == [-2, -2]
    for bad in (0, -1):
        with pytest.raises(ValueError, match="max_group must be >= 1"):
            stagger_from_rows(rows, ro, 0.5, max_group=bad)
        with pytest.raises(ValueError, match="max_group must be >= 1"):
            layer_from_rows(rows_at, ro, 0.5, max_group=bad)


def test_a_group_of_259_is_examined_with_a_number_and_not_with_none():
    from uav_ac.scoring import layer_from_rows, layer_obstacles_from_rows, stagger_from_rows
    paths = parked(257) + [ALONG_X, ALONG_Y]
    B = len(paths)
    rows, ro = rows_of(*paths)
    narrow = stagger_from_rows(rows, ro, 0.5)
    assert (narrow[1] == -2).all() and (narrow[0] == 0).all() and (narrow[2] == 0).all()
    wide = stagger_from_rows(rows, ro, 0.5, max_group=300)
    assert (wide[1, :258] == 0).all() and wide[:, 258].tolist() == [6, 6, 258] and wide[2].tolist() == list(range(B))
    assert (stagger_from_rows(rows, ro, 0.5, max_group=258)[1] == -2).all()       # the limit is the number
    assert np.array_equal(stagger_from_rows(rows, ro, 0.5, max_group=259), wide)
    # two groups: the limit is per group, and the other group does not care
    go = [0, 257, B]
    assert np.array_equal(stagger_from_rows(rows, ro, 0.5, group_offsets=go)[1], [-2] * 257 + [0, 6])
    assert np.array_equal(stagger_from_rows(rows, ro, 0.5, group_offsets=go, max_group=257)[1], [0] * 257 + [0, 6])
    rows_at, ro = rows_at_of(paths)
    assert (layer_from_rows(rows_at, ro, 0.5)[1] == -2).all() and (layer_obstacles_from_rows(rows_at, ro, 0.5, CUBOID)[1] == -2).all()
    lay = layer_from_rows(rows_at, ro, 0.5, max_group=300)
    assert (lay[1, :258] == 0).all() and lay[:, 258].tolist() == [1, 1, 258]
    obs = layer_obstacles_from_rows(rows_at, ro, 0.5, CUBOID, max_group=300)
    assert (obs[1, :257] == 0).all() and obs[:, 257].tolist() == [1, 1, 257, 1] and obs[:, 258].tolist() == [2, 2, 258, 1]


# ------------------------------------------------------------------------------------------------ the ABI
@pytest.mark.parametrize("name, count", (("uavac_minsnap_stagger_wide_dev", 15), ("uavac_minsnap_layer_wide_dev", 20)))
def test_entry_points_are_exported_and_declared_like_the_header(name, count):
    from uav_ac import _native as nat
    assert name in nat.exported_symbols()
    fn = getattr(nat.lib(), name)
    restype, argtypes = nat._SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == count
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "uavac.h")).read(), flags=re.S)
    params = [" ".join(a.split()) for a in re.search(rf"int\s+{name}\s*\(([^)]*)\)\s*;", text).group(1).split(",")]
    kinds = [C.c_void_p if "*" in a else {"int": C.c_int, "double": C.c_double}[a.split()[0]] for a in params]
    assert kinds == list(argtypes), params
    assert params[9] == "int group_cap" and params[8] == "int G"
    # the narrow calls' prototypes with group_cap put in behind G
    narrow = nat._SIGNATURES[name.replace("stagger_wide", "stagger").replace("layer_wide", "layer_obs")][1]
    assert list(argtypes) == list(narrow[:9]) + [C.c_int] + list(narrow[9:])
    # a NULL context is refused before anything else is looked at (pure host code: no GPU needed)
    assert fn(*([None] * 4 + [1, 1, 0.01, None, 0, 1, None, 0.5] + ([1, 255, None] if count == 15 else [0.0, 0.0, -0.5, 63, None, 0, None, None]))) \
        == nat.EINVAL
    assert nat.SEARCH_BLOCKS == (64, 128, 256) and nat.VERSION == nat.lib().uavac_version()


def test_the_build_budgets_the_two_new_object_files():
    from uav_ac import _buildcheck as bc
    rows = {r.key: r for r in bc.BUDGETS if r.key in ("stagger_wide_kernels", "layer_wide_kernels")}
    assert rows["stagger_wide_kernels"].obj == "minsnap_stagger_wide.o" and rows["layer_wide_kernels"].obj == "minsnap_layer_wide.o"
    assert all(r.limit is bc.FROM_LDS and r.scratch_free and not r.extra and not r.at_least for r in rows.values())
    assert rows["stagger_wide_kernels"].kernels == ("stagger_prepass_kernel", "wide_stagger_seed_kernel", "wide_stagger_kernel")
    assert rows["layer_wide_kernels"].kernels == ("layer_prepass_kernel", "wide_layer_seed_kernel", "wide_layer_kernel")
    # the narrow objects' rows are what they were
    assert next(r for r in bc.BUDGETS if r.key == "stagger_kernels").kernels == ("stagger_prepass_kernel", "minsnap_stagger_kernel")
    assert next(r for r in bc.BUDGETS if r.key == "layer_obs_kernels").kernels == ("layer_prepass_kernel", "minsnap_layer_kernel")
    # a block search with two workgroups per CU is refused like the layer's decision kernel; the seed kernel is held to its LDS alone
    ns, lds = "_ZN12_GLOBAL__N_1", bc.LDS_BYTES_PER_CU // 3 + 1

    def K(name, vgpr, group):
        return bc.Kernel(ns + name, vgpr, 0, 22, 0, 0, 0, group)
    for key, pre, noun in (("stagger_wide_kernels", "22stagger_prepass_kernelEPKd", "stagger"), ("layer_wide_kernels", "20layer_prepass_kernelILb1EEEvPKd", "layer")):
        seed, search = f"{len(noun) + 17}wide_{noun}_seed_kernelEPKd", f"{len(noun) + 12}wide_{noun}_kernelEPKd"
        good = [K(pre, 64, 0), K(seed, 168, 49168), K(search, 168, lds - 1)]
        assert len(bc.check_budget(rows[key], good)) == 3
        for bad, words in (([good[0], good[1], K(search, 24, lds)], "fewer than three workgroups"), ([good[0], K(seed, 169, 49168), good[2]], "169"),
                           ([good[0], K(seed, 168, 49168)._replace(private_segment_fixed_size=8), good[2]], "8 private-segment bytes"),
                           (good[1:], "missing"), (good + [K("17fill_f64_kernelEPdmd", 10, 0)], "4 kernels found")):
            with pytest.raises(RuntimeError, match=words):
                bc.check_budget(rows[key], bad)
        assert len(bc.check_budget(rows[key], [good[0], K(seed, 256, lds), good[2]])) == 3        # (two workgroups of the seed: 256 registers)
    for check in (bc.check_stagger_wide_kernels, bc.check_layer_wide_kernels):
        counts = check()
        if counts is None:
            pytest.skip("no object files here (a library that was built elsewhere)")
        assert len(counts) == 3 and max(counts.values()) <= 168


# ------------------------------------------------------------------------------------------------ the engine's group_cap
def test_group_cap_is_taken_from_the_groups_where_they_are_known():
    import torch
    from uav_ac.engine import Engine
    eng = object.__new__(Engine)                             # (no context: the helper needs nothing)
    eng._torch, eng.device = torch, torch.device("cpu")
    assert eng._group_cap(None, 300) == 300 and eng._group_cap(None, 300, 4096) == 300
    assert eng._group_cap(1024, 4096) == 1024 and eng._group_cap(1024, 300) == 300 and eng._group_cap(np.int64(7), 300) == 7
    assert eng._group_cap([0, 63, 127, 192, 193, 193, 322], 322) == 129 and eng._group_cap(np.array([0, 0]), 1) == 1
    assert eng._group_cap(torch.tensor([0, 10, 300]), 300) == 290
    for call, words in ((lambda: eng._group_cap(None, 300, 0), "group_cap must be >= 1"),
                        (lambda: eng._group_cap(None, 300, 299), "a group of 300 missions; group_cap is 299"),
                        (lambda: eng._group_cap([0, 10, 300], 300, 256), "a group of 290 missions; group_cap is 256")):
        with pytest.raises(ValueError) as err:
            call()
        assert str(err.value) == words
