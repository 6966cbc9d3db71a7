"""Missions of a plan selected, reordered and merged, and priorities for the fleet's searches -- the part that needs no GPU: the three
entry points are exported and declared as the header declares them, a NULL context is refused, the build keeps the kernels inside
their budget, and the rules themselves -- `uav_ac.scoring.priority_order`, `take_parts` and `take_rows`, the NumPy statements the
kernels are tested against exactly (tests/test_gpu_take.py, tests/test_gpu_priority.py) -- give what hand-made input has by
inspection.  The host side of `Engine.take`, `concat` and `put` (the mask, the refusals and their words) runs on an Engine without a
context, and the composition behind `priority=` is checked on two crossing paths: with the priorities swapped, the other mission waits."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO

KINDS = {"int": C.c_int, "double": C.c_double, "int64_t": C.c_int64}
NAN, INF = float("nan"), float("inf")
PRIORITIES = [2, 1, 1, NAN, -INF, INF, -0.0, 0.0, NAN]


def declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "uavac.h")).read(), flags=re.S)
    args = re.search(rf"int\s+{name}\s*\(([^)]*)\)\s*;", text).group(1)
    params = [" ".join(a.split()) for a in args.split(",")]
    return [C.c_void_p if "*" in a else KINDS[a.split()[0]] for a in params], params


def test_entry_points_are_exported_and_declared_like_the_header():
    from uav_ac import _native as nat
    for name, n_args in (("uavac_minsnap_take_offsets_dev", 7), ("uavac_minsnap_take_dev", 15), ("uavac_fleet_order_dev", 7)):
        assert name in nat.exported_symbols()
        getattr(nat.lib(), name)
        restype, argtypes = nat._SIGNATURES[name]
        kinds, params = declared(name)
        assert restype is C.c_int and len(argtypes) == n_args and kinds == list(argtypes), params
    # a NULL context is refused before anything else is looked at (pure host code: no GPU needed)
    lib = nat.lib()
    assert lib.uavac_minsnap_take_offsets_dev(None, None, 1, 1, None, 1, None) == nat.EINVAL
    assert lib.uavac_minsnap_take_dev(None, None, None, None, None, 1, 1, None, None, 1, None, None, None, None, None) == nat.EINVAL
    assert lib.uavac_fleet_order_dev(None, None, None, 0, 1, None, None) == nat.EINVAL


def test_the_build_keeps_the_take_kernels_in_registers():
    from uav_ac import _buildcheck
    counts = _buildcheck.check_take_kernels()
    if counts is None:
        pytest.skip("no object files here (a library that was built elsewhere)")
    assert len(counts) == 3 and max(counts.values()) <= 64
    for kernel in ("take_counts_kernel", "minsnap_take_kernel", "fleet_order_kernel"):
        assert any(kernel in k for k in counts), kernel


# ------------------------------------------------------------------------------------------------ the order rule
def test_priority_order_by_inspection():
    from uav_ac.scoring import priority_order
    # one group: -inf, the two zeros in index order, the 1s in index order, 2, +inf, the NaNs in index order
    order, rank = priority_order(PRIORITIES)
    assert order.dtype == np.int32 and rank.dtype == np.int32
    assert order.tolist() == [4, 6, 7, 1, 2, 0, 5, 3, 8] and rank.tolist() == [5, 3, 4, 7, 0, 6, 1, 2, 8]
    # groups [0, 1), [1, 3), [3, 9): sizes 1 and 2 -- a tie keeps the index order -- and the rest
    order, rank = priority_order(PRIORITIES, [0, 1, 3, 9])
    assert order.tolist() == [0, 1, 2, 4, 6, 7, 5, 3, 8] and rank.tolist() == [0, 1, 2, 7, 3, 6, 4, 5, 8]
    order, _ = priority_order([5.0, 3.0, 4.0], [0, 1, 3])
    assert order.tolist() == [0, 1, 2]
    order, _ = priority_order([5.0, 4.0, 3.0], [0, 1, 3])
    assert order.tolist() == [0, 2, 1]
    # a head (0, 1) and a tail (7, 8) that no group holds keep their places; 20 is clamped to B as group_range clamps it, and so is -3
    order, rank = priority_order(PRIORITIES, [2, 5, 7])
    assert order.tolist() == [0, 1, 4, 2, 3, 6, 5, 7, 8] and rank.tolist() == [0, 1, 3, 4, 2, 6, 5, 7, 8]
    order, rank = priority_order(PRIORITIES, [2, 5, 20])
    assert order.tolist() == [0, 1, 4, 2, 3, 6, 7, 5, 8]
    assert priority_order(PRIORITIES, [-3, 9])[0].tolist() == priority_order(PRIORITIES)[0].tolist()
    for go in (None, [0, 1, 3, 9], [2, 5, 7], [0, 4, 4, 9]):
        order, rank = priority_order(PRIORITIES, go)
        assert np.array_equal(rank[order], np.arange(9)) and np.array_equal(order[rank], np.arange(9))
        assert sorted(order.tolist()) == list(range(9))
        ident = priority_order(np.arange(9.0), go)
        assert np.array_equal(ident[0], np.arange(9)) and np.array_equal(ident[1], np.arange(9))
    assert priority_order(-np.arange(9.0), [0, 4, 9])[0].tolist() == [3, 2, 1, 0, 8, 7, 6, 5, 4]
    with pytest.raises(ValueError):
        priority_order(PRIORITIES, [0])


# ------------------------------------------------------------------------------------------------ the gather
def parts(counts):
    """Hand-made parts of missions with `counts` segments: every value names its segment, so a copy shows where it came from."""
    S = int(np.sum(counts))
    co = (np.arange(S * 24, dtype=np.float64) + 0.5).reshape(S, 8, 3)
    return co, 100.0 + np.arange(S), (7 + np.arange(S)).astype(np.int32), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


@pytest.mark.parametrize("counts, uniform", [([2, 2, 2], True), ([1, 3, 2], False)])
def test_take_parts_and_take_rows_on_hand_made_parts(counts, uniform):
    from uav_ac.scoring import take_parts, take_rows
    co, tm, sr, so = parts(counts)
    how = 2 if uniform else so
    ro = np.array([0, 3, 4, 9], dtype=np.int64)                               # rows: 3, 1 and 5, each naming its mission and its row
    rows = np.stack([np.repeat(np.arange(3), np.diff(ro)), np.arange(9)], axis=1).astype(np.float64)
    for idx in ([2, 1, 0], [1, 1, 0, 1], [0, 1, 2, 2, 1, 0, 0], [2]):         # reversed, duplicates, n > B, n == 1
        oc, ot, osr, oso = take_parts(co, tm, sr, how, idx)
        assert oso.dtype == np.int64 and osr.dtype == np.int32 and oso.tolist() == np.concatenate([[0], np.cumsum(np.asarray(counts)[idx])]).tolist()
        for i, b in enumerate(idx):
            a, z = so[b], so[b + 1]
            assert np.array_equal(oc[oso[i]:oso[i + 1]], co[a:z]) and np.array_equal(ot[oso[i]:oso[i + 1]], tm[a:z])
            assert np.array_equal(osr[oso[i]:oso[i + 1]], sr[a:z])
        assert take_parts(co, None, sr, how, idx)[1] is None
        orows, oro = take_rows(rows, ro, idx)
        assert oro.tolist() == np.concatenate([[0], np.cumsum(np.diff(ro)[idx])]).tolist() and len(orows) == oro[-1]
        for i, b in enumerate(idx):
            assert np.array_equal(orows[oro[i]:oro[i + 1]], rows[ro[b]:ro[b + 1]])
    same = take_parts(co, tm, sr, how, [0, 1, 2])
    assert np.array_equal(same[0], co) and np.array_equal(same[1], tm) and np.array_equal(same[2], sr) and np.array_equal(same[3], so)
    assert same[0] is not co
    for bad in ([], [3], [-1]):
        with pytest.raises(ValueError):
            take_parts(co, tm, sr, how, bad)
        with pytest.raises(ValueError):
            take_rows(rows, ro, bad)
    with pytest.raises(ValueError):
        take_parts(co, tm[:-1], sr, how, [0])
    with pytest.raises(ValueError):
        take_parts(co, tm, sr, 4 if uniform else so[:-1], [0])


# ------------------------------------------------------------------------------------------------ the host side of the Engine
def cpu_engine():
    import torch
    from uav_ac.engine import Engine
    eng = object.__new__(Engine)                             # (no context: these helpers need the device and torch only)
    eng._torch, eng.device = torch, torch.device("cpu")
    return eng


def cpu_batch(counts, dt=0.01, velocity=3.0, with_times=True, velocities=None, scale=1.0):
    """A RaggedBatch on the CPU from hand-made parts (1 row per segment more than its number, first heading 0.25 * mission)."""
    import torch
    from uav_ac.engine import RaggedBatch
    co, tm, sr, so = parts(counts)
    B = len(counts)
    rows = np.array([sr[so[b]:so[b + 1]].sum() for b in range(B)])
    ro = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    return RaggedBatch(B, int(max(counts)), velocity, dt, torch.as_tensor(so), so, None, torch.as_tensor(tm * scale) if with_times else None,
                       torch.as_tensor(sr), torch.as_tensor(ro), torch.as_tensor(co * scale), torch.arange(B, dtype=torch.int32), None,
                       int(ro[-1]), torch.as_tensor(0.25 * np.arange(B) * scale), None,
                       None if velocities is None else torch.as_tensor(np.asarray(velocities, dtype=np.float64)), True)


def test_what_take_selects_a_mask_indices_and_the_refusals():
    import torch
    eng = cpu_engine()
    for index, want in (([3, 0, 3], [3, 0, 3]), (np.array([1], dtype=np.int64)[:1], [1]), (torch.tensor([2, 2], dtype=torch.int16), [2, 2]),
                        (np.array([False, True, False, True]), [1, 3]), (torch.tensor([True, False, False, False]), [0]),
                        (~torch.tensor([True, True, False, True]), [2]), (range(4), [0, 1, 2, 3])):
        got = eng._take_index(list(index) if isinstance(index, range) else index, 4)
        assert got.dtype == torch.int32 and got.is_contiguous() and got.tolist() == want
    for index, words in (([], "an empty selection: take needs at least one mission"),
                         (np.zeros(4, dtype=bool), "an empty selection: take needs at least one mission"),
                         (np.ones(3, dtype=bool), "a mask holds one entry per mission: expected 4, got 3"),
                         ([0.0, 1.0], "index must hold integers or be a boolean mask"),
                         ([0, 4], "index must be in 0 .. 3"), ([-1], "index must be in 0 .. 3")):
        with pytest.raises(ValueError) as err:
            eng._take_index(index, 4)
        assert str(err.value) == words


def test_concat_joins_the_parts_and_refuses_what_does_not_fit():
    import torch
    eng = cpu_engine()
    a, b = cpu_batch([1, 3, 2]), cpu_batch([2, 2], scale=-2.0)
    c = eng.concat([a, b])
    assert c.B == 5 and c.max_m == 3 and c.velocity == 3.0 and c.dt == 0.01 and c.velocities is None and c.free_times
    assert c.waypoints is None and c.traj is None and c.total_rows == a.total_rows + b.total_rows
    assert c.seg_offsets.tolist() == [0, 1, 4, 6, 8, 10] == c.seg_offsets_host.tolist() and c.seg_offsets.dtype == torch.int64
    assert c.row_offsets.tolist() == a.row_offsets.tolist() + (b.row_offsets[1:] + a.total_rows).tolist()
    for name in ("coeffs", "times", "seg_rows", "first_yaw", "status"):
        assert torch.equal(getattr(c, name), torch.cat([getattr(a, name), getattr(b, name)])), name
    assert c.coeffs.shape == (10, 8, 3)
    # durations only when every part has them; one speed only when the parts share it
    assert eng.concat([a, cpu_batch([2, 2], with_times=False)]).times is None
    d = eng.concat([a, cpu_batch([2, 2], velocity=2.0)])
    assert np.isnan(d.velocity) and d.velocities.tolist() == [3.0, 3.0, 3.0, 2.0, 2.0]
    d = eng.concat([cpu_batch([2, 2], velocities=[1.0, 1.5]), a])
    assert np.isnan(d.velocity) and d.velocities.tolist() == [1.0, 1.5, 3.0, 3.0, 3.0]
    one = eng.concat([a])
    assert one.B == 3 and torch.equal(one.coeffs, a.coeffs) and one.seg_offsets.tolist() == a.seg_offsets.tolist()
    for plans, words in (([], "concat needs at least one plan"),
                         ([a, cpu_batch([2, 2], dt=0.02)], "the plans differ in dt ([0.01, 0.02]): their rows would not share a clock")):
        with pytest.raises(ValueError) as err:
            eng.concat(plans)
        assert str(err.value) == words


def test_where_put_puts_and_what_it_refuses():
    import torch
    eng = cpu_engine()
    for index, want in (([3, 0], [3, 0]), (torch.tensor([1, 2]), [1, 2]), (np.array([True, False, False, True]), [0, 3]),
                        (~torch.tensor([True, False, True, False]), [1, 3])):
        got = eng._put_index(index, 4, 2)
        assert got.dtype == np.int64 and got.tolist() == want
    for index, n, words in (([0, 1, 2], 2, "one index per mission of `other`: expected 2, got 3"),
                            ([1, 1], 2, "index must not name a mission twice"), ([0, 4], 2, "index must be in 0 .. 3"),
                            ([-1, 0], 2, "index must be in 0 .. 3"), ([0.0, 1.0], 2, "index must hold integers or be a boolean mask"),
                            (np.ones(3, dtype=bool), 3, "a mask holds one entry per mission: expected 4, got 3"),
                            (np.array([True, False, False, False]), 2, "one index per mission of `other`: expected 2, got 1")):
        with pytest.raises(ValueError) as err:
            eng._put_index(index, 4, n)
        assert str(err.value) == words
    # put refuses before it copies anything: no context is needed to get there
    with pytest.raises(ValueError) as err:
        eng.put(cpu_batch([1, 3, 2]), [0, 0], cpu_batch([2, 2]))
    assert str(err.value) == "index must not name a mission twice"


# ------------------------------------------------------------------------------------------------ the composition behind priority=
def rows_of(*paths):
    """Missions given as (N_b, 3) position lists -> (rows (N, 11), row_offsets (B + 1,)): the sampler's layout, positions in 0-2."""
    ro = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    rows = np.zeros((int(ro[-1]), 11))
    for b, p in enumerate(paths):
        rows[ro[b]:ro[b + 1], 0:3] = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    return rows, ro


def line(p0, p1, n=81):
    return np.linspace(np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64), n)


ALONG_X = line([0, 5, -3], [10, 5, -3])                      # both pass (5, 5, -3) at their own row 40 (tests/test_stagger_host.py)
ALONG_Y = line([5, 0, -3], [5, 10, -3])


def test_swapped_priorities_delay_the_other_mission_on_two_crossing_paths():
    from uav_ac.scoring import priority_order, stagger_from_rows, take_rows
    rows, ro = rows_of(ALONG_X, ALONG_Y)

    def staggered(priority):
        order, rank = priority_order(priority)
        trows, tro = take_rows(rows, ro, order)
        return order, stagger_from_rows(trows, tro, 0.5)[:, rank]

    order, istag = staggered([0.0, 1.0])
    assert order.tolist() == [0, 1] and np.array_equal(istag, stagger_from_rows(rows, ro, 0.5))
    assert istag[0].tolist() == [0, 6] and istag[1].tolist() == [0, 6] and istag[2].tolist() == [0, 1]
    order, istag = staggered([1.0, 0.0])
    assert order.tolist() == [1, 0]
    assert istag[0].tolist() == [6, 0] and istag[1].tolist() == [6, 0] and istag[2].tolist() == [1, 0]
    # a tie, and a NaN against a number: the lower index, and the number, go first
    assert staggered([4.0, 4.0])[1][0].tolist() == [0, 6] and staggered([NAN, 1e300])[1][0].tolist() == [6, 0]
