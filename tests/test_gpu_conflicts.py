"""Conflict list on the GPU (`uavac_minsnap_conflict_offsets_dev`, `uavac_minsnap_conflicts_dev`, csrc/minsnap_conflicts.hip), through
the C ABI and `Engine.conflicts`: the separation audit's conflict graph in CSR form -- per mission every partner of its group that comes
inside the radius, with the first and the last clock row inside, the rows inside, and the pair's closest approach and its row.

What is compared with what:
  * against the PRODUCT'S OWN ROWS everything is exact (no tolerance): `uav_ac.scoring.conflicts_from_rows` on the sampled rows is the
    rule, and the kernels use the sampler's arithmetic, form d^2 = (dx dx + dy dy) + dz dz without contraction, take exact reductions
    and one correctly rounded sqrt;
  * against `Engine.separation` the three identities of the header hold exactly, and the two directions of a pair agree
    (`scoring.conflict_pairs`);
  * against the ORACLE (oracle.c_oracle.plan_threads: its own solve and sampler, through the same NumPy rule) offsets, partner, first,
    last and rows inside are exact, `min_distance` holds to 2e-5 absolute -- two positions, each at the project's 1e-5 bar for sampled
    positions --, and for `min_row` the oracle's distance of the pair at the reported row lies within 2e-5 of the oracle's minimum of
    the pair.  A difference in the exact quantities could only be excused by a pair-row whose oracle distance lies within 2e-5 of the
    radius; the cap on such cases is 0, which is a condition on the sets, asserted in the test: the oracle's nearest pair-row is
    1.35e-4 / 5.3e-4 / 6.6e-4 from the radius for (8, 96) / (8, 37) / (1, 48) in one group, and 1.27e-4 / 7.9e-4 / 2.1e-3 with the
    groups and staggered starts below (checked on the CPU; all above 4e-5, twice the bar).
The tile of the pair kernel is 64 missions wide: groups of 63, 64 and 65 missions (and windows that straddle groups) are cut from the
(8, 96) set, 19 of whose missions have partners in both j-tiles and two of whose entries have an incursion with a gap -- asserted, so
that the set cannot silently stop exercising the tile order and the gap."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VEL, DT, RADIUS = 3.0, 0.01, 0.5
SETS = ((8, 96), (8, 37), (1, 48))
SENT_F, SENT_I, SENT_O, PAD = -1.2345e300, -7777, -5555, 96
DIST_TOL, RADIUS_MARGIN = 2e-5, 4e-5
TILE = 64
PARTNER, FIRST, LAST, INSIDE, MIN_ROW = range(5)


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    e = Engine("cuda:0")
    yield e
    e.ctx.set_option("separation_split", 0)
    e.ctx.set_option("conflict_slots", 0)


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _i64(eng, a):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.int64)).to(eng.device)


def _i32(eng, a):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(eng.device)


def offsets_abi(eng, coeffs, seg_rows, seg_offsets, B, m, dt, go=None, start=None, radius=RADIUS):
    """uavac_minsnap_conflict_offsets_dev -> pair_offsets (B + 1,) as NumPy, from the middle of a larger sentinel-filled buffer."""
    import torch
    obuf = torch.full((PAD + B + 1 + PAD,), SENT_O, dtype=torch.int64, device=eng.device)
    g, s = _i64(eng, go), _i32(eng, start)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_conflict_offsets_dev", _p(coeffs), _p(seg_rows), _p(seg_offsets), int(B), int(m), float(dt), _p(g),
                 0 if go is None else len(go) - 1, _p(s), float(radius), _p(obuf[PAD:]))
    torch.cuda.synchronize()
    o = obuf.cpu().numpy()
    assert (o[:PAD] == SENT_O).all() and (o[PAD + B + 1:] == SENT_O).all() and not (o[PAD:PAD + B + 1] == SENT_O).any()
    return o[PAD:PAD + B + 1].copy()


def fill_abi(eng, coeffs, seg_rows, seg_offsets, B, m, dt, offsets, capacity, go=None, start=None, radius=RADIUS):
    """uavac_minsnap_conflicts_dev into the middle of larger sentinel-filled buffers -> (pair_d (capacity,), pair_i (5, capacity)) as
    NumPy with the sentinels where nothing was written; nothing outside [capacity] / [5][capacity] may be written."""
    import torch
    dev = dict(device=eng.device)
    dbuf = torch.full((PAD + capacity + PAD,), SENT_F, dtype=torch.float64, **dev)
    ibuf = torch.full((PAD + 5 * capacity + PAD,), SENT_I, dtype=torch.int32, **dev)
    g, s, o = _i64(eng, go), _i32(eng, start), _i64(eng, offsets)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_conflicts_dev", _p(coeffs), _p(seg_rows), _p(seg_offsets), int(B), int(m), float(dt), _p(g),
                 0 if go is None else len(go) - 1, _p(s), float(radius), _p(o), int(capacity), _p(dbuf[PAD:]), _p(ibuf[PAD:]))
    torch.cuda.synchronize()
    d, i = dbuf.cpu().numpy(), ibuf.cpu().numpy()
    assert (d[:PAD] == SENT_F).all() and (d[PAD + capacity:] == SENT_F).all()
    assert (i[:PAD] == SENT_I).all() and (i[PAD + 5 * capacity:] == SENT_I).all()
    return d[PAD:PAD + capacity].copy(), i[PAD:PAD + 5 * capacity].reshape(5, capacity).copy()


def conf_abi(eng, coeffs, seg_rows, seg_offsets, B, m, dt, **kw):
    """Both calls -> (offsets, pair_d, pair_i) as NumPy; everything inside [0, E) must be written."""
    off = offsets_abi(eng, coeffs, seg_rows, seg_offsets, B, m, dt, **kw)
    E = int(off[-1])
    d, i = fill_abi(eng, coeffs, seg_rows, seg_offsets, B, m, dt, off, E, **kw)
    assert not (d == SENT_F).any() and not (i == SENT_I).any()
    return off, d, i


def parts(plan):
    ragged = hasattr(plan, "seg_offsets")
    return plan.coeffs, plan.seg_rows, plan.seg_offsets if ragged else None, plan.B, plan.max_m if ragged else plan.m, plan.dt


def conf_of_plan(eng, plan, **kw):
    return conf_abi(eng, *parts(plan), **kw)


def of_engine(cl):
    """A ConflictList -> (offsets, pair_d, pair_i) as NumPy"""
    fields = (cl.partner, cl.first_row, cl.last_row, cl.rows_inside, cl.min_row)
    return cl.offsets.cpu().numpy(), cl.min_distance.cpu().numpy(), np.stack([t.cpu().numpy() for t in fields])


def same(got, want):
    return all(g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))


def configs(B):
    """(name, group_offsets, start_rows): one group of all B without start rows; four groups (one of them of one mission, one empty)
    with staggered starts."""
    return (("one group", None, None),
            ("groups, staggered", np.array([0, 1, B // 3, B // 3, B]), (np.arange(B) % 5) * 37))


_CACHE = {}


def case(eng, m, B):
    """Per mission set, computed once and left unchanged: the plan with rows, the rows-free plan, the rows on the host and what the
    rule gives on them for both configurations."""
    if (m, B) not in _CACHE:
        from oracle import minsnap_oracle as mo
        from uav_ac.scoring import conflicts_from_rows
        wps = mo.synthetic_missions(B, m)
        plan = eng.plan(wps, VEL, DT)
        free = eng.plan(wps, VEL, DT, rows=False)
        rows, ro = plan.traj.cpu().numpy(), plan.row_offsets.cpu().numpy()
        want = {name: conflicts_from_rows(rows, ro, RADIUS, go, st) for name, go, st in configs(B)}
        _CACHE[(m, B)] = dict(wps=wps, plan=plan, free=free, rows=rows, ro=ro, want=want)
    return _CACHE[(m, B)]


# ------------------------------------------------------------------------------------------------ 1: the product's own rows
@pytest.mark.parametrize("m, B", SETS)
def test_the_list_equals_what_the_products_rows_show(eng, m, B):
    k = case(eng, m, B)
    assert k["free"].traj is None
    for name, go, st in configs(B):
        got_free = conf_of_plan(eng, k["free"], go=go, start=st)
        got_rows = conf_of_plan(eng, k["plan"], go=go, start=st)
        assert same(got_free, got_rows), (m, B, name)
        want = k["want"][name]
        assert same(got_free, want), (m, B, name, got_free[0][-1], want[0][-1])
    off, d, i = k["want"]["one group"]
    assert off[-1] == {(8, 96): 120, (8, 37): 20, (1, 48): 14}[(m, B)]
    if (m, B) == (8, 96):                                                            # what the set is here for
        assert np.diff(off).max() == 4
        both = sum(bool((i[PARTNER, off[b]:off[b + 1]] < TILE).any() and (i[PARTNER, off[b]:off[b + 1]] >= TILE).any()) for b in range(B))
        assert both == 19                                                            # partners in both j-tiles: the tile order decides the slice
        assert int((i[INSIDE] < i[LAST] - i[FIRST] + 1).sum()) == 2                  # incursions with a gap


def test_engine_conflicts(eng):
    from uav_ac.scoring import conflicts_from_rows
    k = case(eng, 8, 96)
    for plan in (k["free"], k["plan"]):
        for name, go, st in configs(96):
            cl = eng.conflicts(plan, RADIUS, groups=go, start_rows=st)
            assert cl.offsets.is_cuda and cl.min_distance.is_cuda and cl.partner.is_cuda
            assert cl.total == int(k["want"][name][0][-1]) and cl.block.shape == (5, cl.total)
            assert same(of_engine(cl), k["want"][name]), name
    # groups given as a size: consecutive groups of that many, the last one shorter
    by_size = of_engine(eng.conflicts(k["free"], RADIUS, groups=36))
    assert same(by_size, of_engine(eng.conflicts(k["free"], RADIUS, groups=[0, 36, 72, 96])))
    assert same(by_size, conflicts_from_rows(k["rows"], k["ro"], RADIUS, [0, 36, 72, 96]))
    # no entries: empty tensors, all offsets 0
    none = eng.conflicts(k["free"], 0.0)
    assert none.total == 0 and none.partner.shape == (0,) and none.min_distance.shape == (0,) and none.block.shape == (5, 0)
    assert none.offsets.cpu().numpy().tolist() == [0] * 97
    with pytest.raises(ValueError):
        eng.conflicts(k["free"], RADIUS, start_rows=np.zeros(5))
    with pytest.raises(ValueError):
        eng.conflicts(k["free"], RADIUS, groups=0)


def test_ragged_batches(eng):
    from uav_ac.scoring import conflicts_from_rows
    k = case(eng, 8, 96)
    # the uniform set as a ragged batch: the same bytes
    as_ragged = eng.plan_ragged(list(k["wps"]), VEL, DT, rows=False)
    for name, go, st in configs(96):
        assert same(conf_of_plan(eng, as_ragged, go=go, start=st), k["want"][name]), name
    # missions of 1, 2 and 8 segments side by side
    from oracle import minsnap_oracle as mo
    sets = {1: case(eng, 1, 48)["wps"], 2: mo.synthetic_missions(48, 2), 8: k["wps"]}
    missions = [sets[(1, 2, 8)[b % 3]][b] for b in range(45)]
    with_rows = eng.plan_ragged(missions, VEL, DT)
    free = eng.plan_ragged(missions, VEL, DT, rows=False)
    assert free.traj is None
    rows, ro = with_rows.traj.cpu().numpy(), with_rows.row_offsets.cpu().numpy()
    for name, go, st in configs(45):
        want = conflicts_from_rows(rows, ro, RADIUS, go, st)
        assert same(conf_of_plan(eng, free, go=go, start=st), want), name
        assert same(conf_of_plan(eng, with_rows, go=go, start=st), want), name
        assert same(of_engine(eng.conflicts(free, RADIUS, groups=go, start_rows=st)), want), name
    assert want[0][-1] > 0


# ------------------------------------------------------------------------------------------------------------ 2: tile edges
def test_groups_of_one_tile_one_less_and_one_more(eng):
    from uav_ac.scoring import conflicts_from_rows
    k = case(eng, 8, 96)
    starts = (np.arange(96) % 7) * 23
    for n, go in enumerate(([0, TILE - 1, 96], [0, TILE, 96], [0, TILE + 1, 96], [0, 96 - TILE - 1, 96], [0, 31, 31 + TILE, 96], [0, 32, 96],
                            [0, 5, 10, 10, 74, 75, 96])):
        st = (None, starts)[n % 2]
        got = conf_of_plan(eng, k["free"], go=np.array(go), start=st)
        assert same(got, conflicts_from_rows(k["rows"], k["ro"], RADIUS, go, st)), (go, st is not None)
    # the same groups as batches of their own
    free = k["free"]
    for b0, n in ((0, TILE - 1), (3, TILE), (7, TILE + 1), (31, TILE + 1)):
        got = conf_abi(eng, free.coeffs[b0:b0 + n], free.seg_rows[b0:b0 + n], None, n, 8, DT)
        ro = k["ro"][b0:b0 + n + 1]
        assert same(got, conflicts_from_rows(k["rows"][ro[0]:ro[-1]], ro - ro[0], RADIUS)), (b0, n)


# ------------------------------------------------------------------------------------------------------------ 3: independence
def test_every_launch_shape_and_a_group_alone_give_the_same_bytes(eng):
    from uav_ac import _native as nat
    try:
        for split, slots in ((1, 0), (2, 0), (3, 0), (nat.SEP_MAX_SPLIT, 0), (0, 1), (3, 1), (2, 2), (0, 64)):
            eng.ctx.set_option("separation_split", split)
            eng.ctx.set_option("conflict_slots", slots)                              # 1 slot: the two j-tiles of 96 missions in two rounds
            for m, B in ((8, 96), (8, 37)):
                k = case(eng, m, B)
                for name, go, st in configs(B):
                    assert same(conf_of_plan(eng, k["free"], go=go, start=st), k["want"][name]), (split, slots, m, B, name)
    finally:
        eng.ctx.set_option("separation_split", 0)
        eng.ctx.set_option("conflict_slots", 0)
    with pytest.raises(nat.UavacError):
        eng.ctx.set_option("conflict_slots", 65)
    with pytest.raises(nat.UavacError):
        eng.ctx.set_option("conflict_slots", -1)
    # a group listed alone: the same records, the partners shifted
    k = case(eng, 8, 96)
    free = k["free"]
    name, go, st = configs(96)[1]
    off, d, i = k["want"][name]
    for g in (1, 3):                                                                  # the second and the fourth group
        b0, b1 = int(go[g]), int(go[g + 1])
        alone = conf_abi(eng, free.coeffs[b0:b1], free.seg_rows[b0:b1], None, b1 - b0, 8, DT, start=st[b0:b1])
        e0, e1 = int(off[b0]), int(off[b1])
        assert e1 > e0
        shifted = i[:, e0:e1].copy()
        shifted[PARTNER] -= b0
        assert same(alone, (off[b0:b1 + 1] - e0, d[e0:e1], shifted)), g


# ------------------------------------------------------------------------------------------------ 4: the audit's guarantees
@pytest.mark.parametrize("m, B", SETS)
def test_the_guarantees_against_the_audit(eng, m, B):
    from uav_ac.scoring import conflict_pairs
    k = case(eng, m, B)
    for name, go, st in configs(B):
        a = eng.separation(k["free"], RADIUS, groups=go, start_rows=st)
        cl = eng.conflicts(k["free"], RADIUS, groups=go, start_rows=st)
        sep, partner, row = a.min_distance.cpu().numpy(), a.partner.cpu().numpy(), a.row.cpu().numpy()
        conflicts, first = a.conflicts.cpu().numpy(), a.first_conflict.cpu().numpy()
        off, d, i = of_engine(cl)
        assert off[0] == 0 and np.array_equal(np.diff(off), conflicts) and conflicts.sum() > 0
        for b in range(B):
            e = slice(off[b], off[b + 1])
            if conflicts[b] == 0:
                assert first[b] == -1
                continue
            assert i[FIRST, e].min() == first[b]
            assert min(zip(d[e], i[MIN_ROW, e], i[PARTNER, e])) == (sep[b], row[b], partner[b]), (name, b)
        pairs = conflict_pairs(cl)                                                    # raises if the two directions of a pair disagree
        assert 2 * len(pairs["i"]) == cl.total and (pairs["i"] < pairs["j"]).all()


# ------------------------------------------------------------------------------------------- 5: a hand-made coefficient plan
def test_a_hand_made_plan_with_a_gap_and_a_shared_first_waypoint(eng):
    from uav_ac.scoring import conflicts_from_rows
    # A hovers at (4, 0.25, -3) for 200 rows.  B flies out along y = 0 at 0.1 m per row (80 rows, x = 0 .. 7.9) and back (81 rows, x = 8
    # .. 0): inside A's radius while 0.0625 + (x - 4)^2 < 0.25 <=> 3.6 <= x <= 4.4 -- rows 36 .. 44 and 116 .. 124, more than one chunk
    # of 32 rows apart.  C and D hold the same first waypoint (20, 0, -3) until their starts (rows 10 and 30) and leave at right
    # angles, 0.1 m per row: distance 0 from row 0, inside while 0.1 (k - 10) < 0.5 <=> k <= 14.
    seg = np.zeros((5, 8, 3))
    seg[0, 0] = [4.0, 0.25, -3.0]
    seg[1, 0], seg[1, 1] = [0.0, 0.0, -3.0], [10.0, 0.0, 0.0]
    seg[2, 0], seg[2, 1] = [8.0, 0.0, -3.0], [-10.0, 0.0, 0.0]
    seg[3, 0], seg[3, 1] = [20.0, 0.0, -3.0], [10.0, 0.0, 0.0]
    seg[4, 0], seg[4, 1] = [20.0, 0.0, -3.0], [0.0, 10.0, 0.0]
    seg_rows = np.array([200, 80, 81, 50, 50])
    batch = eng.ragged_from_parts(seg, seg_rows * DT, seg_rows, [1, 2, 1, 1], 10.0, DT)
    start = [0, 0, 10, 30]
    rows, ro = batch.traj.cpu().numpy(), batch.row_offsets.cpu().numpy()
    assert ro.tolist() == [0, 200, 361, 411, 461]
    want = conflicts_from_rows(rows, ro, RADIUS, None, start)
    for got in (conf_of_plan(eng, batch, start=start), of_engine(eng.conflicts(batch, RADIUS, start_rows=start))):
        assert same(got, want)
        off, d, i = got
        assert off.tolist() == [0, 1, 2, 3, 4] and i[PARTNER].tolist() == [1, 0, 3, 2]
        assert i[FIRST].tolist() == [36, 36, 0, 0] and i[LAST].tolist() == [124, 124, 14, 14] and i[INSIDE].tolist() == [18, 18, 15, 15]
        assert (i[INSIDE, :2] < i[LAST, :2] - i[FIRST, :2] + 1).all()
        assert i[MIN_ROW].tolist() == [40, 40, 0, 0] and d.tolist() == [0.25, 0.25, 0.0, 0.0]
    # two airspaces: (A, B) and (C, D) are found all the same, across them nobody is compared
    assert same(conf_of_plan(eng, batch, go=[0, 2, 4], start=start), conflicts_from_rows(rows, ro, RADIUS, [0, 2, 4], start))
    assert conf_of_plan(eng, batch, go=[0, 1, 3, 4], start=start)[0].tolist() == [0, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------- 6: capacity
def test_bounded_writes(eng):
    k = case(eng, 8, 96)
    free = k["free"]
    off, d, i = k["want"]["one group"]
    E = int(off[-1])
    eng.take_flags()
    assert same(conf_of_plan(eng, free), (off, d, i)) and eng.take_flags() == [0, 0, 0, 0]
    # one entry short: flag 2, everything below the capacity as it should be, nothing at or beyond it
    gd, gi = fill_abi(eng, *parts(free), off, E - 1)
    assert eng.take_flags() == [0, 0, 1, 0]
    assert np.array_equal(gd, d[:E - 1]) and np.array_equal(gi, i[:, :E - 1])
    # a capacity far below: whole slices are dropped
    gd, gi = fill_abi(eng, *parts(free), off, 7)
    assert eng.take_flags() == [0, 0, 1, 0] and np.array_equal(gd, d[:7]) and np.array_equal(gi, i[:, :7])
    # buffers larger than the list: the tail stays untouched
    gd, gi = fill_abi(eng, *parts(free), off, E + 50)
    assert eng.take_flags() == [0, 0, 0, 0]
    assert np.array_equal(gd[:E], d) and np.array_equal(gi[:, :E], i) and (gd[E:] == SENT_F).all() and (gi[:, E:] == SENT_I).all()
    # the plan changed between the calls (here: the radius): offsets of 0.5 under a fill at 0.6.  Every mission fills what fits of its
    # own partners at 0.6, ascending, and writes nothing outside its slice; flag 0
    from uav_ac.scoring import conflicts_from_rows
    off6, d6, i6 = conflicts_from_rows(k["rows"], k["ro"], 0.6)
    assert (np.diff(off6) > np.diff(off)).any()
    gd, gi = fill_abi(eng, *parts(free), off, E, radius=0.6)
    assert eng.take_flags() == [1, 0, 0, 0]
    for b in range(96):
        n = min(off[b + 1] - off[b], off6[b + 1] - off6[b])
        assert np.array_equal(gi[:, off[b]:off[b] + n], i6[:, off6[b]:off6[b] + n]), b
        assert np.array_equal(gd[off[b]:off[b] + n], d6[off6[b]:off6[b] + n]), b
        assert (gi[:, off[b] + n:off[b + 1]] == SENT_I).all() and (gd[off[b] + n:off[b + 1]] == SENT_F).all(), b
    # ... and the other way round: fewer partners than the slices hold
    gd, gi = fill_abi(eng, *parts(free), off6, int(off6[-1]), radius=RADIUS)
    assert eng.take_flags() == [1, 0, 0, 0]
    for b in range(96):
        n = off[b + 1] - off[b]
        assert np.array_equal(gi[:, off6[b]:off6[b] + n], i[:, off[b]:off[b + 1]]), b
        assert (gi[:, off6[b] + n:off6[b + 1]] == SENT_I).all() and (gd[off6[b] + n:off6[b + 1]] == SENT_F).all(), b
    # offsets that make no sense write nothing out of bounds (the sentinels around the buffers are checked in fill_abi)
    fill_abi(eng, *parts(free), np.concatenate([off[::-1][:50], off[:47] - 40]), E)
    assert eng.take_flags()[0] == 1


def test_no_entries_and_invalid_arguments(eng):
    import torch
    from uav_ac import _native as nat
    k = case(eng, 8, 37)
    free, B, m = k["free"], 37, 8
    dev = dict(device=eng.device)
    # radius 0: all offsets 0, and the fill with NULL buffers is allowed
    off = offsets_abi(eng, *parts(free), radius=0.0)
    assert off.tolist() == [0] * (B + 1)
    eng.take_flags()
    eng.ctx.call("uavac_minsnap_conflicts_dev", _p(free.coeffs), _p(free.seg_rows), None, B, m, DT, None, 0, None, 0.0, _p(_i64(eng, off)), 0,
                 None, None)
    assert eng.take_flags() == [0, 0, 0, 0]
    po = torch.full((B + 1,), SENT_O, dtype=torch.int64, **dev)
    pd = torch.full((64,), SENT_F, dtype=torch.float64, **dev)
    pi = torch.full((5 * 64,), SENT_I, dtype=torch.int32, **dev)
    go = _i64(eng, [0, 10, B])
    good = dict(coeffs=free.coeffs, seg_rows=free.seg_rows, seg_offsets=None, B=B, m=m, dt=DT, go=go, G=2, start=None, radius=RADIUS,
                po=po, cap=64, pd=pd, pi=pi)
    shared = [dict(coeffs=None), dict(seg_rows=None), dict(po=None), dict(B=0), dict(B=-3), dict(m=0), dict(m=nat.MAX_SEGMENTS + 1),
              dict(dt=0.0), dict(dt=-0.01), dict(dt=math.inf), dict(dt=math.nan), dict(radius=-0.5), dict(radius=math.inf),
              dict(radius=math.nan), dict(G=0), dict(G=-2)]
    fill_only = [dict(cap=-1), dict(pd=None), dict(pi=None), dict(pd=None, pi=None)]
    eng._bind_stream()
    lib = nat.lib()

    def offsets_call(ctx, a):
        return lib.uavac_minsnap_conflict_offsets_dev(ctx, _p(a["coeffs"]), _p(a["seg_rows"]), _p(a["seg_offsets"]), a["B"], a["m"], a["dt"],
                                                      _p(a["go"]), a["G"], _p(a["start"]), a["radius"], _p(a["po"]))

    def fill_call(ctx, a):
        return lib.uavac_minsnap_conflicts_dev(ctx, _p(a["coeffs"]), _p(a["seg_rows"]), _p(a["seg_offsets"]), a["B"], a["m"], a["dt"],
                                               _p(a["go"]), a["G"], _p(a["start"]), a["radius"], _p(a["po"]), a["cap"], _p(a["pd"]), _p(a["pi"]))
    for call, bad in ((offsets_call, shared), (fill_call, shared + fill_only)):
        for change in bad:
            rc = call(eng.ctx._h, {**good, **change})
            assert rc == nat.EINVAL, (change, rc)
            assert (lib.uavac_last_error(eng.ctx._h) or b"") != b"", change
        assert call(None, good) == nat.EINVAL                                        # no context
    torch.cuda.synchronize()
    assert bool((po == SENT_O).all()) and bool((pd == SENT_F).all()) and bool((pi == SENT_I).all())
    # the same calls with nothing wrong go through
    from uav_ac.scoring import conflicts_from_rows
    want = conflicts_from_rows(k["rows"], k["ro"], RADIUS, [0, 10, B])
    assert offsets_call(eng.ctx._h, good) == nat.OK and fill_call(eng.ctx._h, good) == nat.OK
    torch.cuda.synchronize()
    E = int(want[0][-1])
    assert 0 < E <= 64 and np.array_equal(po.cpu().numpy(), want[0])
    assert np.array_equal(pd.cpu().numpy()[:E], want[1]) and np.array_equal(pi.cpu().numpy().reshape(5, 64)[:, :E], want[2])


# ------------------------------------------------------------------------------------------------------------ 7: the oracle
def _stand(rows, ro, start, b, k):
    n = ro[b + 1] - ro[b]
    return rows[ro[b] + np.clip(k - start[b], 0, n - 1), 0:3]


@pytest.mark.parametrize("m, B", SETS)
def test_the_list_against_the_oracle(eng, m, B):
    """Margins of the oracle's nearest pair-row from the radius (CPU check): one group 1.35e-4 / 5.3e-4 / 6.6e-4, groups with staggered
    starts 1.27e-4 / 7.9e-4 / 2.1e-3 for (8, 96) / (8, 37) / (1, 48)."""
    from oracle import c_oracle as cc
    from uav_ac.scoring import conflicts_from_rows
    k = case(eng, m, B)
    ref = cc.plan_threads(k["wps"], VEL, DT)
    rows, ro = ref["rows"], ref["row_offsets"]
    assert np.array_equal(ro, k["ro"])                                                 # row counts are exact
    for name, go, st in configs(B):
        want = conflicts_from_rows(rows, ro, RADIUS, go, st)
        got = conf_of_plan(eng, k["free"], go=go, start=st)
        start = np.zeros(B, dtype=np.int64) if st is None else np.asarray(st, dtype=np.int64)
        # the condition under which the cap on excused differences is 0: no pair-row of the oracle near the radius
        bounds = [0, B] if go is None else list(go)
        margin = np.inf
        for g0, g1 in zip(bounds[:-1], bounds[1:]):
            if g1 - g0 < 2:
                continue
            kk = np.arange(max(start[j] + ro[j + 1] - ro[j] for j in range(g0, g1)))
            P = np.stack([_stand(rows, ro, start, j, kk) for j in range(g0, g1)])
            for a in range(g1 - g0 - 1):
                margin = min(margin, float(np.abs(np.sqrt(((P[a][None] - P[a + 1:]) ** 2).sum(axis=-1)) - RADIUS).min()))
        print(f"conflict list vs oracle m={m} B={B} {name}: {int(want[0][-1])} entries, nearest pair-row {margin:.3e} from the radius")
        assert margin >= RADIUS_MARGIN, margin
        assert np.array_equal(got[0], want[0]) and want[0][-1] > 0
        for r in (PARTNER, FIRST, LAST, INSIDE):
            assert np.array_equal(got[2][r], want[2][r]), (name, r, np.flatnonzero(got[2][r] != want[2][r])[:8])
        err = np.abs(got[1] - want[1])
        print(f"    worst distance error {err.max():.3e}")
        assert (err <= DIST_TOL).all(), err.max()
        owner = np.repeat(np.arange(B), np.diff(got[0]))
        for e in range(len(owner)):                                                   # the reported row: as good as the oracle's minimum
            b, j, kk = int(owner[e]), int(got[2][PARTNER, e]), int(got[2][MIN_ROW, e])
            dist = float(np.sqrt(((_stand(rows, ro, start, b, kk) - _stand(rows, ro, start, j, kk)) ** 2).sum()))
            assert abs(dist - want[1][e]) <= DIST_TOL, (name, e, b, j, kk, dist, want[1][e])
