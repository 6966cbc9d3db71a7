"""The cross conflict list on the GPU (`uavac_minsnap_conflict_against_offsets_dev`, `uavac_minsnap_conflicts_against_dev`,
csrc/minsnap_conflicts_against.hip), through the C ABI and through `Engine.conflicts_against`: per mission of a plan every mission of
its group's committed traffic that comes inside the radius, with when and how near.

The fixture is tests/test_gpu_against.py's (`sides`): of `synthetic_missions(220, 3)` at velocity 3, radius 0.5, start rows (b % 5) * 7,
missions 0 .. 69 are the TRAFFIC -- two j-tiles, the second one holding 6 --, missions 70 .. 219 the PLAN: windows of 64, 64 and 22.
Groups: one on each side, or the plan's GO3 = [0, 63, 128, 150] against the traffic's TGO3 = [0, 0, 65, 70], whose group 0 has no
traffic.  The rule is `uav_ac.scoring.conflicts_against_rows` on the PRODUCT'S OWN ROWS, computed once per configuration; every
comparison is equality, on integers and on the bits of doubles.  There is no tolerance anywhere.
A fixture could pass by being trivial, so before a comparison counts `not_trivial` asserts on the rule's own answer: an entry whose
partner lies in the second j-tile, an owner in the third window, a mission with two or more entries, a pair that parts and meets
again."""
import math

import numpy as np
import pytest

from test_gpu_against import GO3, N_P, N_T, TGO3, sep_against, sides, snapshot, t_args, unchanged
from test_gpu_layer import PAD, SENT_F, SENT_I, _i32, _i64, _p, same_bits
from test_gpu_wide import RADIUS, TILE, case, once, parts

pytestmark = pytest.mark.gpu

DT = 0.02
SENT_O = -5555
PARTNER, FIRST, LAST, INSIDE, MIN_ROW = range(5)
OFFSETS_CALL, FILL_CALL = "uavac_minsnap_conflict_against_offsets_dev", "uavac_minsnap_conflicts_against_dev"


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    e = Engine("cuda:0")
    yield e
    e.ctx.set_option("separation_split", 0)
    e.ctx.set_option("conflict_slots", 0)


def head(eng, plan, traffic, go, tgo, start, tstart, radius, uniform_traffic=None):
    """the leading arguments of both calls, up to and with the radius, and the tensors behind them"""
    co, sr, so, B, m, dt = parts(plan)
    g, s = _i64(eng, go), _i32(eng, start)
    if uniform_traffic is None:
        held, targs = t_args(eng, traffic, tgo, tstart)
    else:                                                    # the traffic as a uniform batch: t_seg_offsets NULL
        tco, tsr, mt = uniform_traffic
        tg, ts = _i64(eng, tgo), _i32(eng, tstart)
        held, targs = (tco, tsr, tg, ts), (_p(tco), _p(tsr), _p(None), int(tco.shape[0]), int(mt), _p(tg), _p(ts))
    return (co, sr, so, g, s, held), (_p(co), _p(sr), _p(so), B, m, dt, _p(g), 0 if go is None else len(go) - 1, *targs, _p(s), float(radius))


def offsets_abi(eng, plan, traffic, go=None, tgo=None, start=None, tstart=None, radius=RADIUS, uniform_traffic=None):
    """the offsets call -> pair_offsets (B + 1,), from the middle of a larger sentinel-filled buffer"""
    import torch
    B = int(plan.B)
    obuf = torch.full((PAD + B + 1 + PAD,), SENT_O, dtype=torch.int64, device=eng.device)
    held, args = head(eng, plan, traffic, go, tgo, start, tstart, radius, uniform_traffic)
    eng._bind_stream()
    eng.ctx.call(OFFSETS_CALL, *args, _p(obuf[PAD:]))
    torch.cuda.synchronize()
    o = obuf.cpu().numpy()
    assert (o[:PAD] == SENT_O).all() and (o[PAD + B + 1:] == SENT_O).all() and not (o[PAD:PAD + B + 1] == SENT_O).any()
    return o[PAD:PAD + B + 1].copy()


def fill_abi(eng, plan, traffic, offsets, capacity, go=None, tgo=None, start=None, tstart=None, radius=RADIUS, uniform_traffic=None):
    """the fill call into the middle of larger sentinel-filled buffers -> (pair_d (capacity,), pair_i (5, capacity)) with the sentinels
    where nothing was written; nothing outside [capacity] / [5][capacity] may be written."""
    import torch
    dbuf = torch.full((PAD + capacity + PAD,), SENT_F, dtype=torch.float64, device=eng.device)
    ibuf = torch.full((PAD + 5 * capacity + PAD,), SENT_I, dtype=torch.int32, device=eng.device)
    o = _i64(eng, offsets)
    held, args = head(eng, plan, traffic, go, tgo, start, tstart, radius, uniform_traffic)
    eng._bind_stream()
    eng.ctx.call(FILL_CALL, *args, _p(o), int(capacity), _p(dbuf[PAD:]), _p(ibuf[PAD:]))
    torch.cuda.synchronize()
    d, i = dbuf.cpu().numpy(), ibuf.cpu().numpy()
    assert (d[:PAD] == SENT_F).all() and (d[PAD + capacity:] == SENT_F).all()
    assert (i[:PAD] == SENT_I).all() and (i[PAD + 5 * capacity:] == SENT_I).all()
    return d[PAD:PAD + capacity].copy(), i[PAD:PAD + 5 * capacity].reshape(5, capacity).copy()


def cross(eng, plan, traffic, **kw):
    """Both calls -> (offsets, pair_d, pair_i); everything inside [0, E) must be written."""
    off = offsets_abi(eng, plan, traffic, **kw)
    E = int(off[-1])
    d, i = fill_abi(eng, plan, traffic, off, E, **kw)
    assert not (d == SENT_F).any() and not (i == SENT_I).any()
    return off, d, i


def of_engine(cl):
    fields = (cl.partner, cl.first_row, cl.last_row, cl.rows_inside, cl.min_row)
    return cl.offsets.cpu().numpy(), cl.min_distance.cpu().numpy(), np.stack([t.cpu().numpy() for t in fields])


def identical(got, want):
    """offsets, the five integer rows, the distances' bits"""
    return (got[0].dtype == want[0].dtype == np.int64 and np.array_equal(got[0], want[0])
            and got[2].dtype == want[2].dtype == np.int32 and got[2].shape == want[2].shape and np.array_equal(got[2], want[2])
            and got[1].dtype == want[1].dtype == np.float64 and same_bits(got[1], want[1]))


def groups_of(grouped):
    return dict(go=GO3, tgo=TGO3) if grouped else {}


def rule(s, grouped, radius=RADIUS):
    """`conflicts_against_rows` on the product's own rows, computed once"""
    from uav_ac.scoring import conflicts_against_rows
    go, tgo = (GO3, TGO3) if grouped else (None, None)
    return once(s, ("cross list", grouped, radius), lambda: conflicts_against_rows(s["prows"], s["pro"], s["trows"], s["tro"], radius, go, tgo,
                                                                                  s["pst"], s["tst"]))


def not_trivial(want):
    off, d, i = want
    owner = np.repeat(np.arange(len(off) - 1), np.diff(off))
    n = dict(entries=int(off[-1]), second_tile=int((i[PARTNER] >= TILE).sum()), third_window=int((owner >= 2 * TILE).sum()),
             several=int((np.diff(off) >= 2).sum()), reentry=int((i[INSIDE] < i[LAST] - i[FIRST] + 1).sum()))
    assert n["second_tile"] > 0 and n["third_window"] > 0 and n["several"] > 0 and n["reentry"] > 0, n
    return n


# ------------------------------------------------------------------------------------------------ 1: the product's own rows
@pytest.mark.parametrize("grouped", (False, True), ids=("one group", "three groups"))
def test_the_cross_list_equals_what_the_products_rows_show(eng, grouped):
    s = sides(eng, DT)
    want = rule(s, grouped)
    if not grouped:
        print("cross list, 150 against 70, one group:", not_trivial(want))
    else:
        assert want[0][-1] > 0 and (want[0][:GO3[1] + 1] == 0).all()                  # group 0 has no traffic
        owner = np.repeat(np.arange(N_P), np.diff(want[0]))
        assert (owner >= 2 * TILE).any() and (want[2][PARTNER] >= TILE).any() and (want[2][PARTNER, owner < GO3[2]] < TGO3[2]).all()
    before = snapshot(s["traffic"]), snapshot(s["plan"])
    eng.take_flags()
    kw = dict(start=s["pst"], tstart=s["tst"], **groups_of(grouped))
    for plan in (s["plan"], s["plan_rows"]):
        assert identical(cross(eng, plan, s["traffic"], **kw), want)
    # the traffic as a uniform batch (t_seg_offsets NULL): the first 70 of the 220 as they were planned
    free = case(eng, 220, DT)["free"]
    assert not hasattr(free, "seg_offsets") and hasattr(s["traffic"], "seg_offsets")
    uniform = (free.coeffs[:N_T], free.seg_rows[:N_T], int(free.m))
    assert identical(cross(eng, s["plan"], None, uniform_traffic=uniform, **kw), want)
    assert eng.take_flags() == [0, 0, 0, 0]
    assert unchanged(s["traffic"], before[0]) and unchanged(s["plan"], before[1])
    # without start rows on either side another list (so the start rows were looked at), and the rule's
    from uav_ac.scoring import conflicts_against_rows
    go, tgo = (GO3, TGO3) if grouped else (None, None)
    plain = conflicts_against_rows(s["prows"], s["pro"], s["trows"], s["tro"], RADIUS, go, tgo)
    assert not identical(plain, want)
    assert identical(cross(eng, s["plan"], s["traffic"], **groups_of(grouped)), plain)


# ------------------------------------------------------------------------------------------------ 2: independence of the launch shape
def test_every_launch_shape_and_a_group_alone_give_the_same_bytes(eng):
    from uav_ac import _native as nat
    s = sides(eng, DT)
    not_trivial(rule(s, False))
    try:
        for split, slots in ((1, 0), (2, 0), (nat.SEP_MAX_SPLIT, 0), (0, 1), (2, 1), (nat.SEP_MAX_SPLIT, 1), (0, 64)):
            eng.ctx.set_option("separation_split", split)
            eng.ctx.set_option("conflict_slots", slots)                              # 1 slot: the traffic's two j-tiles in two rounds
            for grouped in (False, True):
                got = cross(eng, s["plan"], s["traffic"], start=s["pst"], tstart=s["tst"], **groups_of(grouped))
                assert identical(got, rule(s, grouped)), (split, slots, grouped)
    finally:
        eng.ctx.set_option("separation_split", 0)
        eng.ctx.set_option("conflict_slots", 0)
    # a group of both sides listed alone: the same records, the partners renumbered
    off, d, i = rule(s, True)
    for g in (1, 2):
        b0, b1, t0, t1 = int(GO3[g]), int(GO3[g + 1]), int(TGO3[g]), int(TGO3[g + 1])
        plan, traffic = eng.take(s["plan"], np.arange(b0, b1)), eng.take(s["traffic"], np.arange(t0, t1))
        alone = cross(eng, plan, traffic, start=s["pst"][b0:b1], tstart=s["tst"][t0:t1])
        e0, e1 = int(off[b0]), int(off[b1])
        assert e1 > e0
        shifted = i[:, e0:e1].copy()
        shifted[PARTNER] -= t0
        assert identical(alone, (off[b0:b1 + 1] - e0, d[e0:e1], shifted)), g


# ------------------------------------------------------------------------------------------------ 3: the cross audit's guarantees
@pytest.mark.parametrize("grouped", (False, True), ids=("one group", "three groups"))
def test_the_guarantees_against_the_cross_audit(eng, grouped):
    s = sides(eng, DT)
    kw = dict(start=s["pst"], tstart=s["tst"], **groups_of(grouped))
    sep, isep = sep_against(eng, s["plan"], s["traffic"], **kw)
    off, d, i = cross(eng, s["plan"], s["traffic"], **kw)
    assert off[0] == 0 and np.array_equal(np.diff(off), isep[2]) and isep[2].sum() > 0
    if not grouped:
        not_trivial((off, d, i))
    for b in range(N_P):
        e = slice(off[b], off[b + 1])
        if off[b] == off[b + 1]:
            assert isep[3, b] == -1
            continue
        assert i[FIRST, e].min() == isep[3, b]
        least = min(zip(d[e], i[MIN_ROW, e], i[PARTNER, e]))
        assert same_bits(np.float64(least[0]), sep[b]) and (least[1], least[2]) == (isep[1, b], isep[0, b]), b


# ------------------------------------------------------------------------------------------------ 4: the sides swapped
@pytest.mark.parametrize("grouped", (False, True), ids=("one group", "three groups"))
def test_the_sides_swapped_give_the_transpose(eng, grouped):
    from uav_ac.scoring import conflicts_transposed
    s = sides(eng, DT)
    first = cross(eng, s["plan"], s["traffic"], start=s["pst"], tstart=s["tst"], **groups_of(grouped))
    swapped = cross(eng, s["traffic"], s["plan"], start=s["tst"], tstart=s["pst"], **(dict(go=TGO3, tgo=GO3) if grouped else {}))
    if not grouped:
        not_trivial(first)
    assert first[0][-1] > 0 and identical(swapped, conflicts_transposed(first, N_T))
    assert identical(first, conflicts_transposed(swapped, N_P))
    if not grouped:                                          # here the PLAN is the partners' side: three j-tiles, the owners in two windows
        assert (swapped[2][PARTNER] >= 2 * TILE).any() and (np.flatnonzero(np.diff(swapped[0])) >= TILE).any()


# ------------------------------------------------------------------------------------------------ 5: the list of the concatenation
def test_the_cross_entries_of_the_list_of_the_concatenation(eng):
    s = sides(eng, DT)
    both = eng.concat([s["traffic"], s["plan"]])
    off, d, i = of_engine(eng.conflicts(both, RADIUS, start_rows=np.concatenate([s["tst"], s["pst"]])))
    owner = np.repeat(np.arange(N_T + N_P), np.diff(off))
    keep = (owner >= N_T) & (i[PARTNER] < N_T)
    assert keep.any() and ((owner >= N_T) & (i[PARTNER] >= N_T)).any() and ((owner < N_T) & (i[PARTNER] < N_T)).any()
    counts = np.bincount(owner[keep] - N_T, minlength=N_P)
    want = (np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), d[keep], np.ascontiguousarray(i[:, keep]))
    not_trivial(want)
    assert identical(cross(eng, s["plan"], s["traffic"], start=s["pst"], tstart=s["tst"]), want)


# ------------------------------------------------------------------------------------------------ 6: the horizon covers both sides
def test_a_pair_that_meets_after_the_plan_missions_own_last_row_and_its_mirror(eng):
    from uav_ac.scoring import conflicts_against_rows
    # Mission A, one segment of 20 rows, flies from x = 0 along y = 0 at 0.1 m per row and ends at P = (1.9, 0, -3).  Mission L, one
    # segment of 40 rows with start row 50, flies from x = 5.85 back along y = 0 at 0.1 m per row and ends 0.05 m from P: it is inside
    # A's radius of 0.5 from its own row 35 on (x = 2.35; row 34: x = 2.45), clock rows 85 .. 89 -- long after A's own last clock row,
    # 19 -- and nearest on its last.  The horizon is 90, L's end.
    seg = np.zeros((2, 8, 3))
    seg[0, 0], seg[0, 1] = [0.0, 0.0, -3.0], [0.1 / DT, 0.0, 0.0]
    seg[1, 0], seg[1, 1] = [5.85, 0.0, -3.0], [-0.1 / DT, 0.0, 0.0]
    made = [eng.ragged_from_parts(seg[q:q + 1], np.array([n * DT]), np.array([n]), [1], 5.0, DT) for q, n in ((0, 20), (1, 40))]
    rows = [b.traj.cpu().numpy()[:, 0:3] for b in made]
    assert [len(r) for r in rows] == [20, 40]
    (a, ra), (late, rl) = zip(made, rows)
    eng.take_flags()
    for plan, prow, pstart, traffic, trow, tstart in ((a, ra, [0], late, rl, [50]), (late, rl, [50], a, ra, [0])):      # ... and the mirror image
        want = conflicts_against_rows(prow, [0, len(prow)], trow, [0, len(trow)], RADIUS, start_rows=pstart, traffic_start_rows=tstart)
        assert want[0].tolist() == [0, 1] and want[2][:, 0].tolist() == [0, 85, 89, 5, 89]
        assert want[2][FIRST, 0] > 0 + 20                    # beyond S + N of the short mission, which is held on its last row
        got = cross(eng, plan, traffic, start=pstart, tstart=tstart)
        assert identical(got, want)
        assert identical(of_engine(eng.conflicts_against(plan, traffic, RADIUS, start_rows=pstart, traffic_start_rows=tstart)), want)
        sep, isep = sep_against(eng, plan, traffic, start=pstart, tstart=tstart)
        assert isep[:, 0].tolist() == [0, 89, 1, 85, 1] and same_bits(sep, want[1])
    assert eng.take_flags() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 7: capacity
def test_bounded_writes(eng):
    s = sides(eng, DT)
    off, d, i = rule(s, False)
    not_trivial((off, d, i))
    E = int(off[-1])
    kw = dict(start=s["pst"], tstart=s["tst"])
    eng.take_flags()
    assert identical(cross(eng, s["plan"], s["traffic"], **kw), (off, d, i)) and eng.take_flags() == [0, 0, 0, 0]
    # one entry short: flag 2, everything below the capacity as it should be, nothing at or beyond it (the padding: fill_abi)
    gd, gi = fill_abi(eng, s["plan"], s["traffic"], off, E - 1, **kw)
    assert eng.take_flags() == [0, 0, 1, 0]
    assert same_bits(gd, d[:E - 1]) and np.array_equal(gi, i[:, :E - 1])
    # a capacity far below: whole slices are dropped
    gd, gi = fill_abi(eng, s["plan"], s["traffic"], off, 7, **kw)
    assert eng.take_flags() == [0, 0, 1, 0] and same_bits(gd, d[:7]) and np.array_equal(gi, i[:, :7])
    # buffers larger than the list: the tail stays untouched
    gd, gi = fill_abi(eng, s["plan"], s["traffic"], off, E + 50, **kw)
    assert eng.take_flags() == [0, 0, 0, 0]
    assert same_bits(gd[:E], d) and np.array_equal(gi[:, :E], i) and (gd[E:] == SENT_F).all() and (gi[:, E:] == SENT_I).all()
    # offsets of another radius: every mission fills what fits of its own partners, ascending, and nothing outside its slice; flag 0
    off6, d6, i6 = rule(s, False, 0.6)
    assert (np.diff(off6) > np.diff(off)).any()
    gd, gi = fill_abi(eng, s["plan"], s["traffic"], off, E, radius=0.6, **kw)
    assert eng.take_flags() == [1, 0, 0, 0]
    for b in range(N_P):
        n = min(off[b + 1] - off[b], off6[b + 1] - off6[b])
        assert np.array_equal(gi[:, off[b]:off[b] + n], i6[:, off6[b]:off6[b] + n]), b
        assert same_bits(gd[off[b]:off[b] + n], d6[off6[b]:off6[b] + n]), b
        assert (gi[:, off[b] + n:off[b + 1]] == SENT_I).all() and (gd[off[b] + n:off[b + 1]] == SENT_F).all(), b
    # ... and the other way round: fewer partners than the slices hold
    gd, gi = fill_abi(eng, s["plan"], s["traffic"], off6, int(off6[-1]), **kw)
    assert eng.take_flags() == [1, 0, 0, 0]
    for b in range(N_P):
        n = off[b + 1] - off[b]
        assert np.array_equal(gi[:, off6[b]:off6[b] + n], i[:, off[b]:off[b + 1]]), b
        assert (gi[:, off6[b] + n:off6[b + 1]] == SENT_I).all() and (gd[off6[b] + n:off6[b + 1]] == SENT_F).all(), b
    # offsets that make no sense write nothing out of bounds (the sentinels around the buffers are checked in fill_abi)
    fill_abi(eng, s["plan"], s["traffic"], np.concatenate([off[::-1][:80], off[:71] - 40]), E, **kw)
    assert eng.take_flags()[0] == 1


# ------------------------------------------------------------------------------------------------ 8: nothing to list, and what is refused
def test_no_entries_and_invalid_arguments(eng, monkeypatch):
    import torch
    from uav_ac import _native as nat
    s = sides(eng, DT)
    plan, traffic = s["plan"], s["traffic"]
    # a radius below every distance: all offsets 0, the fill with NULL buffers is allowed, and the engine skips it
    off = offsets_abi(eng, plan, traffic, radius=0.0)
    assert off.tolist() == [0] * (N_P + 1)
    eng.take_flags()
    held, args = head(eng, plan, traffic, None, None, None, None, 0.0)
    eng.ctx.call(FILL_CALL, *args, _p(_i64(eng, off)), 0, None, None)
    assert eng.take_flags() == [0, 0, 0, 0]
    calls = []
    real = eng.ctx.call
    monkeypatch.setattr(eng.ctx, "call", lambda name, *a: (calls.append(name) if "conflict" in name else None, real(name, *a))[1])
    none = eng.conflicts_against(plan, traffic, 0.0)
    assert calls == [OFFSETS_CALL]
    assert none.total == 0 and none.partner.shape == (0,) and none.min_distance.shape == (0,) and none.block.shape == (5, 0)
    assert none.offsets.cpu().numpy().tolist() == [0] * (N_P + 1)
    some = eng.conflicts_against(plan, traffic, RADIUS)
    assert calls == [OFFSETS_CALL, OFFSETS_CALL, FILL_CALL] and some.total > 0
    monkeypatch.undo()
    # what is refused, before anything is enqueued
    dev = dict(device=eng.device)
    po = torch.full((N_P + 1,), SENT_O, dtype=torch.int64, **dev)
    pd = torch.full((64,), SENT_F, dtype=torch.float64, **dev)
    pi = torch.full((5 * 64,), SENT_I, dtype=torch.int32, **dev)
    co, sr, so, B, m, dt = parts(plan)
    tco, tsr, tso, Bt, mt, _ = parts(traffic)
    go, tgo = _i64(eng, GO3), _i64(eng, TGO3)
    good = dict(coeffs=co, seg_rows=sr, seg_offsets=so, B=B, m=m, dt=dt, go=go, G=3, t_coeffs=tco, t_seg_rows=tsr, t_seg_offsets=tso, Bt=Bt, mt=mt,
                tgo=tgo, tstart=None, start=None, radius=RADIUS, po=po, cap=64, pd=pd, pi=pi)
    shared = [dict(coeffs=None), dict(seg_rows=None), dict(po=None), dict(B=0), dict(B=-3), dict(m=0), dict(m=nat.MAX_SEGMENTS + 1),
              dict(dt=0.0), dict(dt=-0.01), dict(dt=math.inf), dict(dt=math.nan), dict(radius=-0.5), dict(radius=math.inf),
              dict(radius=math.nan), dict(G=0), dict(G=-2),
              dict(t_coeffs=None), dict(t_seg_rows=None), dict(Bt=0), dict(Bt=-1), dict(mt=0), dict(mt=nat.MAX_SEGMENTS + 1),
              dict(go=None), dict(tgo=None)]                 # offsets on one side only
    fill_only = [dict(cap=-1), dict(pd=None), dict(pi=None), dict(pd=None, pi=None)]
    eng._bind_stream()
    lib = nat.lib()

    def leading(a):
        return (_p(a["coeffs"]), _p(a["seg_rows"]), _p(a["seg_offsets"]), a["B"], a["m"], a["dt"], _p(a["go"]), a["G"], _p(a["t_coeffs"]),
                _p(a["t_seg_rows"]), _p(a["t_seg_offsets"]), a["Bt"], a["mt"], _p(a["tgo"]), _p(a["tstart"]), _p(a["start"]), a["radius"])

    def offsets_call(ctx, a):
        return lib.uavac_minsnap_conflict_against_offsets_dev(ctx, *leading(a), _p(a["po"]))

    def fill_call(ctx, a):
        return lib.uavac_minsnap_conflicts_against_dev(ctx, *leading(a), _p(a["po"]), a["cap"], _p(a["pd"]), _p(a["pi"]))
    for call, bad in ((offsets_call, shared), (fill_call, shared + fill_only)):
        for change in bad:
            rc = call(eng.ctx._h, {**good, **change})
            assert rc == nat.EINVAL, (change, rc)
            assert (lib.uavac_last_error(eng.ctx._h) or b"") != b"", change
        assert call(None, good) == nat.EINVAL                                        # no context
    torch.cuda.synchronize()
    assert bool((po == SENT_O).all()) and bool((pd == SENT_F).all()) and bool((pi == SENT_I).all())
    # the same calls with nothing wrong go through
    assert offsets_call(eng.ctx._h, good) == nat.OK
    torch.cuda.synchronize()
    assert po[0].item() == 0 and bool((po != SENT_O).all())


# ------------------------------------------------------------------------------------------------ 9: the engine
def test_engine_conflicts_against(eng):
    s = sides(eng, DT)
    before = snapshot(s["traffic"]), snapshot(s["plan"])
    not_trivial(rule(s, False))
    eng.take_flags()
    for grouped in (False, True):
        kw = dict(groups=GO3, traffic_groups=TGO3) if grouped else {}
        for plan in (s["plan"], s["plan_rows"]):
            cl = eng.conflicts_against(plan, s["traffic"], RADIUS, start_rows=s["pst"], traffic_start_rows=s["tst"], **kw)
            assert cl.offsets.is_cuda and cl.min_distance.is_cuda and cl.partner.is_cuda
            want = rule(s, grouped)
            assert cl.total == int(want[0][-1]) and cl.block.shape == (5, cl.total)
            assert identical(of_engine(cl), want)
            assert identical(of_engine(cl), cross(eng, plan, s["traffic"], start=s["pst"], tstart=s["tst"], **groups_of(grouped)))
    assert eng.take_flags() == [0, 0, 0, 0]
    assert unchanged(s["traffic"], before[0]) and unchanged(s["plan"], before[1])
    # the transpose takes the engine's list as it is
    from uav_ac.scoring import conflicts_transposed
    assert identical(conflicts_transposed(cl, N_T), conflicts_transposed(of_engine(cl), N_T))
    other_dt = sides(eng, 0.04)["traffic"]
    for bad in (dict(traffic=other_dt), dict(groups=GO3), dict(traffic_groups=TGO3), dict(groups=GO3, traffic_groups=[0, N_T]),
                dict(start_rows=np.zeros(5)), dict(traffic_start_rows=np.zeros(5))):
        with pytest.raises(ValueError):
            eng.conflicts_against(**{**dict(plan=s["plan"], traffic=s["traffic"], radius=RADIUS), **bad})
