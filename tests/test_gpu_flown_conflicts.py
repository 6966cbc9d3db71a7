"""The conflict list of a flight on the GPU (`uavac_flown_conflict_offsets_dev`, `uavac_flown_conflicts_dev`, csrc/flown_conflicts.hip),
through the C ABI and `Engine.flown_conflicts`: the flown separation audit's conflict graph in CSR form -- per vehicle every partner of
its group that the flight brought inside the radius, with the first and the last tick inside, the ticks inside, and the pair's closest
approach and its tick -- from the positions in a state log.

Everything is exact, there is no tolerance anywhere: `uav_ac.scoring.conflicts_from_log` on the same log is the rule, the kernels form
d^2 = (dx dx + dy dy) + dz dz without contraction, and every reduction is a lexicographic minimum, an integer sum, a minimum or a maximum.
  * The seeded synthetic logs of tests/test_gpu_flown_separation.py (tests/flown_conflicts_ref.py: the same recipe and seeds): a grid of
    0.125, so ties between ticks are real; 193 vehicles in groups of 63, 64, 65 and 1 (window and j-tile are 64 wide), 1, 33 and 100
    ticks (a chunk is 32 ticks, a wavefront's share 8), the pitches 193 and 208, one vehicle NaN at some ticks and one throughout.
  * Against `Engine.flown_separation` on the same logs the three identities of the header hold.
  * Every launch shape ("separation_split" x "conflict_slots"), one airspace of all, a group listed alone.
  * The bounds of the fill: capacities, offsets from another radius, offsets that make no sense.
  * A real flight: the (8, 96) set staggered, delayed, flown with a state log for 2 000 ticks."""
import ctypes as C
import math

import numpy as np
import pytest

from flown_conflicts_ref import B, FIGURES, FIRST, GO, INSIDE, LAST, MIN_TICK, NAN_ALWAYS, PARTNER, RADIUS, figures, synthetic

pytestmark = pytest.mark.gpu

SENT_F, SENT_I, SENT_O, PAD = -1.2345e300, -7777, -5555, 96


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


_DEV = {}


def on_device(eng, log, pitch):
    """A host log (K, 13, n) laid out at `pitch` on the device (the columns past n hold vehicles that stand in the middle of the box:
    reading one would show); uploaded once per log and pitch."""
    import torch
    key = (id(log), pitch)
    if key not in _DEV:
        K, _, n = log.shape
        wide = np.full((K, 13, pitch), 1.5)
        wide[:, :, :n] = log
        _DEV[key] = (log, torch.as_tensor(wide).to(eng.device))      # (the host log is kept: its id stays its own)
    return _DEV[key][1]


def offsets_abi(eng, log, pitch, go=None, radius=RADIUS):
    """uavac_flown_conflict_offsets_dev -> pair_offsets (n + 1,) as NumPy, from the middle of a larger sentinel-filled buffer."""
    import torch
    K, _, n = log.shape
    dev, g = on_device(eng, log, pitch), _i64(eng, go)
    obuf = torch.full((PAD + n + 1 + PAD,), SENT_O, dtype=torch.int64, device=eng.device)
    eng._bind_stream()
    eng.ctx.call("uavac_flown_conflict_offsets_dev", _p(dev), K, n, pitch, _p(g), 0 if go is None else len(go) - 1, float(radius),
                 _p(obuf[PAD:]))
    torch.cuda.synchronize()
    o = obuf.cpu().numpy()
    assert (o[:PAD] == SENT_O).all() and (o[PAD + n + 1:] == SENT_O).all() and not (o[PAD:PAD + n + 1] == SENT_O).any()
    return o[PAD:PAD + n + 1].copy()


def fill_abi(eng, log, pitch, offsets, capacity, go=None, radius=RADIUS):
    """uavac_flown_conflicts_dev into the middle of larger sentinel-filled buffers -> (pair_d (capacity,), pair_i (5, capacity)) as NumPy
    with the sentinels where nothing was written; nothing outside [capacity] / [5][capacity] may be written."""
    import torch
    K, _, n = log.shape
    dev, g, o = on_device(eng, log, pitch), _i64(eng, go), _i64(eng, offsets)
    dbuf = torch.full((PAD + capacity + PAD,), SENT_F, dtype=torch.float64, device=eng.device)
    ibuf = torch.full((PAD + 5 * capacity + PAD,), SENT_I, dtype=torch.int32, device=eng.device)
    eng._bind_stream()
    eng.ctx.call("uavac_flown_conflicts_dev", _p(dev), K, n, pitch, _p(g), 0 if go is None else len(go) - 1, float(radius), _p(o),
                 int(capacity), _p(dbuf[PAD:]), _p(ibuf[PAD:]))
    torch.cuda.synchronize()
    d, i = dbuf.cpu().numpy(), ibuf.cpu().numpy()
    assert (d[:PAD] == SENT_F).all() and (d[PAD + capacity:] == SENT_F).all()
    assert (i[:PAD] == SENT_I).all() and (i[PAD + 5 * capacity:] == SENT_I).all()
    return d[PAD:PAD + capacity].copy(), i[PAD:PAD + 5 * capacity].reshape(5, capacity).copy()


def conf_abi(eng, log, pitch, go=None, radius=RADIUS):
    """Both calls -> (offsets, pair_d, pair_i) as NumPy; everything inside [0, E) must be written."""
    off = offsets_abi(eng, log, pitch, go, radius)
    E = int(off[-1])
    d, i = fill_abi(eng, log, pitch, off, E, go, radius)
    assert not (d == SENT_F).any() and not (i == SENT_I).any()
    return off, d, i


def of_engine(cl):
    """A ConflictList -> (offsets, pair_d, pair_i) as NumPy"""
    fields = (cl.partner, cl.first_row, cl.last_row, cl.rows_inside, cl.min_row)
    return cl.offsets.cpu().numpy(), cl.min_distance.cpu().numpy(), np.stack([t.cpu().numpy() for t in fields])


def same(got, want):
    return all(g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g.view(np.int64) if g.dtype == np.float64 else g,
                                                                            w.view(np.int64) if w.dtype == np.float64 else w)
               for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ 1: synthetic logs
@pytest.mark.parametrize("pitch", (193, 208))
@pytest.mark.parametrize("K", (1, 33, 100))
def test_both_calls_equal_the_rule_on_synthetic_logs(eng, K, pitch):
    log, want, _ = synthetic(K)
    got = conf_abi(eng, log, pitch, GO)
    assert same(got, want), (got[0][-1], want[0][-1])
    # the set cannot go trivial: many entries, incursions with gaps, minima tied between ticks, partners in both j-tiles of the 65-group
    assert figures(log, want)[:len(FIGURES[K])] == FIGURES[K]
    off, d, i = want
    assert off[NAN_ALWAYS + 1] == off[NAN_ALWAYS] and not (i[PARTNER] == NAN_ALWAYS).any()      # lists nothing, listed by nobody
    assert off[B] == off[B - 1]                                                                  # the group of one


# ------------------------------------------------------------------------------------------------ 2: the audit's guarantees
@pytest.mark.parametrize("K", (1, 33, 100))
def test_the_guarantees_against_the_flown_audit(eng, K):
    from uav_ac.scoring import conflict_pairs
    log, want, _ = synthetic(K)
    slog = on_device(eng, log, 208)[:, :, :B]
    a = eng.flown_separation(slog, RADIUS, GO)
    cl = eng.flown_conflicts(slog, RADIUS, GO)
    assert cl.offsets.is_cuda and cl.min_distance.is_cuda and cl.partner.is_cuda and cl.block.shape == (5, cl.total)
    off, d, i = of_engine(cl)
    assert same((off, d, i), want)
    sep, partner, tick = a.min_distance.cpu().numpy(), a.partner.cpu().numpy(), a.row.cpu().numpy()
    conflicts, first = a.conflicts.cpu().numpy(), a.first_conflict.cpu().numpy()
    assert off[0] == 0 and np.array_equal(np.diff(off), conflicts) and conflicts.sum() > 0
    for b in range(B):
        e = slice(off[b], off[b + 1])
        if conflicts[b] == 0:
            assert first[b] == -1
            continue
        assert i[FIRST, e].min() == first[b]
        assert min(zip(d[e], i[MIN_TICK, e], i[PARTNER, e])) == (sep[b], tick[b], partner[b]), b
    pairs = conflict_pairs(cl)                                                        # raises if the two directions of a pair disagree
    assert 2 * len(pairs["i"]) == cl.total and (pairs["i"] < pairs["j"]).all()


# ------------------------------------------------------------------------------------------------ 3: launch shapes
def test_every_launch_shape_one_airspace_and_a_group_alone_give_the_same_bytes(eng):
    from uav_ac.scoring import conflicts_from_log
    log, want, _ = synthetic(100)
    one = conflicts_from_log(log, RADIUS)                                             # all 193 as one airspace: four j-tiles
    assert one[0][-1] > want[0][-1]
    try:
        for split in (0, 1, 3, 64):
            for slots in (0, 1, 2, 64):                                               # 1 slot: the 65-group needs two rounds, the airspace four
                eng.ctx.set_option("separation_split", split)
                eng.ctx.set_option("conflict_slots", slots)
                assert same(conf_abi(eng, log, 193, GO), want), (split, slots)
                assert same(conf_abi(eng, log, 208), one), (split, slots)
    finally:
        eng.ctx.set_option("separation_split", 0)
        eng.ctx.set_option("conflict_slots", 0)
    # groups 1 and 2 cut out and listed alone: the same records, the partners shifted
    off, d, i = want
    for g in (1, 2):
        lo, hi = int(GO[g]), int(GO[g + 1])
        alone = conf_abi(eng, np.ascontiguousarray(log[:, :, lo:hi]), hi - lo)
        e0, e1 = int(off[lo]), int(off[hi])
        assert e1 > e0
        shifted = i[:, e0:e1].copy()
        shifted[PARTNER] -= lo
        assert same(alone, (off[lo:hi + 1] - e0, d[e0:e1], shifted)), g
    # radius 0: all offsets 0, and the fill with NULL buffers is allowed
    zero = offsets_abi(eng, log, 193, GO, radius=0.0)
    assert zero.tolist() == [0] * (B + 1)
    eng.take_flags()
    eng.ctx.call("uavac_flown_conflicts_dev", _p(on_device(eng, log, 193)), 100, B, 193, _p(_i64(eng, GO)), len(GO) - 1, 0.0,
                 _p(_i64(eng, zero)), 0, None, None)
    assert eng.take_flags() == [0, 0, 0, 0]
    none = eng.flown_conflicts(on_device(eng, log, 193), 0.0, GO)
    assert none.total == 0 and none.partner.shape == (0,) and none.min_distance.shape == (0,) and none.block.shape == (5, 0)


# ------------------------------------------------------------------------------------------------ 4: bounded writes
def test_bounded_writes(eng):
    from uav_ac.scoring import conflicts_from_log
    log, (off, d, i), _ = synthetic(33)
    E = int(off[-1])
    eng.take_flags()
    assert same(conf_abi(eng, log, 208, GO), (off, d, i)) and eng.take_flags() == [0, 0, 0, 0]
    # one entry short: flag 2, everything below the capacity as it should be, nothing at or beyond it
    gd, gi = fill_abi(eng, log, 208, off, E - 1, GO)
    assert eng.take_flags() == [0, 0, 1, 0]
    assert np.array_equal(gd, d[:E - 1]) and np.array_equal(gi, i[:, :E - 1])
    # a capacity far below: whole slices are dropped
    gd, gi = fill_abi(eng, log, 208, off, 7, GO)
    assert eng.take_flags() == [0, 0, 1, 0] and np.array_equal(gd, d[:7]) and np.array_equal(gi, i[:, :7])
    # buffers larger than the list: the tail stays untouched
    gd, gi = fill_abi(eng, log, 208, off, E + 50, GO)
    assert eng.take_flags() == [0, 0, 0, 0]
    assert np.array_equal(gd[:E], d) and np.array_equal(gi[:, :E], i) and (gd[E:] == SENT_F).all() and (gi[:, E:] == SENT_I).all()
    # the radius changed between the calls: offsets of 0.5 under a fill at 0.6.  Every vehicle fills what fits of its own partners at
    # 0.6, ascending, and writes nothing outside its slice; flag 0
    off6, d6, i6 = conflicts_from_log(log, 0.6, GO)
    assert (np.diff(off6) > np.diff(off)).any()
    gd, gi = fill_abi(eng, log, 208, off, E, GO, radius=0.6)
    assert eng.take_flags() == [1, 0, 0, 0]
    for b in range(B):
        n = min(off[b + 1] - off[b], off6[b + 1] - off6[b])
        assert np.array_equal(gi[:, off[b]:off[b] + n], i6[:, off6[b]:off6[b] + n]), b
        assert np.array_equal(gd[off[b]:off[b] + n], d6[off6[b]:off6[b] + n]), b
        assert (gi[:, off[b] + n:off[b + 1]] == SENT_I).all() and (gd[off[b] + n:off[b + 1]] == SENT_F).all(), b
    # ... and the other way round: fewer partners than the slices hold
    gd, gi = fill_abi(eng, log, 208, off6, int(off6[-1]), GO, radius=RADIUS)
    assert eng.take_flags() == [1, 0, 0, 0]
    for b in range(B):
        n = off[b + 1] - off[b]
        assert np.array_equal(gi[:, off6[b]:off6[b] + n], i[:, off[b]:off[b + 1]]), b
        assert np.array_equal(gd[off6[b]:off6[b] + n], d[off[b]:off[b + 1]]), b
        assert (gi[:, off6[b] + n:off6[b + 1]] == SENT_I).all() and (gd[off6[b] + n:off6[b + 1]] == SENT_F).all(), b
    # offsets that make no sense write nothing out of bounds (the sentinels around the buffers are checked in fill_abi)
    fill_abi(eng, log, 208, np.concatenate([off[::-1][:100], off[:94] - 40]), E, GO)
    assert eng.take_flags()[0] == 1


# ------------------------------------------------------------------------------------------------ 5: a real flight
def test_flown_conflicts_of_a_real_flight_equal_the_rule_on_the_downloaded_log(eng):
    import torch
    from oracle import minsnap_oracle as mo
    from uav_ac.scoring import conflict_diff, conflicts_from_log
    plan = eng.plan(mo.synthetic_missions(96, 8), 3.0, 0.01, rows=False)
    stag = eng.stagger(plan, RADIUS, 32)
    K = 2000
    for what, flown_plan in (("staggered", eng.delay(plan, stag.start_rows)), ("not staggered", plan)):
        fleet = eng.fleet(flown_plan)
        slog, _ = fleet.rollout(K, state_log=True, log_pitch=112)
        assert tuple(slog.shape) == (K, 13, 96) and slog.stride(1) == 112 and not slog.is_contiguous()
        cl = eng.flown_conflicts(slog, RADIUS, 32)
        if cl.total:                                         # (the staggered flight if it lists anything: the test cannot go empty)
            break
    assert cl.total > 0
    want = conflicts_from_log(slog.cpu().numpy(), RADIUS, np.arange(0, 97, 32))
    assert same(of_engine(cl), want), (cl.total, want[0][-1])
    dense = eng.flown_conflicts(slog.contiguous(), RADIUS, 32)
    assert torch.equal(dense.offsets, cl.offsets) and torch.equal(dense.block, cl.block) and torch.equal(dense.min_distance, cl.min_distance)
    assert torch.equal(cl.partner, cl.block[0]) and torch.equal(cl.min_row, cl.block[4])
    audit = eng.flown_separation(slog, RADIUS, 32)
    assert torch.equal(cl.offsets[1:] - cl.offsets[:-1], audit.conflicts.to(torch.int64))
    diff = conflict_diff(eng.conflicts(flown_plan, RADIUS, 32), cl, fleet.vehicle.inner_per_outer)
    print(f"flown conflict list of the {what} (8, 96) flight: {cl.total // 2} pairs inside {RADIUS} m; against the plan's list "
          f"{len(diff['both'])} in both, {len(diff['only_planned'])} only planned, {len(diff['only_flown'])} only flown; first ticks "
          f"(flown, planned) of those in both: {list(zip(diff['flown_first_tick'].tolist(), diff['planned_first_tick'].tolist()))[:6]}")


# ------------------------------------------------------------------------------------------------ 6: refusals
def test_mismatched_logs_and_bad_arguments_are_refused(eng):
    import torch
    from uav_ac import _native as nat
    from uav_ac.scoring import conflicts_from_log
    host, _, _ = synthetic(33)
    host = np.ascontiguousarray(host[:, :, :37])             # the first 37 vehicles of the 63-group
    log = torch.as_tensor(host).to(eng.device)
    eng.flown_conflicts(log, RADIUS)                         # (the well-formed one goes through)
    for bad in (log.float(), log[:, :12], log.permute(0, 2, 1), log[:, :, ::2], log[::2], log.cpu(), log[0], log.cpu().numpy()):
        with pytest.raises(ValueError):
            eng.flown_conflicts(bad, RADIUS)
    with pytest.raises(ValueError):
        eng.flown_conflicts(log, RADIUS, groups=0)
    K, n = 33, 37
    dev = dict(device=eng.device)
    po = torch.full((n + 1,), SENT_O, dtype=torch.int64, **dev)
    pd = torch.full((1024,), SENT_F, dtype=torch.float64, **dev)
    pi = torch.full((5 * 1024,), SENT_I, dtype=torch.int32, **dev)
    go = _i64(eng, [0, 10, n])
    good = dict(log=log, K=K, B=n, pitch=n, go=go, G=2, radius=RADIUS, po=po, cap=1024, pd=pd, pi=pi)
    shared = [dict(log=None), dict(po=None), dict(K=0), dict(K=-1), dict(B=0), dict(B=-3), dict(pitch=n - 1), dict(radius=-0.5),
              dict(radius=math.inf), dict(radius=math.nan), dict(G=0), dict(G=-2)]
    fill_only = [dict(cap=-1), dict(pd=None), dict(pi=None), dict(pd=None, pi=None)]
    eng._bind_stream()
    lib = nat.lib()

    def offsets_call(ctx, a):
        return lib.uavac_flown_conflict_offsets_dev(ctx, _p(a["log"]), a["K"], a["B"], a["pitch"], _p(a["go"]), a["G"], a["radius"], _p(a["po"]))

    def fill_call(ctx, a):
        return lib.uavac_flown_conflicts_dev(ctx, _p(a["log"]), a["K"], a["B"], a["pitch"], _p(a["go"]), a["G"], a["radius"], _p(a["po"]),
                                             a["cap"], _p(a["pd"]), _p(a["pi"]))
    for call, bad in ((offsets_call, shared), (fill_call, shared + fill_only)):
        for change in bad:
            rc = call(eng.ctx._h, {**good, **change})
            assert rc == nat.EINVAL, (change, rc)
            assert (lib.uavac_last_error(eng.ctx._h) or b"") != b"", change
        assert call(None, good) == nat.EINVAL                                        # no context
    torch.cuda.synchronize()
    assert bool((po == SENT_O).all()) and bool((pd == SENT_F).all()) and bool((pi == SENT_I).all())
    # the same calls with nothing wrong go through
    want = conflicts_from_log(host, RADIUS, [0, 10, n])
    assert offsets_call(eng.ctx._h, good) == nat.OK and fill_call(eng.ctx._h, good) == nat.OK
    torch.cuda.synchronize()
    E = int(want[0][-1])
    assert 0 < E <= 1024 and np.array_equal(po.cpu().numpy(), want[0])
    assert np.array_equal(pd.cpu().numpy()[:E], want[1]) and np.array_equal(pi.cpu().numpy().reshape(5, 1024)[:, :E], want[2])
