"""The separation the fleet flew, on the GPU (`uavac_flown_separation_dev`, csrc/flown_separation.hip), through the C ABI and
`Engine.flown_separation`: per vehicle the closest approach to any other vehicle of its group, the partner, the tick, the conflicts
inside a radius, the first tick with anybody inside and the partners compared -- from the positions in a state log.

Everything is exact: `uav_ac.scoring.separation_from_log` on the same log is the rule, the kernel forms d^2 = (dx dx + dy dy) + dz dz
without contraction, and every reduction is a lexicographic minimum, an integer sum, an OR or an integer minimum.
  * Seeded synthetic logs on a grid of 0.125, so equal distances -- between ticks and between partners -- are real and the tie rules
    decide; 193 vehicles in groups of 63, 64, 65 and 1 (the kernel's window and j-tile are 64 wide: a group inside one window, one that
    fills a tile, one that needs two, windows that hold two groups), 1, 33 and 100 ticks (a chunk is 32 ticks, a wavefront's share 8),
    at the pitches 193 and 208, one vehicle NaN at some ticks and one throughout.
  * A real flight: the (8, 96) set staggered, delayed, flown with a state log for 2 000 ticks."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, SIZES = 193, (63, 64, 65, 1)
GO = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
PAD, SENT_F, SENT_I = 96, -7777.25, -7777
RADIUS = 0.5
NAN_SOMETIMES, NAN_ALWAYS = 70, 130


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    return Engine("cuda:0")


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


_LOGS = {}


def synthetic(K):
    """(the log (K, 13, B) on the host, what the rule gives on it): computed once per K and left unchanged.  Positions on the 0.125 grid
    inside a 3 m box; the other ten rows hold junk that must never be read."""
    if K not in _LOGS:
        from uav_ac.scoring import separation_from_log
        rng = np.random.default_rng(100 + K)
        log = rng.uniform(-1e3, 1e3, (K, 13, B))
        log[:, 0:3, :] = rng.integers(0, 25, (K, 3, B)) * 0.125
        log[::3, 0, NAN_SOMETIMES] = np.nan                  # (with K = 1 that is its only tick)
        log[:, 0:3, NAN_ALWAYS] = np.nan
        _LOGS[K] = (log, separation_from_log(log, RADIUS, GO))
    return _LOGS[K]


def flown_abi(eng, log, pitch, go=None, radius=RADIUS):
    """One call of uavac_flown_separation_dev on a host log (K, 13, n) laid out at `pitch` (the columns past n hold vehicles that
    stand in the middle of the box: reading one would show) -> (sep (n,), isep (5, n)) as NumPy.  Both outputs are the middle of a
    larger sentinel-filled buffer: nothing outside may be written, and everything inside must be."""
    import torch
    K, _, n = log.shape
    wide = np.full((K, 13, pitch), 1.5)
    wide[:, :, :n] = log
    dev = torch.as_tensor(wide).to(eng.device)
    g = None if go is None else torch.as_tensor(np.ascontiguousarray(go, dtype=np.int64)).to(eng.device)
    sbuf = torch.full((PAD + n + PAD,), SENT_F, dtype=torch.float64, device=eng.device)
    ibuf = torch.full((PAD + 5 * n + PAD,), SENT_I, dtype=torch.int32, device=eng.device)
    eng._bind_stream()
    eng.ctx.call("uavac_flown_separation_dev", _p(dev), K, n, pitch, _p(g), 0 if go is None else len(go) - 1, float(radius),
                 _p(sbuf[PAD:]), _p(ibuf[PAD:]))
    torch.cuda.synchronize()
    s, i = sbuf.cpu().numpy(), ibuf.cpu().numpy()
    assert (s[:PAD] == SENT_F).all() and (s[PAD + n:] == SENT_F).all() and not (s[PAD:PAD + n] == SENT_F).any()
    assert (i[:PAD] == SENT_I).all() and (i[PAD + 5 * n:] == SENT_I).all() and not (i[PAD:PAD + 5 * n] == SENT_I).any()
    return s[PAD:PAD + n].copy(), i[PAD:PAD + 5 * n].reshape(5, n).copy()


def same(got, want):
    (gs, gi), (ws, wi) = got, want
    return gs.dtype == ws.dtype == np.float64 and gi.dtype == wi.dtype == np.int32 and np.array_equal(gs.view(np.int64), ws.view(np.int64)) \
        and np.array_equal(gi, wi)


def differing(got, want):
    bad = np.flatnonzero((got[0].view(np.int64) != want[0].view(np.int64)) | (got[1] != want[1]).any(axis=0))[:6]
    return [(int(b), float(got[0][b]), got[1][:, b].tolist(), float(want[0][b]), want[1][:, b].tolist()) for b in bad]


# ------------------------------------------------------------------------------------------------ 1: synthetic logs
@pytest.mark.parametrize("pitch", (193, 208))
@pytest.mark.parametrize("K", (1, 33, 100))
def test_flown_separation_equals_the_rule_on_synthetic_logs(eng, K, pitch):
    log, want = synthetic(K)
    got = flown_abi(eng, log, pitch, GO)
    assert same(got, want), differing(got, want)
    sep, isep = want
    # the set cannot go trivial: ties between ticks and between partners decide minima, there are conflicts, and the NaN vehicles show
    assert isep[4, NAN_ALWAYS] == 0 and np.isinf(sep[NAN_ALWAYS]) and isep[0, NAN_ALWAYS] == -1
    assert isep[:, B - 1].tolist() == [-1, -1, 0, -1, 0] and np.isinf(sep[B - 1])       # the group of one
    in_group = np.flatnonzero((np.arange(B) >= GO[2]) & (np.arange(B) < GO[3]) & (np.arange(B) != NAN_ALWAYS))
    assert (isep[4, in_group] == SIZES[2] - 2).all()          # everybody in its group sees that one partner was never compared
    if K == 1:
        assert isep[4, NAN_SOMETIMES] == 0 and (isep[4, GO[1]:NAN_SOMETIMES] == SIZES[1] - 2).all()
    else:
        assert isep[4, NAN_SOMETIMES] == SIZES[1] - 1 and (isep[4, GO[1]:NAN_SOMETIMES] == SIZES[1] - 1).all()
        assert (isep[2] > 0).sum() > B // 2 and (isep[1] > 0).sum() > B // 2


def test_a_group_audited_alone_and_other_launch_shapes_give_the_same_bits(eng):
    log, want = synthetic(100)
    for g in (1, 2):                                         # 64 vehicles from column 63 on; 65 from 127 on
        lo, hi = int(GO[g]), int(GO[g + 1])
        alone = flown_abi(eng, np.ascontiguousarray(log[:, :, lo:hi]), hi - lo)
        shifted = alone[1].copy()
        shifted[0] = np.where(shifted[0] >= 0, shifted[0] + lo, -1)
        assert same((alone[0], shifted), (want[0][lo:hi], np.ascontiguousarray(want[1][:, lo:hi]))), g
    # one airspace of all 193, at the automatic split and at fixed ones: the same bits
    from uav_ac.scoring import separation_from_log
    one = separation_from_log(log, RADIUS)
    try:
        for split in (0, 1, 3, 64):
            eng.ctx.set_option("separation_split", split)
            assert same(flown_abi(eng, log, 208), one), split
            assert same(flown_abi(eng, log, 193, GO), want), split
    finally:
        eng.ctx.set_option("separation_split", 0)
    # radius 0: nobody is inside, the minima stay
    zero = flown_abi(eng, log, 193, GO, radius=0.0)
    assert np.array_equal(zero[0].view(np.int64), want[0].view(np.int64)) and (zero[1][2] == 0).all() and (zero[1][3] == -1).all()


# ------------------------------------------------------------------------------------------------ 2: a real flight
def test_flown_separation_of_a_staggered_flight_equals_the_rule_on_the_downloaded_log(eng):
    import torch
    from oracle import minsnap_oracle as mo
    from uav_ac.scoring import separation_from_log, separation_ok
    plan = eng.plan(mo.synthetic_missions(96, 8), 3.0, 0.01, rows=False)
    stag = eng.stagger(plan, RADIUS, 32)
    fleet = eng.fleet(eng.delay(plan, stag.start_rows))
    K = 2000
    slog, _ = fleet.rollout(K, state_log=True, log_pitch=112)
    assert tuple(slog.shape) == (K, 13, 96) and slog.stride(1) == 112 and not slog.is_contiguous()
    audit = eng.flown_separation(slog, RADIUS, 32)
    want = separation_from_log(slog.cpu().numpy(), RADIUS, np.arange(0, 97, 32))
    got = (audit.min_distance.cpu().numpy(), audit.block.cpu().numpy())
    assert same(got, want), differing(got, want)
    dense = eng.flown_separation(slog.contiguous(), RADIUS, 32)
    assert torch.equal(dense.min_distance, audit.min_distance) and torch.equal(dense.block, audit.block)
    assert torch.equal(audit.row, audit.block[1]) and torch.equal(audit.compared, audit.block[4])
    assert bool((audit.compared == 31).all()) and bool(torch.isfinite(audit.min_distance).all()) and bool((audit.row >= 0).all())
    ok = separation_ok(audit, 32)
    assert ok["complete"].all()
    print(f"flown separation of the staggered (8, 96) flight: closest {float(audit.min_distance.min()):.4f} m, "
          f"{int((~ok['clear']).sum())} vehicles with somebody inside {RADIUS} m")


# ------------------------------------------------------------------------------------------------ 3: refusals
def test_mismatched_logs_and_bad_arguments_are_refused(eng):
    import torch
    from uav_ac import _native as nat
    log = torch.zeros((4, 13, 8), dtype=torch.float64, device=eng.device)
    eng.flown_separation(log, RADIUS)                        # (the well-formed one goes through)
    for bad in (log.float(), log[:, :12], log.permute(0, 2, 1), log[:, :, ::2], log[::2], log.cpu(), log[0], log.cpu().numpy()):
        with pytest.raises(ValueError):
            eng.flown_separation(bad, RADIUS)
    with pytest.raises(ValueError):
        eng.flown_separation(log, RADIUS, groups=0)
    sep = torch.zeros((8,), dtype=torch.float64, device=eng.device)
    isep = torch.zeros((5, 8), dtype=torch.int32, device=eng.device)
    go = torch.as_tensor(np.array([0, 8], dtype=np.int64)).to(eng.device)
    for args in ((_p(log), 4, 8, 7, None, 0, RADIUS, _p(sep), _p(isep)),         # pitch < B
                 (_p(log), 0, 8, 8, None, 0, RADIUS, _p(sep), _p(isep)),         # K < 1
                 (_p(log), 4, 0, 8, None, 0, RADIUS, _p(sep), _p(isep)),
                 (None, 4, 8, 8, None, 0, RADIUS, _p(sep), _p(isep)),
                 (_p(log), 4, 8, 8, None, 0, RADIUS, None, _p(isep)),
                 (_p(log), 4, 8, 8, None, 0, RADIUS, _p(sep), None),
                 (_p(log), 4, 8, 8, None, 0, -0.5, _p(sep), _p(isep)),
                 (_p(log), 4, 8, 8, None, 0, float("nan"), _p(sep), _p(isep)),
                 (_p(log), 4, 8, 8, _p(go), 0, RADIUS, _p(sep), _p(isep))):
        with pytest.raises(nat.UavacError) as exc:
            eng.ctx.call("uavac_flown_separation_dev", *args)
        assert exc.value.code == nat.EINVAL
