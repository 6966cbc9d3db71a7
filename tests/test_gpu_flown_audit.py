"""The plan audit of a flight, on the GPU (`uavac_flown_audit_dev`, csrc/flown_audit.hip), through the C ABI and `Engine.flown_audit`:
per vehicle the valid ticks, the flown peaks of horizontal speed, climb, descent, speed, the two rotation-matrix elements that max_tilt
clips in the command and the body rate, and per cuboid the ticks inside it, the first of them and the closest approach with its tick --
from a rollout's state log.

Everything is exact: `uav_ac.scoring.audit_from_log` on the same log is the rule, the kernel rounds every product and sum on its own, and
every reduction is a maximum, an integer sum, an integer minimum or a lexicographic minimum.
  * Seeded synthetic logs: 193 vehicles (three full windows of 64 and one lane), 1, 33 and 100 ticks, at the pitches 193 and 208, with 0,
    1 and 16 cuboids, at the automatic split and at 1, 2 and 7 shares per window.  Positions and cuboid faces stand on a grid of 0.125, so
    hits on faces and equal clearances are real and the tie rule decides; the other rows are random; one vehicle is NaN at every third
    tick, one has an inf in q3 at some, one is NaN throughout, and one sinks at +0.0 and -0.0 in turn.
  * A real flight: the (8, 96) set staggered, delayed, flown for 2 000 ticks past four cuboids, against the rollout's `collided` bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 193
PAD, SENT_F, SENT_I = 96, -7777.25, -7777
NAN_SOMETIMES, INF_Q3, NAN_ALWAYS, ZEROS = 70, 71, 130, 5
KEYS = ("audit", "first_bad", "hit_ticks", "first_hit", "clearance", "clearance_tick")


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    return Engine("cuda:0")


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def cuboids_of(n):
    """n cuboids with their faces on the 0.125 grid, inside the 3 m box the positions stand in."""
    rng = np.random.default_rng(7)
    lo = rng.integers(0, 20, (16, 3)) * 0.125
    hi = lo + rng.integers(1, 9, (16, 3)) * 0.125
    return np.stack([lo[:, 0], hi[:, 0], lo[:, 1], hi[:, 1], lo[:, 2], hi[:, 2]], axis=1)[:n].copy()


_LOGS, _WANT = {}, {}


def synthetic(K):
    """The log (K, 13, B) on the host: computed once per K and left unchanged."""
    if K not in _LOGS:
        rng = np.random.default_rng(200 + K)
        log = rng.uniform(-1e3, 1e3, (K, 13, B))
        log[:, 0:3, :] = rng.integers(0, 25, (K, 3, B)) * 0.125
        log[::3, 8, NAN_SOMETIMES] = np.nan                  # (with K = 1 that is its only tick)
        log[1::4, 6, INF_Q3] = np.inf                        # q3 is in no peak: the tick is invalid all the same
        log[:, :, NAN_ALWAYS] = np.nan
        log[0::2, 9, ZEROS], log[1::2, 9, ZEROS] = 0.0, -0.0
        _LOGS[K] = log
    return _LOGS[K]


def wanted(K, n):
    if (K, n) not in _WANT:
        from uav_ac.scoring import audit_from_log
        _WANT[K, n] = audit_from_log(synthetic(K), cuboids_of(n) if n else None)
    return _WANT[K, n]


def flown_abi(eng, log, pitch, cuboids):
    """One call of uavac_flown_audit_dev on a host log (K, 13, v) laid out at `pitch` (the columns past v hold values that would show in
    every peak if they were read) -> the six outputs as NumPy.  Every output is the middle of a larger sentinel-filled buffer: nothing
    outside may be written, and everything inside must be."""
    import torch
    K, _, v = log.shape
    n = 0 if cuboids is None else len(cuboids)
    wide = np.full((K, 13, pitch), 1e9)
    wide[:, :, :v] = log
    dev = torch.as_tensor(wide).to(eng.device)
    cub = None if not n else torch.as_tensor(np.ascontiguousarray(cuboids, dtype=np.float64)).to(eng.device)
    sizes = {"audit": 8 * v, "first_bad": v, "hit_ticks": n * v, "first_hit": n * v, "clearance": n * v, "clearance_tick": n * v}
    bufs = {k: torch.full((PAD + s + PAD,), SENT_F if k in ("audit", "clearance") else SENT_I,
                          dtype=torch.float64 if k in ("audit", "clearance") else torch.int32, device=eng.device) for k, s in sizes.items()}
    eng._bind_stream()
    eng.ctx.call("uavac_flown_audit_dev", _p(dev), K, v, pitch, _p(cub), n, _p(bufs["audit"][PAD:]), _p(bufs["first_bad"][PAD:]),
                 *(_p(bufs[k][PAD:]) if n else None for k in KEYS[2:]))
    torch.cuda.synchronize()
    out = {}
    for k, s in sizes.items():
        a = bufs[k].cpu().numpy()
        sent = SENT_F if a.dtype == np.float64 else SENT_I
        assert (a[:PAD] == sent).all() and (a[PAD + s:] == sent).all() and not (a[PAD:PAD + s] == sent).any(), k
        out[k] = a[PAD:PAD + s].reshape((8, v) if k == "audit" else (v,) if k == "first_bad" else (n, v)).copy()
    return out


def bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def differing(got, want):
    """[] when every output has the dtype, the shape and the bits of the rule's; else the first few (output, index, got, wanted)."""
    bad = []
    for k in KEYS:
        if got[k].dtype != want[k].dtype or got[k].shape != want[k].shape:
            bad.append((k, str(got[k].dtype), got[k].shape, want[k].shape))
            continue
        for idx in np.argwhere(bits(got[k]) != bits(want[k]))[:4]:
            bad.append((k, tuple(int(i) for i in idx), got[k][tuple(idx)].item(), want[k][tuple(idx)].item()))
    return bad


def columns(want, lo, hi):
    return {k: np.ascontiguousarray(a[..., lo:hi]) for k, a in want.items()}


# ------------------------------------------------------------------------------------------------ 1: synthetic logs
@pytest.mark.parametrize("pitch", (193, 208))
@pytest.mark.parametrize("K", (1, 33, 100))
def test_flown_audit_equals_the_rule_on_synthetic_logs(eng, K, pitch):
    log = synthetic(K)
    try:
        for n in (0, 1, 16):
            want = wanted(K, n)
            for split in (0, 1, 2, 7):
                eng.ctx.set_option("flown_audit_split", split)
                got = flown_abi(eng, log, pitch, cuboids_of(n) if n else None)
                assert not differing(got, want), (n, split, differing(got, want))
    finally:
        eng.ctx.set_option("flown_audit_split", 0)
    # the set cannot go trivial: the marked vehicles show, faces are hit, clearances tie, and both classes of vehicle are there
    want = wanted(K, 16)
    audit, first_bad = want["audit"], want["first_bad"]
    assert audit[0, NAN_ALWAYS] == 0 and np.isnan(audit[1:, NAN_ALWAYS]).all() and first_bad[NAN_ALWAYS] == 0
    assert np.isnan(want["clearance"][:, NAN_ALWAYS]).all() and (want["clearance_tick"][:, NAN_ALWAYS] == -1).all()
    assert audit[0, NAN_SOMETIMES] == K - len(range(0, K, 3)) and first_bad[NAN_SOMETIMES] == 0
    assert audit[0, INF_Q3] == K - len(range(1, K, 4)) and first_bad[INF_Q3] == (1 if K > 1 else -1)
    assert audit[2, ZEROS] == 0 and audit[3, ZEROS] == 0 and not np.signbit(audit[3, ZEROS])
    assert not np.signbit(audit[2, ZEROS]) or K == 1         # (+0.0 and -0.0 met: +0.0; at K = 1 the only value is -(+0.0))
    others = np.setdiff1d(np.arange(B), (NAN_SOMETIMES, INF_Q3, NAN_ALWAYS))
    assert (audit[0, others] == K).all() and (first_bad[others] == -1).all()
    hit = want["hit_ticks"] > 0
    assert ((want["clearance"] == 0) == hit).all() and ((want["first_hit"] >= 0) == hit).all()
    if K > 1:
        assert hit.any(axis=0).sum() > B // 4 and (~hit.any(axis=0)).sum() > 0
        pos, cub = log[:, 0:3, :], cuboids_of(16)
        on_face = (pos[:, 0, :] == cub[0, 0]) | (pos[:, 0, :] == cub[0, 1])
        inside0 = (pos[:, 0] >= cub[0, 0]) & (pos[:, 0] <= cub[0, 1]) & (pos[:, 1] >= cub[0, 2]) & (pos[:, 1] <= cub[0, 3]) \
            & (pos[:, 2] >= cub[0, 4]) & (pos[:, 2] <= cub[0, 5])
        assert (on_face & inside0).any()                     # a hit that only the inclusive test finds


def test_vehicles_audited_alone_give_the_same_records(eng):
    log = synthetic(100)
    for n in (0, 16):
        alone = flown_abi(eng, np.ascontiguousarray(log[:, :, 64:128]), 64, cuboids_of(n) if n else None)
        want = columns(wanted(100, n), 64, 128)
        assert not differing(alone, want), (n, differing(alone, want))
    # ... and so does a window that ends inside the batch's last one, at a pitch of its own
    tail = flown_abi(eng, np.ascontiguousarray(log[:, :, 120:193]), 80, cuboids_of(16))
    assert not differing(tail, columns(wanted(100, 16), 120, 193))


# ------------------------------------------------------------------------------------------------ 2: a real flight
def test_flown_audit_of_a_real_flight_equals_the_rule_and_the_collided_bit(eng):
    import torch
    from oracle import minsnap_oracle as mo
    from uav_ac.scoring import audit_from_log, flight_feasibility
    plan = eng.plan(mo.synthetic_missions(96, 8), 3.0, 0.01, rows=False)
    stag = eng.stagger(plan, 0.5, 32)
    flown = eng.delay(plan, stag.start_rows)
    K = 2000
    # a first flight shows where the vehicles go: two cuboids on flown paths, two away from every path
    scout, _ = eng.fleet(flown).rollout(K, state_log=True)
    where = scout.cpu().numpy()[:, 0:3, :]
    a, b = where[1500, :, 3], where[700, :, 40]
    lo, hi = where.min(axis=(0, 2)), where.max(axis=(0, 2))
    boxes = np.array([[a[0] - 0.125, a[0] + 0.125, a[1] - 0.125, a[1] + 0.125, a[2] - 0.125, a[2] + 0.125],
                      [b[0] - 0.25, b[0] + 0.25, b[1] - 0.25, b[1] + 0.25, b[2] - 0.25, b[2] + 0.25],
                      [hi[0] + 1.0, hi[0] + 2.0, lo[1], hi[1], lo[2], hi[2]],
                      [lo[0], hi[0], lo[1], hi[1], hi[2] + 0.5, hi[2] + 1.5]])
    fleet = eng.fleet(flown)
    slog, _ = fleet.rollout(K, state_log=True, aabbs=boxes, log_pitch=112)
    assert tuple(slog.shape) == (K, 13, 96) and slog.stride(1) == 112 and not slog.is_contiguous()
    audit = eng.flown_audit(slog, boxes)
    want = audit_from_log(slog.cpu().numpy(), boxes)
    got = {"audit": audit.block, "first_bad": audit.first_bad, "hit_ticks": audit.hit_ticks, "first_hit": audit.first_hit,
           "clearance": audit.clearance, "clearance_tick": audit.clearance_tick}
    got = {k: t.cpu().numpy() for k, t in got.items()}
    assert not differing(got, want), differing(got, want)
    dense = eng.flown_audit(slog.contiguous(), boxes)
    assert torch.equal(dense.block, audit.block) and torch.equal(dense.hit_ticks, audit.hit_ticks) \
        and torch.equal(dense.clearance, audit.clearance) and torch.equal(dense.clearance_tick, audit.clearance_tick)
    assert torch.equal(audit.ticks, audit.block[0]) and torch.equal(audit.bank_x, audit.block[5]) and torch.equal(audit.body_rate, audit.block[7])
    # the cross-check against the rollout's own kernel: a vehicle spent a tick inside a cuboid iff its sticky bit is set
    hit = (audit.hit_ticks > 0).any(dim=0)
    assert torch.equal(hit, fleet.collided != 0)
    assert bool(hit.any()) and bool((~hit).any()) and bool(hit[3]) and bool(hit[40])
    assert bool((audit.hit_ticks[2:] == 0).all()) and bool((audit.clearance[2:] > 0).all())
    assert bool((audit.ticks == K).all()) and bool((audit.first_bad == -1).all())
    assert torch.equal(audit.clearance == 0, audit.hit_ticks > 0)
    # without obstacles: the same peaks, and empty per-cuboid outputs
    bare = eng.flown_audit(slog)
    assert torch.equal(bare.block, audit.block) and tuple(bare.hit_ticks.shape) == (0, 96) and tuple(bare.clearance.shape) == (0, 96)
    ok = flight_feasibility(audit, K)
    assert ok["complete"].all() and np.array_equal(ok["clear"], ~hit.cpu().numpy())
    print(f"flown audit of the staggered (8, 96) flight: {int(hit.sum())} vehicles inside a cuboid, peak speed "
          f"{float(audit.speed.max()):.3f} m/s, peak |R13| {float(audit.bank_x.max()):.3f}, {int(ok['flown_ok'].sum())} of 96 flown_ok")


# ------------------------------------------------------------------------------------------------ 3: refusals
def test_mismatched_logs_and_bad_arguments_are_refused(eng):
    import torch
    from uav_ac import _native as nat
    log = torch.zeros((4, 13, 8), dtype=torch.float64, device=eng.device)
    log[:, 3] = 1.0
    box = np.array([[0.0, 1.0, 0.0, 1.0, 0.0, 1.0]])
    ok = eng.flown_audit(log, box)                           # (the well-formed one goes through)
    assert ok.hit_ticks.cpu().numpy().tolist() == [[4] * 8] and ok.ticks.cpu().numpy().tolist() == [4.0] * 8
    for bad in (log.float(), log[:, :12], log.permute(0, 2, 1), log[:, :, ::2], log[::2], log.cpu(), log[0], log.cpu().numpy()):
        with pytest.raises(ValueError):
            eng.flown_audit(bad)
    for bad in (np.zeros((2, 5)), np.zeros(7), np.zeros((17, 6))):
        with pytest.raises(ValueError):
            eng.flown_audit(log, bad)
    with pytest.raises(nat.UavacError):
        eng.ctx.set_option("flown_audit_split", 65)
    kw = dict(device=eng.device)
    audit = torch.zeros((8, 8), dtype=torch.float64, **kw)
    bad_tick = torch.zeros((8,), dtype=torch.int32, **kw)
    cub = torch.as_tensor(box).to(eng.device)
    i1, i2, i3 = (torch.zeros((1, 8), dtype=torch.int32, **kw) for _ in range(3))
    d1 = torch.zeros((1, 8), dtype=torch.float64, **kw)
    full = (_p(cub), 1, _p(audit), _p(bad_tick), _p(i1), _p(i2), _p(d1), _p(i3))
    none = (None, 0, _p(audit), _p(bad_tick), None, None, None, None)
    eng.ctx.call("uavac_flown_audit_dev", _p(log), 4, 8, 8, *full)
    eng.ctx.call("uavac_flown_audit_dev", _p(log), 4, 8, 8, *none)
    for args in ((_p(log), 4, 8, 7) + none,                                              # pitch < B
                 (_p(log), 0, 8, 8) + none,                                              # K < 1
                 (_p(log), 4, 0, 8) + none,
                 (None, 4, 8, 8) + none,
                 (_p(log), 4, 8, 8, None, 0, None, _p(bad_tick), None, None, None, None),
                 (_p(log), 4, 8, 8, None, 0, _p(audit), None, None, None, None, None),
                 (_p(log), 4, 8, 8, _p(cub), -1) + full[2:],                             # n_cuboids outside the range
                 (_p(log), 4, 8, 8, _p(cub), 17) + full[2:],
                 (_p(log), 4, 8, 8, None, 1) + full[2:],                                 # a NULL with n_cuboids > 0
                 (_p(log), 4, 8, 8) + full[:4] + (None,) + full[5:],
                 (_p(log), 4, 8, 8) + full[:7] + (None,),
                 (_p(log), 4, 8, 8, _p(cub), 0) + none[2:],                              # a pointer with n_cuboids == 0
                 (_p(log), 4, 8, 8) + none[:7] + (_p(i3),)):
        with pytest.raises(nat.UavacError) as exc:
            eng.ctx.call("uavac_flown_audit_dev", *args)
        assert exc.value.code == nat.EINVAL
