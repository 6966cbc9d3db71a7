"""Separation audit on the GPU (`uavac_minsnap_separation_dev`, csrc/minsnap_separation.hip), through the C ABI and `Engine.separation`:
per mission of a group that shares an airspace the closest approach to any other mission of the group, to which one and at which row
of the group's clock, how many others come inside a protection radius and when the first does -- from coefficients and row counts.

What is compared with what:
  * against the PRODUCT'S OWN ROWS everything is exact (no tolerance, NaN equal to NaN): `uav_ac.scoring.separation_from_rows` on the
    sampled rows is the rule, and the kernel uses the sampler's arithmetic, forms d^2 = (dx dx + dy dy) + dz dz without contraction,
    takes the lexicographic minimum of (d^2, row, partner) and one correctly rounded sqrt;
  * against the ORACLE (oracle.c_oracle.plan_threads: its own solve and sampler, through the same NumPy rule) `min_distance` holds to
    2e-5 absolute -- two positions, each at the project's 1e-5 bar for sampled positions --; partner, conflicts,
    first_conflict and compared are exact; for `row` the oracle's distance of the reported pair at the reported row lies within 2e-5
    of the oracle's minimum (adjacent rows at a minimum differ by less than any parity bar).  A difference in the exact quantities is
    tolerated only where the oracle's distance lies within 1e-9 of the radius or the gap to the second-nearest partner is under 4e-5;
    such cases are counted and the cap is 0.  For these sets, both configurations and radius 0.5 the oracle's nearest pair-row is
    >= 1.1e-4 from the radius and the smallest gap between nearest and second-nearest partner is 1.12e-4 (checked on the CPU).
The tile of the pair kernel is 64 missions wide: groups of 63, 64 and 65 missions (and windows that straddle groups) are cut from the
(8, 96) set."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VEL, DT, RADIUS = 3.0, 0.01, 0.5
SETS = ((1, 48), (2, 48), (8, 96), (20, 24), (8, 37))
SENT_F, SENT_I, PAD = -1.2345e300, -7777, 96
DIST_TOL, RADIUS_TIE, PARTNER_GAP = 2e-5, 1e-9, 4e-5
TILE = 64


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    e = Engine("cuda:0")
    yield e
    e.ctx.set_option("separation_split", 0)


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _i64(eng, a):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.int64)).to(eng.device)


def _i32(eng, a):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(eng.device)


def sep_abi(eng, coeffs, seg_rows, seg_offsets, B, m, dt, go=None, start=None, radius=RADIUS):
    """One call of uavac_minsnap_separation_dev -> (sep (B,), isep (5, B)) as NumPy.  The outputs are the middle of larger
    sentinel-filled buffers: nothing outside [B] / [5][B] may be written, and everything inside must be."""
    import torch
    dev = dict(device=eng.device)
    sbuf = torch.full((PAD + B + PAD,), SENT_F, dtype=torch.float64, **dev)
    ibuf = torch.full((PAD + 5 * B + PAD,), SENT_I, dtype=torch.int32, **dev)
    g, s = _i64(eng, go), _i32(eng, start)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_separation_dev", _p(coeffs), _p(seg_rows), _p(seg_offsets), int(B), int(m), float(dt), _p(g),
                 0 if go is None else len(go) - 1, _p(s), float(radius), _p(sbuf[PAD:]), _p(ibuf[PAD:]))
    torch.cuda.synchronize()
    a, i = sbuf.cpu().numpy(), ibuf.cpu().numpy()
    assert (a[:PAD] == SENT_F).all() and (a[PAD + B:] == SENT_F).all() and (i[:PAD] == SENT_I).all() and (i[PAD + 5 * B:] == SENT_I).all()
    assert not (a[PAD:PAD + B] == SENT_F).any() and not (i[PAD:PAD + 5 * B] == SENT_I).any()
    return a[PAD:PAD + B].copy(), i[PAD:PAD + 5 * B].reshape(5, B).copy()


def sep_of_plan(eng, plan, **kw):
    ragged = hasattr(plan, "seg_offsets")
    return sep_abi(eng, plan.coeffs, plan.seg_rows, plan.seg_offsets if ragged else None, plan.B, plan.max_m if ragged else plan.m,
                   plan.dt, **kw)


def same(got, want):
    return all(g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w, equal_nan=g.dtype.kind == "f") for g, w in zip(got, want))


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
        from uav_ac.scoring import separation_from_rows
        wps = mo.synthetic_missions(B, m)
        plan = eng.plan(wps, VEL, DT)
        free = eng.plan(wps, VEL, DT, rows=False)
        rows, ro = plan.traj.cpu().numpy(), plan.row_offsets.cpu().numpy()
        want = {name: separation_from_rows(rows, ro, RADIUS, go, st) for name, go, st in configs(B)}
        _CACHE[(m, B)] = dict(wps=wps, plan=plan, free=free, rows=rows, ro=ro, want=want)
    return _CACHE[(m, B)]


# ------------------------------------------------------------------------------------------------ 1: the product's own rows
@pytest.mark.parametrize("m, B", SETS)
def test_separation_equals_what_the_products_rows_show(eng, m, B):
    k = case(eng, m, B)
    assert k["free"].traj is None
    for name, go, st in configs(B):
        got_free = sep_of_plan(eng, k["free"], go=go, start=st)
        got_rows = sep_of_plan(eng, k["plan"], go=go, start=st)
        assert same(got_free, got_rows), (m, B, name)
        assert same(got_free, k["want"][name]), (m, B, name, np.flatnonzero(got_free[0] != k["want"][name][0]),
                                                 np.argwhere(got_free[1] != k["want"][name][1])[:8])
    assert (k["want"]["one group"][1][2] > 0).any()                                  # the counts are not trivially zero


def test_groups_of_one_tile_one_less_and_one_more(eng):
    from uav_ac.scoring import separation_from_rows
    k = case(eng, 8, 96)
    starts = (np.arange(96) % 7) * 23
    for n, go in enumerate(([0, TILE - 1, 96], [0, TILE, 96], [0, TILE + 1, 96], [0, 96 - TILE - 1, 96], [0, 31, 31 + TILE, 96], [0, 32, 96],
                            [0, 5, 10, 10, 74, 96])):
        for st in ((None,), (starts,))[n % 2]:
            got = sep_of_plan(eng, k["free"], go=np.array(go), start=st)
            assert same(got, separation_from_rows(k["rows"], k["ro"], RADIUS, go, st)), (go, st is not None)
    # the same groups as batches of their own
    for b0, n in ((0, TILE - 1), (3, TILE), (7, TILE + 1), (31, TILE + 1)):
        free = k["free"]
        got = sep_abi(eng, free.coeffs[b0:b0 + n], free.seg_rows[b0:b0 + n], None, n, 8, DT)
        ro = k["ro"][b0:b0 + n + 1]
        assert same(got, separation_from_rows(k["rows"][ro[0]:ro[-1]], ro - ro[0], RADIUS)), (b0, n)


# ------------------------------------------------------------------------------------------------------------ 2: the oracle
def _stand(rows, ro, start, b, k):
    n = ro[b + 1] - ro[b]
    return rows[ro[b] + np.clip(k - start[b], 0, n - 1), 0:3]


@pytest.mark.parametrize("m, B", SETS)
def test_separation_against_the_oracle(eng, m, B):
    from oracle import c_oracle as cc
    from uav_ac.scoring import separation_from_rows
    k = case(eng, m, B)
    ref = cc.plan_threads(k["wps"], VEL, DT)
    rows, ro = ref["rows"], ref["row_offsets"]
    assert np.array_equal(ro, k["ro"])                                                 # row counts are exact
    for name, go, st in configs(B):
        want = separation_from_rows(rows, ro, RADIUS, go, st)
        got = k["want"][name]                                                         # (== the device's outputs, test 1)
        dev = sep_of_plan(eng, k["free"], go=go, start=st)
        assert same(dev, got)
        live = np.isfinite(want[0])
        assert np.array_equal(np.isfinite(got[0]), live) and np.array_equal(np.isinf(got[0]), np.isinf(want[0]))
        err = np.abs(got[0][live] - want[0][live])
        print(f"separation vs oracle m={m} B={B} {name}: worst distance error {err.max():.3e}, "
              f"{int((want[1][2] > 0).sum())} missions with a conflict")
        assert (err <= DIST_TOL).all(), err.max()
        start = np.zeros(B, dtype=np.int64) if st is None else np.asarray(st, dtype=np.int64)
        ties = 0
        for row_id in (0, 2, 3, 4):                                                   # partner, conflicts, first conflict, compared
            for b in np.flatnonzero(got[1][row_id] != want[1][row_id]):
                bounds = (0, B) if go is None else next((go[g], go[g + 1]) for g in range(len(go) - 1) if go[g] <= b < go[g + 1])
                H = max(start[j] + ro[j + 1] - ro[j] for j in range(*bounds))
                kk = np.arange(H)
                d = np.array([np.sqrt(((_stand(rows, ro, start, b, kk) - _stand(rows, ro, start, j, kk)) ** 2).sum(axis=1))
                              if j != b else np.full(H, np.inf) for j in range(*bounds)])
                near_radius = float(np.abs(d - RADIUS).min())
                per_partner = np.sort(d.min(axis=1))
                gap = float(per_partner[1] - per_partner[0]) if len(per_partner) > 1 else np.inf
                assert near_radius <= RADIUS_TIE or (row_id == 0 and gap < PARTNER_GAP), (m, B, name, row_id, int(b), got[1][:, b],
                                                                                           want[1][:, b], near_radius, gap)
                ties += 1
        assert ties == 0
        for b in np.flatnonzero(live):                                                # the reported row: as good as the oracle's minimum
            j, kk = int(got[1][0, b]), int(got[1][1, b])
            d = float(np.sqrt(((_stand(rows, ro, start, b, kk) - _stand(rows, ro, start, j, kk)) ** 2).sum()))
            assert abs(d - want[0][b]) <= DIST_TOL, (m, B, name, int(b), j, kk, d, want[0][b])
        assert (want[1][2] > 0).sum() > 0
        if name == "one group":
            assert 6 <= (want[1][2] > 0).sum() <= 65


# ------------------------------------------------------------------------------------------------------------ 3: independence
def test_a_group_audited_alone_and_every_split_give_the_same_bits(eng):
    k = case(eng, 8, 96)
    free = k["free"]
    name, go, st = configs(96)[1]
    whole = sep_of_plan(eng, free, go=go, start=st)
    for g in (1, 3):                                                                  # the second and the fourth group
        b0, b1 = int(go[g]), int(go[g + 1])
        alone = sep_abi(eng, free.coeffs[b0:b1], free.seg_rows[b0:b1], None, b1 - b0, 8, DT, start=st[b0:b1])
        shifted = whole[1][:, b0:b1].copy()
        shifted[0] = np.where(shifted[0] >= 0, shifted[0] - b0, shifted[0])
        assert same(alone, (whole[0][b0:b1], shifted)), g
    from uav_ac import _native as nat
    for m, B in ((8, 96), (20, 24), (8, 37)):
        kk = case(eng, m, B)
        for split in (1, 2, 3, 5, nat.SEP_MAX_SPLIT, 0):
            eng.ctx.set_option("separation_split", split)
            for name, go, st in configs(B):
                assert same(sep_of_plan(eng, kk["free"], go=go, start=st), kk["want"][name]), (m, B, split, name)
    with pytest.raises(nat.UavacError):
        eng.ctx.set_option("separation_split", nat.SEP_MAX_SPLIT + 1)
    with pytest.raises(nat.UavacError):
        eng.ctx.set_option("separation_split", -1)


# ------------------------------------------------------------------------------------------------------------------ 4: ragged
def test_a_ragged_batch_is_exact_against_its_own_rows(eng):
    from uav_ac.scoring import separation_from_rows
    sets = {m: case(eng, m, B)["wps"] for m, B in ((1, 48), (2, 48), (8, 96))}
    missions = [sets[(1, 2, 8)[b % 3]][b] for b in range(45)]
    assert sorted({len(w) - 1 for w in missions}) == [1, 2, 8]
    with_rows = eng.plan_ragged(missions, VEL, DT)
    free = eng.plan_ragged(missions, VEL, DT, rows=False)
    assert free.traj is None
    rows, ro = with_rows.traj.cpu().numpy(), with_rows.row_offsets.cpu().numpy()
    for name, go, st in configs(45):
        want = separation_from_rows(rows, ro, RADIUS, go, st)
        assert same(sep_of_plan(eng, free, go=go, start=st), want), name
        assert same(sep_of_plan(eng, with_rows, go=go, start=st), want), name
    assert (want[1][2] > 0).any()


# ------------------------------------------------------------------------------------------ 5: excluded and degenerate missions
def test_a_singular_mission_a_copy_radius_zero_and_a_negative_start(eng):
    from uav_ac.scoring import separation_from_rows
    B = 37
    wps = case(eng, 8, B)["wps"].copy()
    wps[5, 3] = wps[5, 2]                                                            # a repeated waypoint: singular knot system
    wps[20] = wps[11]                                                                # an exact copy of another mission
    plan = eng.plan(wps, VEL, DT, strict=False)
    assert plan.status.cpu().tolist() == [1 if b == 5 else 0 for b in range(B)]
    sep, isep = sep_of_plan(eng, plan)
    assert same((sep, isep), separation_from_rows(plan.traj.cpu().numpy(), plan.row_offsets.cpu().numpy(), RADIUS))
    assert np.isnan(sep[5]) and isep[:, 5].tolist() == [-1, -1, 0, -1, 0]
    others = np.setdiff1d(np.arange(B), [5])
    assert (isep[4, others] == B - 2).all()                                          # the skipped neighbour is visible
    assert sep[11] == 0.0 and sep[20] == 0.0 and isep[0, 11] == 20 and isep[0, 20] == 11 and isep[1, 11] == 0 and isep[1, 20] == 0
    assert isep[2, 11] >= 1 and isep[3, 11] == 0
    # radius 0: the test is strict, so not even the copy is inside
    sep0, isep0 = sep_of_plan(eng, plan, radius=0.0)
    assert np.array_equal(sep0, sep, equal_nan=True) and (isep0[2] == 0).all() and (isep0[3] == -1).all()
    assert np.array_equal(isep0[[0, 1, 4]], isep[[0, 1, 4]])
    # a negative start row behaves as 0 and raises flag 0
    eng.take_flags()
    st = (np.arange(B) % 4) * 11
    want = sep_of_plan(eng, plan, start=st)
    assert eng.take_flags() == [0, 0, 0, 0]
    neg = st.copy()
    neg[st == 0] = -1 - np.arange((st == 0).sum())
    assert same(sep_of_plan(eng, plan, start=neg), want)
    assert eng.take_flags() == [1, 0, 0, 0]
    # a mission without rows is excluded as well (seg_rows zeroed: what a bad speed leaves)
    seg_rows = plan.seg_rows.clone()
    seg_rows[7] = 0
    sep7, isep7 = sep_abi(eng, plan.coeffs, seg_rows, None, B, 8, DT)
    assert np.isnan(sep7[[5, 7]]).all() and isep7[:, 7].tolist() == [-1, -1, 0, -1, 0]
    assert (isep7[4, np.setdiff1d(np.arange(B), [5, 7])] == B - 3).all()
    # all the others excluded, and a group of one: +inf, nobody
    lonely = plan.coeffs.clone()
    lonely[1:] = float("nan")
    sep1, isep1 = sep_abi(eng, lonely, plan.seg_rows, None, B, 8, DT)
    assert sep1[0] == np.inf and isep1[:, 0].tolist() == [-1, -1, 0, -1, 0] and np.isnan(sep1[1:]).all()


# -------------------------------------------------------------------------------------------------------------- 6: validation
def test_invalid_arguments_are_refused_before_anything_is_enqueued(eng):
    import torch
    from uav_ac import _native as nat
    k = case(eng, 8, 37)
    free, B, m = k["free"], 37, 8
    dev = dict(device=eng.device)
    sep = torch.full((B,), SENT_F, dtype=torch.float64, **dev)
    isep = torch.full((5 * B,), SENT_I, dtype=torch.int32, **dev)
    go = _i64(eng, [0, 10, B])
    good = dict(coeffs=free.coeffs, seg_rows=free.seg_rows, seg_offsets=None, B=B, m=m, dt=DT, go=go, G=2, start=None, radius=RADIUS,
                sep=sep, isep=isep)
    bad = [dict(coeffs=None), dict(seg_rows=None), dict(sep=None), dict(isep=None), dict(B=0), dict(B=-3), dict(m=0),
           dict(m=nat.MAX_SEGMENTS + 1), dict(dt=0.0), dict(dt=-0.01), dict(dt=math.inf), dict(dt=math.nan), dict(radius=-0.5),
           dict(radius=math.inf), dict(radius=math.nan), dict(G=0), dict(G=-2)]
    eng._bind_stream()
    fn = nat.lib().uavac_minsnap_separation_dev

    def call(ctx, a):
        return fn(ctx, _p(a["coeffs"]), _p(a["seg_rows"]), _p(a["seg_offsets"]), a["B"], a["m"], a["dt"], _p(a["go"]), a["G"], _p(a["start"]),
                  a["radius"], _p(a["sep"]), _p(a["isep"]))
    for change in bad:
        rc = call(eng.ctx._h, {**good, **change})
        assert rc == nat.EINVAL, (change, rc)
        assert (nat.lib().uavac_last_error(eng.ctx._h) or b"") != b"", change
    assert call(None, good) == nat.EINVAL                                            # no context
    torch.cuda.synchronize()
    assert bool((sep == SENT_F).all()) and bool((isep == SENT_I).all())
    # the same call with nothing wrong goes through; G is ignored without offsets
    from uav_ac.scoring import separation_from_rows
    assert call(eng.ctx._h, good) == nat.OK
    torch.cuda.synchronize()
    assert same((sep.cpu().numpy(), isep.cpu().numpy().reshape(5, B)), separation_from_rows(k["rows"], k["ro"], RADIUS, [0, 10, B]))
    assert call(eng.ctx._h, {**good, "go": None, "G": 0}) == nat.OK
    torch.cuda.synchronize()
    assert same((sep.cpu().numpy(), isep.cpu().numpy().reshape(5, B)), k["want"]["one group"])


# ------------------------------------------------------------------------------------------------------ 7: Engine.separation
def test_engine_separation(eng):
    from conftest import load_golden
    from uav_ac.scoring import separation_from_rows, separation_ok
    k = case(eng, 8, 96)
    for plan in (k["free"], k["plan"]):
        for name, go, st in configs(96):
            a = eng.separation(plan, RADIUS, groups=go, start_rows=st)
            assert a.min_distance.is_cuda and a.block.shape == (5, 96)
            fields = (a.partner, a.row, a.conflicts, a.first_conflict, a.compared)
            got = (a.min_distance.cpu().numpy(), np.stack([t.cpu().numpy() for t in fields]))
            assert same(got, k["want"][name]) and np.array_equal(a.block.cpu().numpy(), got[1]), name
    # groups given as a size: consecutive groups of that many, the last one shorter
    by_size = eng.separation(k["free"], RADIUS, groups=36)
    by_offsets = eng.separation(k["free"], RADIUS, groups=[0, 36, 72, 96])
    assert np.array_equal(by_size.block.cpu().numpy(), by_offsets.block.cpu().numpy())
    assert np.array_equal(by_size.min_distance.cpu().numpy(), by_offsets.min_distance.cpu().numpy())
    assert same((by_size.min_distance.cpu().numpy(), by_size.block.cpu().numpy()),
                separation_from_rows(k["rows"], k["ro"], RADIUS, [0, 36, 72, 96]))
    verdict = separation_ok(by_size, group_sizes=np.repeat([36, 36, 24], [36, 36, 24]))
    assert verdict["complete"].all() and not verdict["clear"].all() and verdict["clear"].any()
    assert np.array_equal(verdict["ok"], by_size.conflicts.cpu().numpy() == 0)
    with pytest.raises(ValueError):
        eng.separation(k["free"], RADIUS, start_rows=np.zeros(5))
    with pytest.raises(ValueError):
        eng.separation(k["free"], RADIUS, groups=0)
    # a RaggedPlan from the obstacle loop goes through, and equals what its rows show
    g = load_golden("fixed_missions.npz")
    wp, aabbs = np.asarray(g["lab_wp"], dtype=np.float64), np.asarray(g["lab_aabbs"], dtype=np.float64)
    rp = eng.plan_collision_free([wp, wp[:4], wp[1:]], aabbs, VEL, DT, strict=False)
    a = eng.separation(rp, RADIUS)
    want = separation_from_rows(rp.traj.cpu().numpy(), rp.row_offsets.cpu().numpy(), RADIUS)
    assert same((a.min_distance.cpu().numpy(), a.block.cpu().numpy()), want)
    v = separation_ok(a, group_sizes=3)
    assert v["complete"].all() and set(v) == {"clear", "complete", "ok"}
