"""Independent airspaces on the GPU: the swept boxes (`uavac_minsnap_envelope_dev`, csrc/minsnap_envelope.hip), the labelling
(`uavac_fleet_airspaces_dev`, csrc/fleet_airspaces.hip) and `Engine.envelope / airspaces / stagger / layer / deconflict(...,
airspaces=True)`.

What is compared with what:
  * the BOXES against `uav_ac.scoring.envelope_from_rows` on the product's own sampled rows, as numbers with NaN in the same places (a
    minimum is exact; -0.0 and +0.0 are the same number), at both settings of "audit_lanes", uniform and ragged; with a reach against
    the hull of the rows of the plan and of `Engine.shift(plan, reach)`, and every row of every layer in between lies inside it;
  * the LABELS and the round count against `uav_ac.scoring.airspaces_from_envelopes` exactly, and against a plain component search;
  * the SEARCHES per airspace against the product's own search over the whole group (`wide=True`, which tests/test_gpu_wide.py holds
    to the rule on sampled rows): the same start rows, steps, layers, blocked counts and the same plan bit for bit; `earlier` against
    the count within the airspace.
The method is tests/test_gpu_layer.py's: sentinel-padded output buffers and `same()` on int32.  A fixture could pass by being trivial,
so before a comparison counts the test asserts on the rule's own answer what the fixture must show (tests/test_airspaces_host.py
`nontrivial`), and for the searches which route the engine has to take.  Missions: tests/test_airspaces_host.py `spread_missions` at
velocity 3, dt 0.02, radius 0.5, start rows (b % 5) * 7."""
import numpy as np
import pytest

from test_airspaces_host import (CUBOIDS_3, DELTA, DT, MAX_LAYERS, RADIUS, VEL, base_starts, components, nontrivial, per_airspace_earlier,
                                 spread_missions)
from test_gpu_layer import PAD, SENT_F, SENT_I, _i32, _i64, _p, product_rows_at, same, same_bits

pytestmark = pytest.mark.gpu

REACH = MAX_LAYERS * DELTA                                  # fl(max_steps * delta) per axis
RAGGED_GROUPS = np.cumsum([0, 63, 64, 65, 1, 0, 129])       # 322 missions


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    return Engine("cuda:0")


_CACHE = {}


def case(eng, B, spread):
    """Per (B, spread), computed once and left unchanged: the plan with rows, the rows-free plan, rows and offsets on the host, and the
    answers of the rules that several tests need."""
    if (B, spread) not in _CACHE:
        wps = spread_missions(B, spread)
        plan = eng.plan(wps, VEL, DT)
        _CACHE[(B, spread)] = dict(plan=plan, free=eng.plan(wps, VEL, DT, rows=False), rows=plan.traj.cpu().numpy(),
                                   ro=plan.row_offsets.cpu().numpy(), at={}, memo={})
    return _CACHE[(B, spread)]


def once(k, key, make):
    if key not in k["memo"]:
        k["memo"][key] = make()
    return k["memo"][key]


def rule_boxes(eng, k, reach=False):
    """`envelope_from_rows` on the product's own rows; `reach`: the hull with the rows of the plan shifted by REACH."""
    from uav_ac.scoring import envelope_from_rows
    return once(k, ("boxes", reach), lambda: envelope_from_rows(k["rows"], k["ro"], product_rows_at(eng, k, DELTA)(MAX_LAYERS) if reach else None))


def parts(plan):
    ragged = hasattr(plan, "seg_offsets")
    return plan.coeffs, plan.seg_rows, plan.seg_offsets if ragged else None, int(plan.B), int(plan.max_m if ragged else plan.m), float(plan.dt)


def same_numbers(got, want):
    return got.shape == want.shape and got.dtype == want.dtype == np.float64 and np.array_equal(got, want, equal_nan=True)


def envelope_abi(eng, plan, reach=None, coeffs=None, seg_rows=None):
    """One call of uavac_minsnap_envelope_dev -> (lo, hi) (B, 3) as NumPy, from the middle of a sentinel-filled buffer: nothing outside
    may be written, and everything inside must be."""
    import torch
    co, sr, so, B, m, dt = parts(plan)
    buf = torch.full((PAD + 6 * B + PAD,), SENT_F, dtype=torch.float64, device=eng.device)
    r = None if reach is None else torch.as_tensor(np.array(np.broadcast_to(reach, (B, 3)), dtype=np.float64, order="C")).to(eng.device)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_envelope_dev", _p(co if coeffs is None else coeffs), _p(sr if seg_rows is None else seg_rows), _p(so), B, m, dt,
                 _p(r), _p(buf[PAD:]))
    torch.cuda.synchronize()
    f = buf.cpu().numpy()
    assert (f[:PAD] == SENT_F).all() and (f[PAD + 6 * B:] == SENT_F).all() and not (f[PAD:PAD + 6 * B] == SENT_F).any()
    env = f[PAD:PAD + 6 * B].reshape(B, 6)
    return env[:, :3].copy(), env[:, 3:].copy()


def labels_abi(eng, lo, hi, radius, go=None, rounds=32, resume=0, labels=None):
    """One call of uavac_fleet_airspaces_dev on boxes from the host -> (labels (B,), info (2,)) as NumPy, from sentinel-padded buffers."""
    import torch
    B = len(lo)
    env = torch.as_tensor(np.ascontiguousarray(np.concatenate([lo, hi], axis=1))).to(eng.device)
    lbuf = torch.full((PAD + B + PAD,), SENT_I, dtype=torch.int32, device=eng.device)
    ibuf = torch.full((PAD + 2 + PAD,), SENT_I, dtype=torch.int32, device=eng.device)
    if labels is not None:
        lbuf[PAD:PAD + B] = _i32(eng, labels)
    g = _i64(eng, go)
    eng._bind_stream()
    eng.ctx.call("uavac_fleet_airspaces_dev", _p(env), _p(g), 0 if go is None else len(go) - 1, B, float(radius), int(rounds), int(resume),
                 _p(lbuf[PAD:]), _p(ibuf[PAD:]))
    torch.cuda.synchronize()
    out = []
    for buf, n in ((lbuf, B), (ibuf, 2)):
        i = buf.cpu().numpy()
        assert (i[:PAD] == SENT_I).all() and (i[PAD + n:] == SENT_I).all() and not (i[PAD:PAD + n] == SENT_I).any()
        out.append(i[PAD:PAD + n].copy())
    return out


class lanes:
    """the ctx option "audit_lanes" for the calls inside, the default again behind them"""
    def __init__(self, eng, value):
        self.eng, self.value = eng, value

    def __enter__(self):
        self.eng.ctx.set_option("audit_lanes", self.value)

    def __exit__(self, *exc):
        self.eng.ctx.set_option("audit_lanes", 16)


# ------------------------------------------------------------------------------------------------------------ 1: the boxes
def test_the_boxes_are_the_minimum_and_maximum_of_the_sampled_rows(eng):
    k = case(eng, 150, 3)
    want = rule_boxes(eng, k)
    assert np.isfinite(want[0]).all() and (want[1] > want[0]).any()
    mixed = np.random.default_rng(5).permutation(150)[:97]
    taken = eng.take(k["free"], mixed)                      # a ragged batch of the same missions
    for n in (16, 64):
        with lanes(eng, n):
            for plan in (k["plan"], k["free"]):
                lo, hi = envelope_abi(eng, plan)
                assert same_numbers(lo, want[0]) and same_numbers(hi, want[1]), n
            lo, hi = envelope_abi(eng, taken)
            assert same_numbers(lo, want[0][mixed]) and same_numbers(hi, want[1][mixed]), n
    env = eng.envelope(k["free"])
    assert same_numbers(env.lo.cpu().numpy(), want[0]) and same_numbers(env.hi.cpu().numpy(), want[1]) and tuple(env.block.shape) == (150, 6)


def test_with_a_reach_the_box_is_the_hull_and_holds_every_layer(eng):
    from uav_ac.scoring import envelope_from_rows
    k = case(eng, 150, 3)
    want = rule_boxes(eng, k, reach=True)
    plain = rule_boxes(eng, k)
    assert (want[0][:, 2] < plain[0][:, 2]).all() and np.array_equal(want[1], plain[1])           # NED: the layers go up, z falls
    for n in (16, 64):
        with lanes(eng, n):
            lo, hi = envelope_abi(eng, k["free"], REACH)
            assert same_numbers(lo, want[0]) and same_numbers(hi, want[1]), n
    rows_at = product_rows_at(eng, k, DELTA)
    for q in range(MAX_LAYERS + 1):                         # every row of every layer lies inside
        lq, hq = envelope_from_rows(rows_at(q), k["ro"])
        assert (lq >= want[0]).all() and (hq <= want[1]).all(), q
    # a reach per mission; one that is all zero is not added: that mission's box is the plain one
    per = np.tile(REACH, (150, 1))
    per[::3] = 0.0
    lo, hi = envelope_abi(eng, k["free"], per)
    pick = np.arange(150) % 3 == 0
    assert same_numbers(lo, np.where(pick[:, None], plain[0], want[0])) and same_numbers(hi, want[1])
    for reach in (REACH, per):
        env = eng.envelope(k["free"], reach)
        assert same_numbers(env.lo.cpu().numpy(), lo if reach is per else want[0])
    with pytest.raises(ValueError, match="reach"):
        eng.envelope(k["free"], np.zeros((149, 3)))


def test_a_mission_without_a_box_reports_nan_and_leaves_its_neighbours_alone(eng):
    k = case(eng, 150, 3)
    want = rule_boxes(eng, k)
    free = k["free"]
    co = free.coeffs.clone()
    co[7, 5, 1] = float("nan")                              # a coefficient of mission 7's first segment
    co[20, 8 + 0, 2] = float("inf")                         # c0 of mission 20's second segment
    sr = free.seg_rows.clone()
    sr[33] = 0                                              # mission 33 has no rows at all
    sr[40, 1] = 0                                           # mission 40 lacks a segment: the box of the others' rows
    gone = [7, 20, 33]
    for n in (16, 64):
        with lanes(eng, n):
            for reach in (None, REACH):
                lo, hi = envelope_abi(eng, free, reach, coeffs=co, seg_rows=sr)
                assert np.isnan(lo[gone]).all() and np.isnan(hi[gone]).all()
                if reach is None:
                    keep = np.setdiff1d(np.arange(150), gone + [40])
                    assert same_numbers(lo[keep], want[0][keep]) and same_numbers(hi[keep], want[1][keep])
                    assert np.isfinite(lo[40]).all() and (lo[40] >= want[0][40]).all() and (hi[40] <= want[1][40]).all()
    lo, hi = envelope_abi(eng, free, np.array([0.0, np.nan, 0.0]))                     # a NaN reach: no box for anybody
    assert np.isnan(lo).all() and np.isnan(hi).all()


# ------------------------------------------------------------------------------------------------------------ 2: the labels
def check_labels(eng, lo, hi, radius, go=None):
    from uav_ac.scoring import airspaces_from_envelopes
    want, changed, converged = airspaces_from_envelopes(lo, hi, radius, go)
    truth, link = components(lo, hi, radius, go)
    assert converged and np.array_equal(want, truth)
    labels, info = labels_abi(eng, lo, hi, radius, go)
    assert same(labels, want) and info.tolist() == [changed, 1], (info, changed)
    # one round per call, resumed to convergence: the same labels, the same count
    lab, total, calls = None, 0, 0
    while True:
        lab, info1 = labels_abi(eng, lo, hi, radius, go, rounds=1, resume=0 if lab is None else 1, labels=lab)
        step = airspaces_from_envelopes(lo, hi, radius, go, rounds=calls + 1)
        assert same(lab, step[0]), calls
        total, calls = total + int(info1[0]), calls + 1
        assert info1.tolist() in ([1, 0], [0, 1]) and calls <= changed + 1
        if info1[1]:
            break
    assert same(lab, want) and total == changed and calls == changed + 1
    return want, link, changed


def test_the_labels_are_the_rules_with_no_groups(eng):
    k = case(eng, 150, 3)
    lo, hi = rule_boxes(eng, k)
    labels, link, changed = check_labels(eng, lo, hi, RADIUS)
    nontrivial(labels, link)
    assert changed >= 3
    # too few rounds: info says so, and the labels are a finer partition
    short, info = labels_abi(eng, lo, hi, RADIUS, rounds=2)
    assert info.tolist() == [2, 0] and (short >= labels).all() and (short != labels).any()
    # a NaN box links to nobody
    lo2, hi2 = lo.copy(), hi.copy()
    hub = int(np.argmax(link.sum(axis=1)))
    lo2[hub, 1] = np.nan
    labels2, link2, _ = check_labels(eng, lo2, hi2, RADIUS)
    assert not link2[hub].any() and (labels2 == hub).sum() == 1


def test_the_labels_with_ragged_groups_radius_zero_and_one_airspace(eng):
    k = case(eng, 322, 4)
    lo, hi = rule_boxes(eng, k)
    labels, link, _ = check_labels(eng, lo, hi, RADIUS, RAGGED_GROUPS)
    nontrivial(labels, link)
    for g0, g1 in zip(RAGGED_GROUPS[:-1], RAGGED_GROUPS[1:]):
        assert ((labels[g0:g1] >= g0) & (labels[g0:g1] < g1)).all()                      # no airspace crosses a group
    whole, _, _ = check_labels(eng, lo, hi, RADIUS)
    assert len(np.unique(whole)) < len(np.unique(labels))                                  # (the groups cut links)
    zero, link0, _ = check_labels(eng, lo, hi, 0.0, RAGGED_GROUPS)
    assert link0.sum() < link.sum() and len(np.unique(zero)) > len(np.unique(labels)) and (np.bincount(zero) >= 2).any()
    far = float(np.nanmax(hi) - np.nanmin(lo)) + 1.0                                       # a radius that links everything
    one, _, changed = check_labels(eng, lo, hi, far)
    assert (one == 0).all() and changed == 1
    grouped, _, _ = check_labels(eng, lo, hi, far, RAGGED_GROUPS)
    assert sorted(set(grouped.tolist())) == [0, 63, 127, 192, 193]


def test_engine_airspaces_chains_boxes_labels_order_and_offsets(eng):
    from uav_ac.scoring import airspace_order, airspaces_from_envelopes
    k = case(eng, 322, 4)
    for reach, groups in ((None, None), (REACH, RAGGED_GROUPS)):
        lo, hi = rule_boxes(eng, k, reach is not None)
        labels, changed, _ = airspaces_from_envelopes(lo, hi, RADIUS, groups)
        order, rank, offs = airspace_order(labels, groups)
        for rounds in (32, 1):                              # one round per call: the engine resumes until the labels are final
            a = eng.airspaces(k["free"], RADIUS, groups, reach, rounds=rounds)
            assert same(a.labels.cpu().numpy(), labels) and same(a.order.cpu().numpy(), order) and same(a.rank.cpu().numpy(), rank)
            assert np.array_equal(a.offsets_host, offs) and np.array_equal(a.offsets.cpu().numpy(), offs) and a.offsets_host.dtype == np.int64
            assert np.array_equal(a.sizes_host, np.diff(offs)) and a.largest == np.diff(offs).max() and a.rounds == changed
    for bad in (dict(radius=-1.0), dict(radius=float("nan")), dict(radius=RADIUS, rounds=0)):
        with pytest.raises(ValueError):
            eng.airspaces(k["free"], **bad)


# ------------------------------------------------------------------------------------------------------------ 3: the searches
def cuboids_for(spread):
    return CUBOIDS_3 * np.array([spread / 3.0, spread / 3.0, spread / 3.0, spread / 3.0, 1.0, 1.0])


def route(eng, k, spread, reach):
    """The airspaces of the rule for a search case, and the assertion that the case takes the route it is there for."""
    from uav_ac.scoring import airspaces_from_envelopes
    labels = once(k, ("labels", reach), lambda: airspaces_from_envelopes(*rule_boxes(eng, k, reach), RADIUS)[0])
    sizes = np.bincount(labels)
    assert (sizes > 0).sum() >= 2 and len(labels) > 256
    assert sizes.max() > 256 if spread == 3 else sizes.max() <= 256, sizes.max()            # wide route / narrow route
    return labels


@pytest.mark.parametrize("spread", (3, 4))
def test_stagger_per_airspace_is_stagger_over_the_whole_group(eng, spread):
    B = 300
    k = case(eng, B, spread)
    labels = route(eng, k, spread, False)
    start = base_starts(B)
    whole = once(k, "stagger", lambda: eng.stagger(k["free"], RADIUS, start_rows=start, wide=True))
    split = eng.stagger(k["free"], RADIUS, start_rows=start, airspaces=True)
    w, s = whole.block.cpu().numpy(), split.block.cpu().numpy()
    assert (w[1] > 0).any() and (w[1] == -1).any() and not (w[1] == -2).any(), np.unique(w[1], return_counts=True)
    assert same(s[:2], w[:2])                                                            # start rows and steps
    assert same(s[2], per_airspace_earlier(labels, w[1] != -2)) and (s[2] != w[2]).any()
    assert eng.take_flags() == [0, 0, 0, 0]


@pytest.mark.parametrize("spread", (3, 4))
def test_layer_and_deconflict_per_airspace_are_those_of_the_whole_group(eng, spread):
    B = 300
    k = case(eng, B, spread)
    labels = route(eng, k, spread, True)
    cub = cuboids_for(spread)
    granted = once(k, "stagger", lambda: eng.stagger(k["free"], RADIUS, start_rows=base_starts(B), wide=True)).start_rows
    kw = dict(start_rows=granted, delta=DELTA, max_steps=MAX_LAYERS, obstacles=cub)
    whole = eng.layer(k["free"], RADIUS, wide=True, **kw)
    split = eng.layer(k["free"], RADIUS, airspaces=True, **kw)
    w, s = whole.block.cpu().numpy(), split.block.cpu().numpy()
    assert (w[0] > 0).any() and (w[1] == -1).any() and (w[3] > 0).any(), "nobody moved, unresolved or blocked"
    assert same(s[[0, 1, 3]], w[[0, 1, 3]])                                              # layer, steps, blocked
    assert same(s[2], per_airspace_earlier(labels, w[1] != -2)) and (s[2] != w[2]).any()
    assert same_bits(split.offsets.cpu().numpy(), whole.offsets.cpu().numpy())
    # the chain as one call: the plan to fly, bit for bit
    kw = dict(obstacles=cub, start_rows=base_starts(B), delta=DELTA, max_layers=MAX_LAYERS)
    a, b = eng.deconflict(k["free"], RADIUS, wide=True, **kw), eng.deconflict(k["free"], RADIUS, airspaces=True, **kw)
    assert same(b.stagger.block.cpu().numpy()[:2], a.stagger.block.cpu().numpy()[:2])
    assert same(b.layer.block.cpu().numpy()[[0, 1, 3]], w[[0, 1, 3]]) and same(a.layer.block.cpu().numpy(), w)
    assert np.array_equal(a.resolved.cpu().numpy(), b.resolved.cpu().numpy())
    assert np.array_equal(a.plan.seg_offsets_host, b.plan.seg_offsets_host) and a.plan.total_rows == b.plan.total_rows
    for name in ("coeffs", "times"):
        assert same_bits(getattr(a.plan, name).cpu().numpy(), getattr(b.plan, name).cpu().numpy()), name
    assert same(a.plan.seg_rows.cpu().numpy(), b.plan.seg_rows.cpu().numpy())
    assert eng.take_flags() == [0, 0, 0, 0]


def test_a_priority_orders_the_missions_within_an_airspace(eng):
    B = 300
    k = case(eng, B, 4)
    route(eng, k, 4, False)
    priority = np.random.default_rng(11).permutation(B).astype(np.float64)
    start = base_starts(B)
    whole = eng.stagger(k["free"], RADIUS, start_rows=start, priority=priority, wide=True).block.cpu().numpy()
    split = eng.stagger(k["free"], RADIUS, start_rows=start, priority=priority, airspaces=True).block.cpu().numpy()
    plain = once(k, "stagger", lambda: eng.stagger(k["free"], RADIUS, start_rows=start, wide=True)).block.cpu().numpy()
    assert (whole[1] != plain[1]).any() and (whole[1] > 0).any()                         # the priority matters here
    assert same(split[:2], whole[:2])
    tied = np.zeros(B)                                                                    # all tied: the batch order
    assert same(eng.stagger(k["free"], RADIUS, start_rows=start, priority=tied, airspaces=True).block.cpu().numpy()[:2], plain[:2])
    assert eng.take_flags() == [0, 0, 0, 0]


def test_without_the_keyword_nothing_changes(eng):
    k = case(eng, 150, 3)
    start, groups, cub = base_starts(150), 50, cuboids_for(3)
    for call, kw in ((eng.stagger, dict(start_rows=start)), (eng.layer, dict(start_rows=start, delta=DELTA, max_steps=MAX_LAYERS)),
                     (eng.layer, dict(start_rows=start, delta=DELTA, max_steps=MAX_LAYERS, obstacles=cub)),
                     (eng.stagger, dict(start_rows=start, wide=True)), (eng.stagger, dict(start_rows=start, priority=-np.arange(150.0)))):
        a, b = call(k["free"], RADIUS, groups, **kw), call(k["free"], RADIUS, groups, airspaces=False, **kw)
        assert same(a.block.cpu().numpy(), b.block.cpu().numpy())
    a = eng.deconflict(k["free"], RADIUS, groups, obstacles=cub, start_rows=start)
    b = eng.deconflict(k["free"], RADIUS, groups, obstacles=cub, start_rows=start, airspaces=False)
    assert same(a.stagger.block.cpu().numpy(), b.stagger.block.cpu().numpy()) and same(a.layer.block.cpu().numpy(), b.layer.block.cpu().numpy())
    assert same_bits(a.plan.coeffs.cpu().numpy(), b.plan.coeffs.cpu().numpy()) and same(a.plan.seg_rows.cpu().numpy(), b.plan.seg_rows.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------ 4: the refusals
def test_refusals_come_before_anything_is_written(eng):
    import torch
    from uav_ac import _native as nat
    free = case(eng, 150, 3)["free"]
    B, m = 150, 3
    fbuf = torch.full((6 * B + PAD,), SENT_F, dtype=torch.float64, device=eng.device)
    ibuf = torch.full((B + 2 + PAD,), SENT_I, dtype=torch.int32, device=eng.device)
    env = eng.envelope(free).block
    reach = torch.zeros((B, 3), dtype=torch.float64, device=eng.device)
    good_e = dict(coeffs=free.coeffs, seg_rows=free.seg_rows, seg_offsets=None, B=B, m=m, dt=DT, reach=reach, env=fbuf)
    bad_e = (dict(coeffs=None), dict(seg_rows=None), dict(env=None), dict(B=0), dict(m=0), dict(m=nat.MAX_SEGMENTS + 1), dict(dt=0.0),
             dict(dt=-DT), dict(dt=float("nan")), dict(dt=float("inf")))
    go = _i64(eng, [0, 100, B])
    good_a = dict(env=env, go=go, G=2, B=B, radius=RADIUS, rounds=4, resume=0, labels=ibuf, info=ibuf[B:])
    bad_a = (dict(env=None), dict(labels=None), dict(info=None), dict(B=0), dict(G=0), dict(radius=-0.5), dict(radius=float("inf")),
             dict(radius=float("nan")), dict(rounds=0), dict(rounds=-3), dict(resume=2), dict(resume=-1))

    def call_e(ctx, a):
        return nat.lib().uavac_minsnap_envelope_dev(ctx, _p(a["coeffs"]), _p(a["seg_rows"]), _p(a["seg_offsets"]), a["B"], a["m"], a["dt"],
                                                    _p(a["reach"]), _p(a["env"]))

    def call_a(ctx, a):
        return nat.lib().uavac_fleet_airspaces_dev(ctx, _p(a["env"]), _p(a["go"]), a["G"], a["B"], a["radius"], a["rounds"], a["resume"],
                                                   _p(a["labels"]), _p(a["info"]))
    eng._bind_stream()
    for call, good, bad in ((call_e, good_e, bad_e), (call_a, good_a, bad_a)):
        for change in bad:
            rc = call(eng.ctx._h, {**good, **change})
            assert rc == nat.EINVAL, (change, rc)
            assert (nat.lib().uavac_last_error(eng.ctx._h) or b"") != b"", change
        assert call(None, good) == nat.EINVAL                                            # no context
    torch.cuda.synchronize()
    assert bool((fbuf == SENT_F).all()) and bool((ibuf == SENT_I).all())
    # the same calls with nothing wrong go through, within their bounds; G is ignored without offsets and reach may be NULL
    assert call_e(eng.ctx._h, good_e) == nat.OK and call_e(eng.ctx._h, {**good_e, "reach": None}) == nat.OK
    assert call_a(eng.ctx._h, good_a) == nat.OK and call_a(eng.ctx._h, {**good_a, "go": None, "G": -1}) == nat.OK
    torch.cuda.synchronize()
    assert not bool((fbuf[:6 * B] == SENT_F).any()) and bool((fbuf[6 * B:] == SENT_F).all())
    assert not bool((ibuf[:B + 2] == SENT_I).any()) and bool((ibuf[B + 2:] == SENT_I).all())
