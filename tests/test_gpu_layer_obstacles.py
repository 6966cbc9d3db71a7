"""Offset layers that keep out of cuboids, and the fleet chain as one call, on the GPU (`uavac_minsnap_layer_obs_dev`,
csrc/minsnap_layer_obs.hip), through the C ABI, `Engine.layer(..., obstacles=)` and `Engine.deconflict`.

The method is tests/test_gpu_layer.py's, and its mission sets, its memoised product rows and its helpers are taken from that module
(one cache for both files): sentinel-padded output buffers, `same()` on int32, and
  * the SEARCH against the PRODUCT'S OWN ROWS exactly, all four rows: `uav_ac.scoring.layer_obstacles_from_rows` with rows_at(q) = the
    rows the sampler writes for `Engine.shift(plan, q * delta)`.  The kernel evaluates the same coefficients with the sampler's
    arithmetic and tests them with the audit's comparison, so every output is an integer decided by comparisons on the same doubles;
  * the search against the ORACLE (oracle.c_oracle.plan_threads; rows_at(q) = rows[:, :3] + q * delta) with a cap of 0 differing
    missions.  Every decision is a comparison of a position with a face or of a distance with the radius: the test first recomputes,
    on the oracle's rows, how far the nearest cuboid decision is from a face and the nearest pair decision from the radius, and asserts
    both >= 1e-4 -- the bar of tests/test_gpu_layer.py and its reason: twenty times what positions at the project's 1e-5 bar can move
    a distance.  Measured on the CPU for the three configurations, in order: faces 1.8e-3, 1.2e-3, 2.8e-3; radius 5.5e-2, 7.0e-4, 1.3e-2.
The cuboids' faces lie off the grid of the waypoints on purpose (round faces put samples exactly on a face).  The sets are the smallest
that still reach a second candidate round (layers beyond 63) and a second j-tile (groups above 64)."""
import ctypes as C
import math

import numpy as np
import pytest

import test_gpu_layer as base
from test_gpu_layer import DT, PAD, SENT_F, SENT_I, TILE, VEL, _i32, _i64, _p, case, offsets, product_rows_at, same, same_bits, up

pytestmark = pytest.mark.gpu

# (m, B, radius, dz, max_steps, group size); delta = (0, 0, -dz)
CONFIGS = ((8, 96, 0.5, 0.25, 15, 32), (8, 96, 0.5, 0.025, 80, 96), (20, 24, 1.0, 0.03, 90, 24))
CUBOIDS = np.array([[11.13, 12.37, 6.21, 7.43, -20.0, 20.0],        # pillar: every upward layer blocked for who crosses it
                    [3.17, 21.29, 1.61, 15.83, -4.613, -4.087],     # slab: a band of layers blocked
                    [22.31, 25.87, 11.19, 14.57, -9.011, -2.203],
                    [1.09, 4.91, -1.27, 2.33, -5.897, -3.511]])
MARGIN = 1e-4
IDS = dict(ids=lambda c: "m%d-B%d-r%g-dz%g-max%d-groups%d" % c)


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    return Engine("cuda:0")


def _f64(eng, a):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(eng.device)


def obs_abi(eng, coeffs, seg_rows, seg_offsets, B, m, dt, cuboids=CUBOIDS, go=None, start=None, radius=0.5, delta=(0.0, 0.0, -0.25),
            max_steps=63):
    """One call of uavac_minsnap_layer_obs_dev -> (ilayer (4, B), offsets (B, 3)) as NumPy.  Each output is the middle of a larger
    sentinel-filled buffer: nothing outside may be written, and everything inside must be."""
    import torch
    ibuf = torch.full((PAD + 4 * B + PAD,), SENT_I, dtype=torch.int32, device=eng.device)
    fbuf = torch.full((PAD + 3 * B + PAD,), SENT_F, dtype=torch.float64, device=eng.device)
    g, s = _i64(eng, go), _i32(eng, start)
    n = 0 if cuboids is None else len(cuboids)
    cub = _f64(eng, cuboids) if n else None
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_layer_obs_dev", _p(coeffs), _p(seg_rows), _p(seg_offsets), int(B), int(m), float(dt), _p(g),
                 0 if go is None else len(go) - 1, _p(s), float(radius), float(delta[0]), float(delta[1]), float(delta[2]), int(max_steps),
                 _p(cub), n, _p(ibuf[PAD:]), _p(fbuf[PAD:]))
    torch.cuda.synchronize()
    i, f = ibuf.cpu().numpy(), fbuf.cpu().numpy()
    assert (i[:PAD] == SENT_I).all() and (i[PAD + 4 * B:] == SENT_I).all() and not (i[PAD:PAD + 4 * B] == SENT_I).any()
    assert (f[:PAD] == SENT_F).all() and (f[PAD + 3 * B:] == SENT_F).all() and not (f[PAD:PAD + 3 * B] == SENT_F).any()
    il, off = i[PAD:PAD + 4 * B].reshape(4, B).copy(), f[PAD:PAD + 3 * B].reshape(B, 3).copy()
    assert np.array_equal(off, il[0][:, None] * np.asarray(delta, dtype=np.float64)[None, :])       # the granted fl(layer * delta)
    return il, off


def obs_of_plan(eng, plan, **kw):
    ragged = hasattr(plan, "seg_offsets")
    return obs_abi(eng, plan.coeffs, plan.seg_rows, plan.seg_offsets if ragged else None, plan.B, plan.max_m if ragged else plan.m,
                   plan.dt, **kw)[0]


_RULE = {}


def rule(eng, cfg):
    """What the rule gives on the product's own rows for a configuration: computed once, shared by the tests that need it."""
    if cfg not in _RULE:
        from uav_ac.scoring import layer_obstacles_from_rows
        m, B, radius, dz, max_steps, size = cfg
        k = case(eng, m, B)
        _RULE[cfg] = layer_obstacles_from_rows(product_rows_at(eng, k, up(dz)), k["ro"], radius, CUBOIDS, offsets(B, size), None, max_steps)
    return _RULE[cfg]


def kinds(il, go):
    first = [int(il[0, b]) for b in go[:-1]]
    return dict(blocked=int((il[3] > 0).sum()), unresolved=int((il[1] == -1).sum()), later_round=int((il[1] >= TILE).sum()),
                first_of_group=first, unresolved_and_blocked=int(((il[1] == -1) & (il[3] > 0)).sum()))


def differ(got, want):
    bad = (got != want).any(axis=0)
    return np.flatnonzero(bad)[:8], got[:, bad][:, :8], want[:, bad][:, :8]


# ------------------------------------------------------------------------------------------------ 1: the product's own rows
@pytest.mark.parametrize("cfg", CONFIGS, **IDS)
def test_the_search_equals_the_rule_on_the_products_rows(eng, cfg):
    m, B, radius, dz, max_steps, size = cfg
    k = case(eng, m, B)
    want = rule(eng, cfg)
    go = offsets(B, size)
    kw = dict(go=go, radius=radius, delta=up(dz), max_steps=max_steps)
    got_free, got_rows = obs_of_plan(eng, k["free"], **kw), obs_of_plan(eng, k["plan"], **kw)
    assert same(got_free, got_rows), cfg
    assert same(got_free, want), (cfg, differ(got_free, want))
    n = kinds(want, go)
    plain = base.layer_of_plan(eng, k["free"], **kw)
    print(f"layer with obstacles {cfg}: {n}, highest layer {int(want[0].max())}, granted layer differs from the plain search for "
          f"{int((plain[0] != want[0]).sum())}")
    assert n["blocked"] > 0 and n["unresolved"] > 0 and (plain[0] != want[0]).any(), n      # the sets cannot go trivial
    if size != 24:                                           # (the one group of 24: its first mission meets no cuboid)
        assert max(n["first_of_group"]) > 0, n               # the first of a group is moved by a cuboid
        assert ((want[1] > 0) & (want[3] == 0) & (want[2] > 0)).any()                       # and somebody by partners alone
    if max_steps >= TILE:
        assert n["later_round"] > 0, n                       # the second candidate round grants
    assert (want[0] == np.maximum(want[1], 0)).all() and (want[3] <= np.where(want[1] < 0, max_steps + 1, want[1])).all()


def test_a_sideways_delta_lets_the_x_and_y_bounds_decide(eng):
    from uav_ac.scoring import layer_obstacles_from_rows
    B, delta = 96, np.array([0.3, 0.1, 0.0])
    k = case(eng, 8, B)
    go = offsets(B, 32)
    want = layer_obstacles_from_rows(product_rows_at(eng, k, delta), k["ro"], 0.5, CUBOIDS, go, None, 15)
    got = obs_of_plan(eng, k["free"], go=go, delta=delta, max_steps=15)
    assert same(got, want), differ(got, want)
    # z never changes, so every freed mission left a cuboid through an x or y face
    assert ((want[1] > 0) & (want[3] > 0)).any() and (want[1] == -1).any() and ((want[1] == 0) & (want[2] > 0)).any()


def test_groups_of_one_tile_one_less_one_more_and_two_tiles(eng):
    from uav_ac.scoring import layer_obstacles_from_rows
    k = case(eng, 8, 192)
    free = k["free"]
    for go, dz, max_steps in (([0, TILE - 1, 2 * TILE - 1, 192], 0.125, 15), ([0, 2 * TILE + 1, 192], 0.25, 5)):
        want = layer_obstacles_from_rows(product_rows_at(eng, k, up(dz)), k["ro"], 0.5, CUBOIDS, go, None, max_steps)
        got = obs_of_plan(eng, free, go=np.array(go), delta=up(dz), max_steps=max_steps)
        assert same(got, want), (go, differ(got, want))
        assert (want[3] > 0).any() and (want[1] > 0).any()
        if go[1] > TILE:                                     # the second j-tile decides something, and cuboids block past index 64
            assert (want[1, TILE:go[1]] > 0).any() and (want[3, TILE:go[1]] > 0).any()


def test_a_ragged_batch_with_fixed_starts(eng):
    from uav_ac.scoring import layer_obstacles_from_rows
    mix = base.ragged_mix(eng)
    free, with_rows = mix["free"], mix["with_rows"]
    ro = with_rows.row_offsets.cpu().numpy()
    kk = mix.setdefault("obs_rows", dict(free=free, at={}))
    delta = np.array([0.25, 0.0, -0.125])
    for go, st in ((None, (np.arange(45) % 4) * 53 + 11), (np.array([0, 1, 15, 15, 45]), (np.arange(45) % 5) * 37)):
        want = layer_obstacles_from_rows(product_rows_at(eng, kk, delta), ro, 0.5, CUBOIDS, go, st, 9)
        assert same(obs_of_plan(eng, free, go=go, start=st, delta=delta, max_steps=9), want), go
        assert same(obs_of_plan(eng, with_rows, go=go, start=st, delta=delta, max_steps=9), want), go
        assert (want[3] > 0).any() and (want[1] > 0).any() and (want[1] == 0).any()
    # the uniform set with uneven groups and non-zero starts
    B = 96
    k = case(eng, 8, B)
    go, st = np.array([0, 1, B // 3, B // 3, B]), (np.arange(B) % 5) * 37
    want = layer_obstacles_from_rows(product_rows_at(eng, k, up(0.25)), k["ro"], 0.5, CUBOIDS, go, st, 7)
    assert same(obs_of_plan(eng, k["free"], go=go, start=st, max_steps=7), want)
    assert not same(want, layer_obstacles_from_rows(product_rows_at(eng, k, up(0.25)), k["ro"], 0.5, CUBOIDS, go, None, 7))


# ------------------------------------------------------------------------------------------------------------ 2: the oracle
def inside_measure(p, cuboids):
    """(rows, 3) positions -> the largest, over rows and cuboids, of min(x - xmin, xmax - x, ..., zmax - z): >= 0 iff a row lies inside a
    cuboid (inclusive), and its absolute value is how far the nearest row is from changing that."""
    worst = -np.inf
    for x in cuboids:
        s = np.minimum.reduce([p[:, 0] - x[0], x[1] - p[:, 0], p[:, 1] - x[2], x[3] - p[:, 1], p[:, 2] - x[4], x[5] - p[:, 2]])
        worst = max(worst, float(s.max()))
    return worst


def decision_margins(rows_at, ro, radius, cuboids, go, il, max_steps):
    """On these rows (starts 0): the smallest |inside measure| of an examined candidate -- how far the nearest cuboid decision is from
    a face -- and the smallest |minimum distance - radius| of an examined candidate that no cuboid blocks -- how far the nearest pair
    decision is from the radius.  Examined are the candidates q = 0 .. steps of a resolved mission and all of an unresolved one."""
    N = np.diff(ro)
    face, pair = np.inf, np.inf
    for g in range(len(go) - 1):
        done = []
        for i in range(int(go[g]), int(go[g + 1])):
            if il[1, i] == -2:
                continue
            last = max_steps if il[1, i] < 0 else int(il[1, i])
            if done:
                kk = np.arange(max(max(int(N[j]) for j in done), int(N[i])))
                others = np.stack([rows_at(int(il[0, j]))[ro[j] + np.minimum(kk, N[j] - 1), 0:3] for j in done])
                at = ro[i] + np.minimum(kk, N[i] - 1)
            blocked = 0
            for q in range(last + 1):
                s = inside_measure(rows_at(q)[ro[i]:ro[i + 1], 0:3], cuboids)
                face = min(face, abs(s))
                if s >= 0:
                    blocked += 1
                    continue
                if done:
                    own = rows_at(q)[at, 0:3]
                    d = math.sqrt(float(((own[None] - others) ** 2).sum(axis=2).min()))
                    pair = min(pair, abs(d - radius))
            assert blocked == il[3, i], (i, blocked, il[:, i])
            done.append(i)
    return face, pair


@pytest.mark.parametrize("cfg", CONFIGS, **IDS)
def test_the_search_against_the_oracle(eng, cfg):
    from oracle import c_oracle as cc
    from uav_ac.scoring import layer_obstacles_from_rows
    m, B, radius, dz, max_steps, size = cfg
    k = case(eng, m, B)
    ref = cc.plan_threads(k["wps"], VEL, DT)
    rows, ro = ref["rows"], ref["row_offsets"]
    assert np.array_equal(ro, k["ro"])                                                 # row counts are exact
    go = offsets(B, size)
    memo = {}

    def rows_at(q):
        if q not in memo:
            memo[q] = rows[:, 0:3] + q * up(dz)
        return memo[q]
    want = layer_obstacles_from_rows(rows_at, ro, radius, CUBOIDS, go, None, max_steps)
    face, pair = decision_margins(rows_at, ro, radius, CUBOIDS, go, want, max_steps)
    print(f"layer with obstacles vs oracle {cfg}: nearest cuboid decision {face:.3e} from a face, nearest pair decision {pair:.3e} from "
          f"the radius; {kinds(want, go)}")
    assert face >= MARGIN and pair >= MARGIN, (face, pair)
    got = obs_of_plan(eng, k["free"], go=go, radius=radius, delta=up(dz), max_steps=max_steps)
    differing = int((got != want).any(axis=0).sum())
    assert differing == 0 and same(got, want), (cfg, differing, differ(got, want))
    assert same(got, rule(eng, cfg))


# ------------------------------------------------------------------------------------------------- 3: the guarantee, end to end
def resolved_alone(eng, shifted, keep, go, m, start=None):
    """The separation audit of the missions `keep` of a uniform shifted batch as a batch of their own, in their groups."""
    import torch
    from types import SimpleNamespace
    sel = torch.as_tensor(keep, device=eng.device)
    B = shifted.B
    sub = SimpleNamespace(coeffs=shifted.coeffs.reshape(B, 8 * m, 3)[sel].contiguous(), seg_rows=shifted.seg_rows.reshape(B, m)[sel].contiguous(),
                          B=len(keep), m=m, dt=DT)
    return sub, np.searchsorted(keep, go), None if start is None else start[sel].contiguous()


def test_the_audits_of_the_shifted_plan_confirm_the_granted_layers_and_show_the_hole(eng):
    from uav_ac.scoring import blocked_out, layer_ok
    cfg = CONFIGS[0]
    m, B, radius, dz, max_steps, size = cfg
    k = case(eng, m, B)
    free, go = k["free"], offsets(B, size)
    res = eng.layer(free, radius, groups=size, delta=up(dz), max_steps=max_steps, obstacles=CUBOIDS)
    assert res.layers.is_cuda and res.block.shape == (4, B) and res.offsets.shape == (B, 3) and res.blocked.shape == (B,)
    block = res.block.cpu().numpy()
    assert np.array_equal(block, np.stack([t.cpu().numpy() for t in (res.layers, res.steps, res.earlier, res.blocked)]))
    assert same(block, rule(eng, cfg))
    ok = layer_ok(res)
    assert ok["examined"].all() and np.array_equal(ok["resolved"], block[1] >= 0) and not ok["resolved"].all()
    assert np.array_equal(blocked_out(res, max_steps), (block[1] == -1) & (block[3] == max_steps + 1)) and blocked_out(res, max_steps).any()
    shifted = eng.shift(free, res.offsets)
    hits = eng.audit(shifted, CUBOIDS).hit_rows.cpu().numpy()                          # (4, B)
    assert (hits[:, ok["resolved"]] == 0).all()              # no row of a resolved mission inside any cuboid
    keep = np.flatnonzero(ok["resolved"])
    sub, sub_go, _ = resolved_alone(eng, shifted, keep, go, m)
    alone = eng.separation(sub, radius, groups=sub_go)
    assert int(alone.conflicts.sum()) == 0 and bool((alone.first_conflict == -1).all())  # no pair of resolved missions inside the radius
    # the hole this closes: the search without obstacles resolves missions INTO a cuboid
    plain = eng.layer(free, radius, groups=size, delta=up(dz), max_steps=max_steps)
    assert plain.block.shape == (3, B) and plain.blocked is None
    plain_hits = eng.audit(eng.shift(free, plain.offsets), CUBOIDS).hit_rows.cpu().numpy()
    inside = (plain_hits > 0).any(axis=0) & (plain.steps.cpu().numpy() >= 0)
    print(f"layer with obstacles, the guarantee: {int(ok['resolved'].sum())} of {B} resolved and outside every cuboid; the search "
          f"without obstacles leaves {int(inside.sum())} resolved missions inside a cuboid")
    assert inside.sum() > 0
    # the other forms of `groups`, a plan with rows, obstacles as a tensor
    again = eng.layer(k["plan"], radius, groups=_i64(eng, go), delta=up(dz), max_steps=max_steps, obstacles=_f64(eng, CUBOIDS))
    assert np.array_equal(again.block.cpu().numpy(), block) and same_bits(again.offsets.cpu().numpy(), res.offsets.cpu().numpy())


# ------------------------------------------------------------------------------------------- 4: identity and reproducibility
def test_without_cuboids_the_answers_are_the_plain_searchs(eng):
    for cfg in CONFIGS[:2]:
        m, B, radius, dz, max_steps, size = cfg
        k = case(eng, m, B)
        free = k["free"]
        kw = dict(go=offsets(B, size), radius=radius, delta=up(dz), max_steps=max_steps)
        want, want_off = base.layer_abi(eng, free.coeffs, free.seg_rows, None, B, m, DT, **kw)
        for none in (None, np.zeros((0, 6))):
            got, off = obs_abi(eng, free.coeffs, free.seg_rows, None, B, m, DT, cuboids=none, **kw)
            assert same(np.ascontiguousarray(got[:3]), want) and (got[3] == 0).all() and same_bits(off, want_off)
        res = eng.layer(free, radius, groups=size, delta=up(dz), max_steps=max_steps, obstacles=np.zeros((0, 6)))
        assert res.block.shape == (4, B) and same(np.ascontiguousarray(res.block.cpu().numpy()[:3]), want)
        assert bool((res.blocked == 0).all()) and same_bits(res.offsets.cpu().numpy(), want_off)
        # cuboids that contain nothing: NaN bounds, inverted boxes
        nothing = np.array([[np.nan, 30.0, -30.0, 30.0, -30.0, 30.0], [-30.0, 30.0, -30.0, np.nan, -30.0, 30.0],
                            [30.0, -30.0, -30.0, 30.0, -30.0, 30.0], [-30.0, 30.0, -30.0, 30.0, 30.0, -30.0]])
        got = obs_of_plan(eng, free, cuboids=nothing, **kw)
        assert same(np.ascontiguousarray(got[:3]), want) and (got[3] == 0).all()


def test_sixteen_cuboids_a_group_alone_other_company_and_a_second_call(eng):
    import torch
    cfg = CONFIGS[0]
    m, B, radius, dz, max_steps, size = cfg
    k = case(eng, m, B)
    free, want = k["free"], rule(eng, cfg)
    kw = dict(radius=radius, delta=up(dz), max_steps=max_steps)
    go = offsets(B, size)
    first = obs_of_plan(eng, free, go=go, **kw)
    second = obs_of_plan(eng, free, go=go, **kw)
    assert same(first, want) and same(second, first)
    # sixteen cuboids: the four, in another order, among twelve that contain nothing or lie far away
    far = np.array([100.0, 101.0, 100.0, 101.0, -50.0, -49.0])
    sixteen = np.stack([far, CUBOIDS[3], far + 7.0, [np.nan] * 6, CUBOIDS[1], [5.0, 4.0, 0.0, 9.0, -9.0, 0.0], far - 300.0, CUBOIDS[0]] +
                       [far + 3.0 * i for i in range(7)] + [CUBOIDS[2]])
    assert sixteen.shape == (16, 6)
    assert same(obs_of_plan(eng, free, cuboids=sixteen, go=go, **kw), want)
    for g in range(len(go) - 1):                             # every group as a batch of its own
        b0, b1 = int(go[g]), int(go[g + 1])
        alone = obs_abi(eng, free.coeffs[b0:b1], free.seg_rows[b0:b1], None, b1 - b0, m, DT, **kw)[0]
        assert same(alone, want[:, b0:b1]), g
    # other company: the groups in another order, and one of them beside a stranger
    order = [2, 0, 1]
    idx = np.concatenate([np.arange(go[g], go[g + 1]) for g in order])
    sel = torch.as_tensor(idx, device=eng.device)
    mixed = obs_abi(eng, free.coeffs[sel].contiguous(), free.seg_rows[sel].contiguous(), None, B, m, DT, go=go, **kw)[0]
    assert same(mixed, want[:, idx])
    other = case(eng, 8, 192)["free"]
    coeffs = torch.cat([other.coeffs[100:140], free.coeffs[size:2 * size]])
    seg_rows = torch.cat([other.seg_rows[100:140], free.seg_rows[size:2 * size]])
    beside = obs_abi(eng, coeffs, seg_rows, None, 40 + size, m, DT, go=np.array([0, 40, 40 + size]), **kw)[0]
    assert same(np.ascontiguousarray(beside[:, 40:]), want[:, size:2 * size])


def test_excluded_missions_and_a_group_above_the_limit_behave_as_before(eng):
    import torch
    from oracle import minsnap_oracle as mo
    from uav_ac import _native as nat
    from uav_ac.scoring import layer_obstacles_from_rows
    B = 37
    wps = mo.synthetic_missions(B, 8).copy()
    wps[5, 3] = wps[5, 2]                                                            # a repeated waypoint: singular knot system
    plan = eng.plan(wps, VEL, DT, strict=False)
    free = eng.plan(wps, VEL, DT, strict=False, rows=False)
    ro = plan.row_offsets.cpu().numpy()
    st = (np.arange(B) % 4) * 11
    rows_at = product_rows_at(eng, dict(free=free, at={}), up(0.25))
    eng.take_flags()
    il = obs_of_plan(eng, plan, start=st, max_steps=7)
    assert same(il, layer_obstacles_from_rows(rows_at, ro, 0.5, CUBOIDS, None, st, 7)) and eng.take_flags() == [0, 0, 0, 0]
    assert il[:, 5].tolist() == [0, -2, 0, 0]                                         # excluded: not examined, nothing blocked
    assert il[2].tolist() == [b if b < 5 else (0 if b == 5 else b - 1) for b in range(B)] and (il[3] > 0).any()
    # an excluded FIRST mission: the next one is the first of the group and runs the blocked pass only
    seg_rows = plan.seg_rows.clone()
    seg_rows[0] = 0
    got = obs_abi(eng, plan.coeffs, seg_rows, None, B, 8, DT, start=st, max_steps=7)[0]
    alone = obs_abi(eng, plan.coeffs[1:], plan.seg_rows[1:], None, B - 1, 8, DT, start=st[1:], max_steps=7)[0]
    assert got[:, 0].tolist() == [0, -2, 0, 0] and same(np.ascontiguousarray(got[:, 1:]), alone) and alone[2, 0] == 0
    # negative starts are clamped to 0 and raise flag 0
    neg = st.copy()
    neg[st == 0] = -1 - np.arange((st == 0).sum())
    assert same(obs_of_plan(eng, plan, start=neg, max_steps=7), il) and eng.take_flags() == [1, 0, 0, 0]
    # a group above the limit given on the device: not examined, flag 0; its neighbour decides as if alone
    k = case(eng, 8, 96)
    big = k["free"]
    n = nat.LAYER_MAX_GROUP + 1
    B3 = 3 * 96
    coeffs, seg_rows = torch.cat([big.coeffs] * 3), torch.cat([big.seg_rows] * 3)
    st = np.arange(B3) % 9
    got = obs_abi(eng, coeffs, seg_rows, None, B3, 8, DT, go=np.array([0, n, B3]), start=st, max_steps=7)[0]
    assert eng.take_flags() == [1, 0, 0, 0]
    assert (got[0, :n] == 0).all() and (got[1, :n] == -2).all() and (got[2, :n] == 0).all() and (got[3, :n] == 0).all()
    b0 = n - 2 * 96
    alone = obs_abi(eng, big.coeffs[b0:], big.seg_rows[b0:], None, 96 - b0, 8, DT, start=st[n:], max_steps=7)[0]
    assert same(np.ascontiguousarray(got[:, n:]), alone) and (alone[1] > 0).any() and eng.take_flags() == [0, 0, 0, 0]
    from types import SimpleNamespace
    plan3 = SimpleNamespace(coeffs=coeffs, seg_rows=seg_rows, B=B3, m=8, dt=DT)
    with pytest.raises(ValueError):
        eng.layer(plan3, 0.5, groups=[0, n, B3], obstacles=CUBOIDS)
    res = eng.layer(plan3, 0.5, groups=_i64(eng, [0, n, B3]), start_rows=st, delta=up(0.25), max_steps=7, obstacles=CUBOIDS)
    assert np.array_equal(res.block.cpu().numpy(), got) and eng.take_flags() == [1, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------ 5: the one call
def test_deconflict_is_the_chain_and_its_plan_is_clean_and_flies(eng):
    import torch
    B, m, radius, size, dz, max_layers = 96, 8, 0.5, 32, 0.25, 15
    k = case(eng, m, B)
    free, go = k["free"], offsets(B, size)
    out = eng.deconflict(free, radius, groups=size, obstacles=CUBOIDS, delta=up(dz), max_layers=max_layers)
    # its parts are the hand-written chain's, bit for bit
    stag = eng.stagger(free, radius, groups=size)
    lay = eng.layer(free, radius, groups=size, start_rows=stag.start_rows, delta=up(dz), max_steps=max_layers, obstacles=CUBOIDS)
    shifted = eng.shift(free, lay.offsets)
    flown = eng.delay(shifted, stag.start_rows)
    assert torch.equal(out.stagger.block, stag.block) and torch.equal(out.layer.block, lay.block) and out.layer.block.shape == (4, B)
    assert same_bits(out.layer.offsets.cpu().numpy(), lay.offsets.cpu().numpy())
    assert out.resolved.is_cuda and out.resolved.dtype == torch.bool and torch.equal(out.resolved, lay.steps >= 0)
    plan = out.plan
    assert plan.traj is None and plan.B == B and plan.max_m == m + 1 and np.array_equal(plan.seg_offsets_host, flown.seg_offsets_host)
    assert same_bits(plan.coeffs.cpu().numpy(), flown.coeffs.cpu().numpy()) and torch.equal(plan.seg_rows, flown.seg_rows)
    assert torch.equal(plan.row_offsets, flown.row_offsets) and same_bits(plan.times.cpu().numpy(), flown.times.cpu().numpy())
    resolved = out.resolved.cpu().numpy()
    layers = lay.layers.cpu().numpy()
    print(f"deconflict, groups of {size}: {int((stag.steps > 0).sum())} delayed, {int((layers > 0).sum())} layered, "
          f"{int((lay.blocked > 0).sum())} met a cuboid, {int((~resolved).sum())} unresolved")
    assert (layers > 0).any() and bool((stag.steps > 0).any()) and (~resolved).any() and resolved.sum() > B // 2
    # the plan to fly: no row of a resolved mission inside a cuboid, no pair of resolved missions inside the radius
    assert (eng.audit(plan, CUBOIDS).hit_rows.cpu().numpy()[:, resolved] == 0).all()
    whole = eng.separation(plan, radius, groups=size)
    at_starts = eng.separation(shifted, radius, groups=size, start_rows=stag.start_rows)
    assert torch.equal(whole.block, at_starts.block) and same_bits(whole.min_distance.cpu().numpy(), at_starts.min_distance.cpu().numpy())
    keep = np.flatnonzero(resolved)
    sub, sub_go, sub_start = resolved_alone(eng, shifted, keep, go, m, stag.start_rows)
    alone = eng.separation(sub, radius, groups=sub_go, start_rows=sub_start)
    assert int(alone.conflicts.sum()) == 0 and bool((alone.first_conflict == -1).all())
    # without obstacles it is the existing chain, and a (3, B) layer block
    bare = eng.deconflict(free, radius, groups=size, delta=up(dz), max_layers=max_layers)
    bare_lay = eng.layer(free, radius, groups=size, start_rows=stag.start_rows, delta=up(dz), max_steps=max_layers)
    assert bare.layer.block.shape == (3, B) and torch.equal(bare.layer.block, bare_lay.block) and bare.layer.blocked is None
    assert same_bits(bare.plan.coeffs.cpu().numpy(), eng.delay(eng.shift(free, bare_lay.offsets), stag.start_rows).coeffs.cpu().numpy())
    # it flies: plan-fed, a few ticks, no flag
    eng.take_flags()
    fleet = eng.fleet(plan)
    assert fleet.from_plan and torch.equal(fleet.state[0:3].T.contiguous(), plan.start_positions)
    fleet.rollout(60, score=True)
    t = fleet.tracking()
    assert bool(torch.isfinite(fleet.state).all()) and bool(torch.isfinite(t["max_error"]).all()) and eng.take_flags() == [0, 0, 0, 0]


# -------------------------------------------------------------------------------------------------------------- 6: validation
def test_invalid_arguments_are_refused_before_anything_is_enqueued(eng):
    import torch
    from uav_ac import _native as nat
    B, m = 96, 8
    k = case(eng, m, B)
    free = k["free"]
    il = torch.full((4 * B,), SENT_I, dtype=torch.int32, device=eng.device)
    off = torch.full((3 * B,), SENT_F, dtype=torch.float64, device=eng.device)
    go = _i64(eng, [0, 32, 64, B])
    cub = _f64(eng, CUBOIDS)
    good = dict(coeffs=free.coeffs, seg_rows=free.seg_rows, seg_offsets=None, B=B, m=m, dt=DT, go=go, G=3, start=None, radius=0.5,
                dx=0.0, dy=0.0, dz=-0.25, max_steps=15, cub=cub, n=4, il=il, off=off)
    bad = [dict(coeffs=None), dict(seg_rows=None), dict(il=None), dict(off=None), dict(B=0), dict(B=-3), dict(m=0),
           dict(m=nat.MAX_SEGMENTS + 1), dict(dt=0.0), dict(dt=-0.01), dict(dt=math.inf), dict(dt=math.nan), dict(radius=-0.5),
           dict(radius=math.inf), dict(radius=math.nan), dict(G=0), dict(G=-2), dict(dx=math.nan), dict(dy=math.inf), dict(dz=-math.inf),
           dict(dz=math.nan), dict(max_steps=-1), dict(max_steps=nat.LAYER_MAX_STEPS + 1),
           dict(n=-1), dict(n=nat.AUDIT_MAX_CUBOIDS + 1), dict(cub=None), dict(cub=None, n=1)]
    eng._bind_stream()
    fn = nat.lib().uavac_minsnap_layer_obs_dev

    def call(ctx, a):
        return fn(ctx, _p(a["coeffs"]), _p(a["seg_rows"]), _p(a["seg_offsets"]), a["B"], a["m"], a["dt"], _p(a["go"]), a["G"], _p(a["start"]),
                  a["radius"], a["dx"], a["dy"], a["dz"], a["max_steps"], _p(a["cub"]), a["n"], _p(a["il"]), _p(a["off"]))
    for change in bad:
        rc = call(eng.ctx._h, {**good, **change})
        assert rc == nat.EINVAL, (change, rc)
        assert (nat.lib().uavac_last_error(eng.ctx._h) or b"") != b"", change
    assert call(None, good) == nat.EINVAL                                            # no context
    big = torch.cat([free.coeffs] * 3), torch.cat([free.seg_rows] * 3)               # one group of all B above the limit
    wide_i = torch.full((4 * 3 * B,), SENT_I, dtype=torch.int32, device=eng.device)
    wide_f = torch.full((3 * 3 * B,), SENT_F, dtype=torch.float64, device=eng.device)
    assert call(eng.ctx._h, {**good, "coeffs": big[0], "seg_rows": big[1], "B": 3 * B, "go": None, "G": 0, "il": wide_i, "off": wide_f}) == nat.EINVAL
    torch.cuda.synchronize()
    assert bool((il == SENT_I).all()) and bool((off == SENT_F).all()) and bool((wide_i == SENT_I).all()) and bool((wide_f == SENT_F).all())
    # the same call with nothing wrong goes through; cuboids may be NULL or given with n_cuboids = 0
    assert call(eng.ctx._h, good) == nat.OK
    torch.cuda.synchronize()
    assert same(il.cpu().numpy().reshape(4, B), rule(eng, CONFIGS[0]))
    assert call(eng.ctx._h, {**good, "n": 0}) == nat.OK and call(eng.ctx._h, {**good, "cub": None, "n": 0, "go": None, "G": 0, "max_steps": 0}) == nat.OK
    torch.cuda.synchronize()
    # Engine.layer and Engine.deconflict refuse on the host what the host can see
    for obstacles in (np.zeros((nat.AUDIT_MAX_CUBOIDS + 1, 6)), np.zeros((2, 5)), np.zeros(5), np.zeros((3, 4))):
        with pytest.raises(ValueError):
            eng.layer(free, 0.5, groups=32, obstacles=obstacles)
        with pytest.raises(ValueError):
            eng.deconflict(free, 0.5, groups=32, obstacles=obstacles)
    for kw in (dict(max_steps=-1), dict(groups=0), dict(delta=(0.0, math.nan, -0.5)), dict(start_rows=np.zeros(5))):
        with pytest.raises(ValueError):
            eng.layer(free, 0.5, obstacles=CUBOIDS, **{"groups": 32, **kw})
    for kw in (dict(step=0), dict(max_delay_steps=-1), dict(max_layers=nat.LAYER_MAX_STEPS + 1), dict(groups=0), dict(delta=(0.0, 0.0))):
        with pytest.raises(ValueError):
            eng.deconflict(free, 0.5, **{"groups": 32, **kw})
    assert eng.layer(free, 0.5, groups=32, obstacles=np.zeros((nat.AUDIT_MAX_CUBOIDS, 6)) + 500.0).block.shape == (4, B)
