"""Priorities for the fleet's searches on the GPU: `uavac_fleet_order_dev` (csrc/minsnap_take.hip) through the C ABI, and `priority=` on
`Engine.stagger`, `Engine.layer` and `Engine.deconflict`.  Every comparison is exact: an order is a permutation, and the searches'
outputs are integers decided by comparisons on the same doubles as the rules'.

What is compared with what:
  * order and rank against `uav_ac.scoring.priority_order`, from the middle of sentinel-filled buffers;
  * `priority=None` and `priority=arange(B)` against the call without a priority, bit for bit;
  * a reversed priority against the rules on `take_rows` of the PRODUCT'S OWN ROWS, mapped back with `rank` -- the specification of
    the `priority=` forms: `stagger_from_rows`, `layer_from_rows`, `layer_obstacles_from_rows`;
  * the guarantees in the caller's batch order: no pair of resolved missions inside the radius, no resolved mission inside a cuboid.
The missions, their memoised product rows and the helpers are tests/test_gpu_layer.py's (one cache for the three files): the stagger
tests' synthetic_missions(96, 8) at velocity 3.0, dt 0.01, radius 0.5; the cuboids are tests/test_gpu_layer_obstacles.py's."""
import numpy as np
import pytest

from test_gpu_layer import PAD, SENT_I, _i64, _p, case, offsets, product_rows_at, same, same_bits, up

pytestmark = pytest.mark.gpu

B, M, RADIUS, DZ, MAX_LAYERS = 96, 8, 0.5, 0.25, 15
CUBOIDS = np.array([[11.13, 12.37, 6.21, 7.43, -20.0, 20.0], [3.17, 21.29, 1.61, 15.83, -4.613, -4.087],
                    [22.31, 25.87, 11.19, 14.57, -9.011, -2.203], [1.09, 4.91, -1.27, 2.33, -5.897, -3.511]])
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    return Engine("cuda:0")


def order_abi(eng, priority, go=None):
    """One call of uavac_fleet_order_dev -> (order, rank) as NumPy, each from the middle of a larger sentinel-filled buffer: nothing
    outside may be written, and everything inside must be."""
    import torch
    n = len(priority)
    pr = torch.as_tensor(np.ascontiguousarray(priority, dtype=np.float64)).to(eng.device)
    bufs = [torch.full((PAD + n + PAD,), SENT_I, dtype=torch.int32, device=eng.device) for _ in range(2)]
    g = _i64(eng, go)
    eng._bind_stream()
    eng.ctx.call("uavac_fleet_order_dev", _p(pr), _p(g), 0 if go is None else len(go) - 1, n, _p(bufs[0][PAD:]), _p(bufs[1][PAD:]))
    torch.cuda.synchronize()
    out = []
    for buf in bufs:
        h = buf.cpu().numpy()
        assert (h[:PAD] == SENT_I).all() and (h[PAD + n:] == SENT_I).all() and not (h[PAD:PAD + n] == SENT_I).any()
        out.append(h[PAD:PAD + n].copy())
    return out


# ------------------------------------------------------------------------------------------------ 7: the order, through the C ABI
def test_the_order_equals_priority_order(eng):
    import torch
    from uav_ac import _native as nat
    from uav_ac.scoring import priority_order
    n = 1000
    rng = np.random.default_rng(11)
    values = np.array([-2.25, -1e-300, 1e-300, 0.5, 1.0, 1.5, 7.0, 1e300, NAN, INF, -INF, 0.0, -0.0])
    priority = values[rng.integers(0, len(values), size=n)]
    assert np.isnan(priority).sum() > 20 and (np.signbit(priority) & (priority == 0)).sum() > 20 and len(set(priority[~np.isnan(priority)])) == 11
    sizes = [1, 2, 63, 64, 65, 256, 257]
    go = np.concatenate([[0], np.cumsum(sizes), [n]])                        # ... and the rest: 292
    for offs in (None, go, [0, n], [5, 300, 900], [-4, 500, 2000], [0, 10, 10, 10, n], np.arange(n + 1)):
        want = priority_order(priority, offs)
        got = order_abi(eng, priority, offs)
        assert same(got[0], want[0]) and same(got[1], want[1]), offs
        assert np.array_equal(got[1][got[0]], np.arange(n))
    ident = order_abi(eng, np.arange(n, dtype=np.float64), go)
    assert np.array_equal(ident[0], np.arange(n)) and np.array_equal(ident[1], np.arange(n))
    # a group that spans many workgroups and tiles, all ties: the identity; reversed: the reverse
    big = 5000
    assert np.array_equal(order_abi(eng, np.zeros(big))[0], np.arange(big))
    assert np.array_equal(order_abi(eng, -np.arange(big, dtype=np.float64))[0], np.arange(big)[::-1])
    # the refusals of the header: nothing is enqueued
    pr = torch.zeros((8,), dtype=torch.float64, device=eng.device)
    out = torch.full((16,), SENT_I, dtype=torch.int32, device=eng.device)
    g = _i64(eng, [0, 8])
    for args in ((None, None, 0, 8, _p(out), _p(out[8:])), (_p(pr), None, 0, 8, None, _p(out[8:])), (_p(pr), None, 0, 8, _p(out), None),
                 (_p(pr), None, 0, 0, _p(out), _p(out[8:])), (_p(pr), _p(g), 0, 8, _p(out), _p(out[8:]))):
        with pytest.raises(nat.UavacError) as exc:
            eng.ctx.call("uavac_fleet_order_dev", *args)
        assert exc.value.code == nat.EINVAL
    torch.cuda.synchronize()
    assert bool((out == SENT_I).all())


# ------------------------------------------------------------------------------------------------ 8: no priority, and the identity
def same_stagger(a, b):
    import torch
    return torch.equal(a.block, b.block) and torch.equal(a.start_rows, b.start_rows) and torch.equal(a.steps, b.steps)


def same_layer(a, b):
    import torch
    return (torch.equal(a.block, b.block) and same_bits(a.offsets.cpu().numpy(), b.offsets.cpu().numpy()) and torch.equal(a.layers, b.layers)
            and a.block.shape == b.block.shape)


def same_plan(a, b):
    import torch
    return (same_bits(a.coeffs.cpu().numpy(), b.coeffs.cpu().numpy()) and torch.equal(a.seg_rows, b.seg_rows) and torch.equal(a.row_offsets, b.row_offsets)
            and same_bits(a.times.cpu().numpy(), b.times.cpu().numpy()) and np.array_equal(a.seg_offsets_host, b.seg_offsets_host)
            and same_bits(a.first_yaw.cpu().numpy(), b.first_yaw.cpu().numpy()))


def test_no_priority_and_the_identity_give_the_calls_as_they_were(eng, monkeypatch):
    import torch
    free = case(eng, M, B)["free"]
    start = (np.arange(B) * 7) % 5
    calls = []
    real = eng.ctx.call
    monkeypatch.setattr(eng.ctx, "call", lambda name, *args: (calls.append(name), real(name, *args))[1])

    def traced(fn):
        del calls[:]
        out = fn()
        return out, [c for c in calls if c != "uavac_set_stream"]

    kw = dict(delta=up(DZ), max_steps=MAX_LAYERS)
    stag, names = traced(lambda: eng.stagger(free, RADIUS, 32, start))
    stag_none, names_none = traced(lambda: eng.stagger(free, RADIUS, 32, start, priority=None))
    assert names == names_none == ["uavac_minsnap_stagger_dev"] and same_stagger(stag, stag_none)
    lay, names = traced(lambda: eng.layer(free, RADIUS, 32, stag.start_rows, **kw))
    lay_none, names_none = traced(lambda: eng.layer(free, RADIUS, 32, stag.start_rows, priority=None, **kw))
    assert names == names_none == ["uavac_minsnap_layer_dev"] and same_layer(lay, lay_none)
    obs, names = traced(lambda: eng.layer(free, RADIUS, 32, stag.start_rows, obstacles=CUBOIDS, **kw))
    obs_none, names_none = traced(lambda: eng.layer(free, RADIUS, 32, stag.start_rows, obstacles=CUBOIDS, priority=None, **kw))
    assert names == names_none == ["uavac_minsnap_layer_obs_dev"] and same_layer(obs, obs_none) and obs.block.shape == (4, B)
    dkw = dict(groups=32, obstacles=CUBOIDS, start_rows=start, delta=up(DZ), max_layers=MAX_LAYERS)
    dec, names = traced(lambda: eng.deconflict(free, RADIUS, **dkw))
    dec_none, names_none = traced(lambda: eng.deconflict(free, RADIUS, priority=None, **dkw))
    assert names == names_none and not any("take" in n or "order" in n for n in names)
    assert names[:2] == ["uavac_minsnap_stagger_dev", "uavac_minsnap_layer_obs_dev"]
    assert same_stagger(dec.stagger, dec_none.stagger) and same_layer(dec.layer, dec_none.layer) and same_plan(dec.plan, dec_none.plan)
    # the identity, as an array and as a device tensor: the same answers through the take
    for ident in (np.arange(B), torch.arange(B, dtype=torch.float64, device=eng.device)):
        got, names = traced(lambda: eng.stagger(free, RADIUS, 32, start, priority=ident))
        assert same_stagger(got, stag) and names[0] == "uavac_fleet_order_dev" and "uavac_minsnap_take_dev" in names
        assert same_layer(eng.layer(free, RADIUS, 32, stag.start_rows, priority=ident, **kw), lay)
        assert same_layer(eng.layer(free, RADIUS, 32, stag.start_rows, obstacles=CUBOIDS, priority=ident, **kw), obs)
        got, names = traced(lambda: eng.deconflict(free, RADIUS, priority=ident, **dkw))
        assert same_stagger(got.stagger, dec.stagger) and same_layer(got.layer, dec.layer) and same_plan(got.plan, dec.plan)
        assert torch.equal(got.resolved, dec.resolved) and names.count("uavac_minsnap_take_dev") == 1      # one take for both searches
    assert same_stagger(eng.stagger(free, RADIUS, priority=np.zeros(B)), eng.stagger(free, RADIUS))        # all ties, one group of 96
    with pytest.raises(ValueError):
        eng.stagger(free, RADIUS, 32, priority=np.arange(B - 1))
    with pytest.raises(ValueError):
        eng.deconflict(free, RADIUS, 0, priority=np.arange(B))
    assert eng.take_flags() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 9: a reversed priority against the rules
_RULES = {}


def reversed_rules(eng, size):
    """What the rules give on the taken rows of the product for the reversed priority in groups of `size`, mapped back with rank:
    computed once, shared by the tests that need it.  -> dict(order, rank, stagger, layer, layer_obs)."""
    if size not in _RULES:
        from uav_ac.scoring import layer_from_rows, layer_obstacles_from_rows, priority_order, stagger_from_rows, take_rows
        k = case(eng, M, B)
        go = offsets(B, size)
        order, rank = priority_order(-np.arange(B, dtype=np.float64), go)
        trows, tro = take_rows(k["rows"], k["ro"], order)
        stag = stagger_from_rows(trows, tro, RADIUS, go)
        at = product_rows_at(eng, k, up(DZ))
        memo = {}

        def rows_at(q):
            if q not in memo:
                memo[q] = take_rows(at(q), k["ro"], order)[0]
            return memo[q]

        starts = stag[0]                                                 # (in slot order, as the search takes them)
        lay = layer_from_rows(rows_at, tro, RADIUS, go, starts, MAX_LAYERS)
        obs = layer_obstacles_from_rows(rows_at, tro, RADIUS, CUBOIDS, go, starts, MAX_LAYERS)
        _RULES[size] = dict(order=order, rank=rank, go=go, stagger=stag[:, rank], layer=lay[:, rank], layer_obs=obs[:, rank])
    return _RULES[size]


@pytest.mark.parametrize("size, unresolved", [(32, 7), (96, 16)])
def test_a_reversed_priority_equals_the_rules_on_the_taken_rows(eng, size, unresolved):
    free = case(eng, M, B)["free"]
    want = reversed_rules(eng, size)
    go, priority = want["go"], -np.arange(B, dtype=np.float64)
    assert want["order"].tolist() == np.concatenate([np.arange(a, b)[::-1] for a, b in zip(go[:-1], go[1:])]).tolist()
    stag = eng.stagger(free, RADIUS, size, priority=priority)
    got = stag.block.cpu().numpy()
    assert same(got, want["stagger"]), np.flatnonzero((got != want["stagger"]).any(axis=0))
    plain = eng.stagger(free, RADIUS, size).block.cpu().numpy()
    n_diff = int((got[1] != plain[1]).sum())
    print(f"reversed priority, groups of {size}: {int((got[1] == -1).sum())} unresolved ({int((plain[1] == -1).sum())} in index order), "
          f"{int((got[1] > 0).sum())} delayed ({int((plain[1] > 0).sum())}), steps differ for {n_diff}")
    assert int((got[1] == -1).sum()) == unresolved and n_diff > 0
    last = go[1:] - 1                                                    # the first of each group's order: never delayed, checked against nobody
    assert (got[1][last] == 0).all() and (got[2][last] == 0).all() and (got[0][last] == 0).all()
    assert (plain[1][go[:-1]] == 0).all() and (got[1][go[:-1]] != 0).any()
    # the layers at those starts, without and with cuboids
    kw = dict(start_rows=stag.start_rows, delta=up(DZ), max_steps=MAX_LAYERS, priority=priority)
    lay = eng.layer(free, RADIUS, size, **kw)
    got_l = lay.block.cpu().numpy()
    assert same(got_l, want["layer"]), np.flatnonzero((got_l != want["layer"]).any(axis=0))
    assert np.array_equal(lay.offsets.cpu().numpy(), got_l[0][:, None] * up(DZ)[None, :])
    obs = eng.layer(free, RADIUS, size, obstacles=CUBOIDS, **kw)
    got_o = obs.block.cpu().numpy()
    assert same(got_o, want["layer_obs"]), np.flatnonzero((got_o != want["layer_obs"]).any(axis=0))
    assert np.array_equal(obs.offsets.cpu().numpy(), got_o[0][:, None] * up(DZ)[None, :])
    assert (got_l[1][last] == 0).all() and (got_o[3] > 0).any() and (got_l[1] > 0).any()
    plain_l = eng.layer(free, RADIUS, size, start_rows=stag.start_rows, delta=up(DZ), max_steps=MAX_LAYERS).block.cpu().numpy()
    assert not np.array_equal(plain_l, got_l)                            # (the order matters for the layers too)
    assert eng.take_flags() == [0, 0, 0, 0]


def test_base_starts_follow_their_missions_through_the_order(eng):
    from uav_ac.scoring import priority_order, stagger_from_rows, take_rows
    k = case(eng, M, B)
    go = offsets(B, 32)
    priority = np.random.default_rng(5).permutation(B).astype(np.float64)
    priority[[3, 20]] = NAN
    start = (np.arange(B) * 7) % 50
    order, rank = priority_order(priority, go)
    trows, tro = take_rows(k["rows"], k["ro"], order)
    want = stagger_from_rows(trows, tro, RADIUS, go, start[order], step=3, max_steps=60)[:, rank]
    for plan in (k["free"], k["plan"]):
        got = eng.stagger(plan, RADIUS, go, start, step=3, max_steps=60, priority=priority).block.cpu().numpy()
        assert same(got, want), np.flatnonzero((got != want).any(axis=0))
    assert ((want[0] - start) == np.maximum(want[1], 0) * 3).all() and (want[1] > 0).any()
    assert want[2][3] == 30 and want[2][20] == 31                        # the NaNs go last in their group, the lower index first


# ------------------------------------------------------------------------------------------------ 10: the guarantees, in the caller's order
def resolved_pairs(eng, plan, groups, resolved, start_rows=None):
    """How many pairs of RESOLVED missions `Engine.conflicts` finds inside the radius."""
    cl = eng.conflicts(plan, RADIUS, groups, start_rows)
    off, partner = cl.offsets.cpu().numpy(), cl.partner.cpu().numpy()
    assert np.array_equal(eng.separation(plan, RADIUS, groups, start_rows).conflicts.cpu().numpy(), np.diff(off))      # (the audit's own pairs)
    own = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return int((resolved[own] & resolved[partner]).sum()) // 2, int(cl.total) // 2


@pytest.mark.parametrize("size", [32, 96])
def test_the_granted_starts_clear_the_audit_in_the_callers_order(eng, size):
    free = case(eng, M, B)["free"]
    stag = eng.stagger(free, RADIUS, size, priority=-np.arange(B, dtype=np.float64))
    resolved = stag.steps.cpu().numpy() >= 0
    among, every = resolved_pairs(eng, free, size, resolved, stag.start_rows)
    before, _ = resolved_pairs(eng, free, size, resolved)
    print(f"reversed priority, groups of {size}: {before} pairs of resolved missions inside the radius before, {among} at the granted starts "
          f"({every} pairs with unresolved missions in all)")
    assert among == 0 and before > 0


def test_deconflict_with_a_priority_keeps_its_guarantees_and_the_callers_order(eng):
    import torch
    free = case(eng, M, B)["free"]
    priority = np.random.default_rng(3).permutation(B).astype(np.float64)
    kw = dict(delta=up(DZ), max_steps=MAX_LAYERS)
    out = eng.deconflict(free, RADIUS, 32, obstacles=CUBOIDS, delta=up(DZ), max_layers=MAX_LAYERS, priority=priority)
    # its parts are the calls' with the same priority, and its plan is built from the caller's plan
    stag = eng.stagger(free, RADIUS, 32, priority=priority)
    lay = eng.layer(free, RADIUS, 32, stag.start_rows, obstacles=CUBOIDS, priority=priority, **kw)
    assert same_stagger(out.stagger, stag) and same_layer(out.layer, lay) and torch.equal(out.resolved, lay.steps >= 0)
    assert same_plan(out.plan, eng.delay(eng.shift(free, lay.offsets), stag.start_rows))
    assert torch.equal(out.plan.start_positions[:, :2], free.waypoints[:, 0, :2])          # mission b is still mission b
    resolved = out.resolved.cpu().numpy()
    plain = eng.deconflict(free, RADIUS, 32, obstacles=CUBOIDS, delta=up(DZ), max_layers=MAX_LAYERS)
    print(f"deconflict with a random priority: {int((~resolved).sum())} unresolved ({int((~plain.resolved).sum())} in index order), "
          f"{int((stag.steps > 0).sum())} delayed, {int((lay.layers > 0).sum())} layered")
    assert not same_stagger(out.stagger, plain.stagger) and resolved.sum() > B // 2
    among, _ = resolved_pairs(eng, out.plan, 32, resolved)
    assert among == 0
    assert (eng.audit(out.plan, CUBOIDS).hit_rows.cpu().numpy()[:, resolved] == 0).all()
    assert int(eng.audit(free, CUBOIDS).hit_rows.cpu().numpy()[:, resolved].sum()) > 0      # (the cuboids were in the way)
    # the first of each group's order is never delayed and moved only by a cuboid
    order = np.concatenate([g0 + np.argsort(priority[g0:g0 + 32], kind="stable") for g0 in (0, 32, 64)])
    first = order[[0, 32, 64]]
    assert (stag.steps.cpu().numpy()[first] == 0).all() and (lay.earlier.cpu().numpy()[first] == 0).all()
    granted = lay.steps.cpu().numpy()[first] >= 0
    assert (lay.layers.cpu().numpy()[first] == lay.blocked.cpu().numpy()[first])[granted].all()
    assert eng.take_flags() == [0, 0, 0, 0]
