"""The prioritised searches for groups of any size, on the GPU (`uavac_minsnap_stagger_wide_dev`, `uavac_minsnap_layer_wide_dev`,
csrc/fleet_wide.h), through the C ABI and through `Engine.stagger / layer / deconflict(..., wide=True)`.

The method is tests/test_gpu_stagger.py's and tests/test_gpu_layer.py's: sentinel-padded output buffers, `same()` on int32, and
  * inside the narrow limit the wide call against the NARROW CALL on the same inputs, integer for integer and bit for bit, at every
    block size -- a group of 150 is blocks of 64, 64 and 22 --, and against the rule on the product's own rows;
  * beyond the limit against the rule alone: `uav_ac.scoring.stagger_from_rows / layer_obstacles_from_rows(..., max_group=)`.
A fixture could pass by being trivial -- nobody of a later block meeting anybody of an earlier one --, so before a comparison counts
the test asserts on the rule's answer, among the missions past block 0: somebody's answer differs from the rule run on the blocks as
groups of their own; somebody is granted a candidate above 63 (a second seed word, and a last round of fewer than 64 live lanes);
somebody is unresolved.  Beyond the limit "past block 0" is read for the largest block, 256: it then holds for every block size.
Missions: oracle.minsnap_oracle.synthetic_missions(B, 3) at velocity 3, radius 0.5, start rows (b % 5) * 7; three segments and a few
hundred rows each, so a 32-row chunk holds segment changes.  The rule in NumPy dominates the time; every answer of it is computed
once and shared."""
import math

import numpy as np
import pytest

from test_gpu_layer import PAD, SENT_F, SENT_I, _i32, _i64, _p, product_rows_at, same, same_bits

pytestmark = pytest.mark.gpu

VEL, RADIUS, TILE = 3.0, 0.5, 64
CUBOIDS = np.array([[11.13, 12.37, 6.21, 7.43, -20.0, 20.0],        # a pillar and a slab, faces off the waypoints' grid
                    [3.17, 21.29, 1.61, 15.83, -4.613, -4.087]])
UP = np.array([0.0, 0.0, -0.01])


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    return Engine("cuda:0")


def starts(B):
    return (np.arange(B) % 5) * 7


_CACHE = {}


def case(eng, B, dt):
    """Per (B, dt), computed once and left unchanged: the plan with rows, the rows-free plan, rows and offsets on the host."""
    if (B, dt) not in _CACHE:
        from oracle import minsnap_oracle as mo
        wps = mo.synthetic_missions(B, 3)
        plan = eng.plan(wps, VEL, dt)
        _CACHE[(B, dt)] = dict(plan=plan, free=eng.plan(wps, VEL, dt, rows=False), rows=plan.traj.cpu().numpy(),
                               ro=plan.row_offsets.cpu().numpy(), at={}, memo={})
    return _CACHE[(B, dt)]


def once(k, key, make):
    """an answer of the rule for the case k: computed when first asked for, then shared"""
    if key not in k["memo"]:
        k["memo"][key] = make()
    return k["memo"][key]


def parts(plan):
    ragged = hasattr(plan, "seg_offsets")
    return plan.coeffs, plan.seg_rows, plan.seg_offsets if ragged else None, int(plan.B), int(plan.max_m if ragged else plan.m), float(plan.dt)


def out_i(eng, rows, B):
    import torch
    return torch.full((PAD + rows * B + PAD,), SENT_I, dtype=torch.int32, device=eng.device)


def read_i(buf, rows, B):
    i = buf.cpu().numpy()
    assert (i[:PAD] == SENT_I).all() and (i[PAD + rows * B:] == SENT_I).all() and not (i[PAD:PAD + rows * B] == SENT_I).any()
    return i[PAD:PAD + rows * B].reshape(rows, B).copy()


def stag(eng, plan, wide, go=None, cap=None, start=None, step=1, max_steps=100, radius=RADIUS, seg_rows=None, coeffs=None):
    """One call of uavac_minsnap_stagger_wide_dev (`wide`) or uavac_minsnap_stagger_dev -> istag (3, B), from a sentinel-padded buffer."""
    import torch
    co, sr, so, B, m, dt = parts(plan)
    buf = out_i(eng, 3, B)
    g, s = _i64(eng, go), _i32(eng, start)
    G = 0 if go is None else len(go) - 1
    head = (_p(co if coeffs is None else coeffs), _p(sr if seg_rows is None else seg_rows), _p(so), B, m, dt, _p(g), G)
    tail = (_p(s), float(radius), int(step), int(max_steps), _p(buf[PAD:]))
    eng._bind_stream()
    if wide:
        eng.ctx.call("uavac_minsnap_stagger_wide_dev", *head, int(B if cap is None else cap), *tail)
    else:
        eng.ctx.call("uavac_minsnap_stagger_dev", *head, *tail)
    torch.cuda.synchronize()
    return read_i(buf, 3, B)


def lay(eng, plan, which, go=None, cap=None, start=None, delta=UP, max_steps=100, cuboids=None, radius=RADIUS):
    """One call of uavac_minsnap_layer_wide_dev ("wide"), uavac_minsnap_layer_obs_dev ("obs") or uavac_minsnap_layer_dev ("plain")
    -> (ilayer (4 or 3, B), offsets (B, 3))."""
    import torch
    co, sr, so, B, m, dt = parts(plan)
    rows = 3 if which == "plain" else 4
    buf = out_i(eng, rows, B)
    fbuf = torch.full((PAD + 3 * B + PAD,), SENT_F, dtype=torch.float64, device=eng.device)
    g, s = _i64(eng, go), _i32(eng, start)
    n = 0 if cuboids is None else len(cuboids)
    cub = torch.as_tensor(np.ascontiguousarray(cuboids, dtype=np.float64)).to(eng.device) if n else None
    head = (_p(co), _p(sr), _p(so), B, m, dt, _p(g), 0 if go is None else len(go) - 1)
    mid = (_p(s), float(radius), float(delta[0]), float(delta[1]), float(delta[2]), int(max_steps))
    eng._bind_stream()
    if which == "wide":
        eng.ctx.call("uavac_minsnap_layer_wide_dev", *head, int(B if cap is None else cap), *mid, _p(cub), n, _p(buf[PAD:]), _p(fbuf[PAD:]))
    elif which == "obs":
        eng.ctx.call("uavac_minsnap_layer_obs_dev", *head, *mid, _p(cub), n, _p(buf[PAD:]), _p(fbuf[PAD:]))
    else:
        assert n == 0
        eng.ctx.call("uavac_minsnap_layer_dev", *head, *mid, _p(buf[PAD:]), _p(fbuf[PAD:]))
    torch.cuda.synchronize()
    f = fbuf.cpu().numpy()
    assert (f[:PAD] == SENT_F).all() and (f[PAD + 3 * B:] == SENT_F).all() and not (f[PAD:PAD + 3 * B] == SENT_F).any()
    il, off = read_i(buf, rows, B), f[PAD:PAD + 3 * B].reshape(B, 3).copy()
    assert np.array_equal(off, il[0][:, None] * np.asarray(delta, dtype=np.float64)[None, :])       # the granted fl(layer * delta)
    return il, off


class block_size:
    """the ctx option "search_block" for the calls inside, the default again behind them"""
    def __init__(self, eng, value):
        self.eng, self.value = eng, value

    def __enter__(self):
        self.eng.ctx.set_option("search_block", self.value)

    def __exit__(self, *exc):
        self.eng.ctx.set_option("search_block", 0)


def blocks_of(B, blk):
    return np.array(list(range(0, B, blk)) + [B])


def not_trivial(want, alone, blk, second_word=True):
    """The conditions of the module's head on the rule's answer `want` and on the rule's answer for the blocks alone."""
    later = np.arange(want.shape[1]) >= blk
    n = dict(differ=int(((want[:2] != alone[:2]).any(axis=0) & later).sum()), above_63=int(((want[1] >= TILE) & later).sum()),
             unresolved=int(((want[1] == -1) & later).sum()), moved=int((want[1] > 0).sum()))
    assert n["differ"] > 0 and n["unresolved"] > 0 and (n["above_63"] > 0 or not second_word), n
    return n


# ------------------------------------------------------------------------------------------------ 1, 2: blocks inside the narrow limit
def test_stagger_in_blocks_of_64_equals_the_narrow_call_and_the_rule(eng):
    from uav_ac.scoring import stagger_from_rows
    B = 150
    k, st = case(eng, B, 0.01), starts(B)
    want = once(k, "stagger", lambda: stagger_from_rows(k["rows"], k["ro"], RADIUS, None, st, 1, 100))
    alone = once(k, "stagger alone", lambda: stagger_from_rows(k["rows"], k["ro"], RADIUS, blocks_of(B, 64), st, 1, 100))
    print("stagger, 150 missions in blocks of 64:", not_trivial(want, alone, 64))
    narrow = stag(eng, k["free"], False, start=st)
    assert same(narrow, want)
    eng.take_flags()
    for blk in (64, 128, 256, 0):
        with block_size(eng, blk):
            assert same(stag(eng, k["free"], True, start=st), narrow), blk
            assert same(stag(eng, k["plan"], True, start=st, cap=1000), narrow), blk
    assert eng.take_flags() == [0, 0, 0, 0]


def test_layer_in_blocks_of_64_equals_the_narrow_calls_with_and_without_cuboids(eng):
    from uav_ac.scoring import layer_from_rows
    B, dt = 150, 0.04
    k, st = case(eng, B, dt), starts(B)
    rows_at = product_rows_at(eng, k, UP)
    want = once(k, "layer", lambda: layer_from_rows(rows_at, k["ro"], RADIUS, None, st, 100))
    alone = once(k, "layer alone", lambda: layer_from_rows(rows_at, k["ro"], RADIUS, blocks_of(B, 64), st, 100))
    print("layer, 150 missions in blocks of 64:", not_trivial(want, alone, 64))
    plain, plain_off = lay(eng, k["free"], "plain", start=st)
    obs, obs_off = lay(eng, k["free"], "obs", start=st, cuboids=CUBOIDS)
    assert same(plain, want)
    later = np.arange(B) >= 64
    assert (obs[3][later] > 0).any() and (obs[:3] != plain).any(), "the cuboids refuse nobody of a later block"
    eng.take_flags()
    for blk in (64, 128, 256, 0):
        with block_size(eng, blk):
            got, off = lay(eng, k["free"], "wide", start=st)
            assert same(np.ascontiguousarray(got[:3]), plain) and same_bits(off, plain_off) and (got[3] == 0).all(), blk
            got, off = lay(eng, k["free"], "wide", start=st, cuboids=CUBOIDS)
            assert same(got, obs) and same_bits(off, obs_off), blk
    assert eng.take_flags() == [0, 0, 0, 0]


def test_ragged_groups_in_one_batch(eng):
    from uav_ac.scoring import stagger_from_rows
    sizes = (63, 64, 65, 1, 0, 129)
    go = np.concatenate([[0], np.cumsum(sizes)])
    B = int(go[-1])
    k, st = case(eng, B, 0.02), starts(B)
    want = once(k, "stagger ragged", lambda: stagger_from_rows(k["rows"], k["ro"], RADIUS, go, st, 4, 70))
    narrow = stag(eng, k["free"], False, go=go, start=st, step=4, max_steps=70)
    assert same(narrow, want) and (want[1, go[5]:] == -1).any() and (want[1, go[5] + 64:] > 0).any()
    plain = lay(eng, k["free"], "plain", go=go, start=st, delta=(0.0, 0.0, -0.05), max_steps=20)
    obs = lay(eng, k["free"], "obs", go=go, start=st, delta=(0.0, 0.0, -0.05), max_steps=20, cuboids=CUBOIDS)
    eng.take_flags()
    for blk in (64, 128, 0):
        with block_size(eng, blk):
            assert same(stag(eng, k["free"], True, go=go, cap=129, start=st, step=4, max_steps=70), narrow), blk
            got, off = lay(eng, k["free"], "wide", go=go, cap=129, start=st, delta=(0.0, 0.0, -0.05), max_steps=20)
            assert same(np.ascontiguousarray(got[:3]), plain[0]) and same_bits(off, plain[1]), blk
            got, off = lay(eng, k["free"], "wide", go=go, cap=129, start=st, delta=(0.0, 0.0, -0.05), max_steps=20, cuboids=CUBOIDS)
            assert same(got, obs[0]) and same_bits(off, obs[1]), blk
    assert eng.take_flags() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 3: beyond the narrow limit
def rule300(eng, step, max_steps):
    from uav_ac.scoring import stagger_from_rows
    k, st = case(eng, 300, 0.02), starts(300)
    return once(k, ("stagger", step, max_steps), lambda: stagger_from_rows(k["rows"], k["ro"], RADIUS, None, st, step, max_steps, max_group=300))


def test_stagger_of_one_group_of_300_equals_the_rule(eng):
    from uav_ac.scoring import stagger_from_rows
    B = 300
    k, st = case(eng, B, 0.02), starts(B)
    want = rule300(eng, 8, 70)
    ro = k["ro"]

    def last_block_alone():                                  # (block 0 alone is the rule's own beginning: only the 44 behind it are asked)
        alone = want.copy()
        alone[:, 256:] = stagger_from_rows(k["rows"][ro[256]:], ro[256:] - ro[256], RADIUS, None, st[256:], 8, 70)
        return alone
    alone = once(k, "stagger alone", last_block_alone)
    print("stagger, one group of 300, step 8:", not_trivial(want, alone, 256, second_word=False))
    eng.take_flags()
    assert same(stag(eng, k["free"], True, start=st, step=8, max_steps=70), want)
    for blk in (64, 256):
        with block_size(eng, blk):
            assert same(stag(eng, k["plan"], True, start=st, step=8, max_steps=70), want), blk
    assert eng.take_flags() == [0, 0, 0, 0]
    # the narrow call is what it was: the group is not examined, and flag 0 says so
    narrow = stag(eng, k["free"], False, go=np.array([0, B]), start=st, step=8, max_steps=70)
    assert narrow[0].tolist() == st.tolist() and (narrow[1] == -2).all() and (narrow[2] == 0).all() and eng.take_flags() == [1, 0, 0, 0]
    with pytest.raises(ValueError):
        eng.stagger(k["free"], RADIUS, start_rows=st)


def test_stagger_of_300_grants_from_the_second_seed_word(eng):
    B = 300
    k, st = case(eng, B, 0.02), starts(B)
    want = rule300(eng, 1, 100)
    later = np.arange(B) >= 256
    print(f"stagger, one group of 300, step 1: {int((want[1] >= TILE).sum())} grants above 63, {int(((want[1] >= TILE) & later).sum())} past 256")
    assert ((want[1] >= TILE) & later).any() and ((want[1] == -1) & later).any()
    for blk in (0, 64):
        with block_size(eng, blk):
            assert same(stag(eng, k["free"], True, start=st, max_steps=100), want), blk


def test_layer_with_cuboids_of_one_group_of_257_equals_the_rule(eng):
    from uav_ac.scoring import layer_obstacles_from_rows
    B, delta = 257, np.array([0.0, 0.0, -0.25])
    k300 = case(eng, 300, 0.02)
    taken = once(k300, "first 257", lambda: eng.take(k300["free"], np.arange(B)))
    k = dict(free=taken, at=k300["memo"].setdefault("at 257", {}))
    ro, st = k300["ro"][:B + 1], starts(B)
    rows_at = product_rows_at(eng, k, delta)
    want = once(k300, "layer 257", lambda: layer_obstacles_from_rows(rows_at, ro, RADIUS, CUBOIDS, None, st, 15, max_group=B))
    print(f"layer, one group of 257: {int((want[1] > 0).sum())} moved, {int((want[1] == -1).sum())} unresolved, {int((want[3] > 0).sum())} blocked, "
          f"the last mission {want[:, B - 1].tolist()}")
    assert (want[1] != -2).all() and (want[1] > 0).any() and (want[3] > 0).any() and want[2, B - 1] == B - 1
    eng.take_flags()
    for blk in (0, 64, 256):
        with block_size(eng, blk):
            got, _ = lay(eng, taken, "wide", start=st, delta=delta, max_steps=15, cuboids=CUBOIDS)
            assert same(got, want), blk
    res = eng.layer(taken, RADIUS, start_rows=st, delta=delta, max_steps=15, obstacles=CUBOIDS, wide=True)
    assert same(res.block.cpu().numpy(), want) and same(res.blocked.cpu().numpy(), want[3]) and eng.take_flags() == [0, 0, 0, 0]
    free = eng.layer(taken, RADIUS, start_rows=st, delta=delta, max_steps=15, wide=True)      # no obstacles: (4, B), blocked all 0
    assert tuple(free.block.shape) == (4, B) and not bool(free.blocked.any()) and bool((free.steps != -2).all())


# ------------------------------------------------------------------------------------------------ 4: the audits confirm
def test_the_audits_confirm_a_wide_deconflict(eng):
    k = case(eng, 300, 0.02)
    res = eng.deconflict(k["free"], RADIUS, obstacles=CUBOIDS, wide=True)
    ok = res.resolved.cpu().numpy()
    assert ok[:256].any() and ok[256:].any() and (res.stagger.steps.cpu().numpy() != -2).all() and (res.layer.steps.cpu().numpy() != -2).all()
    assert (res.stagger.steps.cpu().numpy() > 0).any() and (res.layer.steps.cpu().numpy() > 0).any()
    from uav_ac.scoring import conflict_pairs
    pairs = conflict_pairs(eng.conflicts(res.plan, RADIUS))
    assert not [p for p in zip(pairs["i"].tolist(), pairs["j"].tolist()) if ok[p[0]] and ok[p[1]]]
    sep = eng.separation(res.plan, RADIUS)
    if ok.all():
        assert int(sep.conflicts.sum()) == 0
    assert (eng.audit(res.plan, CUBOIDS).hit_rows.cpu().numpy().reshape(-1, 300).sum(axis=0)[ok] == 0).all()
    assert eng.take_flags() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 5: priority
def test_priority_composes_with_the_wide_search(eng):
    from uav_ac.scoring import priority_order, stagger_from_rows, take_rows
    B = 300
    k, st = case(eng, B, 0.02), starts(B)
    pr = np.random.default_rng(5).permutation(B).astype(np.float64)
    order, rank = priority_order(pr)
    rows, ro = take_rows(k["rows"], k["ro"], order)
    want = stagger_from_rows(rows, ro, RADIUS, None, st[order], 8, 70, max_group=B)[:, rank]
    got = eng.stagger(k["free"], RADIUS, start_rows=st, step=8, max_steps=70, priority=pr, wide=True)
    assert same(got.block.cpu().numpy(), np.ascontiguousarray(want)) and (want[1] > 0).any() and (want[1] == -1).any()
    by_index = eng.stagger(k["free"], RADIUS, start_rows=st, step=8, max_steps=70, priority=np.arange(B), wide=True)
    plain = eng.stagger(k["free"], RADIUS, start_rows=st, step=8, max_steps=70, wide=True)
    assert same(by_index.block.cpu().numpy(), plain.block.cpu().numpy()) and same(plain.block.cpu().numpy(), rule300(eng, 8, 70))
    with pytest.raises(ValueError):
        eng.stagger(k["free"], RADIUS, start_rows=st, priority=pr)


# ------------------------------------------------------------------------------------------------ 6: edges
def test_a_group_above_group_cap_on_the_device_and_its_neighbour(eng):
    import torch
    k = case(eng, 150, 0.01)
    st, go = starts(150), np.array([0, 100, 150])
    narrow = stag(eng, k["free"], False, go=go, start=st)
    eng.take_flags()
    got = stag(eng, k["free"], True, go=go, cap=99, start=st)
    assert eng.take_flags() == [1, 0, 0, 0]
    assert got[0, :100].tolist() == st[:100].tolist() and (got[1, :100] == -2).all() and (got[2, :100] == 0).all()
    assert same(np.ascontiguousarray(got[:, 100:]), np.ascontiguousarray(narrow[:, 100:])) and (narrow[1, 100:] > 0).any()
    with block_size(eng, 64):
        assert same(stag(eng, k["free"], True, go=go, cap=100, start=st), narrow) and eng.take_flags() == [0, 0, 0, 0]
        il, _ = lay(eng, k["free"], "wide", go=go, cap=50, start=st, max_steps=3, cuboids=CUBOIDS)
    assert eng.take_flags() == [1, 0, 0, 0] and (il[1, :100] == -2).all() and (il[[0, 2, 3], :100] == 0).all() and (il[1, 100:] != -2).all()
    # the engine: sizes on the host are known, offsets on the device take the caller's bound (B without one)
    dev = torch.as_tensor(go).to(eng.device)
    assert same(eng.stagger(k["free"], RADIUS, groups=dev, start_rows=st, max_steps=100, wide=True).block.cpu().numpy(), narrow)
    assert same(eng.stagger(k["free"], RADIUS, groups=go, start_rows=st, max_steps=100, wide=True, group_cap=120).block.cpu().numpy(), narrow)
    assert eng.take_flags() == [0, 0, 0, 0]
    assert same(eng.stagger(k["free"], RADIUS, groups=dev, start_rows=st, max_steps=100, wide=True, group_cap=99).block.cpu().numpy(), got)
    assert eng.take_flags() == [1, 0, 0, 0]
    with pytest.raises(ValueError, match="a group of 100 missions; group_cap is 99"):
        eng.stagger(k["free"], RADIUS, groups=go, wide=True, group_cap=99)


def test_excluded_missions_on_both_sides_of_a_block_boundary(eng):
    from uav_ac.scoring import stagger_from_rows
    B = 150
    k, st = case(eng, B, 0.01), starts(B)
    plan = k["plan"]
    coeffs = plan.coeffs.clone()
    coeffs.reshape(B, -1)[10, 5] = math.nan                                           # block 0: a coefficient that is no number
    seg_rows = plan.seg_rows.clone()
    seg_rows.reshape(B, -1)[70] = 0                                                   # block 1: no rows
    rows, ro = k["rows"].copy(), k["ro"].copy()
    rows[ro[10]:ro[11], 0:3] = np.nan
    rows = np.delete(rows, np.s_[ro[70]:ro[71]], axis=0)
    ro[71:] -= ro[71] - ro[70]
    want = stagger_from_rows(rows, ro, RADIUS, None, st, 1, 100)
    assert want[2].tolist() == [b - (b > 10) - (b > 70) if b not in (10, 70) else 0 for b in range(B)] and want[1, 10] == want[1, 70] == -2
    narrow = stag(eng, plan, False, start=st, coeffs=coeffs, seg_rows=seg_rows)
    assert same(narrow, want)
    eng.take_flags()
    for blk in (64, 128, 0):
        with block_size(eng, blk):
            assert same(stag(eng, plan, True, start=st, coeffs=coeffs, seg_rows=seg_rows), want), blk
    assert eng.take_flags() == [0, 0, 0, 0]


def test_no_candidates_but_the_first_and_a_group_of_whole_blocks(eng):
    k = case(eng, 150, 0.01)
    st = starts(150)
    narrow = stag(eng, k["free"], False, start=st, max_steps=0)
    assert set(narrow[1].tolist()) == {0, -1}
    go = np.array([0, 128, 150])                                                      # two blocks of 64 exactly, and one of 128
    by_group = stag(eng, k["free"], False, go=go, start=st)
    eng.take_flags()
    for blk in (64, 128):
        with block_size(eng, blk):
            assert same(stag(eng, k["free"], True, start=st, max_steps=0), narrow), blk
            assert same(stag(eng, k["free"], True, go=go, cap=128, start=st), by_group), blk
            il, _ = lay(eng, k["free"], "wide", go=go, cap=128, start=st, max_steps=0, cuboids=CUBOIDS)
            assert same(il, lay(eng, k["free"], "obs", go=go, start=st, max_steps=0, cuboids=CUBOIDS)[0]), blk
    assert eng.take_flags() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 7: refusals
def test_the_block_size_takes_four_values(eng):
    from uav_ac import _native as nat
    for value in (0,) + nat.SEARCH_BLOCKS:
        eng.ctx.set_option("search_block", value)
    for value in (-1, 1, 32, 63, 65, 96, 192, 255, 257, 512):
        with pytest.raises(nat.UavacError, match="search_block is 0 .default., 64, 128 or 256"):
            eng.ctx.set_option("search_block", value)
    eng.ctx.set_option("search_block", 0)


def test_invalid_arguments_are_refused_before_anything_is_enqueued(eng):
    import torch
    from uav_ac import _native as nat
    B = 150
    k = case(eng, B, 0.01)
    free = k["free"]
    ibuf = torch.full((4 * B,), SENT_I, dtype=torch.int32, device=eng.device)
    fbuf = torch.full((3 * B,), SENT_F, dtype=torch.float64, device=eng.device)
    cub = torch.as_tensor(CUBOIDS).to(eng.device)
    go = _i64(eng, [0, 10, B])
    common = dict(coeffs=free.coeffs, seg_rows=free.seg_rows, seg_offsets=None, B=B, m=3, dt=0.01, go=go, G=2, cap=140, start=None, radius=0.5)
    shared = [dict(coeffs=None), dict(seg_rows=None), dict(B=0), dict(B=-3), dict(m=0), dict(m=nat.MAX_SEGMENTS + 1), dict(dt=0.0),
              dict(dt=-0.01), dict(dt=math.inf), dict(dt=math.nan), dict(radius=-0.5), dict(radius=math.inf), dict(radius=math.nan), dict(G=0),
              dict(G=-2), dict(max_steps=-1), dict(cap=0), dict(cap=-5), dict(go=None, G=0, cap=B - 1)]
    good_s = dict(common, step=8, max_steps=31, istag=ibuf)
    bad_s = shared + [dict(istag=None), dict(step=0), dict(step=-1), dict(max_steps=nat.STAGGER_MAX_STEPS + 1), dict(step=2 ** 20, max_steps=513),
                      dict(step=2 ** 30, max_steps=1)]
    good_l = dict(common, dx=0.0, dy=0.0, dz=-0.25, max_steps=15, cuboids=cub, n=2, ilayer=ibuf, offsets=fbuf)
    bad_l = shared + [dict(ilayer=None), dict(offsets=None), dict(dx=math.nan), dict(dy=math.inf), dict(dz=-math.inf),
                      dict(max_steps=nat.LAYER_MAX_STEPS + 1), dict(n=-1), dict(n=nat.AUDIT_MAX_CUBOIDS + 1), dict(cuboids=None)]
    eng._bind_stream()

    def call_s(ctx, a):
        return nat.lib().uavac_minsnap_stagger_wide_dev(ctx, _p(a["coeffs"]), _p(a["seg_rows"]), _p(a["seg_offsets"]), a["B"], a["m"], a["dt"],
                                                       _p(a["go"]), a["G"], a["cap"], _p(a["start"]), a["radius"], a["step"], a["max_steps"],
                                                       _p(a["istag"]))

    def call_l(ctx, a):
        return nat.lib().uavac_minsnap_layer_wide_dev(ctx, _p(a["coeffs"]), _p(a["seg_rows"]), _p(a["seg_offsets"]), a["B"], a["m"], a["dt"],
                                                     _p(a["go"]), a["G"], a["cap"], _p(a["start"]), a["radius"], a["dx"], a["dy"], a["dz"],
                                                     a["max_steps"], _p(a["cuboids"]), a["n"], _p(a["ilayer"]), _p(a["offsets"]))
    for call, good, bad in ((call_s, good_s, bad_s), (call_l, good_l, bad_l)):
        for change in bad:
            rc = call(eng.ctx._h, {**good, **change})
            assert rc == nat.EINVAL, (change, rc)
            assert (nat.lib().uavac_last_error(eng.ctx._h) or b"") != b"", change
        assert call(None, good) == nat.EINVAL                                        # no context
    torch.cuda.synchronize()
    assert bool((ibuf == SENT_I).all()) and bool((fbuf == SENT_F).all())
    # the same calls with nothing wrong go through; one group of all B takes a bound of exactly B, and G is ignored without offsets
    for call, good, rows in ((call_s, good_s, 3), (call_l, good_l, 4)):
        assert call(eng.ctx._h, good) == nat.OK and call(eng.ctx._h, {**good, "go": None, "G": -1, "cap": B}) == nat.OK
        torch.cuda.synchronize()
        assert not bool((ibuf[:rows * B] == SENT_I).any())
    assert call_l(eng.ctx._h, {**good_l, "cuboids": None, "n": 0}) == nat.OK
    torch.cuda.synchronize()
    # the engine refuses on the host what the host can see
    for call in (lambda: eng.stagger(free, RADIUS, wide=True, group_cap=0), lambda: eng.layer(free, RADIUS, wide=True, group_cap=-1),
                 lambda: eng.stagger(free, RADIUS, wide=True, step=0), lambda: eng.layer(free, RADIUS, wide=True, max_steps=-1),
                 lambda: eng.stagger(free, RADIUS, groups=0, wide=True)):
        with pytest.raises(ValueError):
            call()
    assert eng.take_flags() == [0, 0, 0, 0]
