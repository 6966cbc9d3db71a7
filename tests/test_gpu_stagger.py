"""Start delays that clear the separation audit, on the GPU (`uavac_minsnap_stagger_dev`, csrc/minsnap_stagger.hip), through the C ABI and
`Engine.stagger`: per group the missions in ascending batch index, each granted the smallest start delay that keeps it outside the
protection radius of every mission decided before it -- from coefficients and row counts.

What is compared with what:
  * against the PRODUCT'S OWN ROWS everything is exact: `uav_ac.scoring.stagger_from_rows` on the sampled rows is the rule, the kernel
    uses the sampler's arithmetic and forms d^2 = (dx dx + dy dy) + dz dz without contraction, and every output is an integer decided by
    comparisons d^2 < r^2;
  * against the ORACLE (oracle.c_oracle.plan_threads: its own solve and sampler, through the same NumPy rule) all three rows are exact
    as well, and the cap on differing missions is 0.  That can hold because every decision is a comparison with the radius: on the
    oracle's rows the smallest |minimum distance of an examined candidate - radius| is 7.4e-4, 6.1e-4, 4.2e-4 and 1.19e-3 for the four
    configurations below (checked on the CPU) -- twenty times the 2e-5 by which two positions at the project's 1e-5 bar
    can move a distance.  The test recomputes that margin and asserts >= 1e-4 before it demands equality.
The j-tile of the decision kernel is 64 missions wide and a round holds 64 candidates: groups of 63, 64, 65 and 129 missions are cut
from two (8, 96) sets side by side, and the configurations reach the second and third candidate round."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VEL, DT = 3.0, 0.01
# (m, B, radius, step, max_steps, group size)
CONFIGS = ((8, 96, 0.5, 1, 255, 32), (8, 96, 0.5, 8, 31, 96), (8, 96, 1.0, 1, 255, 24), (20, 24, 0.5, 1, 127, 24))
SENT_I, PAD = -7777, 96
TILE = 64
MARGIN = 1e-4


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    return Engine("cuda:0")


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _i64(eng, a):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.int64)).to(eng.device)


def _i32(eng, a):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(eng.device)


def stag_abi(eng, coeffs, seg_rows, seg_offsets, B, m, dt, go=None, start=None, radius=0.5, step=1, max_steps=255):
    """One call of uavac_minsnap_stagger_dev -> istag (3, B) as NumPy.  The output is the middle of a larger sentinel-filled buffer:
    nothing outside [3][B] may be written, and everything inside must be."""
    import torch
    ibuf = torch.full((PAD + 3 * B + PAD,), SENT_I, dtype=torch.int32, device=eng.device)
    g, s = _i64(eng, go), _i32(eng, start)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_stagger_dev", _p(coeffs), _p(seg_rows), _p(seg_offsets), int(B), int(m), float(dt), _p(g),
                 0 if go is None else len(go) - 1, _p(s), float(radius), int(step), int(max_steps), _p(ibuf[PAD:]))
    torch.cuda.synchronize()
    i = ibuf.cpu().numpy()
    assert (i[:PAD] == SENT_I).all() and (i[PAD + 3 * B:] == SENT_I).all()
    assert not (i[PAD:PAD + 3 * B] == SENT_I).any()
    return i[PAD:PAD + 3 * B].reshape(3, B).copy()


def stag_of_plan(eng, plan, **kw):
    ragged = hasattr(plan, "seg_offsets")
    return stag_abi(eng, plan.coeffs, plan.seg_rows, plan.seg_offsets if ragged else None, plan.B, plan.max_m if ragged else plan.m,
                    plan.dt, **kw)


def same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype == np.int32 and np.array_equal(got, want)


def offsets(B, size):
    return np.array(list(range(0, B, size)) + [B])


_CACHE = {}


def case(eng, m, B):
    """Per mission set, computed once and left unchanged: the plan with rows, the rows-free plan and the rows on the host.  B = 192
    with m = 8 is two (8, 96) sets side by side, the second one shifted."""
    if (m, B) not in _CACHE:
        from oracle import minsnap_oracle as mo
        if (m, B) == (8, 192):
            w = mo.synthetic_missions(96, 8)
            wps = np.concatenate([w, w + np.array([1.3, 0.7, 0.0])])
        else:
            wps = mo.synthetic_missions(B, m)
        plan = eng.plan(wps, VEL, DT)
        free = eng.plan(wps, VEL, DT, rows=False)
        _CACHE[(m, B)] = dict(wps=wps, plan=plan, free=free, rows=plan.traj.cpu().numpy(), ro=plan.row_offsets.cpu().numpy())
    return _CACHE[(m, B)]


_RULE = {}


def rule(eng, cfg):
    """What the rule gives on the product's own rows for a configuration: computed once, shared by the tests that need it."""
    if cfg not in _RULE:
        from uav_ac.scoring import stagger_from_rows
        m, B, radius, step, max_steps, size = cfg
        k = case(eng, m, B)
        _RULE[cfg] = stagger_from_rows(k["rows"], k["ro"], radius, offsets(B, size), None, step, max_steps)
    return _RULE[cfg]


def kinds(istag):
    q = istag[1]
    return dict(first_round=int(((q > 0) & (q < TILE)).sum()), later_round=int((q >= TILE).sum()), unresolved=int((q == -1).sum()),
                never=int((q == 0).sum()))


# ------------------------------------------------------------------------------------------------ 1: the product's own rows
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "m%d-B%d-r%g-step%d-max%d-groups%d" % c)
def test_stagger_equals_the_rule_on_the_products_rows(eng, cfg):
    m, B, radius, step, max_steps, size = cfg
    k = case(eng, m, B)
    assert k["free"].traj is None
    want = rule(eng, cfg)
    kw = dict(go=offsets(B, size), radius=radius, step=step, max_steps=max_steps)
    got_free = stag_of_plan(eng, k["free"], **kw)
    got_rows = stag_of_plan(eng, k["plan"], **kw)
    assert same(got_free, got_rows), cfg
    assert same(got_free, want), (cfg, np.argwhere(got_free != want)[:8], got_free[:, (got_free != want).any(axis=0)][:, :8],
                                  want[:, (got_free != want).any(axis=0)][:, :8])
    n = kinds(want)
    print(f"stagger {cfg}: {n}, largest q {int(want[1].max())}")
    assert n["first_round"] > 0 and n["unresolved"] > 0 and n["never"] > 0, n
    if max_steps >= TILE:
        assert n["later_round"] > 0, n                       # the sets cannot go trivial: every kind is there
    assert ((want[0] == want[1] * step) | (want[1] < 0)).all() and (want[0][want[1] < 0] == 0).all()


def test_uneven_groups_with_base_starts(eng):
    from uav_ac.scoring import stagger_from_rows
    B = 96
    k = case(eng, 8, B)
    go, st = np.array([0, 1, B // 3, B // 3, B]), (np.arange(B) % 5) * 37
    want = stagger_from_rows(k["rows"], k["ro"], 0.5, go, st)
    assert same(stag_of_plan(eng, k["free"], go=go, start=st), want)
    assert same(stag_of_plan(eng, k["plan"], go=go, start=st), want)
    n = kinds(want)
    assert min(n.values()) > 0, n
    assert (want[0] == st + np.maximum(want[1], 0)).all()
    assert want[2].tolist() == [0] + list(range(B // 3 - 1)) + list(range(B - B // 3))


# ---------------------------------------------------------------------------------------------------------- 2: tile edges
def test_groups_of_one_tile_one_less_one_more_and_two_tiles(eng):
    from uav_ac.scoring import stagger_from_rows
    k = case(eng, 8, 192)
    free = k["free"]
    for go, step, max_steps in (([0, TILE - 1, 2 * TILE - 1, 192], 2, 127), ([0, 2 * TILE + 1, 192], 8, 31)):
        want = stagger_from_rows(k["rows"], k["ro"], 0.5, go, None, step, max_steps)
        got = stag_of_plan(eng, free, go=np.array(go), step=step, max_steps=max_steps)
        assert same(got, want), (go, np.argwhere(got != want)[:8])
        # the same groups as batches of their own, without offsets
        for b0, b1 in zip(go[:-1], go[1:]):
            alone = stag_abi(eng, free.coeffs[b0:b1], free.seg_rows[b0:b1], None, b1 - b0, 8, DT, step=step, max_steps=max_steps)
            assert same(alone, want[:, b0:b1]), (go, b0, b1)
        if go[1] > TILE:                                     # the second j-tile decides something: delays and dead ends past index 64
            assert (want[1, TILE:go[1]] > 0).any() and (want[1, TILE:go[1]] == -1).any() and (want[1, TILE:go[1]] == 0).any()


# ------------------------------------------------------------------------------------------------------------ 3: the oracle
def candidate_margin(rows, ro, radius, go, istag, step, max_steps):
    """The smallest |minimum distance of an examined candidate - radius| on these rows: how far the nearest decision is from flipping.
    Examined are the candidates q = 0 .. steps of a resolved mission and all of an unresolved one, each against the missions decided
    before it at their granted starts."""
    N = np.diff(ro)
    worst = np.inf
    for g in range(len(go) - 1):
        done = []
        for i in range(int(go[g]), int(go[g + 1])):
            if istag[1, i] == -2:
                continue
            if done:
                last = max_steps if istag[1, i] < 0 else int(istag[1, i])
                base = int(istag[0, i]) - max(int(istag[1, i]), 0) * step
                h_prev = max(int(istag[0, j]) + int(N[j]) for j in done)
                kk = np.arange(max(h_prev, base + last * step + int(N[i])))
                others = np.stack([rows[ro[j] + np.clip(kk - istag[0, j], 0, N[j] - 1), 0:3] for j in done])
                for q in range(last + 1):
                    s = base + q * step
                    H = max(h_prev, s + int(N[i]))
                    own = rows[ro[i] + np.clip(kk[:H] - s, 0, N[i] - 1), 0:3]
                    d = math.sqrt(float(((own[None] - others[:, :H]) ** 2).sum(axis=2).min()))
                    worst = min(worst, abs(d - radius))
            done.append(i)
    return worst


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "m%d-B%d-r%g-step%d-max%d-groups%d" % c)
def test_stagger_against_the_oracle(eng, cfg):
    """On the oracle's rows the nearest decision is 7.4e-4 / 6.1e-4 / 4.2e-4 / 1.19e-3 away from the radius (the four configurations in
    order; measured on the CPU): positions at the 1e-5 bar cannot flip one, so all three rows are exact and the cap is 0."""
    from oracle import c_oracle as cc
    from uav_ac.scoring import stagger_from_rows
    m, B, radius, step, max_steps, size = cfg
    k = case(eng, m, B)
    ref = cc.plan_threads(k["wps"], VEL, DT)
    rows, ro = ref["rows"], ref["row_offsets"]
    assert np.array_equal(ro, k["ro"])                                                 # row counts are exact
    go = offsets(B, size)
    want = stagger_from_rows(rows, ro, radius, go, None, step, max_steps)
    margin = candidate_margin(rows, ro, radius, go, want, step, max_steps)
    print(f"stagger vs oracle {cfg}: nearest decision {margin:.3e} from the radius; {kinds(want)}")
    assert margin >= MARGIN, margin
    got = stag_of_plan(eng, k["free"], go=go, radius=radius, step=step, max_steps=max_steps)
    differing = int((got != want).any(axis=0).sum())
    assert differing == 0 and same(got, want), (cfg, differing, np.argwhere(got != want)[:8])
    assert same(got, rule(eng, cfg))


# ------------------------------------------------------------------------------------------------------------------ 4: ragged
def test_a_ragged_batch_is_exact_against_its_own_rows(eng):
    from oracle import minsnap_oracle as mo
    from uav_ac.scoring import stagger_from_rows
    sets = {m: mo.synthetic_missions(B, m) for m, B in ((1, 48), (2, 48), (8, 96))}
    missions = [sets[(1, 2, 8)[b % 3]][b] for b in range(45)]
    assert sorted({len(w) - 1 for w in missions}) == [1, 2, 8]
    with_rows = eng.plan_ragged(missions, VEL, DT)
    free = eng.plan_ragged(missions, VEL, DT, rows=False)
    assert free.traj is None
    rows, ro = with_rows.traj.cpu().numpy(), with_rows.row_offsets.cpu().numpy()
    B = 45
    for go, st in ((None, None), (np.array([0, 1, B // 3, B // 3, B]), (np.arange(B) % 5) * 37)):
        want = stagger_from_rows(rows, ro, 0.5, go, st)
        assert same(stag_of_plan(eng, free, go=go, start=st), want), go
        assert same(stag_of_plan(eng, with_rows, go=go, start=st), want), go
        assert (want[1] > 0).any() and (want[1] == 0).any()


# ------------------------------------------------------------------------------------------------- 5: the guarantee, end to end
@pytest.mark.parametrize("size", (16, 12))
def test_the_audit_confirms_the_granted_starts(eng, size):
    from uav_ac.scoring import stagger_ok
    B, radius = 96, 0.5
    k = case(eng, 8, B)
    res = eng.stagger(k["free"], radius, groups=size)
    assert res.start_rows.is_cuda and res.block.shape == (3, B) and res.block.dtype.is_floating_point is False
    assert np.array_equal(res.block.cpu().numpy(), np.stack([t.cpu().numpy() for t in (res.start_rows, res.steps, res.earlier)]))
    before = eng.separation(k["free"], radius, groups=size)
    after = eng.separation(k["free"], radius, groups=size, start_rows=res.start_rows)
    steps = res.steps.cpu().numpy()
    ok = stagger_ok(res)
    assert ok["examined"].all() and np.array_equal(ok["resolved"], steps >= 0)
    conflicts, first = after.conflicts.cpu().numpy(), after.first_conflict.cpu().numpy()
    go = offsets(B, size)
    whole = [g for g in range(len(go) - 1) if ok["resolved"][go[g]:go[g + 1]].all()]
    for g in whole:
        assert (conflicts[go[g]:go[g + 1]] == 0).all() and (first[go[g]:go[g + 1]] == -1).all(), g
    assert any((steps[go[g]:go[g + 1]] > 0).any() for g in whole)
    assert (before.conflicts.cpu().numpy() > 0).sum() > (conflicts > 0).sum() > 0     # fewer than before; the dead ends remain
    # the same through the other forms of `groups`, and with rows
    again = eng.stagger(k["plan"], radius, groups=go)
    assert np.array_equal(again.block.cpu().numpy(), res.block.cpu().numpy())
    on_device = eng.stagger(k["free"], radius, groups=_i64(eng, go))
    assert np.array_equal(on_device.block.cpu().numpy(), res.block.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------ 6: independence
def test_a_group_alone_other_company_and_a_second_call_give_the_same_bits(eng):
    import torch
    cfg = CONFIGS[0]
    m, B, radius, step, max_steps, size = cfg
    k = case(eng, m, B)
    free, want = k["free"], rule(eng, cfg)
    kw = dict(radius=radius, step=step, max_steps=max_steps)
    go = offsets(B, size)
    first = stag_of_plan(eng, free, go=go, **kw)
    second = stag_of_plan(eng, free, go=go, **kw)
    assert same(first, want) and same(second, first)
    for g in range(len(go) - 1):                             # every group as a batch of its own
        b0, b1 = int(go[g]), int(go[g + 1])
        alone = stag_abi(eng, free.coeffs[b0:b1], free.seg_rows[b0:b1], None, b1 - b0, m, DT, **kw)
        assert same(alone, want[:, b0:b1]), g
    # other company: the groups in another order, and one of them beside a stranger
    order = [2, 0, 1]
    idx = np.concatenate([np.arange(go[g], go[g + 1]) for g in order])
    sel = torch.as_tensor(idx, device=eng.device)
    mixed = stag_abi(eng, free.coeffs[sel].contiguous(), free.seg_rows[sel].contiguous(), None, B, m, DT, go=go, **kw)
    assert same(mixed, want[:, idx])
    other = case(eng, 8, 192)["free"]
    coeffs = torch.cat([other.coeffs[100:140], free.coeffs[size:2 * size]])
    seg_rows = torch.cat([other.seg_rows[100:140], free.seg_rows[size:2 * size]])
    beside = stag_abi(eng, coeffs, seg_rows, None, 40 + size, m, DT, go=np.array([0, 40, 40 + size]), **kw)
    assert same(np.ascontiguousarray(beside[:, 40:]), want[:, size:2 * size])


# ------------------------------------------------------------------------------------------ 7: excluded and degenerate missions
def test_a_singular_mission_no_rows_a_copy_radius_zero_and_negative_starts(eng):
    from oracle import minsnap_oracle as mo
    from uav_ac.scoring import stagger_from_rows
    B = 37
    wps = mo.synthetic_missions(B, 8).copy()
    wps[5, 3] = wps[5, 2]                                                            # a repeated waypoint: singular knot system
    wps[20] = wps[11]                                                                # an exact copy of an earlier mission
    plan = eng.plan(wps, VEL, DT, strict=False)
    assert plan.status.cpu().tolist() == [1 if b == 5 else 0 for b in range(B)]
    rows, ro = plan.traj.cpu().numpy(), plan.row_offsets.cpu().numpy()
    st = (np.arange(B) % 4) * 11
    istag = stag_of_plan(eng, plan, start=st)
    assert same(istag, stagger_from_rows(rows, ro, 0.5, None, st))
    assert istag[:, 5].tolist() == [int(st[5]), -2, 0]                                # excluded: not examined
    assert istag[2].tolist() == [b if b < 5 else (0 if b == 5 else b - 1) for b in range(B)]      # the skipped neighbour is visible
    assert istag[:, 20].tolist() == [int(st[20]), -1, 19]                             # the copy can never be cleared
    # radius 0 delays nobody: the test is strict, not even the copy is inside
    zero = stag_of_plan(eng, plan, start=st, radius=0.0)
    assert zero[0].tolist() == st.tolist() and zero[1].tolist() == [-2 if b == 5 else 0 for b in range(B)] and (zero[2] == istag[2]).all()
    # negative base starts are clamped to 0 and raise flag 0
    eng.take_flags()
    assert same(stag_of_plan(eng, plan, start=st), istag) and eng.take_flags() == [0, 0, 0, 0]
    neg = st.copy()
    neg[st == 0] = -1 - np.arange((st == 0).sum())
    assert same(stag_of_plan(eng, plan, start=neg), istag)
    assert eng.take_flags() == [1, 0, 0, 0]
    # a mission without rows is excluded as well (seg_rows zeroed: what a bad speed leaves)
    seg_rows = plan.seg_rows.clone()
    seg_rows[7] = 0
    got = stag_abi(eng, plan.coeffs, seg_rows, None, B, 8, DT, start=st)
    ro7 = ro.copy()
    ro7[8:] -= ro[8] - ro[7]
    want = stagger_from_rows(np.delete(rows, np.s_[ro[7]:ro[8]], axis=0), ro7, 0.5, None, st)
    assert same(got, want) and got[:, 7].tolist() == [int(st[7]), -2, 0] and got[:, 5].tolist() == [int(st[5]), -2, 0]
    assert got[2, 36] == 34 and eng.take_flags() == [0, 0, 0, 0]


def test_a_group_above_the_limit_on_the_device(eng):
    import torch
    from uav_ac import _native as nat
    from uav_ac.scoring import stagger_from_rows
    k = case(eng, 8, 96)
    free = k["free"]
    n = nat.STAGGER_MAX_GROUP + 1
    B = 3 * 96
    coeffs, seg_rows = torch.cat([free.coeffs] * 3), torch.cat([free.seg_rows] * 3)
    st = np.arange(B) % 9
    eng.take_flags()
    got = stag_abi(eng, coeffs, seg_rows, None, B, 8, DT, go=np.array([0, n, B]), start=st)
    assert eng.take_flags() == [1, 0, 0, 0]
    assert got[0, :n].tolist() == st[:n].tolist() and (got[1, :n] == -2).all() and (got[2, :n] == 0).all()
    b0 = n - 2 * 96                                                                   # the neighbour: missions b0 .. 95 of the set
    ro = k["ro"][b0:] - k["ro"][b0]
    want = stagger_from_rows(k["rows"][k["ro"][b0]:], ro, 0.5, None, st[n:])
    assert same(np.ascontiguousarray(got[:, n:]), want) and (want[1] > 0).any()
    # a group of exactly the limit is examined
    full = stag_abi(eng, coeffs, seg_rows, None, B, 8, DT, go=np.array([0, n - 1, B]), start=st, max_steps=0)
    assert eng.take_flags() == [0, 0, 0, 0] and (full[1] != -2).all() and full[2, n - 2] == n - 2
    # Engine.stagger: offsets on the host are refused, offsets on the device go through and the flag tells
    plan3 = SimpleNamespace(coeffs=coeffs, seg_rows=seg_rows, B=B, m=8, dt=DT)
    with pytest.raises(ValueError):
        eng.stagger(plan3, 0.5, groups=[0, n, B])
    with pytest.raises(ValueError):
        eng.stagger(plan3, 0.5, groups=n)
    with pytest.raises(ValueError):
        eng.stagger(plan3, 0.5)
    res = eng.stagger(plan3, 0.5, groups=_i64(eng, [0, n, B]), start_rows=st)
    assert np.array_equal(res.block.cpu().numpy(), got) and eng.take_flags() == [1, 0, 0, 0]


# -------------------------------------------------------------------------------------------------------------- 8: validation
def test_invalid_arguments_are_refused_before_anything_is_enqueued(eng):
    import torch
    from uav_ac import _native as nat
    from uav_ac.scoring import stagger_from_rows
    B, m = 96, 8
    k = case(eng, m, B)
    free = k["free"]
    istag = torch.full((3 * B,), SENT_I, dtype=torch.int32, device=eng.device)
    go = _i64(eng, [0, 10, B])
    good = dict(coeffs=free.coeffs, seg_rows=free.seg_rows, seg_offsets=None, B=B, m=m, dt=DT, go=go, G=2, start=None, radius=0.5,
                step=8, max_steps=31, istag=istag)
    bad = [dict(coeffs=None), dict(seg_rows=None), dict(istag=None), dict(B=0), dict(B=-3), dict(m=0), dict(m=nat.MAX_SEGMENTS + 1),
           dict(dt=0.0), dict(dt=-0.01), dict(dt=math.inf), dict(dt=math.nan), dict(radius=-0.5), dict(radius=math.inf),
           dict(radius=math.nan), dict(G=0), dict(G=-2), dict(step=0), dict(step=-1), dict(max_steps=-1),
           dict(max_steps=nat.STAGGER_MAX_STEPS + 1), dict(step=2 ** 20, max_steps=513), dict(step=2 ** 30, max_steps=1)]
    eng._bind_stream()
    fn = nat.lib().uavac_minsnap_stagger_dev

    def call(ctx, a):
        return fn(ctx, _p(a["coeffs"]), _p(a["seg_rows"]), _p(a["seg_offsets"]), a["B"], a["m"], a["dt"], _p(a["go"]), a["G"], _p(a["start"]),
                  a["radius"], a["step"], a["max_steps"], _p(a["istag"]))
    for change in bad:
        rc = call(eng.ctx._h, {**good, **change})
        assert rc == nat.EINVAL, (change, rc)
        assert (nat.lib().uavac_last_error(eng.ctx._h) or b"") != b"", change
    assert call(None, good) == nat.EINVAL                                            # no context
    # one group of all B above the limit: the host can see that
    big = torch.cat([free.coeffs] * 3), torch.cat([free.seg_rows] * 3)
    wide = torch.full((3 * 3 * B,), SENT_I, dtype=torch.int32, device=eng.device)
    assert call(eng.ctx._h, {**good, "coeffs": big[0], "seg_rows": big[1], "B": 3 * B, "go": None, "G": 0, "istag": wide}) == nat.EINVAL
    torch.cuda.synchronize()
    assert bool((istag == SENT_I).all()) and bool((wide == SENT_I).all())
    # the same call with nothing wrong goes through; G is ignored without offsets
    assert call(eng.ctx._h, good) == nat.OK
    torch.cuda.synchronize()
    assert same(istag.cpu().numpy().reshape(3, B), stagger_from_rows(k["rows"], k["ro"], 0.5, [0, 10, B], None, 8, 31))
    assert call(eng.ctx._h, {**good, "go": None, "G": 0}) == nat.OK
    torch.cuda.synchronize()
    assert same(istag.cpu().numpy().reshape(3, B), rule(eng, CONFIGS[1]))
    # Engine.stagger refuses on the host what the host can see
    for kw in (dict(start_rows=np.zeros(5)), dict(groups=0), dict(step=0), dict(max_steps=-1), dict(max_steps=nat.STAGGER_MAX_STEPS + 1),
               dict(step=2 ** 20, max_steps=1023), dict(groups=[0])):
        with pytest.raises(ValueError):
            eng.stagger(free, 0.5, **kw)
