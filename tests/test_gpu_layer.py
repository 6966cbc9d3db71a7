"""Offset layers that clear the separation audit at fixed starts, and the offset as a plan transform, on the GPU
(`uavac_minsnap_layer_dev`, `uavac_minsnap_shift_dev`, csrc/minsnap_layer.hip), through the C ABI and `Engine.layer` / `Engine.shift`.

What is compared with what:
  * the TRANSFORM against `uav_ac.scoring.shift_coeffs`, bit for bit; the rows sampled from the shifted plan against the original's rows
    (columns 3:11, bit for bit) and against the sampler's fma chain restated on the shifted coefficients (columns 0:3; every fma is one
    correctly rounded step through exact rationals);
  * the SEARCH against the PRODUCT'S OWN ROWS exactly: `uav_ac.scoring.layer_from_rows` with rows_at(q) = the rows the sampler writes for
    `Engine.shift(plan, q * delta)`, memoised.  The kernel adds fl(q * delta) to c0 in two roundings and uses the sampler's arithmetic,
    so every output is an integer decided by comparisons d^2 < r^2 on the same doubles;
  * the search against the ORACLE (oracle.c_oracle.plan_threads: its own solve and sampler; rows_at(q) = rows[:, :3] + q * delta) with a
    cap of 0 differing missions.  That can hold because every decision is a comparison with the radius: the test first recomputes the
    smallest |minimum distance of an examined candidate - radius| on the oracle's rows and asserts >= 1e-4 -- twenty times the 2e-5 by
    which two positions at the project's 1e-5 bar can move a distance (the bar of tests/test_gpu_stagger.py).  Measured on the CPU for
    the four configurations below, in order: 5.9e-3, 4.5e-4, 4.9e-4 and 1.0e-3.
The j-tile of the decision kernel is 64 missions wide and a round holds 64 candidates: groups of 63, 64, 65 and 129 missions are cut
from two (8, 96) sets side by side, and three of the four configurations reach the second candidate round."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VEL, DT = 3.0, 0.01
# (m, B, radius, dz, max_steps, group size); delta = (0, 0, -dz)
CONFIGS = ((8, 96, 0.5, 0.25, 3, 32), (8, 96, 0.5, 0.025, 80, 96), (8, 96, 1.0, 0.04, 70, 32), (20, 24, 1.0, 0.03, 90, 24))
SENT_I, SENT_F, PAD = -7777, -7777.25, 96
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


def up(dz):
    return np.array([0.0, 0.0, -dz])


def layer_abi(eng, coeffs, seg_rows, seg_offsets, B, m, dt, go=None, start=None, radius=0.5, delta=(0.0, 0.0, -0.25), max_steps=63):
    """One call of uavac_minsnap_layer_dev -> (ilayer (3, B), offsets (B, 3)) as NumPy.  Each output is the middle of a larger
    sentinel-filled buffer: nothing outside may be written, and everything inside must be."""
    import torch
    ibuf = torch.full((PAD + 3 * B + PAD,), SENT_I, dtype=torch.int32, device=eng.device)
    fbuf = torch.full((PAD + 3 * B + PAD,), SENT_F, dtype=torch.float64, device=eng.device)
    g, s = _i64(eng, go), _i32(eng, start)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_layer_dev", _p(coeffs), _p(seg_rows), _p(seg_offsets), int(B), int(m), float(dt), _p(g),
                 0 if go is None else len(go) - 1, _p(s), float(radius), float(delta[0]), float(delta[1]), float(delta[2]), int(max_steps),
                 _p(ibuf[PAD:]), _p(fbuf[PAD:]))
    torch.cuda.synchronize()
    i, f = ibuf.cpu().numpy(), fbuf.cpu().numpy()
    assert (i[:PAD] == SENT_I).all() and (i[PAD + 3 * B:] == SENT_I).all() and not (i[PAD:PAD + 3 * B] == SENT_I).any()
    assert (f[:PAD] == SENT_F).all() and (f[PAD + 3 * B:] == SENT_F).all() and not (f[PAD:PAD + 3 * B] == SENT_F).any()
    il, off = i[PAD:PAD + 3 * B].reshape(3, B).copy(), f[PAD:PAD + 3 * B].reshape(B, 3).copy()
    assert np.array_equal(off, il[0][:, None] * np.asarray(delta, dtype=np.float64)[None, :])       # the granted fl(layer * delta)
    return il, off


def layer_of_plan(eng, plan, **kw):
    ragged = hasattr(plan, "seg_offsets")
    return layer_abi(eng, plan.coeffs, plan.seg_rows, plan.seg_offsets if ragged else None, plan.B, plan.max_m if ragged else plan.m,
                     plan.dt, **kw)[0]


def shift_abi(eng, coeffs, seg_offsets, B, m, S, off):
    """One call of uavac_minsnap_shift_dev on S segments -> the (S, 8, 3) output as NumPy, from the middle of a sentinel-filled buffer."""
    import torch
    buf = torch.full((PAD + 24 * S + PAD,), SENT_F, dtype=torch.float64, device=eng.device)
    o = torch.as_tensor(np.ascontiguousarray(off, dtype=np.float64)).to(eng.device)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_shift_dev", _p(coeffs), _p(seg_offsets), int(B), int(m), int(S), _p(o), _p(buf[PAD:]))
    torch.cuda.synchronize()
    f = buf.cpu().numpy()
    assert (f[:PAD] == SENT_F).all() and (f[PAD + 24 * S:] == SENT_F).all()
    return f[PAD:PAD + 24 * S].reshape(S, 8, 3).copy()


def same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype == np.int32 and np.array_equal(got, want)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


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
        _CACHE[(m, B)] = dict(wps=wps, plan=plan, free=free, rows=plan.traj.cpu().numpy(), ro=plan.row_offsets.cpu().numpy(), at={})
    return _CACHE[(m, B)]


def product_rows_at(eng, k, delta):
    """rows_at for `layer_from_rows` from the product's own sampler: the positions of the rows of `Engine.shift(free, q * delta)`,
    sampled when first asked for and kept."""
    memo = k["at"].setdefault(tuple(float(v) for v in delta), {})

    def rows_at(q):
        if q not in memo:
            shifted = eng.sample_rows(eng.shift(k["free"], np.tile(q * np.asarray(delta, dtype=np.float64), (k["free"].B, 1))))
            memo[q] = np.ascontiguousarray(shifted.traj[:, 0:3].cpu().numpy())
        return memo[q]
    return rows_at


_RULE = {}


def rule(eng, cfg):
    """What the rule gives on the product's own rows for a configuration: computed once, shared by the tests that need it."""
    if cfg not in _RULE:
        from uav_ac.scoring import layer_from_rows
        m, B, radius, dz, max_steps, size = cfg
        k = case(eng, m, B)
        _RULE[cfg] = layer_from_rows(product_rows_at(eng, k, up(dz)), k["ro"], radius, offsets(B, size), None, max_steps)
    return _RULE[cfg]


def kinds(ilayer):
    q, earlier = ilayer[1], ilayer[2]
    return dict(layer0_with_partners=int(((q == 0) & (earlier > 0)).sum()), first_round=int(((q > 0) & (q < TILE)).sum()),
                later_round=int((q >= TILE).sum()), unresolved=int((q == -1).sum()))


# ------------------------------------------------------------------------------------------------------------ 1: the transform
def fma(a, b, c):
    """a * b + c with ONE rounding (to nearest, ties to even), through exact rationals: what the sampler's fma instruction gives."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def eval_positions(coeffs, seg_rows, dt):
    """The sampler's position chain, restated: for every segment (coeffs (S, 8, 3), seg_rows (S,)) and its rows r = 0 .. n - 1,
    t = (double)r * dt, p = c7, then p = fma(p, t, c_i) for i = 6 .. 0 -> (rows, 3)."""
    out = []
    for c, n in zip(coeffs, seg_rows):
        for r in range(int(n)):
            t = float(r) * dt
            p = [float(c[7, a]) for a in range(3)]
            for i in range(6, -1, -1):
                p = [fma(p[a], t, float(c[i, a])) for a in range(3)]
            out.append(p)
    return np.array(out).reshape(-1, 3)


def ragged_mix(eng):
    if "mix" not in _CACHE:
        from oracle import minsnap_oracle as mo
        sets = {m: mo.synthetic_missions(B, m) for m, B in ((1, 48), (2, 48), (8, 96))}
        missions = [sets[(1, 2, 8)[b % 3]][b] for b in range(45)]
        assert sorted({len(w) - 1 for w in missions}) == [1, 2, 8]
        _CACHE["mix"] = dict(with_rows=eng.plan_ragged(missions, VEL, DT), free=eng.plan_ragged(missions, VEL, DT, rows=False))
    return _CACHE["mix"]


def test_shift_equals_shift_coeffs_and_moves_columns_0_to_2_only(eng):
    import torch
    from uav_ac.scoring import shift_coeffs
    rng = np.random.default_rng(11)
    k = case(eng, 8, 96)
    mix = ragged_mix(eng)
    for name, src, with_rows in (("uniform", k["free"], k["plan"]), ("ragged", mix["free"], mix["with_rows"])):
        ragged = hasattr(src, "seg_offsets")
        B, m = src.B, src.max_m if ragged else src.m
        S = int(src.seg_offsets_host[-1]) if ragged else B * m
        off = rng.uniform(-2.0, 2.0, (B, 3))
        off[::7] = 0.0                                       # not moved
        off[3] = [0.0, -0.0, 0.0]
        off[5] = [0.0, 0.0, -0.75]                           # one axis only
        co = src.coeffs.cpu().numpy().reshape(S, 8, 3)
        want = shift_coeffs(co, src.seg_offsets_host if ragged else m, off)
        got = shift_abi(eng, src.coeffs, src.seg_offsets if ragged else None, B, m, S, off)
        assert same_bits(got, want), name
        assert same_bits(got[:, 1:], co[:, 1:]) and not same_bits(got[:, 0], co[:, 0])
        so = src.seg_offsets_host if ragged else np.arange(B + 1) * m
        for b in (0, 3, 7, 14):                              # zero-offset missions keep every bit
            assert same_bits(got[so[b]:so[b + 1]], co[so[b]:so[b + 1]]), (name, b)
        # Engine.shift: the same coefficients, everything else carried over bit for bit, the input left as it is
        before = src.coeffs.clone()
        sh = eng.shift(src, off)
        assert sh.traj is None and sh.waypoints is None and sh.free_times and sh.B == B and sh.max_m == m
        assert torch.equal(src.coeffs, before) and same_bits(sh.coeffs.cpu().numpy(), want)
        assert torch.equal(sh.seg_rows, src.seg_rows.reshape(-1)) and torch.equal(sh.times, src.times.reshape(-1))
        assert torch.equal(sh.row_offsets, src.row_offsets) and np.array_equal(sh.seg_offsets_host, so)
        assert torch.equal(sh.seg_offsets.cpu(), torch.as_tensor(so)) and sh.total_rows == with_rows.total_rows
        assert torch.equal(sh.first_yaw, with_rows.first_yaw) and torch.equal(eng.first_yaw(sh), with_rows.first_yaw)
        # from the plan with rows and from a device tensor of offsets: the same batch
        again = eng.shift(with_rows, torch.as_tensor(off).to(eng.device))
        assert torch.equal(again.coeffs, sh.coeffs) and again.traj is None
        # the rows: columns 3:11 are the original's, columns 0:3 the fma chain on the shifted coefficients
        rowed = eng.shift(src, off, rows=True)
        rows, orig = rowed.traj.cpu().numpy(), with_rows.traj.cpu().numpy()
        assert rows.shape == orig.shape and same_bits(rows[:, 3:], orig[:, 3:]) and not same_bits(rows[:, 0:3], orig[:, 0:3])
        ro = with_rows.row_offsets.cpu().numpy()
        for b in (0, 3, 7, 14):
            assert same_bits(rows[ro[b]:ro[b + 1]], orig[ro[b]:ro[b + 1]]), (name, b)
        some = [1, 5, B - 1]
        for b in some:
            chain = eval_positions(want[so[b]:so[b + 1]], src.seg_rows.reshape(-1).cpu().numpy()[so[b]:so[b + 1]], DT)
            assert np.array_equal(rows[ro[b]:ro[b + 1], 0:3], chain), (name, b)
            # the row of t = 0 is c0' itself, and the move is the offset up to the roundings of the chain
            firsts = ro[b] + np.concatenate([[0], np.cumsum(src.seg_rows.reshape(-1).cpu().numpy()[so[b]:so[b + 1]])[:-1]])
            assert same_bits(rows[firsts, 0:3], want[so[b]:so[b + 1], 0])
            moved = rows[ro[b]:ro[b + 1], 0:3] - orig[ro[b]:ro[b + 1], 0:3]
            assert np.abs(moved - off[b]).max() < 1e-12
    # in place is allowed: the output may be the input
    inplace = k["free"].coeffs.clone()
    off = rng.uniform(-1.0, 1.0, (96, 3))
    o = torch.as_tensor(off).to(eng.device)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_shift_dev", _p(inplace), None, 96, 8, 0, _p(o), _p(inplace))
    torch.cuda.synchronize()
    assert same_bits(inplace.cpu().numpy().reshape(-1, 8, 3), shift_coeffs(k["free"].coeffs.cpu().numpy(), 8, off).reshape(-1, 8, 3))
    # non-finite offsets pass through, and the mission then counts as excluded downstream
    off = np.zeros((96, 3))
    off[4, 2] = np.nan
    sep = eng.separation(eng.shift(k["free"], off), 0.5, 32)
    assert math.isnan(float(sep.min_distance[4])) and int(sep.compared[5]) == 30


# ------------------------------------------------------------------------------------------------ 2: the product's own rows
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "m%d-B%d-r%g-dz%g-max%d-groups%d" % c)
def test_layer_equals_the_rule_on_the_products_rows(eng, cfg):
    m, B, radius, dz, max_steps, size = cfg
    k = case(eng, m, B)
    assert k["free"].traj is None
    want = rule(eng, cfg)
    kw = dict(go=offsets(B, size), radius=radius, delta=up(dz), max_steps=max_steps)
    got_free = layer_of_plan(eng, k["free"], **kw)
    got_rows = layer_of_plan(eng, k["plan"], **kw)
    assert same(got_free, got_rows), cfg
    assert same(got_free, want), (cfg, np.argwhere(got_free != want)[:8], got_free[:, (got_free != want).any(axis=0)][:, :8],
                                  want[:, (got_free != want).any(axis=0)][:, :8])
    n = kinds(want)
    print(f"layer {cfg}: {n}, highest layer {int(want[0].max())}")
    assert n["layer0_with_partners"] > 0 and n["first_round"] > 0 and n["unresolved"] > 0, n
    if max_steps >= TILE:
        assert n["later_round"] > 0, n                       # the sets cannot go trivial: every kind is there
    assert (want[0] == np.maximum(want[1], 0)).all()


def test_uneven_groups_with_fixed_starts_and_a_ragged_batch(eng):
    from uav_ac.scoring import layer_from_rows
    B = 96
    k = case(eng, 8, B)
    go, st = np.array([0, 1, B // 3, B // 3, B]), (np.arange(B) % 5) * 37
    want = layer_from_rows(product_rows_at(eng, k, up(0.25)), k["ro"], 0.5, go, st, 7)
    assert same(layer_of_plan(eng, k["free"], go=go, start=st, max_steps=7), want)
    assert same(layer_of_plan(eng, k["plan"], go=go, start=st, max_steps=7), want)
    assert (want[1] > 0).any() and ((want[1] == 0) & (want[2] > 0)).any()
    assert want[2].tolist() == [0] + list(range(B // 3 - 1)) + list(range(B - B // 3))
    assert not same(want, layer_from_rows(product_rows_at(eng, k, up(0.25)), k["ro"], 0.5, go, None, 7))     # (the starts matter)
    # ragged: m in {1, 2, 8}, one airspace of 45 and uneven groups, a lateral delta
    mix = ragged_mix(eng)
    free, with_rows = mix["free"], mix["with_rows"]
    ro = with_rows.row_offsets.cpu().numpy()
    kk = dict(free=free, at={})
    delta = np.array([0.25, 0.0, -0.125])
    for go, st in ((None, None), (np.array([0, 1, 15, 15, 45]), (np.arange(45) % 5) * 37)):
        want = layer_from_rows(product_rows_at(eng, kk, delta), ro, 0.5, go, st, 9)
        assert same(layer_of_plan(eng, free, go=go, start=st, delta=delta, max_steps=9), want), go
        assert same(layer_of_plan(eng, with_rows, go=go, start=st, delta=delta, max_steps=9), want), go
        assert (want[1] > 0).any() and (want[1] == 0).any()


# ---------------------------------------------------------------------------------------------------------- 3: tile edges
def test_groups_of_one_tile_one_less_one_more_and_two_tiles(eng):
    from uav_ac.scoring import layer_from_rows
    k = case(eng, 8, 192)
    free = k["free"]
    for go, dz, max_steps in (([0, TILE - 1, 2 * TILE - 1, 192], 0.125, 15), ([0, 2 * TILE + 1, 192], 0.25, 5)):
        want = layer_from_rows(product_rows_at(eng, k, up(dz)), k["ro"], 0.5, go, None, max_steps)
        got = layer_of_plan(eng, free, go=np.array(go), delta=up(dz), max_steps=max_steps)
        assert same(got, want), (go, np.argwhere(got != want)[:8])
        # the same groups as batches of their own, without offsets
        for b0, b1 in zip(go[:-1], go[1:]):
            alone = layer_abi(eng, free.coeffs[b0:b1], free.seg_rows[b0:b1], None, b1 - b0, 8, DT, delta=up(dz), max_steps=max_steps)[0]
            assert same(alone, want[:, b0:b1]), (go, b0, b1)
        if go[1] > TILE:                                     # the second j-tile decides something: layers and layer 0 past index 64
            assert (want[1, TILE:go[1]] > 0).any() and (want[1, TILE:go[1]] == 0).any()


# ------------------------------------------------------------------------------------------------------------ 4: the oracle
def candidate_margin(rows_at, ro, radius, go, ilayer, start, max_steps):
    """The smallest |minimum distance of an examined candidate - radius| on these rows: how far the nearest decision is from flipping.
    Examined are the candidates q = 0 .. steps of a resolved mission and all of an unresolved one, each against the missions decided
    before it on their granted layers."""
    N = np.diff(ro)
    worst = np.inf
    for g in range(len(go) - 1):
        done = []
        for i in range(int(go[g]), int(go[g + 1])):
            if ilayer[1, i] == -2:
                continue
            if done:
                last = max_steps if ilayer[1, i] < 0 else int(ilayer[1, i])
                kk = np.arange(max(max(int(start[j]) + int(N[j]) for j in done), int(start[i]) + int(N[i])))
                others = np.stack([rows_at(int(ilayer[0, j]))[ro[j] + np.clip(kk - start[j], 0, N[j] - 1), 0:3] for j in done])
                at = ro[i] + np.clip(kk - start[i], 0, N[i] - 1)
                for q in range(last + 1):
                    own = rows_at(q)[at, 0:3]
                    d = math.sqrt(float(((own[None] - others) ** 2).sum(axis=2).min()))
                    worst = min(worst, abs(d - radius))
            done.append(i)
    return worst


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "m%d-B%d-r%g-dz%g-max%d-groups%d" % c)
def test_layer_against_the_oracle(eng, cfg):
    from oracle import c_oracle as cc
    from uav_ac.scoring import layer_from_rows
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
    want = layer_from_rows(rows_at, ro, radius, go, None, max_steps)
    margin = candidate_margin(rows_at, ro, radius, go, want, np.zeros(B, dtype=np.int64), max_steps)
    print(f"layer vs oracle {cfg}: nearest decision {margin:.3e} from the radius; {kinds(want)}")
    assert margin >= MARGIN, margin
    got = layer_of_plan(eng, k["free"], go=go, radius=radius, delta=up(dz), max_steps=max_steps)
    differing = int((got != want).any(axis=0).sum())
    assert differing == 0 and same(got, want), (cfg, differing, np.argwhere(got != want)[:8])
    assert same(got, rule(eng, cfg))


# ------------------------------------------------------------------------------------------------- 5: the guarantee, end to end
def test_the_audit_of_the_shifted_plan_confirms_the_granted_layers(eng):
    from uav_ac.scoring import layer_ok
    m, B, radius, dz, max_steps, size = CONFIGS[0]
    k = case(eng, m, B)
    res = eng.layer(k["free"], radius, groups=size, delta=up(dz), max_steps=max_steps)
    assert res.layers.is_cuda and res.block.shape == (3, B) and res.block.dtype.is_floating_point is False and res.offsets.shape == (B, 3)
    assert np.array_equal(res.block.cpu().numpy(), np.stack([t.cpu().numpy() for t in (res.layers, res.steps, res.earlier)]))
    assert same(res.block.cpu().numpy(), rule(eng, CONFIGS[0]))
    assert np.array_equal(res.offsets.cpu().numpy(), res.layers.cpu().numpy()[:, None] * up(dz)[None, :])
    shifted = eng.shift(k["free"], res.offsets)
    before = eng.separation(k["free"], radius, groups=size)
    after = eng.separation(shifted, radius, groups=size)
    ok = layer_ok(res)
    steps = res.steps.cpu().numpy()
    assert ok["examined"].all() and np.array_equal(ok["resolved"], steps >= 0) and not ok["resolved"].all()
    conflicts, first = after.conflicts.cpu().numpy(), after.first_conflict.cpu().numpy()
    go = offsets(B, size)
    whole = [g for g in range(len(go) - 1) if ok["resolved"][go[g]:go[g + 1]].all()]
    # with more layers every group is wholly resolved: the guarantee is checked on both
    more = eng.layer(k["free"], radius, groups=size, delta=up(dz), max_steps=15)
    assert layer_ok(more)["resolved"].all() and int(more.layers.max()) > max_steps
    clean = eng.separation(eng.shift(k["free"], more.offsets), radius, groups=size)
    assert int(clean.conflicts.sum()) == 0 and bool((clean.first_conflict == -1).all())
    for g in whole:
        assert (conflicts[go[g]:go[g + 1]] == 0).all() and (first[go[g]:go[g + 1]] == -1).all(), g
    # no pair of RESOLVED missions is inside: a resolved mission meets unresolved ones at most
    assert (conflicts[ok["resolved"]] <= (~ok["resolved"]).sum()).all()
    n_before, n_after = int((before.conflicts.cpu().numpy() > 0).sum()), int((conflicts > 0).sum())
    print(f"layer guarantee: {n_before} missions in conflict before, {n_after} after {max_steps} layers, 0 after 15")
    assert n_before > n_after
    # the same through the other forms of `groups`, and with rows
    again = eng.layer(k["plan"], radius, groups=go, delta=up(dz), max_steps=max_steps)
    assert np.array_equal(again.block.cpu().numpy(), res.block.cpu().numpy())
    on_device = eng.layer(k["free"], radius, groups=_i64(eng, go), delta=up(dz), max_steps=max_steps)
    assert np.array_equal(on_device.block.cpu().numpy(), res.block.cpu().numpy())
    assert same_bits(on_device.offsets.cpu().numpy(), res.offsets.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------ 6: the chain
@pytest.mark.parametrize("size", (32, 96))
def test_stagger_then_layers_at_the_granted_starts_leaves_nobody_unresolved(eng, size):
    from uav_ac.scoring import layer_ok, stagger_ok
    B, radius = 96, 0.5
    k = case(eng, 8, B)
    free = k["free"]
    stag = eng.stagger(free, radius, groups=size)
    dead = ~stagger_ok(stag)["resolved"]
    assert dead.sum() > 0                                    # waiting alone leaves dead ends
    res = eng.layer(free, radius, groups=size, start_rows=stag.start_rows, delta=up(0.25), max_steps=15)
    ok = layer_ok(res)
    layers = res.layers.cpu().numpy()
    print(f"chain, groups of {size}: {int(dead.sum())} dead ends after stagger, {int((layers > 0).sum())} missions layered, highest layer "
          f"{int(layers.max())}, unresolved {int((~ok['resolved']).sum())}")
    assert ok["examined"].all() and int((~ok["resolved"]).sum()) == 0
    assert (layers[dead] > 0).any()
    shifted = eng.shift(free, res.offsets)
    at_starts = eng.separation(shifted, radius, groups=size, start_rows=stag.start_rows)
    assert int(at_starts.conflicts.sum()) == 0
    flown = eng.delay(shifted, stag.start_rows)              # the plan to fly: layers and delays are part of it
    clean = eng.separation(flown, radius, groups=size)
    assert int(clean.conflicts.sum()) == 0 and bool((clean.first_conflict == -1).all())
    assert int(clean.compared.min()) == size - 1


# ------------------------------------------------------------------------------------------------------------ 7: independence
def test_a_group_alone_other_company_and_a_second_call_give_the_same_bits(eng):
    import torch
    cfg = CONFIGS[0]
    m, B, radius, dz, max_steps, size = cfg
    k = case(eng, m, B)
    free, want = k["free"], rule(eng, cfg)
    kw = dict(radius=radius, delta=up(dz), max_steps=max_steps)
    go = offsets(B, size)
    first = layer_of_plan(eng, free, go=go, **kw)
    second = layer_of_plan(eng, free, go=go, **kw)
    assert same(first, want) and same(second, first)
    for g in range(len(go) - 1):                             # every group as a batch of its own
        b0, b1 = int(go[g]), int(go[g + 1])
        alone = layer_abi(eng, free.coeffs[b0:b1], free.seg_rows[b0:b1], None, b1 - b0, m, DT, **kw)[0]
        assert same(alone, want[:, b0:b1]), g
    # other company: the groups in another order, and one of them beside a stranger
    order = [2, 0, 1]
    idx = np.concatenate([np.arange(go[g], go[g + 1]) for g in order])
    sel = torch.as_tensor(idx, device=eng.device)
    mixed = layer_abi(eng, free.coeffs[sel].contiguous(), free.seg_rows[sel].contiguous(), None, B, m, DT, go=go, **kw)[0]
    assert same(mixed, want[:, idx])
    other = case(eng, 8, 192)["free"]
    coeffs = torch.cat([other.coeffs[100:140], free.coeffs[size:2 * size]])
    seg_rows = torch.cat([other.seg_rows[100:140], free.seg_rows[size:2 * size]])
    beside = layer_abi(eng, coeffs, seg_rows, None, 40 + size, m, DT, go=np.array([0, 40, 40 + size]), **kw)[0]
    assert same(np.ascontiguousarray(beside[:, 40:]), want[:, size:2 * size])


def test_excluded_missions_a_copy_radius_zero_zero_delta_and_negative_starts(eng):
    import torch
    from oracle import minsnap_oracle as mo
    from uav_ac.scoring import layer_from_rows
    B = 37
    wps = mo.synthetic_missions(B, 8).copy()
    wps[5, 3] = wps[5, 2]                                                            # a repeated waypoint: singular knot system
    wps[20] = wps[11]                                                                # an exact copy of an earlier mission
    plan = eng.plan(wps, VEL, DT, strict=False)
    assert plan.status.cpu().tolist() == [1 if b == 5 else 0 for b in range(B)]
    free = eng.plan(wps, VEL, DT, strict=False, rows=False)
    ro = plan.row_offsets.cpu().numpy()
    k = dict(free=free, at={})
    st = (np.arange(B) % 4) * 11
    rows_at = product_rows_at(eng, k, up(0.25))
    il = layer_of_plan(eng, plan, start=st, max_steps=7)
    assert same(il, layer_from_rows(rows_at, ro, 0.5, None, st, 7))
    assert il[:, 5].tolist() == [0, -2, 0]                                            # excluded: not examined
    assert il[2].tolist() == [b if b < 5 else (0 if b == 5 else b - 1) for b in range(B)]        # the skipped neighbour is visible
    assert il[1, 20] != 0 and il[2, 20] == 19                                         # the copy cannot stay on the layer of what it copies
    # radius 0 moves nobody: the test is strict, not even the copy is inside
    zero = layer_of_plan(eng, plan, start=st, radius=0.0)
    assert (zero[0] == 0).all() and zero[1].tolist() == [-2 if b == 5 else 0 for b in range(B)] and (zero[2] == il[2]).all()
    # an all-zero delta is legal: every candidate is the mission itself, so steps is 0, -1 or -2
    flat = layer_of_plan(eng, plan, start=st, delta=(0.0, 0.0, 0.0), max_steps=70)
    assert same(flat, layer_from_rows(lambda q: rows_at(0), ro, 0.5, None, st, 70))
    assert set(flat[1].tolist()) == {0, -1, -2} and flat[1, 20] == -1 and (flat[0] == 0).all()
    # negative starts are clamped to 0 and raise flag 0
    eng.take_flags()
    assert same(layer_of_plan(eng, plan, start=st, max_steps=7), il) and eng.take_flags() == [0, 0, 0, 0]
    neg = st.copy()
    neg[st == 0] = -1 - np.arange((st == 0).sum())
    assert same(layer_of_plan(eng, plan, start=neg, max_steps=7), il)
    assert eng.take_flags() == [1, 0, 0, 0]
    # a mission without rows is excluded as well (seg_rows zeroed: what a bad speed leaves), and one with a non-finite coefficient
    seg_rows = plan.seg_rows.clone()
    seg_rows[7] = 0
    coeffs = plan.coeffs.clone()
    coeffs[9, 13, 1] = float("inf")
    got = layer_abi(eng, coeffs, seg_rows, None, B, 8, DT, start=st, max_steps=7)[0]
    assert got[:, 7].tolist() == [0, -2, 0] and got[:, 5].tolist() == [0, -2, 0] and got[:, 9].tolist() == [0, -2, 0]
    assert got[2, 36] == 33 and eng.take_flags() == [0, 0, 0, 0]
    keep = np.array([b for b in range(B) if b not in (5, 7, 9)])
    sel = torch.as_tensor(keep, device=eng.device)
    alone = layer_abi(eng, plan.coeffs[sel].contiguous(), plan.seg_rows[sel].contiguous(), None, len(keep), 8, DT, start=st[keep], max_steps=7)[0]
    assert same(np.ascontiguousarray(got[:, keep]), alone)                            # the others decide as if the three were not there


def test_a_group_above_the_limit_on_the_device(eng):
    import torch
    from types import SimpleNamespace
    from uav_ac import _native as nat
    k = case(eng, 8, 96)
    free = k["free"]
    n = nat.LAYER_MAX_GROUP + 1
    B = 3 * 96
    coeffs, seg_rows = torch.cat([free.coeffs] * 3), torch.cat([free.seg_rows] * 3)
    st = np.arange(B) % 9
    eng.take_flags()
    got = layer_abi(eng, coeffs, seg_rows, None, B, 8, DT, go=np.array([0, n, B]), start=st, max_steps=7)[0]
    assert eng.take_flags() == [1, 0, 0, 0]
    assert (got[0, :n] == 0).all() and (got[1, :n] == -2).all() and (got[2, :n] == 0).all()
    b0 = n - 2 * 96                                                                   # the neighbour: missions b0 .. 95 of the set
    alone = layer_abi(eng, free.coeffs[b0:], free.seg_rows[b0:], None, 96 - b0, 8, DT, start=st[n:], max_steps=7)[0]
    assert same(np.ascontiguousarray(got[:, n:]), alone) and (alone[1] > 0).any()
    # a group of exactly the limit is examined
    full = layer_abi(eng, coeffs, seg_rows, None, B, 8, DT, go=np.array([0, n - 1, B]), start=st, max_steps=0)[0]
    assert eng.take_flags() == [0, 0, 0, 0] and (full[1] != -2).all() and full[2, n - 2] == n - 2
    # Engine.layer: offsets on the host are refused, offsets on the device go through and the flag tells
    plan3 = SimpleNamespace(coeffs=coeffs, seg_rows=seg_rows, B=B, m=8, dt=DT)
    with pytest.raises(ValueError):
        eng.layer(plan3, 0.5, groups=[0, n, B])
    with pytest.raises(ValueError):
        eng.layer(plan3, 0.5, groups=n)
    with pytest.raises(ValueError):
        eng.layer(plan3, 0.5)
    res = eng.layer(plan3, 0.5, groups=_i64(eng, [0, n, B]), start_rows=st, delta=up(0.25), max_steps=7)
    assert np.array_equal(res.block.cpu().numpy(), got) and eng.take_flags() == [1, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------------ 8: flight
def test_the_shifted_plan_flies(eng):
    import torch
    B = 32
    k = case(eng, 8, 96)
    res = eng.layer(k["free"], 0.5, groups=32, delta=up(0.25), max_steps=15)
    whole = eng.shift(k["free"], res.offsets)
    assert int((res.layers[:B] > 0).sum()) > 0
    from oracle import minsnap_oracle as mo
    wps = mo.synthetic_missions(96, 8)[:B]
    free = eng.plan(wps, VEL, DT, rows=False)
    shifted = eng.shift(free, res.offsets[:B])
    assert torch.equal(shifted.coeffs, whole.coeffs[:B * 8])
    fleet = eng.fleet(shifted)
    assert fleet.from_plan
    start = shifted.coeffs[shifted.seg_offsets[:-1], 0, :]
    assert torch.equal(shifted.start_positions, start) and torch.equal(fleet.state[0:3].T.contiguous(), start)
    assert torch.equal(start, free.coeffs.reshape(B, 8, 8, 3)[:, 0, 0, :] + res.offsets[:B])
    fleet.rollout(300, score=True)
    t = fleet.tracking()
    assert all(bool(torch.isfinite(t[key]).all()) for key in ("mean_error", "rms_error", "max_error"))
    assert bool((t["rows_scored"] > 0).all())
    # the handover: a flying fleet follows the shifted plan like any other
    flying = eng.fleet(free)
    flying.rollout(40)
    flying.follow(shifted)
    flying.rollout(40, score=True)
    assert bool(torch.isfinite(flying.state).all())


# -------------------------------------------------------------------------------------------------------------- 9: validation
def test_invalid_arguments_are_refused_before_anything_is_enqueued(eng):
    import torch
    from uav_ac import _native as nat
    B, m = 96, 8
    k = case(eng, m, B)
    free = k["free"]
    il = torch.full((3 * B,), SENT_I, dtype=torch.int32, device=eng.device)
    off = torch.full((3 * B,), SENT_F, dtype=torch.float64, device=eng.device)
    go = _i64(eng, [0, 32, 64, B])
    good = dict(coeffs=free.coeffs, seg_rows=free.seg_rows, seg_offsets=None, B=B, m=m, dt=DT, go=go, G=3, start=None, radius=0.5,
                dx=0.0, dy=0.0, dz=-0.25, max_steps=3, il=il, off=off)
    bad = [dict(coeffs=None), dict(seg_rows=None), dict(il=None), dict(off=None), dict(B=0), dict(B=-3), dict(m=0),
           dict(m=nat.MAX_SEGMENTS + 1), dict(dt=0.0), dict(dt=-0.01), dict(dt=math.inf), dict(dt=math.nan), dict(radius=-0.5),
           dict(radius=math.inf), dict(radius=math.nan), dict(G=0), dict(G=-2), dict(dx=math.nan), dict(dy=math.inf), dict(dz=-math.inf),
           dict(dz=math.nan), dict(max_steps=-1), dict(max_steps=nat.LAYER_MAX_STEPS + 1)]
    eng._bind_stream()
    fn = nat.lib().uavac_minsnap_layer_dev

    def call(ctx, a):
        return fn(ctx, _p(a["coeffs"]), _p(a["seg_rows"]), _p(a["seg_offsets"]), a["B"], a["m"], a["dt"], _p(a["go"]), a["G"], _p(a["start"]),
                  a["radius"], a["dx"], a["dy"], a["dz"], a["max_steps"], _p(a["il"]), _p(a["off"]))
    for change in bad:
        rc = call(eng.ctx._h, {**good, **change})
        assert rc == nat.EINVAL, (change, rc)
        assert (nat.lib().uavac_last_error(eng.ctx._h) or b"") != b"", change
    assert call(None, good) == nat.EINVAL                                            # no context
    # one group of all B above the limit: the host can see that
    big = torch.cat([free.coeffs] * 3), torch.cat([free.seg_rows] * 3)
    wide_i = torch.full((3 * 3 * B,), SENT_I, dtype=torch.int32, device=eng.device)
    wide_f = torch.full((3 * 3 * B,), SENT_F, dtype=torch.float64, device=eng.device)
    assert call(eng.ctx._h, {**good, "coeffs": big[0], "seg_rows": big[1], "B": 3 * B, "go": None, "G": 0, "il": wide_i, "off": wide_f}) == nat.EINVAL
    # the transform's refusals
    out = torch.full((B * m * 24,), SENT_F, dtype=torch.float64, device=eng.device)
    offs = torch.zeros((B, 3), dtype=torch.float64, device=eng.device)
    so = _i64(eng, np.arange(B + 1) * m)
    shift = nat.lib().uavac_minsnap_shift_dev
    for args in ((None, None, B, m, 0, _p(offs), _p(out)), (_p(free.coeffs), None, B, m, 0, None, _p(out)),
                 (_p(free.coeffs), None, B, m, 0, _p(offs), None), (_p(free.coeffs), None, 0, m, 0, _p(offs), _p(out)),
                 (_p(free.coeffs), None, B, 0, 0, _p(offs), _p(out)), (_p(free.coeffs), None, B, nat.MAX_SEGMENTS + 1, 0, _p(offs), _p(out)),
                 (_p(free.coeffs), _p(so), B, m, 0, _p(offs), _p(out)), (_p(free.coeffs), _p(so), B, m, B * m + 1, _p(offs), _p(out))):
        assert shift(eng.ctx._h, *args) == nat.EINVAL, args
    assert shift(None, _p(free.coeffs), None, B, m, 0, _p(offs), _p(out)) == nat.EINVAL
    torch.cuda.synchronize()
    assert bool((il == SENT_I).all()) and bool((off == SENT_F).all()) and bool((wide_i == SENT_I).all()) and bool((wide_f == SENT_F).all())
    assert bool((out == SENT_F).all())
    # the same calls with nothing wrong go through; G is ignored without offsets
    assert call(eng.ctx._h, good) == nat.OK
    torch.cuda.synchronize()
    assert same(il.cpu().numpy().reshape(3, B), rule(eng, CONFIGS[0]))
    assert call(eng.ctx._h, {**good, "go": None, "G": 0, "max_steps": 0}) == nat.OK
    assert shift(eng.ctx._h, _p(free.coeffs), _p(so), B, m, B * m, _p(offs), _p(out)) == nat.OK
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), free.coeffs.cpu().numpy().reshape(-1))
    # Engine.layer and Engine.shift refuse on the host what the host can see
    for kw in (dict(start_rows=np.zeros(5)), dict(groups=0), dict(max_steps=-1), dict(max_steps=nat.LAYER_MAX_STEPS + 1), dict(groups=[0]),
               dict(delta=(0.0, 0.0)), dict(delta=(0.0, math.nan, -0.5)), dict(delta=(math.inf, 0.0, 0.0))):
        with pytest.raises(ValueError):
            eng.layer(free, 0.5, **kw)
    for bad_off in (np.zeros((B - 1, 3)), np.zeros((B, 2)), np.zeros(3)):
        with pytest.raises(ValueError):
            eng.shift(free, bad_off)
