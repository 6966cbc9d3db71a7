"""Deconfliction against committed traffic that never moves, on the GPU (`uavac_minsnap_separation_against_dev`,
`uavac_minsnap_stagger_against_dev`, `uavac_minsnap_layer_against_dev`, csrc/fleet_against.h), through the C ABI and through
`Engine.separation_against` and `Engine.stagger / layer / deconflict(..., traffic=)`.

The method is tests/test_gpu_wide.py's, whose helpers are imported: sentinel-padded output buffers, `same()` on int32, every answer of
a rule computed once per module on the product's own rows.  Missions: `synthetic_missions(220, 3)` at velocity 3, radius 0.5, start
rows (b % 5) * 7 over the 220.  Missions 0 .. 69 are the TRAFFIC -- two j-tiles, the second one holding 6 --, missions 70 .. 219 the
PLAN: blocks of 64, 64 and 22.  Groups: one on each side, or the plan's [0, 63, 128, 150] against the traffic's [0, 0, 65, 70], whose
group 0 has no traffic.
A fixture could pass by being trivial, so before a comparison counts the test asserts on the rule's own answer: somebody past block
0 differs from the rule without traffic; somebody is granted a candidate >= 64 (a second seed word); somebody is unresolved; the first
mission of a group that has traffic has steps != 0 (it was examined, which without traffic it never is)."""
import math

import numpy as np
import pytest

from test_gpu_layer import PAD, SENT_F, SENT_I, _i32, _i64, _p, product_rows_at, same, same_bits
from test_gpu_wide import CUBOIDS, RADIUS, TILE, block_size, case, once, out_i, parts, read_i, stag, starts

pytestmark = pytest.mark.gpu

N_ALL, N_T = 220, 70
N_P = N_ALL - N_T
GO3, TGO3 = np.array([0, 63, 128, 150]), np.array([0, 0, 65, 70])
UP = np.array([0.0, 0.0, -0.01])


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    return Engine("cuda:0")


def sides(eng, dt):
    """Per dt, computed once and left unchanged: the traffic and the plan as rows-free batches and with rows, their rows and row
    offsets on the host, their start rows."""
    k = case(eng, N_ALL, dt)

    def make():
        rows, ro, st = k["rows"], k["ro"], starts(N_ALL)
        cut = ro[N_T]
        t_idx, p_idx = np.arange(N_T), np.arange(N_T, N_ALL)
        return dict(traffic=eng.take(k["free"], t_idx), plan=eng.take(k["free"], p_idx), plan_rows=eng.take(k["free"], p_idx, rows=True),
                    trows=rows[:cut, 0:3].copy(), tro=ro[:N_T + 1].copy(), prows=rows[cut:, 0:3].copy(), pro=ro[N_T:] - cut,
                    tst=st[:N_T].copy(), pst=st[N_T:].copy(), at={}, memo={})
    return once(k, "sides", make)


def t_args(eng, traffic, tgo, tstart, t_coeffs=None, t_seg_rows=None):
    """the seven arguments of the traffic, and the tensors behind them"""
    co, sr, so, Bt, mt, _ = parts(traffic)
    g, s = _i64(eng, tgo), _i32(eng, tstart)
    held = (co if t_coeffs is None else t_coeffs, sr if t_seg_rows is None else t_seg_rows, so, g, s)
    return held, (_p(held[0]), _p(held[1]), _p(so), Bt, mt, _p(g), _p(s))


def stag_against(eng, plan, traffic, go=None, tgo=None, cap=None, start=None, tstart=None, step=1, max_steps=100, radius=RADIUS,
                 coeffs=None, seg_rows=None, t_coeffs=None, t_seg_rows=None):
    """One call of uavac_minsnap_stagger_against_dev -> istag (3, B), from a sentinel-padded buffer."""
    import torch
    co, sr, so, B, m, dt = parts(plan)
    buf = out_i(eng, 3, B)
    g, s = _i64(eng, go), _i32(eng, start)
    held, targs = t_args(eng, traffic, tgo, tstart, t_coeffs, t_seg_rows)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_stagger_against_dev", _p(co if coeffs is None else coeffs), _p(sr if seg_rows is None else seg_rows), _p(so), B, m,
                 dt, _p(g), 0 if go is None else len(go) - 1, *targs, int(B if cap is None else cap), _p(s), float(radius), int(step),
                 int(max_steps), _p(buf[PAD:]))
    torch.cuda.synchronize()
    return read_i(buf, 3, B)


def lay_against(eng, plan, traffic, go=None, tgo=None, cap=None, start=None, tstart=None, delta=UP, max_steps=100, cuboids=None,
                radius=RADIUS):
    """One call of uavac_minsnap_layer_against_dev -> (ilayer (4, B), offsets (B, 3)); the offsets are fl(layer * delta), bit for bit."""
    import torch
    co, sr, so, B, m, dt = parts(plan)
    buf = out_i(eng, 4, B)
    fbuf = torch.full((PAD + 3 * B + PAD,), SENT_F, dtype=torch.float64, device=eng.device)
    g, s = _i64(eng, go), _i32(eng, start)
    n = 0 if cuboids is None else len(cuboids)
    cub = torch.as_tensor(np.ascontiguousarray(cuboids, dtype=np.float64)).to(eng.device) if n else None
    held, targs = t_args(eng, traffic, tgo, tstart)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_layer_against_dev", _p(co), _p(sr), _p(so), B, m, dt, _p(g), 0 if go is None else len(go) - 1, *targs,
                 int(B if cap is None else cap), _p(s), float(radius), float(delta[0]), float(delta[1]), float(delta[2]), int(max_steps), _p(cub), n,
                 _p(buf[PAD:]), _p(fbuf[PAD:]))
    torch.cuda.synchronize()
    f = fbuf.cpu().numpy()
    assert (f[:PAD] == SENT_F).all() and (f[PAD + 3 * B:] == SENT_F).all() and not (f[PAD:PAD + 3 * B] == SENT_F).any()
    il, off = read_i(buf, 4, B), f[PAD:PAD + 3 * B].reshape(B, 3).copy()
    assert same_bits(off, il[0][:, None] * np.asarray(delta, dtype=np.float64)[None, :])
    return il, off


def sep_against(eng, plan, traffic, go=None, tgo=None, start=None, tstart=None, radius=RADIUS):
    """One call of uavac_minsnap_separation_against_dev -> (sep (B,), isep (5, B)), each from a sentinel-padded buffer."""
    import torch
    co, sr, so, B, m, dt = parts(plan)
    buf = out_i(eng, 5, B)
    fbuf = torch.full((PAD + B + PAD,), SENT_F, dtype=torch.float64, device=eng.device)
    g, s = _i64(eng, go), _i32(eng, start)
    held, targs = t_args(eng, traffic, tgo, tstart)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_separation_against_dev", _p(co), _p(sr), _p(so), B, m, dt, _p(g), 0 if go is None else len(go) - 1, *targs,
                 _p(s), float(radius), _p(fbuf[PAD:]), _p(buf[PAD:]))
    torch.cuda.synchronize()
    f = fbuf.cpu().numpy()
    assert (f[:PAD] == SENT_F).all() and (f[PAD + B:] == SENT_F).all() and not (f[PAD:PAD + B] == SENT_F).any()
    return f[PAD:PAD + B].copy(), read_i(buf, 5, B)


def snapshot(plan):
    return [t.clone() for t in (plan.coeffs, plan.seg_rows, plan.seg_offsets)]


def unchanged(plan, before):
    """bitwise: the coefficients are compared as integers"""
    import torch

    def bits(t):
        return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t
    return all(torch.equal(bits(a), bits(b)) for a, b in zip((plan.coeffs, plan.seg_rows, plan.seg_offsets), before))


def stagger_rules(s, grouped):
    """(the rule with traffic, the rule without) on the product's own rows, computed once"""
    from uav_ac.scoring import stagger_against_rows, stagger_from_rows
    go, tgo = (GO3, TGO3) if grouped else (None, None)
    want = once(s, ("stagger", grouped), lambda: stagger_against_rows(s["prows"], s["pro"], s["trows"], s["tro"], RADIUS, go, tgo, s["pst"],
                                                                       s["tst"], 1, 100, max_group=N_P))
    alone = once(s, ("stagger alone", grouped), lambda: stagger_from_rows(s["prows"], s["pro"], RADIUS, go, s["pst"], 1, 100, max_group=N_P))
    return want, alone


def not_trivial(want, alone, firsts):
    later = np.arange(want.shape[1]) >= TILE
    n = dict(differ=int((want[:2] != alone[:2]).any(axis=0).sum()), differ_later=int(((want[:2] != alone[:2]).any(axis=0) & later).sum()),
             above_63=int((want[1] >= TILE).sum()), unresolved=int((want[1] == -1).sum()), firsts=want[1, firsts].tolist())
    assert n["differ_later"] > 0 and n["above_63"] > 0 and n["unresolved"] > 0 and all(v != 0 for v in n["firsts"]), n
    return n


# ------------------------------------------------------------------------------------------------ 1: stagger against the rule
def test_stagger_against_traffic_equals_the_rule_at_every_block_size(eng):
    s = sides(eng, 0.02)
    traffic, before = s["traffic"], snapshot(s["traffic"])
    want1, alone1 = stagger_rules(s, False)
    want3, alone3 = stagger_rules(s, True)
    print("stagger against 70, one group:", not_trivial(want1, alone1, [0]))
    later = np.arange(N_P) >= TILE
    assert ((want3[:2] != alone3[:2]).any(axis=0) & later).any() and want3[1, GO3[1]] != 0 and want3[2, GO3[1]] == 65
    assert np.array_equal(want3[:, :GO3[1]], alone3[:, :GO3[1]])                       # group 0 has no traffic: the plain rule
    print("stagger against 70, three groups: first of group 1", want3[:, GO3[1]].tolist(), "group 2 changes",
          int((want3[:2, GO3[2]:] != alone3[:2, GO3[2]:]).any(axis=0).sum()))
    eng.take_flags()
    wide3 = stag(eng, s["plan"], True, go=GO3, cap=N_P, start=s["pst"])                # the call without traffic, same groups
    for blk in (64, 128, 256, 0):
        with block_size(eng, blk):
            for plan in (s["plan"], s["plan_rows"]):
                assert same(stag_against(eng, plan, traffic, start=s["pst"], tstart=s["tst"]), want1), blk
                got = stag_against(eng, plan, traffic, go=GO3, tgo=TGO3, cap=65, start=s["pst"], tstart=s["tst"])
                assert same(got, want3), blk
                assert same(np.ascontiguousarray(got[:, :GO3[1]]), np.ascontiguousarray(wide3[:, :GO3[1]])), blk
    assert eng.take_flags() == [0, 0, 0, 0]
    assert unchanged(traffic, before)
    # the engine's keyword makes the same call; `wide` is not looked at
    res = eng.stagger(s["plan"], RADIUS, groups=GO3, start_rows=s["pst"], max_steps=100, traffic=traffic, traffic_groups=TGO3,
                      traffic_start_rows=s["tst"])
    assert same(res.block.cpu().numpy(), want3)
    res = eng.stagger(s["plan"], RADIUS, start_rows=s["pst"], max_steps=100, wide=False, traffic=traffic, traffic_start_rows=s["tst"])
    assert same(res.block.cpu().numpy(), want1) and eng.take_flags() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 2: layer against the rule
@pytest.mark.parametrize("cuboids", (None, CUBOIDS), ids=("no cuboids", "cuboids"))
def test_layer_against_traffic_equals_the_rule(eng, cuboids):
    from uav_ac.scoring import layer_against_rows, layer_obstacles_from_rows
    s = sides(eng, 0.04)
    k = dict(free=s["plan"], at=s["at"])
    rows_at = product_rows_at(eng, k, UP)
    cub = np.zeros((0, 6)) if cuboids is None else cuboids
    key = "cuboids" if cuboids is not None else "free"
    want = once(s, ("layer", key), lambda: layer_against_rows(rows_at, s["pro"], s["trows"], s["tro"], RADIUS, cuboids, None, None, s["pst"],
                                                              s["tst"], 100, max_group=N_P))
    alone = once(s, ("layer alone", key), lambda: layer_obstacles_from_rows(rows_at, s["pro"], RADIUS, cub, None, s["pst"], 100, max_group=N_P))
    later = np.arange(N_P) >= TILE
    n = dict(differ_later=int(((want[:2] != alone[:2]).any(axis=0) & later).sum()), moved=int((want[1] > 0).sum()),
             unresolved=int((want[1] == -1).sum()), blocked=int((want[3] > 0).sum()), first=want[:, 0].tolist())
    print(f"layer against 70 ({key}):", n)
    assert n["differ_later"] > 0 and n["moved"] > 0 and want[2, 0] == N_T and (want[1] != -2).all()
    assert n["blocked"] > 0 if cuboids is not None else n["blocked"] == 0
    before = snapshot(s["traffic"])
    eng.take_flags()
    for blk in (64, 0):
        with block_size(eng, blk):
            got, _ = lay_against(eng, s["plan"], s["traffic"], start=s["pst"], tstart=s["tst"], cuboids=cuboids)
            assert same(got, want), blk
    if cuboids is None:                                      # three groups: the one without traffic is the call without traffic
        want3 = once(s, "layer 3", lambda: layer_against_rows(rows_at, s["pro"], s["trows"], s["tro"], RADIUS, None, GO3, TGO3, s["pst"], s["tst"],
                                                              100, max_group=65))
        assert want3[2, GO3[1]] == 65
        got, off = lay_against(eng, s["plan_rows"], s["traffic"], go=GO3, tgo=TGO3, cap=65, start=s["pst"], tstart=s["tst"])
        assert same(got, want3) and not got[3].any()
        res = eng.layer(s["plan"], RADIUS, groups=GO3, start_rows=s["pst"], delta=UP, max_steps=100, traffic=s["traffic"], traffic_groups=TGO3,
                        traffic_start_rows=s["tst"])
        assert same(res.block.cpu().numpy(), want3) and same_bits(res.offsets.cpu().numpy(), off)
    assert eng.take_flags() == [0, 0, 0, 0] and unchanged(s["traffic"], before)


# ------------------------------------------------------------------------------------------------ 3: the new calls against the old ones
def interleaved(go, tgo, n_t):
    """the index into concat([traffic, plan]) that puts [traffic_g, plan_g] behind each other per group -> (index, group offsets,
    where each plan mission went)"""
    index, off, p_at = [], [0], np.zeros(int(go[-1]), dtype=np.int64)
    for g in range(len(go) - 1):
        index += list(range(int(tgo[g]), int(tgo[g + 1])))
        for i in range(int(go[g]), int(go[g + 1])):
            p_at[i] = len(index)
            index.append(n_t + i)
        off.append(len(index))
    return np.array(index), np.array(off), p_at


@pytest.mark.parametrize("grouped", (False, True), ids=("one group", "three groups"))
def test_mutually_clear_traffic_answers_as_the_wide_call_on_the_concatenation(eng, grouped):
    s = sides(eng, 0.02)
    first = eng.stagger(s["traffic"], RADIUS, groups=TGO3 if grouped else None, start_rows=s["tst"], max_steps=100).block.cpu().numpy()
    ok = np.flatnonzero(first[1] >= 0)
    print(f"traffic alone: {len(ok)} of {N_T} resolved, {int((first[1] > 0).sum())} delayed")
    assert (first[1] > 0).any() and len(ok) > N_T // 2       # somebody was delayed, and most of the traffic is still there
    clear, cstart = eng.take(s["traffic"], ok), first[0][ok]
    go = GO3 if grouped else np.array([0, N_P])
    tgo = np.array([int((ok < o).sum()) for o in TGO3]) if grouped else np.array([0, len(ok)])
    index, off, p_at = interleaved(go, tgo, len(ok))
    whole = eng.take(eng.concat([clear, s["plan"]]), index)
    st = np.concatenate([cstart, s["pst"]])[index]
    want = stag(eng, whole, True, go=off, cap=int(np.diff(off).max()), start=st)
    t_at = np.setdiff1d(np.arange(len(index)), p_at)
    assert (want[1, t_at] == 0).all()                        # clear traffic stays where it is in the re-run too
    res = eng.stagger(s["plan"], RADIUS, groups=go if grouped else None, start_rows=s["pst"], max_steps=100, traffic=clear,
                      traffic_groups=tgo if grouped else None, traffic_start_rows=cstart)
    got = res.block.cpu().numpy()
    assert same(got, np.ascontiguousarray(want[:, p_at])) and (got[1] > 0).any() and (got[1] == -1).any()
    assert eng.take_flags() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 4: the cross audit
def test_the_cross_audit_equals_the_rule_bit_for_bit(eng):
    from uav_ac.scoring import separation_against_rows
    s = sides(eng, 0.02)
    delayed = once(s, "traffic delayed", lambda: eng.delay(s["traffic"], s["tst"], rows=True))      # a ragged traffic plan: hold segments
    trows, tro = delayed.traj[:, 0:3].cpu().numpy(), delayed.row_offsets.cpu().numpy()
    tst = (np.arange(N_T) % 3) * 5
    want = once(s, "cross audit", lambda: separation_against_rows(s["prows"], s["pro"], trows, tro, RADIUS, GO3, TGO3, s["pst"], tst))
    assert np.isposinf(want[0][:GO3[1]]).all() and (want[1][2] > 0).any() and (want[1][2] == 0).any() and (want[1][4, GO3[1]:GO3[2]] == 65).all()
    eng.take_flags()
    for split in (0, 1, 3):
        eng.ctx.set_option("separation_split", split)
        sep, isep = sep_against(eng, s["plan"], delayed, go=GO3, tgo=TGO3, start=s["pst"], tstart=tst)
        assert same_bits(sep, want[0]) and same(isep, want[1]), split
    eng.ctx.set_option("separation_split", 0)
    res = eng.separation_against(s["plan_rows"], delayed, RADIUS, GO3, TGO3, s["pst"], tst)
    assert same_bits(res.min_distance.cpu().numpy(), want[0]) and same(res.block.cpu().numpy(), want[1])
    # one group on each side, no start rows on the traffic's
    want1 = once(s, "cross audit 1", lambda: separation_against_rows(s["prows"], s["pro"], trows, tro, RADIUS, start_rows=s["pst"]))
    sep, isep = sep_against(eng, s["plan"], delayed, start=s["pst"])
    assert same_bits(sep, want1[0]) and same(isep, want1[1]) and (isep[4] == N_T).all()
    # the cross pairs of the conflict list of the concatenation agree in count and first row
    index, off, p_at = interleaved(GO3, TGO3, N_T)
    whole = eng.take(eng.concat([delayed, s["plan"]]), index)
    cl = eng.conflicts(whole, RADIUS, groups=off, start_rows=np.concatenate([tst, s["pst"]])[index])
    offsets, partner, first_row = cl.offsets.cpu().numpy(), cl.partner.cpu().numpy(), cl.first_row.cpu().numpy()
    is_traffic = np.ones(len(index), dtype=bool)
    is_traffic[p_at] = False
    for i, c in enumerate(p_at):
        e = np.arange(offsets[c], offsets[c + 1])
        e = e[is_traffic[partner[e]]]
        assert want[1][2, i] == len(e) and want[1][3, i] == (first_row[e].min() if len(e) else -1), i
    assert eng.take_flags() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 5: excluded missions on both sides
def test_excluded_missions_on_both_sides(eng):
    from uav_ac.scoring import separation_against_rows, stagger_against_rows
    s = sides(eng, 0.02)
    plan, traffic = s["plan"], s["traffic"]
    pso, tso = plan.seg_offsets_host, traffic.seg_offsets_host

    def spoil(batch, so, nan_at, empty_at):
        coeffs, seg_rows = batch.coeffs.clone(), batch.seg_rows.clone()
        coeffs.reshape(-1)[int(so[nan_at]) * 24 + 5] = math.nan
        seg_rows[int(so[empty_at]):int(so[empty_at + 1])] = 0
        return coeffs, seg_rows

    def spoil_rows(rows, ro, nan_at, empty_at):
        rows, ro = rows.copy(), ro.copy()
        rows[ro[nan_at]:ro[nan_at + 1]] = np.nan
        rows = np.delete(rows, np.s_[ro[empty_at]:ro[empty_at + 1]], axis=0)
        ro[empty_at + 1:] -= ro[empty_at + 1] - ro[empty_at]
        return rows, ro
    t_co, t_sr = spoil(traffic, tso, 5, 66)                  # the traffic's first j-tile and its second
    p_co, p_sr = spoil(plan, pso, 10, 70)                    # the plan's block 0 and block 1
    trows, tro = spoil_rows(s["trows"], s["tro"], 5, 66)
    prows, pro = spoil_rows(s["prows"], s["pro"], 10, 70)
    want = stagger_against_rows(prows, pro, trows, tro, RADIUS, None, None, s["pst"], s["tst"], 2, 30, max_group=N_P)
    assert want[1, 10] == want[1, 70] == -2 and want[2, 0] == N_T - 2 and want[2, N_P - 1] == N_T - 2 + N_P - 3
    assert want[2].tolist() == [0 if b in (10, 70) else N_T - 2 + b - (b > 10) - (b > 70) for b in range(N_P)]
    eng.take_flags()
    for blk in (64, 0):
        with block_size(eng, blk):
            got = stag_against(eng, plan, traffic, start=s["pst"], tstart=s["tst"], step=2, max_steps=30, coeffs=p_co, seg_rows=p_sr,
                               t_coeffs=t_co, t_seg_rows=t_sr)
            assert same(got, want), blk
    # the audit: nobody's partner, absent from `compared`; the excluded plan missions report NaN / -1 / -1 / 0 / -1 / 0
    import torch
    wsep, wisep = separation_against_rows(prows, pro, trows, tro, RADIUS, None, None, s["pst"], s["tst"])
    co, sr, so, B, m, dt = parts(plan)
    held, targs = t_args(eng, traffic, None, s["tst"], t_co, t_sr)
    buf, fbuf = out_i(eng, 5, B), torch.full((B,), SENT_F, dtype=torch.float64, device=eng.device)
    start = _i32(eng, s["pst"])
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_separation_against_dev", _p(p_co), _p(p_sr), _p(so), B, m, dt, None, 0, *targs, _p(start), RADIUS, _p(fbuf),
                 _p(buf[PAD:]))
    torch.cuda.synchronize()
    sep, isep = fbuf.cpu().numpy(), read_i(buf, 5, B)
    assert same_bits(sep, wsep) and same(isep, wisep)
    assert np.isnan(sep[[10, 70]]).all() and isep[:, 10].tolist() == isep[:, 70].tolist() == [-1, -1, 0, -1, 0]
    assert not np.isin(isep[0], (5, 66)).any() and (np.delete(isep[4], [10, 70]) == N_T - 2).all()
    assert eng.take_flags() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 6: the guarantee
def test_the_audits_confirm_a_deconflict_against_committed_traffic(eng):
    from uav_ac.scoring import conflict_pairs
    s = sides(eng, 0.02)
    committed = eng.deconflict(s["traffic"], RADIUS, obstacles=CUBOIDS).plan
    before = snapshot(committed)
    res = eng.deconflict(s["plan"], RADIUS, obstacles=CUBOIDS, traffic=committed)
    ok = res.resolved.cpu().numpy()
    assert int(res.plan.B) == N_P and ok.any() and (res.stagger.steps.cpu().numpy() > 0).any() and (res.layer.steps.cpu().numpy() > 0).any()
    assert (res.stagger.earlier.cpu().numpy() == N_T + np.arange(N_P)).all()
    cross = eng.separation_against(res.plan, committed, RADIUS)
    assert (cross.conflicts.cpu().numpy()[ok] == 0).all() and (cross.compared.cpu().numpy() == N_T).all()
    pairs = conflict_pairs(eng.conflicts(eng.concat([committed, res.plan]), RADIUS))
    for i, j in zip(pairs["i"].tolist(), pairs["j"].tolist()):
        assert (i < N_T and j < N_T) or (i >= N_T and not ok[i - N_T]) or (j >= N_T and not ok[j - N_T]), (i, j)
    assert (eng.audit(res.plan, CUBOIDS).hit_rows.cpu().numpy().reshape(-1, N_P).sum(axis=0)[ok] == 0).all()
    assert unchanged(committed, before) and eng.take_flags() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 7: priority
def test_priority_composes_with_traffic(eng):
    from uav_ac.scoring import priority_order, stagger_against_rows, take_rows
    s = sides(eng, 0.02)
    pr = np.random.default_rng(7).permutation(N_P).astype(np.float64)
    order, rank = priority_order(pr)
    rows, ro = take_rows(s["prows"], s["pro"], order)
    want = stagger_against_rows(rows, ro, s["trows"], s["tro"], RADIUS, None, None, s["pst"][order], s["tst"], 4, 30, max_group=N_P)[:, rank]
    got = eng.stagger(s["plan"], RADIUS, start_rows=s["pst"], step=4, max_steps=30, priority=pr, traffic=s["traffic"], traffic_start_rows=s["tst"])
    assert same(got.block.cpu().numpy(), np.ascontiguousarray(want)) and (want[1] > 0).any() and (want[1] == -1).any()
    assert want[2, int(order[0])] == N_T and eng.take_flags() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 8: edges and refusals
def test_a_group_above_group_cap_no_candidates_and_a_negative_traffic_start(eng):
    s = sides(eng, 0.02)
    want3, _ = stagger_rules(s, True)
    eng.take_flags()
    got = stag_against(eng, s["plan"], s["traffic"], go=GO3, tgo=TGO3, cap=64, start=s["pst"], tstart=s["tst"])      # group 1 holds 65
    assert eng.take_flags() == [1, 0, 0, 0]
    g1 = slice(GO3[1], GO3[2])
    assert got[0, g1].tolist() == s["pst"][g1].tolist() and (got[1, g1] == -2).all() and (got[2, g1] == 0).all()
    keep = np.r_[0:GO3[1], GO3[2]:N_P]
    assert same(np.ascontiguousarray(got[:, keep]), np.ascontiguousarray(want3[:, keep])) and (want3[1, GO3[2]:] != 0).any()
    # max_steps = 0: candidate 0 or nothing
    from uav_ac.scoring import stagger_against_rows
    none = stagger_against_rows(s["prows"], s["pro"], s["trows"], s["tro"], RADIUS, None, None, s["pst"], s["tst"], 1, 0, max_group=N_P)
    assert set(none[1].tolist()) == {0, -1}
    assert same(stag_against(eng, s["plan"], s["traffic"], start=s["pst"], tstart=s["tst"], max_steps=0), none)
    il, _ = lay_against(eng, s["plan"], s["traffic"], start=s["pst"], tstart=s["tst"], max_steps=0)
    assert set(il[1].tolist()) <= {0, -1} and (il[2] == N_T + np.arange(N_P)).all() and eng.take_flags() == [0, 0, 0, 0]
    # a traffic start row of -3 is clamped to 0 and raises flag 0
    want1, _ = stagger_rules(s, False)
    tst = s["tst"].copy()
    assert tst[0] == 0
    tst[0] = -3
    assert same(stag_against(eng, s["plan"], s["traffic"], start=s["pst"], tstart=tst), want1) and eng.take_flags() == [1, 0, 0, 0]
    sep0, isep0 = sep_against(eng, s["plan"], s["traffic"], start=s["pst"], tstart=s["tst"])
    assert eng.take_flags() == [0, 0, 0, 0]
    sep, isep = sep_against(eng, s["plan"], s["traffic"], start=s["pst"], tstart=tst)
    assert same_bits(sep, sep0) and same(isep, isep0) and eng.take_flags() == [1, 0, 0, 0]


def test_invalid_arguments_are_refused_before_anything_is_enqueued(eng):
    import torch
    from uav_ac import _native as nat
    s = sides(eng, 0.02)
    plan, traffic = s["plan"], s["traffic"]
    B = N_P
    ibuf = torch.full((5 * B,), SENT_I, dtype=torch.int32, device=eng.device)
    fbuf = torch.full((3 * B,), SENT_F, dtype=torch.float64, device=eng.device)
    cub = torch.as_tensor(CUBOIDS).to(eng.device)
    go, tgo = _i64(eng, GO3), _i64(eng, TGO3)
    common = dict(coeffs=plan.coeffs, seg_rows=plan.seg_rows, seg_offsets=plan.seg_offsets, B=B, m=3, dt=0.02, go=go, G=3,
                  t_coeffs=traffic.coeffs, t_seg_rows=traffic.seg_rows, t_seg_offsets=traffic.seg_offsets, Bt=N_T, mt=3, tgo=tgo, tstart=None,
                  cap=140, start=None, radius=0.5)
    pair = [dict(coeffs=None), dict(seg_rows=None), dict(B=0), dict(B=-3), dict(m=0), dict(m=nat.MAX_SEGMENTS + 1), dict(dt=0.0), dict(dt=-0.02),
            dict(dt=math.inf), dict(dt=math.nan), dict(radius=-0.5), dict(radius=math.inf), dict(radius=math.nan), dict(G=0), dict(G=-2)]
    side = [dict(t_coeffs=None), dict(t_seg_rows=None), dict(Bt=0), dict(Bt=-1), dict(mt=0), dict(mt=nat.MAX_SEGMENTS + 1), dict(tgo=None),
            dict(go=None, G=0, cap=B)]
    wide = [dict(max_steps=-1), dict(cap=0), dict(cap=-5), dict(go=None, tgo=None, G=0, cap=B - 1)]
    good_a = dict(common, sep=fbuf, isep=ibuf)
    bad_a = pair + side + [dict(sep=None), dict(isep=None)]
    good_s = dict(common, step=8, max_steps=31, istag=ibuf)
    bad_s = pair + side + wide + [dict(istag=None), dict(step=0), dict(step=-1), dict(max_steps=nat.STAGGER_MAX_STEPS + 1),
                                  dict(step=2 ** 20, max_steps=513), dict(step=2 ** 30, max_steps=1)]
    good_l = dict(common, dx=0.0, dy=0.0, dz=-0.25, max_steps=15, cuboids=cub, n=2, ilayer=ibuf, offsets=fbuf)
    bad_l = pair + side + wide + [dict(ilayer=None), dict(offsets=None), dict(dx=math.nan), dict(dy=math.inf), dict(dz=-math.inf),
                                  dict(max_steps=nat.LAYER_MAX_STEPS + 1), dict(n=-1), dict(n=nat.AUDIT_MAX_CUBOIDS + 1), dict(cuboids=None)]
    eng._bind_stream()

    def head(ctx, a):
        return (ctx, _p(a["coeffs"]), _p(a["seg_rows"]), _p(a["seg_offsets"]), a["B"], a["m"], a["dt"], _p(a["go"]), a["G"], _p(a["t_coeffs"]),
                _p(a["t_seg_rows"]), _p(a["t_seg_offsets"]), a["Bt"], a["mt"], _p(a["tgo"]), _p(a["tstart"]))

    def call_a(ctx, a):
        return nat.lib().uavac_minsnap_separation_against_dev(*head(ctx, a), _p(a["start"]), a["radius"], _p(a["sep"]), _p(a["isep"]))

    def call_s(ctx, a):
        return nat.lib().uavac_minsnap_stagger_against_dev(*head(ctx, a), a["cap"], _p(a["start"]), a["radius"], a["step"], a["max_steps"],
                                                          _p(a["istag"]))

    def call_l(ctx, a):
        return nat.lib().uavac_minsnap_layer_against_dev(*head(ctx, a), a["cap"], _p(a["start"]), a["radius"], a["dx"], a["dy"], a["dz"],
                                                        a["max_steps"], _p(a["cuboids"]), a["n"], _p(a["ilayer"]), _p(a["offsets"]))
    for call, good, bad in ((call_a, good_a, bad_a), (call_s, good_s, bad_s), (call_l, good_l, bad_l)):
        for change in bad:
            rc = call(eng.ctx._h, {**good, **change})
            assert rc == nat.EINVAL, (change, rc)
            assert (nat.lib().uavac_last_error(eng.ctx._h) or b"") != b"", change
        assert call(None, good) == nat.EINVAL                                        # no context
    torch.cuda.synchronize()
    assert bool((ibuf == SENT_I).all()) and bool((fbuf == SENT_F).all())
    # the same calls with nothing wrong go through, with groups and with one group on each side
    for call, good, rows in ((call_a, good_a, 5), (call_s, good_s, 3), (call_l, good_l, 4)):
        assert call(eng.ctx._h, good) == nat.OK and call(eng.ctx._h, {**good, "go": None, "tgo": None, "G": -1, "cap": B}) == nat.OK
        torch.cuda.synchronize()
        assert not bool((ibuf[:rows * B] == SENT_I).any())
    # the engine refuses on the host what the host can see
    other_dt = case(eng, N_ALL, 0.04)["free"]
    for call in (lambda: eng.stagger(plan, RADIUS, traffic=other_dt), lambda: eng.layer(plan, RADIUS, traffic=other_dt),
                 lambda: eng.separation_against(plan, other_dt, RADIUS), lambda: eng.deconflict(plan, RADIUS, traffic=other_dt),
                 lambda: eng.stagger(plan, RADIUS, traffic=traffic, airspaces=True), lambda: eng.layer(plan, RADIUS, traffic=traffic, airspaces=True),
                 lambda: eng.deconflict(plan, RADIUS, traffic=traffic, airspaces=True),
                 lambda: eng.stagger(plan, RADIUS, groups=GO3, traffic=traffic), lambda: eng.stagger(plan, RADIUS, traffic=traffic, traffic_groups=TGO3),
                 lambda: eng.layer(plan, RADIUS, groups=GO3, traffic=traffic, traffic_groups=[0, 35, 70]),
                 lambda: eng.separation_against(plan, traffic, RADIUS, groups=GO3),
                 lambda: eng.stagger(plan, RADIUS, groups=GO3, traffic=traffic, traffic_groups=TGO3, group_cap=64),
                 lambda: eng.stagger(plan, RADIUS, traffic=traffic, traffic_start_rows=np.zeros(3))):
        with pytest.raises(ValueError):
            call()
    assert eng.take_flags() == [0, 0, 0, 0]
