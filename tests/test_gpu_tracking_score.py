"""Per-UAV tracking scores accumulated inside the fused rollout (include/uavac.h uavac_control_rollout_scored_dev and its plan-fed
twins; uav_ac.scoring), in every kernel form: against the C oracle's flight and rows through a numpy statement of the rule, against
the kernel's own state log and rows, scored against unscored launches of the same flight, split launches against one, upstream's
acceptance test on the lab mission, and a full-size 65 536-UAV scored flight without a log.

The rule (numpy_scores below): a period is the F ticks from an outer update at row r (the cursor) to the end of its F-th tick;
e = |position - row r's xyz| then; scored only if r >= next_row: count += 1, next_row = r + 1, sum += e, sumsq += e*e,
max = max(max, e), last = e."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import col_err, load_golden

pytestmark = pytest.mark.gpu

VEL, DT, B0, M0 = 3.0, 0.01, 4096, 8
TOL, SELF_TOL = 1e-5, 1e-13
CHUNK = 1037                  # log chunks: not a multiple of F, so chunks end inside periods and the carry (rows 6-10) is used


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    e = Engine("cuda:0")
    yield e
    e.ctx.set_option("coeff_dma", -1)


@pytest.fixture(scope="module")
def pool():
    ex = ThreadPoolExecutor(max_workers=3)
    yield ex
    ex.shutdown(wait=True)


def numpy_scores(pos_end, rows_read, targets, drop=()):
    """pos_end (P, 3, B) positions at the ends of the periods 0 .. P-1 of a flight from a fresh start; rows_read (P, B) the row
    each period's outer update read; targets (P, 3, B) that row's xyz.  Periods in `drop` are not scored (dropped).
    -> (6, B): count, next_row, sum, sumsq, max, last -- one period after another, left to right."""
    P, _, B = pos_end.shape
    count, nxt, s, ss, mx, last = (np.zeros(B) for _ in range(6))
    for p in range(P):
        if p in drop:
            continue
        d = pos_end[p] - targets[p]
        e = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        r = rows_read[p]
        sc = r >= nxt
        count = np.where(sc, count + 1.0, count)
        nxt = np.where(sc, r + 1.0, nxt)
        s = np.where(sc, s + e, s)
        ss = np.where(sc, ss + e * e, ss)
        mx = np.where(sc, np.where(e > mx, e, mx), mx)
        last = np.where(sc, e, last)
    return np.stack([count, nxt, s, ss, mx, last])


def period_rows(rows, ro, P):
    """rows (N, >=3) of missions at offsets ro (B+1,), flown from row 0: period p reads row min(p, N_b - 1).
    -> rows_read (P, B), targets (P, 3, B)."""
    n = np.diff(ro)
    p = np.arange(P)[:, None]
    r = np.minimum(p, n[None, :] - 1)
    tg = rows[ro[:-1][None, :] + r][:, :, 0:3]                       # (P, B, 3)
    return r.astype(np.float64), np.ascontiguousarray(tg.transpose(0, 2, 1))


def _check_scores(case, got, exp, tol):
    """got (11, B) tensor / array against exp (6, B): count and next_row exact; sum, sumsq, max, last within tol."""
    g = got[:6].cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)[:6]
    bad = np.flatnonzero((g[0] != exp[0]) | (g[1] != exp[1]))
    assert len(bad) == 0, f"{case}: count / next_row differ on {len(bad)} UAVs, first {bad[:6].tolist()}: {g[:2, bad[:3]]} vs {exp[:2, bad[:3]]}"
    for i, name in ((2, "sum"), (3, "sumsq"), (4, "max"), (5, "last")):
        if tol >= 1e-6:
            e = col_err(g[i][:, None], exp[i][:, None])
        else:
            e = float(np.max(np.abs(g[i] - exp[i]) / np.maximum(np.abs(exp[i]), 1e-300)))
        assert e <= tol, f"{case}: {name} off by {e:.3e}"


# ------------------------------------------------------------------------------------------------- the 4 096-mission batch
@pytest.fixture(scope="module")
def batch(eng, pool):
    """Missions, K, the oracle's rows and three oracle flights (free, ground vehicle, lab obstacles) at the ends of the periods."""
    import bench
    from uav_ac import _native as nat
    from oracle import c_oracle as cc
    wps = bench.missions(B0, M0, 0, B0)
    F = nat.Vehicle.default().inner_per_outer
    pl = cc.plan_threads(wps, VEL, DT)
    ro = pl["row_offsets"]
    P = int(np.diff(ro).max()) + 30
    K = P * F
    aabbs = load_golden("fixed_missions.npz")["lab_aabbs"]
    Vg = cc.Vehicle.default()
    Vg.ground = 1
    sel = list(range(F - 1, K, F))
    futs = {"free": pool.submit(cc.fleet, wps, VEL, DT, K, sel),
            "ground": pool.submit(cc.fleet, wps, VEL, DT, K, sel, (), None, None, Vg),
            "obstacles": pool.submit(cc.fleet, wps, VEL, DT, K, sel, (), aabbs)}
    rows_read, targets = period_rows(pl["rows"], ro, P)

    def oracle(kind):
        ref = futs[kind].result()
        return {"pos": np.ascontiguousarray(ref["sel_log"][:, 0:3, :]), "istate": ref["istate"]}
    return {"wps": wps, "F": F, "P": P, "K": K, "ro": ro, "rows_read": rows_read, "targets": targets, "aabbs": aabbs,
            "oracle": oracle}


FORMS = ["rows", "plan_column", "scan_dma0", "scan_dma1", "scan_dma2", "ragged", "ground", "obstacles"]


def _make_fleet(eng, batch, form):
    from uav_ac import _native as nat
    wps = batch["wps"]
    V = None
    if form == "ground":
        V = nat.Vehicle.default()
        V.ground = 1
    if form == "rows":
        return eng.fleet(eng.plan(wps, VEL, DT), from_plan=False)
    if form == "plan_column":
        return eng.fleet(eng.plan(wps, VEL, DT, dense_yaw=True), from_plan=True, yaw_from="column")
    if form == "ragged":
        return eng.fleet(eng.plan_ragged(list(wps), VEL, DT), from_plan=True)
    return eng.fleet(eng.plan(wps, VEL, DT), vehicle=V, from_plan=True)


def _fly_pair(eng, batch, form, log):
    """The form's flight twice, scored and unscored, launch for launch: one launch without a log, CHUNK-tick launches into a log
    with one.  Asserts state, istate and every log chunk equal between the two (no interference).  -> (scored fleet, positions
    at the ends of the periods from the log or None, kernel names)."""
    import torch
    K, F = batch["K"], batch["F"]
    dma = int(form[-1]) if form.startswith("scan_dma") else -1
    eng.ctx.set_option("coeff_dma", dma)
    ab = batch["aabbs"] if form == "obstacles" else None
    try:
        fa, fb = _make_fleet(eng, batch, form), _make_fleet(eng, batch, form)
        launches = [CHUNK] * (K // CHUNK) + ([K % CHUNK] if K % CHUNK else []) if log else [K]
        ends, t0, names = [], 0, set()
        for k in launches:
            sa, _ = fa.rollout(k, state_log=True if log else None, aabbs=ab, score=True)
            names.add(eng.ctx.last_rollout_kernel())
            sb, _ = fb.rollout(k, state_log=True if log else None, aabbs=ab)
            if log:
                assert torch.equal(sa, sb), f"{form}: the scored launch changed the state log"
                idx = [t - t0 for t in range(t0, t0 + k) if (t + 1) % F == 0]
                ends.append(sa[torch.as_tensor(idx, dtype=torch.int64, device=sa.device), 0:3].cpu().numpy())
            t0 += k
        assert torch.equal(fa.state, fb.state) and torch.equal(fa.istate, fb.istate), f"{form}: scoring changed the flight"
    finally:
        eng.ctx.set_option("coeff_dma", -1)
    pos = np.ascontiguousarray(np.concatenate(ends)) if log else None
    return fa, pos, names


@pytest.mark.parametrize("log", [False, True], ids=["nolog", "log"])
@pytest.mark.parametrize("form", FORMS)
def test_scores_match_oracle_and_own_log(eng, batch, form, log):
    """1 oracle parity, 2 HIP self-consistency (with a log), 3 no interference -- in every kernel form."""
    fleet, pos, names = _fly_pair(eng, batch, form, log)
    assert all(n.startswith("scored_control_rollout_kernel<") for n in names), names
    if form.startswith("scan_dma") and log:
        assert any(n.endswith(f", {form[-1]}>") for n in names), (form, names)
    kind = form if form in ("ground", "obstacles") else "free"
    ref = batch["oracle"](kind)
    exp = numpy_scores(ref["pos"], batch["rows_read"], batch["targets"])
    assert np.array_equal(exp[0], np.diff(batch["ro"]))                 # every mission completed (rows 0 .. N-1 once each)
    _check_scores(f"{form}/{'log' if log else 'nolog'} vs oracle", fleet.score, exp, TOL)
    assert np.array_equal(fleet.istate.T.cpu().numpy(), ref["istate"]), f"{form}: istate differs from the oracle"
    if log:
        p = fleet.plan
        rows = (p.traj if getattr(p, "traj", None) is not None else eng.sample_rows(p)).cpu().numpy()
        rr, tg = period_rows(rows, p.row_offsets.cpu().numpy(), batch["P"])
        own = numpy_scores(pos, rr, tg)
        _check_scores(f"{form} vs its own log", fleet.score, own, SELF_TOL)
    t = fleet.tracking()
    assert bool(t["complete"].all())


def test_split_invariance_and_dropped_period(eng, batch):
    """4: [7, 13, 5F + 3, rest] gives the score bits of one launch; an unscored 4-tick launch inside a period drops that period."""
    import torch
    K, F = batch["K"], batch["F"]
    one = _make_fleet(eng, batch, "scan_dma1")
    one.rollout(K, score=True)
    split = _make_fleet(eng, batch, "scan_dma1")
    for k in (7, 13, 5 * F + 3, K - 7 - 13 - 5 * F - 3):
        split.rollout(k, score=True)
    assert torch.equal(one.score, split.score)
    assert torch.equal(one.state, split.state)
    # row-fed and logged as well (another kernel, other carry sites)
    a, b = _make_fleet(eng, batch, "rows"), _make_fleet(eng, batch, "rows")
    a.rollout(K, score=True)
    for k in (7, 13, 5 * F + 3, K - 7 - 13 - 5 * F - 3):
        b.rollout(k, state_log=True, score=True)
    assert torch.equal(a.score, b.score)
    # an unscored launch of ticks 13 .. 16 (inside period 1, ticks 10 .. 19): period 1 is dropped, nothing else
    d = _make_fleet(eng, batch, "scan_dma1")
    d.rollout(13, score=True)
    d.rollout(4)
    slog, _ = d.rollout(K - 17, state_log=True, score=True)
    exp_one = one.score[:6].cpu().numpy()
    got = d.score[:6].cpu().numpy()
    assert np.array_equal(got[0], exp_one[0] - 1) and np.array_equal(got[1], exp_one[1])
    # the rest still follows the rule: positions at the ends of periods 0, 2, 3, ... from the one-launch twin's state log
    full = _make_fleet(eng, batch, "scan_dma1")
    ends = []
    for t0 in range(0, K, CHUNK):
        k = min(CHUNK, K - t0)
        s, _ = full.rollout(k, state_log=True)
        idx = [t - t0 for t in range(t0, t0 + k) if (t + 1) % F == 0]
        ends.append(s[torch.as_tensor(idx, dtype=torch.int64, device=s.device), 0:3].cpu().numpy())
    pos = np.concatenate(ends)
    p = d.plan
    rr, tg = period_rows(eng.sample_rows(p).cpu().numpy() if getattr(p, "traj", None) is None else p.traj.cpu().numpy(),
                         p.row_offsets.cpu().numpy(), batch["P"])
    _check_scores("dropped period", d.score, numpy_scores(pos, rr, tg, drop={1}), SELF_TOL)
    # reset() and reset_score() start afresh
    d.reset()
    assert not bool(d.score.any())


def test_lab_mission_meets_upstream_acceptance(eng):
    """5: the lab scene's mission (takeoff + course around its obstacles, v = 2.0, F = 10, ground on) as a one-UAV scored flight:
    complete, mean error < 0.5, final error < 0.5, no collision; mean error = the numpy mean over a state log to 1e-12."""
    import torch
    from uav_ac import _native as nat
    from uav_ac.main import _generate_mission_trajectory
    from uav_ac.scoring import acceptance, summarize
    from uav_ac.simulation.mujoco_sim import DEFAULT_SCENE_PATH, MujocoSimulation
    F, v = 10, 2.0
    sim = MujocoSimulation(DEFAULT_SCENE_PATH)
    dt_traj = sim.quad.dt * F
    traj = _generate_mission_trajectory(sim.mission_waypoints, sim.obstacles, v, dt_traj)
    N = len(traj)
    K = N * F + 2000
    V = sim.vehicle(dt_outer=dt_traj)
    V.inner_per_outer = F
    dev = eng.device
    rows = torch.as_tensor(traj, dtype=torch.float64, device=dev).contiguous()
    offs = torch.tensor([0, N], dtype=torch.int64, device=dev)
    aabbs = torch.as_tensor(sim.obstacles, dtype=torch.float64, device=dev).contiguous()
    P = lambda t: C.c_void_p(0 if t is None else t.data_ptr())      # noqa: E731
    out = {}
    for log in (False, True):
        state = torch.zeros((nat.STATE_ROWS, 1), dtype=torch.float64, device=dev)
        state[0:13, 0] = torch.as_tensor(sim.quad.X)
        istate = torch.zeros((nat.ISTATE_ROWS, 1), dtype=torch.int32, device=dev)
        score = torch.zeros((nat.SCORE_ROWS, 1), dtype=torch.float64, device=dev)
        slog = torch.empty((K, 13, 1), dtype=torch.float64, device=dev) if log else None
        eng._bind_stream()
        eng.ctx.call("uavac_control_rollout_scored_dev", C.byref(V), P(rows), P(offs), P(state), P(istate), 1, K, P(slog), None,
                     P(aabbs), int(aabbs.shape[0]), P(score))
        torch.cuda.synchronize()
        out[log] = (score.clone(), istate.clone(), slog)
    assert torch.equal(out[False][0], out[True][0]) and torch.equal(out[False][1], out[True][1])
    score, istate, slog = out[True]
    s = summarize(score, istate, torch.tensor([N], device=dev))
    assert bool(s["complete"][0]) and int(s["rows_scored"][0]) == N
    a = acceptance(s)
    assert bool(a["mean_ok"][0]) and bool(a["final_ok"][0]) and bool(a["no_collision"][0]), {k: float(x[0]) for k, x in s.items()}
    states = slog[:, :, 0].cpu().numpy()
    err = np.linalg.norm(states[F - 1:N * F:F, 0:3] - traj[:N, 0:3], axis=1)
    assert abs(float(s["mean_error"][0]) - float(err.mean())) <= 1e-12
    assert abs(float(s["final_error"][0]) - float(err[-1])) <= 1e-12


def _xcd(block, n):                          # uavac_internal.h xcd_contiguous
    x, q, r = block & 7, n >> 3, n & 7
    return x * q + min(x, r) + (block >> 3)


def _chosen_lanes(B, grid, seed):
    n_tiles = -(-B // 64)
    tiles = {0, 1, n_tiles - 2, n_tiles - 1}
    for t0 in range(0, n_tiles, grid):
        n_here = min(grid, n_tiles - t0)
        tiles |= {t0, t0 + _xcd(n_here - 1, n_here)}
    lanes = {t * 64 + j for t in tiles if t >= 0 for j in range(64)}
    lanes |= set(np.random.default_rng(seed).integers(0, B, 128).tolist())
    return np.array(sorted(b for b in lanes if 0 <= b < B), dtype=np.int64)


def test_full_size_scored_flight(eng, pool):
    """6: 65 536 UAVs x 10 000 ticks, scored, no log: spot lanes against the oracle; the scored kernel within 256 VGPRs."""
    import bench
    import torch
    from oracle import c_oracle as cc
    B, K = 65536, 10000
    wps = bench.missions(B, M0, 0, B)
    lanes = _chosen_lanes(B, -(-B // 64), seed=6)
    F = 10
    fut = pool.submit(cc.fleet, wps[lanes], VEL, DT, K, list(range(F - 1, K, F)))
    plan = eng.plan(wps, VEL, DT, rows=False)
    fleet = eng.fleet(plan)
    fleet.rollout(K, score=True)
    torch.cuda.synchronize()
    assert eng.ctx.last_rollout_kernel().startswith("scored_control_rollout_kernel<")
    assert 0 < eng.ctx.last_rollout_vgprs() <= 256
    ref = fut.result()
    pl = cc.plan_threads(wps[lanes], VEL, DT)
    P = K // F
    rr, tg = period_rows(pl["rows"], pl["row_offsets"], P)
    exp = numpy_scores(np.ascontiguousarray(ref["sel_log"][:, 0:3, :]), rr, tg)
    got = fleet.score[:, torch.as_tensor(lanes, device=fleet.score.device)]
    _check_scores("65 536 x 10 000", got, exp, TOL)


def test_refusals(eng):
    """7: a NULL score, and a score with a command log, are refused (UAVAC_EINVAL; ValueError in Python)."""
    import torch
    from uav_ac import _native as nat
    from oracle import minsnap_oracle as mo
    plan = eng.plan(mo.synthetic_missions(64, 4), VEL, DT)
    fleet = eng.fleet(plan, from_plan=False)
    with pytest.raises(ValueError):
        fleet.rollout(10, cmd_log=True, score=True)
    P = lambda t: C.c_void_p(0 if t is None else t.data_ptr())      # noqa: E731
    V = nat.Vehicle.default()
    score = torch.zeros((nat.SCORE_ROWS, 64), dtype=torch.float64, device=eng.device)
    clog = torch.empty((10, nat.CMD_COLS, 64), dtype=torch.float64, device=eng.device)
    base = (C.byref(V), P(plan.traj), P(plan.row_offsets), P(fleet.state), P(fleet.istate), 64, 10, None)
    for cmd, sc in ((None, None), (clog, score)):
        with pytest.raises(nat.UavacError) as ei:
            eng.ctx.call("uavac_control_rollout_scored_dev", *base, P(cmd), None, 0, P(sc))
        assert ei.value.code == nat.EINVAL
        with pytest.raises(nat.UavacError) as ei:
            eng.ctx.call("uavac_control_rollout_plan_scored_dev", C.byref(V), P(plan.coeffs), P(plan.seg_rows), P(plan.row_offsets),
                         None, P(plan.first_yaw), plan.m, DT, P(fleet.state), P(fleet.istate), 64, 10, None, P(cmd), None, 0, P(sc))
        assert ei.value.code == nat.EINVAL
