"""Pin the C oracle (oracle/uavac_oracle.c; the timed CPU baseline) to the reference's golden vectors."""
import numpy as np
import pytest

from conftest import col_err, load_golden
from oracle import c_oracle as cc

TOL = 1e-5


@pytest.mark.parametrize("m", [1, 2, 8, 12, 20])
def test_c_planner_matches_reference_golden(m):
    g = load_golden("synthetic_missions.npz")
    wps = g[f"m{m}_wp"]
    sub = []
    for i, wp in enumerate(wps):
        traj, coeffs, times = cc.plan(wp, 3.0, 0.01)
        assert np.array_equal(times, g[f"m{m}_times"][i])          # bit for bit (FMA dot product of np.linalg.norm)
        assert np.array_equal(np.bincount(traj[:, 10].astype(int), minlength=m), g[f"m{m}_rows_per_segment"][i])
        assert col_err(coeffs, g[f"m{m}_coeffs_solve"][i]) < 1e-9
        assert col_err(coeffs, g[f"m{m}_coeffs_lstsq"][i]) < TOL
        sub.append(traj[::16])
        if f"m{m}_traj{i}" in g:
            assert col_err(traj, g[f"m{m}_traj{i}"]) < TOL
    assert col_err(np.vstack(sub), g[f"m{m}_traj_every16"]) < TOL


def test_c_planner_config1_and_yaw():
    g = load_golden("fixed_missions.npz")
    traj, coeffs, _ = cc.plan(g["config1_wp"], 3.0, 0.01)
    assert traj.shape == (687, 11)
    assert col_err(traj, g["config1_traj"]) < TOL
    t0, _, _ = cc.plan(g["lab_wp"][:2], 3.0, 0.01)
    t1, _, _ = cc.plan(g["lab_wp"][1:], 3.0, 0.01)
    assert col_err(np.vstack((t0, t1)), g["lab_traj_free"]) < TOL


@pytest.mark.parametrize("name, K", [("config1", 8000), ("lab_v2", 17000)])
def test_c_closed_loop_matches_reference_golden(name, K):
    g = load_golden("closed_loop.npz")
    traj = g[name + "_traj"]
    state, istate = cc.initial_state(traj[0, 0:3])
    slog, clog = cc.rollout(traj, state, istate, K)
    assert col_err(slog[:200], g[name + "_state_first200"]) < 1e-10
    assert col_err(clog[:200], g[name + "_cmd_first200"]) < 1e-10
    assert col_err(slog[9::10], g[name + "_state_every10"]) < TOL
    assert col_err(clog[9::10], g[name + "_cmd_every10"]) < TOL
    assert istate[0] == len(traj) - 1 and istate[1] == K


def test_c_and_python_oracles_agree_with_aabb_flag():
    from oracle import control_oracle as co
    from oracle import minsnap_oracle as mo
    aabbs = load_golden("fixed_missions.npz")["lab_aabbs"]
    wp = mo.synthetic_missions(4, 8)[3]
    traj = mo.plan(wp, 3.0, 0.01, method="solve")
    tc, _, _ = cc.plan(wp, 3.0, 0.01)
    assert col_err(tc, traj) < 1e-9
    u = co.UAV(co.Vehicle(), position=traj[0, 0:3])
    s_py, c_py = co.rollout(u, traj, 1500, aabbs=aabbs)
    state, istate = cc.initial_state(traj[0, 0:3])
    s_c, c_c = cc.rollout(traj, state, istate, 1500, aabbs=aabbs)
    assert col_err(s_c, s_py) < 1e-9 and col_err(c_c, c_py) < 1e-9
    assert istate[2] == u.collided and istate[0] == u.traj_index


def test_cpu_baseline_leg_runs_bounded():
    from oracle import cpu_baseline as cb
    r = cb.run(segments=8, ticks=500, velocity=3.0, dt=0.01, budget_s=1.0, max_missions=3)
    assert r["kind"] == "port" and r["cores"] == 1 and r["value"] > 0 and r["unit"] == "UAV control-steps/s"


@pytest.mark.parametrize("with_boxes", [False, True])
def test_fleet_threads_equals_lane_by_lane_oracle(with_boxes):
    """oracle_fleet_threads (the whole-batch reference of tests/test_gpu_whole_batch_parity.py) is oracle_solve + oracle_sample +
    oracle_rollout lane by lane, bit for bit, whatever the thread count -- B = 37 is a multiple of none of them."""
    from oracle import minsnap_oracle as mo
    B, m, K = 37, 3, 437
    wps = mo.synthetic_missions(B, m)
    aabbs = load_golden("fixed_missions.npz")["lab_aabbs"] if with_boxes else None
    sel, lanes = [0, 1, 10, 200, K - 1], [0, 5, 36]
    state = np.empty((B, 26)); istate = np.empty((B, 4), np.int32); slog = np.empty((K, 13, B)); clog = np.empty((K, 12, B))
    seg_rows = np.empty((B, m), np.int32); coeffs = np.empty((B, 8 * m, 3)); fy = np.empty(B)
    for b in range(B):
        traj, coeffs[b], _ = cc.plan(wps[b], 3.0, 0.01)
        seg_rows[b] = np.bincount(traj[:, 10].astype(int), minlength=m)
        fy[b] = traj[0, 9]
        s, i = cc.initial_state(wps[b, 0])
        sl, cl = cc.rollout(traj, s, i, K, aabbs=aabbs)
        state[b], istate[b], slog[:, :, b], clog[:, :, b] = s, i, sl, cl
    if with_boxes:
        assert 0 < istate[:, 2].sum() < B, "the boxes should stop some missions and not others"
    for n_threads in (1, 3, 16):
        got = cc.fleet(wps, 3.0, 0.01, K, sel_ticks=sel, log_lanes=lanes, aabbs=aabbs, n_threads=n_threads, cmd=True)
        assert np.array_equal(got["state"], state) and np.array_equal(got["istate"], istate)
        assert np.array_equal(got["seg_rows"], seg_rows) and np.array_equal(got["coeffs"], coeffs)
        assert np.array_equal(got["first_yaw"], fy)
        assert np.array_equal(got["sel_log"], slog[sel]) and np.array_equal(got["sel_cmd"], clog[sel])
        assert np.array_equal(got["lane_log"], slog[:, :, lanes].transpose(2, 0, 1))
    with pytest.raises(RuntimeError):
        cc.fleet(wps, 3.0, 0.01, K, sel_ticks=[K])                 # a tick the flight never reaches
    assert 1 <= cc.default_threads() <= 16


# ------------------------------------------------------------------ whole-batch plan reference (oracle_plan_threads)
def _per_mission(missions, velocity, dt, cuboid=None):
    """oracle_solve + oracle_sample mission by mission: (times, seg_rows, coeffs, rows, first_yaw, hit) each concatenated."""
    out = {k: [] for k in ("times", "seg_rows", "coeffs", "rows", "first_yaw", "hit")}
    for wp in missions:
        traj, coeffs, times = cc.plan(wp, velocity, dt)
        m = len(times)
        out["times"].append(times)
        out["seg_rows"].append(np.bincount(traj[:, 10].astype(int), minlength=m).astype(np.int32))
        out["coeffs"].append(coeffs.reshape(m, 8, 3))
        out["rows"].append(traj)
        out["first_yaw"].append(traj[0, 9] if len(traj) else 0.0)
        if cuboid is not None:
            c = cuboid
            inside = ((traj[:, 0] >= c[0]) & (traj[:, 0] <= c[1]) & (traj[:, 1] >= c[2]) & (traj[:, 1] <= c[3]) &
                      (traj[:, 2] >= c[4]) & (traj[:, 2] <= c[5]))
            h = np.zeros(m, np.int32)
            h[traj[inside, 10].astype(int)] = 1
            out["hit"].append(h)
    return {k: (np.concatenate(v) if k != "first_yaw" else np.array(v)) for k, v in out.items() if len(v)}


def _ragged(B, m, seed):
    from oracle import minsnap_oracle as mo
    rng = np.random.default_rng(seed)
    missions = [w[:int(rng.integers(2, m + 2))] for w in mo.synthetic_missions(B, m)]
    so = np.zeros(B + 1, np.int64)
    np.cumsum([len(w) - 1 for w in missions], out=so[1:])
    return missions, so, np.concatenate(missions)


@pytest.mark.parametrize("ragged", [False, True])
def test_plan_threads_equals_mission_by_mission_oracle(ragged):
    """oracle_plan_threads (the plan reference of tests/test_gpu_plan_whole_batch_parity.py) is oracle_solve + oracle_sample
    mission by mission, bit for bit: any thread count, any cut of the batch into ranges, uniform and ragged."""
    from oracle import minsnap_oracle as mo
    B, m, V, DT = 41, 5, 3.0, 0.02
    cub = np.array([5.0, 14.0, 2.0, 9.0, -4.0, -2.5])
    if ragged:
        missions, so, flat = _ragged(B, m, 3)
    else:
        flat = mo.synthetic_missions(B, m)
        missions, so = list(flat), None
    for b0, b1 in ((0, B), (0, 1), (17, 18), (3, 29), (40, 41), (7, 7)):
        want = _per_mission(missions[b0:b1], V, DT, cub)
        for n_threads in (1, 3, 16):
            got = cc.plan_threads(flat, V, DT, b0, b1, seg_offsets=so, cuboid=cub, n_threads=n_threads)
            assert got["row_offsets"][0] == 0 and got["row_offsets"][-1] == len(got["rows"])
            if b1 == b0:
                assert len(got["rows"]) == 0 and len(got["coeffs"]) == 0
                continue
            assert np.array_equal(got["times"].reshape(-1), want["times"])
            assert np.array_equal(got["seg_rows"].reshape(-1), want["seg_rows"])
            assert np.array_equal(np.diff(got["row_offsets"]), [len(cc.plan(w, V, DT)[0]) for w in missions[b0:b1]])
            assert np.array_equal(got["coeffs"].reshape(-1, 8, 3), want["coeffs"])
            assert np.array_equal(got["rows"], want["rows"])
            assert np.array_equal(got["first_yaw"], want["first_yaw"])
            assert np.array_equal(got["hit"].reshape(-1), want["hit"])
    hit = _per_mission(missions, V, DT, cub)["hit"]
    assert 0 < hit.sum() < hit.size                               # (the cuboid cuts some splines and not others)
    with pytest.raises(ValueError):
        cc.plan_threads(flat, V, DT, 5, 4, seg_offsets=so)        # a range the wrong way round
    assert cc.lib().oracle_plan_threads(cc._p(np.ascontiguousarray(flat)), cc._p(so), B, m, 5, 4, V, DT, None, 1,
                                        *[None] * 5, 0, *[None] * 4) == -3


def test_plan_threads_refuses_a_short_row_buffer():
    from oracle import minsnap_oracle as mo
    wps = mo.synthetic_missions(6, 3)
    n = cc.plan_threads(wps, 3.0, 0.01, rows=False)["row_offsets"][-1]
    buf = np.full((n + 4, 11), -7.0)
    cc.plan_threads(wps, 3.0, 0.01, out_rows=buf)
    assert (buf[n:] == -7.0).all()
    with pytest.raises(ValueError):
        cc.plan_threads(wps, 3.0, 0.01, out_rows=buf[: n - 1])
    short = np.ascontiguousarray(buf[: n - 1])
    rc = cc.lib().oracle_plan_threads(cc._p(wps), None, 6, 3, 0, 6, 3.0, 0.01, None, 2, None, None, None, None, cc._p(short),
                                      n - 1, None, None, None, None)
    assert rc == -4


def test_plan_threads_jerk_and_snap():
    """Jerk and snap of the whole-batch reference: the reference's goldens (derivatives.npz) and basis_row(3 | 4, t) @ coeffs."""
    from oracle import minsnap_oracle as mo
    g = load_golden("derivatives.npz")
    for key in ("config1", "m12_0", "m12_1", "m12_2"):
        got = cc.plan_threads(g[key + "_wp"][None], 3.0, 0.01, derivs=True, n_threads=3)
        assert col_err(got["coeffs"][0], g[key + "_coeffs"]) < 1e-9
        assert col_err(got["jerk"], g[key + "_jerk"]) < TOL and col_err(got["snap"], g[key + "_snap"]) < TOL
    wps = mo.synthetic_missions(5, 4)
    got = cc.plan_threads(wps, 3.0, 0.02, derivs=True, n_threads=2)
    ro = got["row_offsets"]
    for b in range(5):
        coeffs, times = got["coeffs"][b], got["times"][b]
        j, s = [], []
        for seg, T in enumerate(times):
            c = coeffs[8 * seg:8 * seg + 8]
            for t in np.arange(0.0, T, 0.02):
                j.append(mo.basis_row(3, t) @ c)
                s.append(mo.basis_row(4, t) @ c)
        assert col_err(got["jerk"][ro[b]:ro[b + 1]], np.array(j)) < 1e-12
        assert col_err(got["snap"][ro[b]:ro[b + 1]], np.array(s)) < 1e-12


def test_plan_threads_hits_match_the_numpy_cuboid_test():
    """Per-spline hit flags: a row of the spline inside the cuboid, bounds inclusive -- minsnap_oracle.in_cuboid on the rows of
    minsnap_oracle.plan (the NumPy restatement), ragged batch, a cuboid with a face exactly on sampled coordinates."""
    from oracle import minsnap_oracle as mo
    missions, so, flat = _ragged(23, 6, 5)
    got = cc.plan_threads(flat, 3.0, 0.01, seg_offsets=so, cuboid=[6.0, 15.0, 1.0, 8.0, -3.5, -3.0])
    want = []
    for w in missions:
        traj = mo.plan(w, 3.0, 0.01, method="solve")
        cub = np.array([6.0, 15.0, 1.0, 8.0, -3.5, -3.0])
        h = np.zeros(len(w) - 1, np.int32)
        for p in traj:
            if mo.in_cuboid(p[0], p[1], p[2], cub):
                h[int(p[10])] = 1
        want.append(h)
    want = np.concatenate(want)
    assert 0 < want.sum() < len(want)
    assert np.array_equal(got["hit"], want)
    # bounds are inclusive: a cuboid of zero thickness through the first row's exact z holds it; one ulp either side does not
    x, y, z = got["rows"][0, :3]
    for zz, want_hit in ((z, 1), (np.nextafter(z, -np.inf), 0), (np.nextafter(z, np.inf), 0)):
        one = cc.plan_threads(flat, 3.0, 0.01, 0, 1, seg_offsets=so, cuboid=[x - 1e-3, x + 1e-3, y - 1e-3, y + 1e-3, zz, zz])
        assert one["hit"][0] == want_hit, (zz, z)


# ------------------------------------------------------------------ long double solve (oracle_solve_ld)
def _mp_solve(wp, times, dps=60):
    """oracle_solve's KKT system in mpmath at `dps` digits, from the same fp64 durations -> coeffs (8m, 3) as floats."""
    import mpmath as mp
    mp.mp.dps = dps
    m = len(times)
    nu, n = 8 * m, 8 * m + 6 * m + 2
    K = mp.zeros(n, n)
    rhs = [mp.zeros(n, 1) for _ in range(3)]

    def poly(order, t):
        row = []
        for i in range(8):
            p, d = mp.mpf(1), i
            for _ in range(order):
                p *= d
                d = max(d - 1, 0)
            row.append(p * mp.mpf(t) ** d)
        return row

    r = 0

    def seta(rr, cc_, v):
        K[nu + rr, cc_] = v
        K[cc_, nu + rr] = v
    for s in range(m):
        for i, v in enumerate(poly(0, 0.0)):
            seta(r, 8 * s + i, v)
        for j in range(3):
            rhs[j][nu + r] = mp.mpf(wp[s, j])
        r += 1
    for s in range(m):
        for i, v in enumerate(poly(0, times[s])):
            seta(r, 8 * s + i, v)
        for j in range(3):
            rhs[j][nu + r] = mp.mpf(wp[s + 1, j])
        r += 1
    for k in (1, 2, 3):
        for i, v in enumerate(poly(k, 0.0)):
            seta(r, i, v)
        r += 1
    for k in (1, 2, 3):
        for i, v in enumerate(poly(k, times[m - 1])):
            seta(r, 8 * (m - 1) + i, v)
        r += 1
    for s in range(1, m):
        for k in (1, 2, 3, 4):
            a, b = poly(k, times[s - 1]), poly(k, 0.0)
            for i in range(8):
                seta(r, 8 * (s - 1) + i, a[i])
                seta(r, 8 * s + i, -b[i])
            r += 1
    for s in range(m):
        for a in range(4, 8):
            for c in range(4, 8):
                e = a + c - 7
                K[8 * s + a, 8 * s + c] = (a * (a - 1) * (a - 2) * (a - 3)) * (c * (c - 1) * (c - 2) * (c - 3)) * mp.mpf(times[s]) ** e / e
    x = [mp.lu_solve(K, rhs[j]) for j in range(3)]
    return np.array([[float(x[j][i]) for j in range(3)] for i in range(nu)])


@pytest.mark.parametrize("m", [1, 2, 8, 12, 20])
def test_solve_ld_matches_solve_goldens(m):
    """The long double solve is within 1e-9 of the reference's `solve` goldens (fp64 LAPACK), and is not fp64 in disguise: its
    coefficients differ from oracle_solve's in the last bits on most missions."""
    g = load_golden("synthetic_missions.npz")
    differ = 0
    for i, wp in enumerate(g[f"m{m}_wp"]):
        c_ld, t_ld = cc.solve_ld(wp, 3.0)
        _, c, t = cc.plan(wp, 3.0, 0.01)
        assert np.array_equal(t_ld, t)
        assert col_err(c_ld, g[f"m{m}_coeffs_solve"][i].reshape(-1, 3)) <= 1e-9
        differ += not np.array_equal(c_ld, c)
    assert differ >= len(g[f"m{m}_wp"]) // 2
    assert cc.lib().oracle_ldbl_mant_dig() >= 64


@pytest.mark.parametrize("m", [1, 2, 4])
def test_solve_ld_is_the_more_precise_solve(m):
    """Against the same system solved at 60 digits (mpmath), the long double solve's error is at most oracle_solve's (fp64) on
    every golden mission, and at most 1e-15 in the column metric: a reference that can tell the true error of an fp64 solve.
    (The fp64 `solve` goldens themselves are no such reference: they share oracle_solve's fp64 rounding and lie 1e-13 from it.)"""
    g = load_golden("synthetic_missions.npz")
    wps = g[f"m{min(m, 2)}_wp"] if m <= 2 else g["m8_wp"][:6, :m + 1]
    e_ld_all = e_64_all = 0.0
    for wp in wps:
        c_ld, times = cc.solve_ld(wp, 3.0)
        _, c64, _ = cc.plan(wp, 3.0, 0.01)
        exact = _mp_solve(wp, times)
        e_ld, e_64 = col_err(c_ld, exact), col_err(c64, exact)
        assert e_ld <= e_64 and e_ld <= 1e-15, (e_ld, e_64)
        e_ld_all, e_64_all = max(e_ld_all, e_ld), max(e_64_all, e_64)
    assert e_64_all > 0.0                                         # (the fp64 solve does carry an error to measure)


# ------------------------------------------------------------------------------------------ one tick from arbitrary states
# (the state families, the bound and the exclusion rule of tests/test_gpu_one_tick_parity.py, on the reference side alone)
def _one_tick():
    if cc.lib().oracle_ldbl_mant_dig() < 64:
        pytest.skip("long double is no wider than double here")
    import test_gpu_one_tick_parity as otp
    return otp


def test_one_tick_families_census():
    """Every branch the one-tick families are meant to take is taken by at least 16 lanes (predicates of control_law.h restated in
    NumPy), the tie lanes are exact ties in fp64, about 4 000 lanes in all and no launch a whole number of 64-lane tiles."""
    otp = _one_tick()
    fams = [otp.build(n) for n in otp.NAMES]
    counts = otp.census(fams)
    short = {k: n for k, n in counts.items() if n < 16}
    assert not short, short
    assert len(counts) >= 70
    total = sum(f["B"] for f in fams)
    assert 3500 <= total <= 4500 and all(f["B"] % 64 for f in fams), [f["B"] for f in fams]
    for f in fams:
        assert np.isfinite(f["state"]).all() and np.isfinite(f["traj"]).all()
        nrows = np.diff(f["row_offsets"])
        assert (f["istate"][0] >= 0).all() and (f["istate"][0] < nrows).all()          # the oracle does not clamp a cursor


def test_one_tick_oracles_agree_within_the_bound():
    """oracle_rollout against oracle_rollout_ld, one tick from every lane: with the fp64 oracle in the kernel's place the bound holds
    at margin 1 (it is attainable by a correct fp64 implementation), every output of both is finite, integer outputs are equal,
    and the long-double twin is not the fp64 oracle in disguise."""
    otp = _one_tick()
    differ = 0
    for name in otp.NAMES:
        fam, ref = otp.build(name), otp.reference(name)
        keep = ~otp.excluded(name)
        for what in ("state", "slog", "clog"):
            t, r = ref[f"t_{what}"], ref[f"r_{what}"]
            assert np.isfinite(t).all() and np.isfinite(r).all(), (name, what)
            otp.assert_within_bound(what, fam, r, t, r, keep, margin=1.0)
            differ += int((t != r).any(axis=tuple(range(t.ndim - 1))).sum())
        assert np.array_equal(ref["t_istate"][:, keep], ref["r_istate"][:, keep])
        assert np.array_equal(ref["t_slog"][0], ref["t_state"][:13]) and np.array_equal(ref["t_clog"][0, 0], ref["t_state"][22])
    assert differ > 1000


def test_one_tick_exclusions_stay_under_half_a_percent():
    otp = _one_tick()
    for name in otp.NAMES:
        ex = otp.excluded(name)
        assert ex.mean() <= 0.005, (name, int(ex.sum()), [otp.build(name)["labels"][i] for i in np.flatnonzero(ex)[:8]])


def test_one_tick_numpy_restatement_tracks_the_oracle():
    """The NumPy restatement of control_law.h that computes the census (numpy_tick) is itself within 64x the bound of the long-double
    oracle on 99 % of the lanes: its branch predicates describe the tick the oracles compute."""
    otp = _one_tick()
    for name in otp.NAMES:
        fam, ref = otp.build(name), otp.reference(name)
        new, cmd, ist, _ = otp.numpy_tick(fam)
        ok = (np.abs(new - ref["t_state"]) <= otp.bound(ref["t_state"], ref["r_state"], 64 * otp.M_BOUND)).all(axis=0)
        assert ok.mean() >= 0.99, (name, ok.mean(), [fam["labels"][i] for i in np.flatnonzero(~ok)[:10]])
        assert (ist == ref["t_istate"]).all(axis=0).mean() >= 0.99
