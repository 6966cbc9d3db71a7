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
