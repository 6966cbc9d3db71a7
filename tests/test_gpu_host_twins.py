"""The host-pointer twins of the C ABI against the `_dev` entry points they stage for: `uavac_minsnap_row_counts`, `uavac_minsnap_solve`,
`uavac_minsnap_sample`, `uavac_minsnap_plan_ragged`, `uavac_minsnap_obstacle_waypoints`, `uavac_yaw_scan`, `uavac_state_init`,
`uavac_control_rollout`, `uavac_controller_tick`, `uavac_dynamics_step` on NumPy arrays, and the same inputs in torch tensors through the
device entry points.  Every comparison is of bytes.  B = 3 missions of m = 2 segments (the ragged batch: 1, 2 and 2), K = 2 ticks; every
twin runs with its optional pieces present and absent.  `uavac_yaw_scan` runs at n = 3, 20 000, 50 000 and 3 again on one ctx: 480 000
bytes in and 160 000 out are two pinned pieces and one, 1.2 MB in goes down the runtime's pageable path and 400 000 out are two pieces,
the arena grows twice and then serves a small request from the grown block.

The six RRT* twins (`uavac_rrt_star`, `uavac_rrt_segment_hits`, `uavac_rrt_edge_lengths`, `uavac_rrt_simplify`, `uavac_rrt_path_cost`,
`uavac_rrt_steer`) the same way: B = 3 problems of 40 iterations with and without a cuboid, E = 5 edges, and `uavac_rrt_edge_lengths` at the
yaw scan's four sizes on one ctx: the arena grows and then serves a small request from the grown block (this twin, one of the four called
per tree operation, copies on the caller's pointers itself, so the sizes are no thresholds of its copies)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, M, K = 3, 2, 2
VEL, DT = 2.0, 0.05
WAYPOINTS = np.array([[[0.0, 0.0, -1.0], [1.5, 0.5, -1.5], [2.5, 2.0, -1.0]],
                      [[0.5, 2.5, -2.0], [1.0, 1.0, -1.2], [2.0, 0.2, -2.2]],
                      [[3.0, 3.0, -1.0], [2.0, 2.2, -2.0], [0.4, 1.6, -1.4]]])
SEG_OFFSETS = np.array([0, 1, 3, 5], dtype=np.int64)
WP_RAGGED = np.concatenate([WAYPOINTS[0, :2], WAYPOINTS[1], WAYPOINTS[2]])
S = 5
# mission 0 of the ragged batch flies from (0, 0, -1) to (1.5, 0.5, -1.5): through this cuboid; the other two stay clear of it
CUBOID = np.array([[0.6, 0.9, 0.1, 0.4, -1.4, -1.1]])


@pytest.fixture(scope="module")
def gpu():
    import torch
    from uav_ac import _native as N
    torch.cuda.set_device(0)
    ctx = N.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    yield ctx, N, torch
    ctx.close()


def P(a):
    if a is None:
        return None
    return a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else C.c_void_p(a.data_ptr())


def same(host, dev):
    a, b = np.ascontiguousarray(host), np.ascontiguousarray(dev.cpu().numpy())
    return a.dtype == b.dtype and a.size == b.size and a.tobytes() == b.tobytes()


class Dev:
    """Zeroed torch tensors on the GPU, and NumPy arrays of the same shapes."""

    def __init__(self, torch):
        self.torch, self.dev = torch, torch.device("cuda:0")

    def f64(self, *s):
        return self.torch.zeros(s, dtype=self.torch.float64, device=self.dev)

    def i32(self, *s):
        return self.torch.zeros(s, dtype=self.torch.int32, device=self.dev)

    def i64(self, *s):
        return self.torch.zeros(s, dtype=self.torch.int64, device=self.dev)

    def up(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a)).to(self.dev)


def dev_plan(ctx, d):
    """The uniform plan through the device entry points: -> times, seg_rows, row_offsets, coeffs, traj (tensors)."""
    wp, times, seg_rows, row_offsets, coeffs = d.up(WAYPOINTS), d.f64(B, M), d.i32(B, M), d.i64(B + 1), d.f64(B, 8 * M, 3)
    ctx.call("uavac_minsnap_row_counts_dev", P(wp), B, M, VEL, DT, P(times), P(seg_rows), P(row_offsets))
    ctx.call("uavac_minsnap_solve_dev", P(wp), P(times), B, M, P(coeffs), None)
    traj = d.f64(int(row_offsets[-1]), 11)
    ctx.call("uavac_minsnap_sample_dev", P(coeffs), P(times), P(seg_rows), P(row_offsets), B, M, DT, P(traj))
    d.torch.cuda.synchronize()
    return times, seg_rows, row_offsets, coeffs, traj


def test_row_counts(gpu):
    ctx, N, torch = gpu
    times_d, seg_rows_d, row_offsets_d, _, _ = dev_plan(ctx, Dev(torch))
    times, seg_rows, row_offsets = np.zeros((B, M)), np.zeros((B, M), np.int32), np.zeros(B + 1, np.int64)
    ctx.call("uavac_minsnap_row_counts", P(WAYPOINTS), B, M, VEL, DT, P(times), P(seg_rows), P(row_offsets))
    assert same(times, times_d) and same(seg_rows, seg_rows_d) and same(row_offsets, row_offsets_d)
    only = np.zeros(B + 1, np.int64)
    ctx.call("uavac_minsnap_row_counts", P(WAYPOINTS), B, M, VEL, DT, None, None, P(only))
    assert same(only, row_offsets_d)


def dev_solve(ctx, d, wp_host):
    """`uavac_minsnap_solve` on the device: the durations at dt = 1 (they do not depend on it), then the solve."""
    wp, times, seg_rows, row_offsets, coeffs = d.up(wp_host), d.f64(B, M), d.i32(B, M), d.i64(B + 1), d.f64(B, 8 * M, 3)
    ctx.call("uavac_minsnap_row_counts_dev", P(wp), B, M, VEL, 1.0, P(times), P(seg_rows), P(row_offsets))
    ctx.call("uavac_minsnap_solve_dev", P(wp), P(times), B, M, P(coeffs), None)
    d.torch.cuda.synchronize()
    return times, coeffs


def test_solve_and_its_documented_error(gpu):
    ctx, N, torch = gpu
    d = Dev(torch)
    times_d, coeffs_d = dev_solve(ctx, d, WAYPOINTS)
    coeffs, times = np.zeros((B, 8 * M, 3)), np.zeros((B, M))
    ctx.call("uavac_minsnap_solve", P(WAYPOINTS), B, M, VEL, P(coeffs), P(times))
    assert same(coeffs, coeffs_d) and same(times, times_d)
    alone = np.zeros((B, 8 * M, 3))
    ctx.call("uavac_minsnap_solve", P(WAYPOINTS), B, M, VEL, P(alone), None)
    assert same(alone, coeffs_d)
    # a repeated waypoint: the knot system of mission 1 is singular; the call says so and its outputs are complete
    twice = WAYPOINTS.copy()
    twice[1, 1] = twice[1, 0]
    flags = (C.c_int32 * 4)()
    ctx.call("uavac_take_flags", flags)
    times_s, coeffs_s = dev_solve(ctx, d, twice)
    ctx.call("uavac_take_flags", flags)
    assert flags[1] != 0                                    # (the device entry points leave the flag; it is taken here)
    bad, bad_times = np.full((B, 8 * M, 3), 7.0), np.full((B, M), 7.0)
    rc = N.lib().uavac_minsnap_solve(ctx._h, P(twice), B, M, VEL, P(bad), P(bad_times))
    assert rc == N.ESINGULAR and N.lib().uavac_last_error(ctx._h) == b"singular knot system (repeated waypoint?)"
    assert same(bad, coeffs_s) and same(bad_times, times_s)
    assert same(bad[0], coeffs_d[0]) and same(bad[2], coeffs_d[2])
    again = np.zeros((B, 8 * M, 3))
    assert N.lib().uavac_minsnap_solve(ctx._h, P(WAYPOINTS), B, M, VEL, P(again), None) == N.OK      # the flags were cleared
    assert same(again, coeffs_d)


def test_sample(gpu):
    ctx, N, torch = gpu
    times_d, _, row_offsets_d, coeffs_d, traj_d = dev_plan(ctx, Dev(torch))
    traj = np.zeros(tuple(traj_d.shape))
    ctx.call("uavac_minsnap_sample", P(coeffs_d.cpu().numpy()), P(times_d.cpu().numpy()), B, M, DT, P(row_offsets_d.cpu().numpy()), P(traj))
    assert traj.shape[0] > 64 and same(traj, traj_d)


def test_plan_ragged(gpu):
    ctx, N, torch = gpu
    d = Dev(torch)
    wp, so, times_d, seg_rows_d, row_offsets_d, coeffs_d = d.up(WP_RAGGED), d.up(SEG_OFFSETS), d.f64(S), d.i32(S), d.i64(B + 1), d.f64(S, 8, 3)
    ctx.call("uavac_minsnap_row_counts_ragged_dev", P(wp), P(so), B, M, VEL, DT, P(times_d), P(seg_rows_d), P(row_offsets_d))
    ctx.call("uavac_minsnap_solve_ragged_dev", P(wp), P(times_d), P(so), B, M, P(coeffs_d), None)
    rows = int(row_offsets_d[-1])
    traj_d = d.f64(rows, 11)
    ctx.call("uavac_minsnap_sample_ragged_dev", P(coeffs_d), P(seg_rows_d), P(so), P(row_offsets_d), B, M, S, DT, P(traj_d), rows, None, None,
             None)
    torch.cuda.synchronize()
    times, row_offsets, coeffs, traj = np.zeros(S), np.zeros(B + 1, np.int64), np.zeros((S, 8, 3)), np.zeros((rows, 11))
    ctx.call("uavac_minsnap_plan_ragged", P(WP_RAGGED), P(SEG_OFFSETS), B, VEL, DT, P(times), P(row_offsets), P(coeffs), P(traj), rows)
    assert same(times, times_d) and same(row_offsets, row_offsets_d) and same(coeffs, coeffs_d) and same(traj, traj_d)
    # without the rows, the durations and the coefficients: the row offsets alone say what a second call needs
    only = np.zeros(B + 1, np.int64)
    ctx.call("uavac_minsnap_plan_ragged", P(WP_RAGGED), P(SEG_OFFSETS), B, VEL, DT, None, P(only), None, None, 0)
    assert same(only, row_offsets_d)


def dev_obstacle_waypoints(ctx, d, cuboid, max_iterations):
    """The loop of `uavac_minsnap_obstacle_waypoints` for one cuboid and no re-check sweep, on `uavac_minsnap_obstacle_round_dev`."""
    cap = B * 64
    wp_a, wp_b, so_a, so_b = d.f64(cap + B, 3), d.f64(cap + B, 3), d.i64(B + 1), d.i64(B + 1)
    wp_a[:S + B] = d.up(WP_RAGGED)
    so_a[:] = d.up(SEG_OFFSETS)
    active, overflow, touched, counters = d.i32(B) + 1, d.i32(B), d.i32(B), d.i32(4)
    times, seg_rows, hit, row_offsets, coeffs, cub = d.f64(cap), d.i32(cap), d.i32(cap), d.i64(B + 1), d.f64(cap, 8, 3), d.up(cuboid)
    max_m, n_active, failed = M, B, np.zeros(B, bool)
    for _ in range(max_iterations + 1):
        if n_active == 0:
            break
        ctx.call("uavac_minsnap_obstacle_round_dev", P(wp_a), P(so_a), B, max_m, VEL, DT, P(cub), P(active), P(overflow), P(touched), P(wp_b),
                 P(so_b), P(counters), P(times), P(seg_rows), P(row_offsets), P(coeffs), P(hit))
        wp_a, wp_b, so_a, so_b = wp_b, wp_a, so_b, so_a
        cnt = counters.cpu().numpy()
        n_active, max_m = int(cnt[0]), max(max_m, int(cnt[2]))
        if cnt[1]:
            failed |= overflow.cpu().numpy() != 0
    if n_active > 0:
        failed |= active.cpu().numpy() != 0
    return wp_a, so_a, failed


def test_obstacle_waypoints(gpu):
    ctx, N, torch = gpu
    d = Dev(torch)
    cap = B * 65
    # no cuboid: the waypoints come back as they went in
    wp_out, so_out, conv = np.zeros((cap, 3)), np.zeros(B + 1, np.int64), np.zeros(B, np.int32)
    ctx.call("uavac_minsnap_obstacle_waypoints", P(WP_RAGGED), P(SEG_OFFSETS), B, VEL, DT, None, 0, 8, 0, P(wp_out), cap, P(so_out), P(conv))
    assert np.array_equal(so_out, SEG_OFFSETS) and wp_out[:S + B].tobytes() == WP_RAGGED.tobytes() and list(conv) == [1, 1, 1]
    # one cuboid that mission 0 crosses
    wp_d, so_d, failed = dev_obstacle_waypoints(ctx, d, CUBOID, 8)
    wp_out, so_out = np.zeros((cap, 3)), np.zeros(B + 1, np.int64)
    ctx.call("uavac_minsnap_obstacle_waypoints", P(WP_RAGGED), P(SEG_OFFSETS), B, VEL, DT, P(CUBOID), 1, 8, 0, P(wp_out), cap, P(so_out), P(conv))
    n_wp = int(so_out[-1]) + B
    assert so_out[1] - so_out[0] > 1 and so_out[2] - so_out[1] == 2 and so_out[3] - so_out[2] == 2      # mission 0 got midpoints, only it
    assert same(so_out, so_d) and same(wp_out[:n_wp], wp_d[:n_wp])
    assert list(conv) == [0 if f else 1 for f in failed]
    # converged may be NULL
    wp_2, so_2 = np.zeros((cap, 3)), np.zeros(B + 1, np.int64)
    ctx.call("uavac_minsnap_obstacle_waypoints", P(WP_RAGGED), P(SEG_OFFSETS), B, VEL, DT, P(CUBOID), 1, 8, 0, P(wp_2), cap, P(so_2), None)
    assert wp_2.tobytes() == wp_out.tobytes() and so_2.tobytes() == so_out.tobytes()


def test_yaw_scan_across_the_staging_thresholds(gpu):
    ctx, N, torch = gpu
    d = Dev(torch)
    rng = np.random.default_rng(5)
    for n in (3, 20_000, 50_000, 3):
        vel = rng.uniform(-3.0, 3.0, (n, 3))
        vel[n // 2] = 0.0                                   # a row without a heading
        vel_d, offsets_d, yaws_d = d.up(vel), d.up(np.array([0, n], dtype=np.int64)), d.f64(n)
        ctx.call("uavac_yaw_scan_dev", P(vel_d), P(offsets_d), 1, P(yaws_d))
        torch.cuda.synchronize()
        yaws = np.full(n, 7.0)
        ctx.call("uavac_yaw_scan", P(vel), n, P(yaws))
        assert same(yaws, yaws_d), n


def dev_state(ctx, N, d, V, positions):
    state, istate, positions_d = d.f64(N.STATE_ROWS, B), d.i32(N.ISTATE_ROWS, B), None if positions is None else d.up(positions)
    ctx.call("uavac_state_init_dev", C.byref(V), P(positions_d), B, 1, P(state), P(istate))
    d.torch.cuda.synchronize()
    return state, istate


def test_state_init(gpu):
    ctx, N, torch = gpu
    d, V = Dev(torch), N.Vehicle.default()
    for positions in (WAYPOINTS[:, 0].copy(), None):
        state_d, istate_d = dev_state(ctx, N, d, V, positions)
        state, istate = np.full((N.STATE_ROWS, B), 7.0), np.full((N.ISTATE_ROWS, B), 7, np.int32)
        ctx.call("uavac_state_init", C.byref(V), P(positions), B, 1, P(state), P(istate))
        assert same(state, state_d) and same(istate, istate_d)


@pytest.mark.parametrize("logs", [False, True])
@pytest.mark.parametrize("obstacle", [False, True])
def test_control_rollout(gpu, logs, obstacle):
    ctx, N, torch = gpu
    d, V = Dev(torch), N.Vehicle.default()
    _, _, row_offsets_d, _, traj_d = dev_plan(ctx, d)
    state_d, istate_d = dev_state(ctx, N, d, V, WAYPOINTS[:, 0].copy())
    state, istate = state_d.cpu().numpy().copy(), istate_d.cpu().numpy().copy()
    box = np.array([[-0.5, 0.5, -0.5, 0.5, -1.5, -0.5]]) if obstacle else None          # vehicle 0 starts inside it
    sl_d, cl_d = (d.f64(K, 13, B), d.f64(K, N.CMD_COLS, B)) if logs else (None, None)
    box_d = None if box is None else d.up(box)
    ctx.call("uavac_control_rollout_dev", C.byref(V), P(traj_d), P(row_offsets_d), P(state_d), P(istate_d), B, K, P(sl_d), P(cl_d), P(box_d),
             1 if obstacle else 0)
    torch.cuda.synchronize()
    sl, cl = (np.zeros((K, 13, B)), np.zeros((K, N.CMD_COLS, B))) if logs else (None, None)
    ctx.call("uavac_control_rollout", C.byref(V), P(traj_d.cpu().numpy()), P(row_offsets_d.cpu().numpy()), P(state), P(istate), B, K, P(sl),
             P(cl), P(box), 1 if obstacle else 0)
    assert same(state, state_d) and same(istate, istate_d)
    assert (istate[2, 0] != 0) == obstacle
    if logs:
        assert same(sl, sl_d) and same(cl, cl_d)


def test_controller_tick(gpu):
    ctx, N, torch = gpu
    d, V = Dev(torch), N.Vehicle.default()
    _, _, row_offsets_d, _, traj_d = dev_plan(ctx, d)
    state_d, istate_d = dev_state(ctx, N, d, V, WAYPOINTS[:, 0].copy())
    state, istate = state_d.cpu().numpy().copy(), istate_d.cpu().numpy().copy()
    ctx.call("uavac_controller_tick_dev", C.byref(V), P(traj_d), P(row_offsets_d), P(state_d), P(istate_d), B)
    torch.cuda.synchronize()
    before = state.copy()
    ctx.call("uavac_controller_tick", C.byref(V), P(traj_d.cpu().numpy()), P(row_offsets_d.cpu().numpy()), P(state), P(istate), B)
    assert same(state, state_d) and same(istate, istate_d) and state.tobytes() != before.tobytes()


@pytest.mark.parametrize("obstacle", [False, True])
def test_dynamics_step(gpu, obstacle):
    ctx, N, torch = gpu
    d, V = Dev(torch), N.Vehicle.default()
    state_d, istate_d = dev_state(ctx, N, d, V, WAYPOINTS[:, 0].copy())
    state, istate = state_d.cpu().numpy().copy(), istate_d.cpu().numpy().copy()
    box = np.array([[-0.5, 0.5, -0.5, 0.5, -1.5, -0.5]]) if obstacle else None
    # without an obstacle (and without a ground plane) the flags are not needed: istate may be NULL
    box_d = None if box is None else d.up(box)
    ctx.call("uavac_dynamics_step_dev", C.byref(V), P(state_d), P(istate_d if obstacle else None), B, P(box_d), 1 if obstacle else 0)
    torch.cuda.synchronize()
    ctx.call("uavac_dynamics_step", C.byref(V), P(state), P(istate if obstacle else None), B, P(box), 1 if obstacle else 0)
    assert same(state, state_d) and same(istate, istate_d)
    assert (istate[2, 0] != 0) == obstacle


# ------------------------------------------------------------------------------------------------------- the RRT* twins
RRT_ITER, RRT_STEP, RRT_SEEDS = 40, 2.0, (0, 1, 2)
RRT_LW, RRT_UP = np.array([0.0, 0.0, 0.0]), np.array([6.0, 6.0, 3.0])
RRT_STARTS = np.array([[0.5, 0.5, 0.5], [0.5, 5.5, 1.0], [1.0, 3.0, 2.0]])
RRT_GOALS = np.array([[5.5, 5.5, 2.5], [5.5, 0.5, 2.0], [5.0, 3.0, 1.0]])
# problem 2 runs from (1, 3, 2) to (5, 3, 1): straight through this cuboid
RRT_CUBOID = np.array([[2.5, 3.5, 2.0, 4.0, 0.0, 3.0]])
EDGES_A = np.array([[0.0, 0.0, 0.0], [1.0, 3.0, 2.0], [5.0, 5.0, 1.0], [0.5, 0.5, 2.5], [3.0, 3.0, 1.5]])
EDGES_B = np.array([[1.0, 1.0, 1.0], [5.0, 3.0, 1.0], [5.0, 1.0, 1.0], [0.5, 0.5, 2.6], [3.0, 3.0, 1.5]])
TWO_CUBOIDS = np.array([[2.5, 3.5, 2.0, 4.0, 0.0, 3.0], [4.5, 5.5, 2.5, 3.5, 0.0, 3.0]])


def both(ctx, torch, twin, args, outs):
    """`twin` on NumPy arrays and `twin`_dev on the same inputs in torch tensors.  `args`: the arguments in order, arrays and numbers, with
    "out" where the outputs go; `outs`: (shape, dtype) of each output.  Outputs start out as sevens.  -> (host outputs, device outputs)"""
    d = Dev(torch)
    host = [np.full(shape, 7, dtype) for shape, dtype in outs]
    dev = [d.up(h) for h in host]
    held = [d.up(a) if isinstance(a, np.ndarray) else a for a in args]           # (kept alive over the call)
    for name, ins, res in ((twin, args, host), (twin + "_dev", held, dev)):
        at = iter(res)
        ctx.call(name, *[P(next(at)) if isinstance(a, str) else a if isinstance(a, (int, float)) else P(a) for a in ins])
    torch.cuda.synchronize()
    return host, dev


def all_same(host, dev):
    return all(same(h, t) for h, t in zip(host, dev))


@pytest.mark.parametrize("cuboids", [RRT_CUBOID, None], ids=["one cuboid", "no cuboid"])
def test_rrt_star_and_simplify(gpu, cuboids):
    ctx, N, torch = gpu
    from uav_ac.planning.rrt import draw_random_nodes_batch
    nb, cap, n_obs = len(RRT_STARTS), RRT_ITER + 1, 0 if cuboids is None else len(cuboids)
    samples = draw_random_nodes_batch(RRT_SEEDS, RRT_LW, RRT_UP, RRT_GOALS, RRT_ITER)
    outs = [((nb, cap, 3), np.float64), ((nb, cap), np.int32), ((nb, cap), np.int32), ((nb, cap), np.int32), ((nb, cap, 3), np.float64),
            ((nb, 6), np.int32), ((nb,), np.float64)]
    host, dev = both(ctx, torch, "uavac_rrt_star", [RRT_STARTS, RRT_GOALS, nb, RRT_STEP, RRT_ITER, samples, cuboids, n_obs] + ["out"] * 7, outs)
    assert all_same(host, dev)
    best_path, counts = host[4], host[5]
    assert (counts[:, 2] == 0).any() and (counts[:, 0] > 1).all()                 # (UAVAC_RRT_OK somewhere, and trees everywhere)
    lens = np.ascontiguousarray(counts[:, 4])
    assert lens.max() > 2
    host, dev = both(ctx, torch, "uavac_rrt_simplify", [best_path, lens, nb, cap, cuboids, n_obs, "out", "out"],
                     [((nb, cap, 3), np.float64), ((nb,), np.int32)])
    assert all_same(host, dev)
    assert (host[1] <= lens).all() and (host[1][lens > 0] >= 2).all()


@pytest.mark.parametrize("cuboids", [TWO_CUBOIDS, None], ids=["two cuboids", "no cuboid"])
def test_rrt_segment_hits(gpu, cuboids):
    ctx, N, torch = gpu
    n_obs = 0 if cuboids is None else len(cuboids)
    host, dev = both(ctx, torch, "uavac_rrt_segment_hits", [EDGES_A, EDGES_B, 5, cuboids, n_obs, "out"], [((5,), np.int32)])
    assert all_same(host, dev)
    assert list(host[0]) == ([0, 1, 1, 0, 1] if n_obs else [0] * 5)      # edge 1 crosses the first cuboid, 2 the second, 4 lies in the first


@pytest.mark.parametrize("single", [0, 1])
def test_rrt_edge_lengths(gpu, single):
    ctx, N, torch = gpu
    host, dev = both(ctx, torch, "uavac_rrt_edge_lengths", [EDGES_A, EDGES_B[1] if single else EDGES_B, single, 5, "out"], [((5,), np.float64)])
    assert all_same(host, dev)
    assert host[0][0] == np.sqrt(35.0 if single else 3.0)


def test_rrt_path_cost(gpu):
    ctx, N, torch = gpu
    for n in (0, 4):
        host, dev = both(ctx, torch, "uavac_rrt_path_cost", [EDGES_A[:n] if n else None, n, "out"], [((1,), np.float64)])
        assert all_same(host, dev)
        assert (host[0][0] > 0.0) == (n > 0)


@pytest.mark.parametrize("E", [1, 3])
def test_rrt_steer(gpu, E):
    ctx, N, torch = gpu
    # (edges 0 and 2 are longer than the step and get cut; edges 3 and 4 of the E = 3 call are not)
    a, b = (EDGES_A[:1], EDGES_B[:1]) if E == 1 else (EDGES_A[2:], EDGES_B[2:])
    host, dev = both(ctx, torch, "uavac_rrt_steer", [np.ascontiguousarray(b), np.ascontiguousarray(a), E, 1.0, "out"], [((E, 3), np.float64)])
    assert all_same(host, dev)
    assert host[0].tobytes() != b.tobytes()


def test_rrt_edge_lengths_as_the_arena_grows(gpu):
    ctx, N, torch = gpu
    rng = np.random.default_rng(6)
    for E in (3, 20_000, 50_000, 3):
        a, b = rng.uniform(-5.0, 5.0, (E, 3)), rng.uniform(-5.0, 5.0, (E, 3))
        host, dev = both(ctx, torch, "uavac_rrt_edge_lengths", [a, b, 0, E, "out"], [((E,), np.float64)])
        assert all_same(host, dev), E
