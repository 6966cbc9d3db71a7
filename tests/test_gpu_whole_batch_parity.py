"""Every lane of the rollout, in the launch forms the batch size selects, against an independent reference: the C oracle plans
every mission itself (oracle_solve / oracle_sample, never the GPU's plan) and flies it (oracle_rollout), on threads
(`c_oracle.fleet`).  Before this file the oracle saw three to five spot lanes of single-pass launches whose tile counts were
multiples of 8; the forms below -- config 4's rank shards (partial last tiles, plan-fed PMODE 1, one 5 000-tick launch, pitched
logs), the four-rank root flying while it samples all 262 144 missions' rows (past 2^31 doubles), PMODE 2, a second persistent
pass of 70 tiles (70 % 8 = 6, so `xcd_contiguous` is not the plain block index) with an odd K across passes, four full passes --
were checked only HIP against HIP.  Every case asserts the launch it reached (`Context.last_rollout_launch`, kernel name).

The bar is the same for every lane, lost or kept: 1e-5 in the SURVEY 8(c) column metric on the final 26-value state, on the
whole state log at the selected ticks and on every tick of the chosen lanes; istate equal; the plan's row counts equal,
coefficients within 1e-9, first headings within 1e-9.  Also here: the rows-free bookkeeping (a rows-free replan that needs more
rows; an undersized root buffer is refused, not overrun; a rows-free ragged batch gets its rows)."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import col_err, load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-5
VEL, DT = 3.0, 0.01
C4_TOTAL, C4_M, C4_K = 262144, 8, 5000
SENTINEL = -1.2345e300
WORST = {}                                    # case -> largest error seen (printed at the end of the module, -s shows it)


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    return Engine("cuda:0")


@pytest.fixture(scope="module")
def pool():
    ex = ThreadPoolExecutor(max_workers=1)    # the oracle runs (on its own threads) while the GPU flies
    yield ex
    ex.shutdown(wait=True)
    for k, v in sorted(WORST.items()):
        print(f"whole-batch parity {k}: worst {v:.3e}")


@pytest.fixture(scope="module")
def c4():
    import bench
    return bench.missions(C4_TOTAL, C4_M, 0, C4_TOTAL)


def _simds():
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


def _xcd(block, n):                          # uavac_internal.h xcd_contiguous
    x, q, r = block & 7, n >> 3, n & 7
    return x * q + min(x, r) + (block >> 3)


def _pad_lds(k):                             # control_rollout.hip launch_shape: the cu_balance pad for k workgroups per CU
    return ((163840 // (k + 1) + 1024) + 1023) & ~1023


def _sel_ticks(K, boundaries):
    t = {0, 1, 9, 10, 11, K // 2, K - 1}
    for b in boundaries:
        t |= {b - 1, b, b + 1}
    return sorted(x for x in t if 0 <= x < K)


def _chosen_lanes(B, grid, seed):
    """All 64 lanes of tiles 0, 1, the last two, the first tile of every pass and the tile the last block of every pass walks;
    plus 128 seeded random lanes."""
    n_tiles = -(-B // 64)
    tiles = {0, 1, n_tiles - 2, n_tiles - 1}
    for t0 in range(0, n_tiles, grid):
        n_here = min(grid, n_tiles - t0)
        tiles |= {t0, t0 + _xcd(n_here - 1, n_here)}
    lanes = {t * 64 + j for t in tiles if t >= 0 for j in range(64)}
    lanes |= set(np.random.default_rng(seed).integers(0, B, 128).tolist())
    return np.array(sorted(b for b in lanes if 0 <= b < B), dtype=np.int64)


def _wrap(a):
    return np.abs(np.mod(a + np.pi, 2 * np.pi) - np.pi)


def _fly(eng, fleet, launches, sel, lanes, pitch=None, cmd=False, aabbs=None, log=True):
    """The launches (tick counts) one after another, each into a fresh log pre-filled with SENTINEL; after each: its shape, the
    selected ticks of the whole log, every tick of the chosen lanes, the padding columns.  -> dict of host arrays."""
    import torch
    B = fleet.B
    P = pitch or B
    lanes_t = torch.as_tensor(lanes, device=eng.device)
    out = {"shapes": [], "sel": [], "sel_cmd": [], "lanes": []}
    t0 = 0
    ab = None if aabbs is None else torch.as_tensor(aabbs, dtype=torch.float64, device=eng.device)
    for k in launches:
        slog = clog = None
        if log:
            slog = torch.full((k, 13, P), SENTINEL, dtype=torch.float64, device=eng.device)
            clog = torch.full((k, 12, P), SENTINEL, dtype=torch.float64, device=eng.device) if cmd else None
        s, c = fleet.rollout(k, state_log=slog, cmd_log=clog, aabbs=ab, log_pitch=pitch)
        out["shapes"].append((eng.ctx.last_rollout_kernel(), eng.ctx.last_rollout_launch()))
        if log:
            here = [t - t0 for t in sel if t0 <= t < t0 + k]
            idx = torch.as_tensor(here, device=eng.device, dtype=torch.int64)
            out["sel"].append(s[idx].cpu().numpy())
            if cmd:
                out["sel_cmd"].append(c[idx].cpu().numpy())
            out["lanes"].append(s[:, :, lanes_t].permute(2, 0, 1).cpu().numpy())
            if P > B:
                for buf in (slog, clog):
                    if buf is not None:
                        assert bool((buf[:, :, B:] == SENTINEL).all()), "a padding column of the log was written"
            del s, c, slog, clog
        t0 += k
    torch.cuda.synchronize()
    res = {"shapes": out["shapes"], "state": fleet.state[:26].T.cpu().numpy(), "istate": fleet.istate.T.cpu().numpy()}
    if log:
        res["sel"] = np.concatenate(out["sel"])
        res["lanes"] = np.concatenate(out["lanes"], axis=1)
        if cmd:
            res["sel_cmd"] = np.concatenate(out["sel_cmd"])
    return res


def _check_flight(case, got, ref, log=True, cmd=False):
    """The oracle's bar on every lane: final state, istate, selected ticks, every tick of the chosen lanes."""
    errs = {"state": col_err(got["state"], ref["state"])}
    bad = np.flatnonzero((got["istate"] != ref["istate"]).any(axis=1))
    assert len(bad) == 0, f"{case}: istate differs on {len(bad)} lanes, first {bad[:8].tolist()}: {got['istate'][bad[:4]]} vs {ref['istate'][bad[:4]]}"
    if log:
        # (n_sel, 13, B) -> one column per state value
        errs["sel"] = col_err(got["sel"].transpose(0, 2, 1), ref["sel_log"].transpose(0, 2, 1))
        errs["lanes"] = col_err(got["lanes"], ref["lane_log"])
        if cmd:
            errs["sel_cmd"] = col_err(got["sel_cmd"].transpose(0, 2, 1), ref["sel_cmd"].transpose(0, 2, 1))
    WORST[case] = max(WORST.get(case, 0.0), *errs.values())
    for k, v in errs.items():
        if v > TOL:
            if k == "state":
                per_lane = np.max(np.abs(got["state"] - ref["state"]) / np.maximum(1.0, np.abs(ref["state"]).max(axis=0)), axis=1)
                worst = np.argsort(per_lane)[-8:][::-1]
                raise AssertionError(f"{case}: final state off by {v:.3e}; worst lanes {worst.tolist()} ({per_lane[worst]})")
            raise AssertionError(f"{case}: {k} off by {v:.3e}")


def _check_plan(case, plan, ref):
    """Row counts equal, coefficients within 1e-9 per mission (column metric), first headings within 1e-9 modulo 2 pi."""
    sr = plan.seg_rows.cpu().numpy()
    bad = np.flatnonzero((sr != ref["seg_rows"]).any(axis=1))
    assert len(bad) == 0, f"{case}: row counts differ for {len(bad)} missions, first {bad[:8].tolist()}"
    co = plan.coeffs.cpu().numpy()
    scale = np.maximum(1.0, np.abs(ref["coeffs"]).max(axis=1))
    e = float((np.abs(co - ref["coeffs"]).max(axis=1) / scale).max())
    assert e <= 1e-9, f"{case}: coefficients off by {e:.3e}"
    fy = float(_wrap(plan.first_yaw.cpu().numpy() - ref["first_yaw"]).max())
    assert fy <= 1e-9, f"{case}: first headings off by {fy:.3e}"


def _assert_shape(case, shapes, pmode=None, poly=True, threads=None, lds=None, lds_below=None, grid=None, n_tiles=None,
                  passes=None, pitch=None):
    for name, sh in shapes:
        args = [a.strip() for a in name[name.index("<") + 1:-1].split(",")]
        assert args[5] == ("true" if poly else "false"), (case, name)
        if pmode is not None:
            assert int(args[8]) == pmode, (case, name)
        for key, want in (("threads", threads), ("lds", lds), ("grid", grid), ("n_tiles", n_tiles), ("passes", passes),
                          ("pitch", pitch)):
            if want is not None:
                assert sh[key] == want, (case, key, sh)
        if lds_below is not None:
            assert sh["lds"] < lds_below, (case, sh)


def _c4_case(eng, pool, c4, case, lo, hi, expect):
    from oracle import c_oracle as cc
    B = hi - lo
    wps = c4[lo:hi]
    S = _simds()
    n_tiles = -(-B // 64)
    assert n_tiles <= S
    lanes = _chosen_lanes(B, n_tiles, seed=lo)
    sel = _sel_ticks(C4_K, [])
    fut = pool.submit(cc.fleet, wps, VEL, DT, C4_K, sel, lanes)
    plan = eng.plan(wps, VEL, DT, rows=False)
    fleet = eng.fleet(plan)
    assert fleet.from_plan
    pitch = -(-B // 16) * 16
    got = _fly(eng, fleet, [C4_K], sel, lanes, pitch=pitch)
    _assert_shape(case, got["shapes"], pitch=pitch, grid=n_tiles, n_tiles=n_tiles, passes=1, **expect)
    ref = fut.result()
    _check_plan(case, plan, ref)
    _check_flight(case, got, ref)


def test_config4_peer_shard_every_lane(eng, pool, c4):
    """Case A: rank 1 of 8 at root_share 0 -- 37 450 UAVs, 586 tiles (586 % 8 = 2), a 10-lane last tile, rows-free plan,
    plan-fed PMODE 1, no placeholder wave, the k = 3 LDS pad, 5 000 ticks in one launch at log pitch 37 456."""
    from uav_ac.sharding import shard_bounds
    lo, hi = shard_bounds(C4_TOTAL, 1, 8, 0.0, 0)
    assert hi - lo == 37450 and (hi - lo) % 64 == 10 and -(-(hi - lo) // 64) == 586
    _c4_case(eng, pool, c4, "A", lo, hi, dict(pmode=1, threads=128, lds=_pad_lds(3)))


def test_config4_last_peer_shard_every_lane(eng, pool, c4):
    """Case B: rank 7 of 8 -- 37 449 UAVs, a 9-lane last tile; the same launch form."""
    from uav_ac.sharding import shard_bounds
    lo, hi = shard_bounds(C4_TOTAL, 7, 8, 0.0, 0)
    assert hi - lo == 37449 and (hi - lo) % 64 == 9
    _c4_case(eng, pool, c4, "B", lo, hi, dict(pmode=1, threads=128, lds=_pad_lds(3)))


def test_config4_four_rank_root_flies_while_it_samples_every_row(eng, pool, c4):
    """Case C: the root of a four-rank job -- 28 740 UAVs (balanced_root_share with the default table), plan-fed PMODE 1 with
    the placeholder wave and the k = 2 pad, 5 000 ticks in one launch on the default stream -- while a world-1 pipelined plan
    gather of all 262 144 rows-free missions samples ~237 M rows (past 2^31 doubles) into one preallocated buffer on a side
    stream.  Flight against the oracle on every lane; rows of the missions at the buffer's 2^31 / 2^32 boundaries, at every part
    boundary, the first, the last and 200 random ones against the oracle's rows."""
    import torch
    import bench
    from uav_ac import _native as nat
    from uav_ac.fleet import RcclComm
    from uav_ac.sharding import PIPELINE_SHARES, balanced_root_share, part_bounds, shard_bounds
    from oracle import c_oracle as cc
    share = balanced_root_share(C4_TOTAL, 4, bench.C4_TICKS, bench.C4_SEGMENTS)
    lo, hi = shard_bounds(C4_TOTAL, 0, 4, share, 0)
    assert (lo, hi) == (0, 28740)
    B = hi - lo
    n_tiles = -(-B // 64)
    lanes = _chosen_lanes(B, n_tiles, seed=3)
    sel = _sel_ticks(C4_K, [])
    fut = pool.submit(cc.fleet, c4[lo:hi], VEL, DT, C4_K, sel, lanes)
    everything = eng.plan(c4, VEL, DT, rows=False)
    mine = eng.plan(c4[lo:hi], VEL, DT, rows=False)
    fleet = eng.fleet(mine)
    buf = C.create_string_buffer(nat.COMM_ID_BYTES)
    eng.ctx.call("uavac_comm_unique_id", buf)
    comm = RcclComm(eng, unique_id=bytes(buf.raw), world=1, rank=0)
    try:
        known = comm.plan_counts(everything)
        total = known[1][0]
        assert total * 11 > 2 ** 31, total
        traj = torch.empty((total, 11), dtype=torch.float64, device=eng.device)
        side = torch.cuda.Stream(device=eng.device)
        ticket = comm.gather_plan_begin(everything, dst=0, stream=side, traj=traj, parts=True, known_counts=known)
        got = _fly(eng, fleet, [C4_K], sel, lanes, pitch=-(-B // 16) * 16)
        gathered, counts = comm.gather_finish(ticket)
        torch.cuda.synchronize()
    finally:
        comm.close()
    assert counts == [total] and gathered.traj.data_ptr() == traj.data_ptr()
    _assert_shape("C", got["shapes"], pmode=1, threads=192, lds=_pad_lds(2), grid=n_tiles, n_tiles=n_tiles, passes=1)
    ro = gathered.row_offsets.cpu().numpy()
    assert ro[-1] == total
    pick = {0, C4_TOTAL - 1}
    for elem in (2 ** 29, 2 ** 31, 2 ** 32):          # byte 2^32, element 2^31, element 2^32 (if the buffer reaches it)
        row = elem // 11
        if row < total:
            pick.add(int(np.searchsorted(ro, row, side="right") - 1))
    for b in part_bounds(C4_TOTAL, PIPELINE_SHARES)[1:-1]:
        pick |= {b - 1, b}
    pick |= set(np.random.default_rng(11).integers(0, C4_TOTAL, 200).tolist())
    worst = 0.0
    for b in sorted(pick):
        rows = gathered.traj[int(ro[b]):int(ro[b + 1])].cpu().numpy()
        want, _, _ = cc.plan(c4[b], VEL, DT)
        assert rows.shape == want.shape, (b, rows.shape, want.shape)
        worst = max(worst, col_err(rows, want))
    WORST["C rows"] = worst
    assert worst <= 1e-8, worst
    ref = fut.result()
    _check_plan("C", mine, ref)
    _check_flight("C", got, ref)


def test_pmode2_with_obstacles_and_a_launch_boundary(eng, pool):
    """Case D: 20 000 UAVs, m = 8 -- plan-fed PMODE 2 (the second wave evaluates the rows), placeholder wave, k = 2 pad -- state
    and command logs, the lab's obstacles, 3 001 ticks as 1 000 + 2 001."""
    from oracle import c_oracle as cc
    from oracle import minsnap_oracle as mo
    B, K = 20000, 3001
    wps = mo.synthetic_missions(B, 8)
    aabbs = load_golden("fixed_missions.npz")["lab_aabbs"]
    n_tiles = -(-B // 64)
    lanes = _chosen_lanes(B, n_tiles, seed=4)
    sel = _sel_ticks(K, [1000])
    fut = pool.submit(cc.fleet, wps, VEL, DT, K, sel, lanes, aabbs, None, None, True)
    plan = eng.plan(wps, VEL, DT)
    fleet = eng.fleet(plan)
    assert fleet.from_plan
    got = _fly(eng, fleet, [1000, 2001], sel, lanes, cmd=True, aabbs=aabbs)
    _assert_shape("D", got["shapes"], pmode=2, threads=192, lds=_pad_lds(2), grid=n_tiles, n_tiles=n_tiles, passes=1, pitch=B)
    ref = fut.result()
    assert 0 < int(ref["istate"][:, 2].sum()) < B          # the obstacles stop some missions and not others
    _check_plan("D", plan, ref)
    _check_flight("D", got, ref, cmd=True)


def test_second_persistent_pass_with_odd_ticks(eng, pool):
    """Case E: 70 001 UAVs, m = 8 -- 1 094 tiles on 1 024 workgroups: a second persistent pass of 70 tiles (70 % 8 = 6) whose
    last tile has 49 lanes; K = 777 (odd: the LDS slab parity (kk + k) & 1 changes between passes) in one logged launch, then
    224 ticks more; row-fed and plan-fed (PMODE 0); and one unlogged plan-fed flight (one launch of all tiles)."""
    from oracle import c_oracle as cc
    from oracle import minsnap_oracle as mo
    B, K1, K2 = 70001, 777, 224
    S = _simds()
    wps = mo.synthetic_missions(B, 8)
    n_tiles = -(-B // 64)
    assert n_tiles == 1094 and B % 64 == 49
    assert S == 1024, "the case is sized for 1 024 SIMDs"
    lanes = _chosen_lanes(B, S, seed=5)
    sel = _sel_ticks(K1 + K2, [K1])
    fut = pool.submit(cc.fleet, wps, VEL, DT, K1 + K2, sel, lanes)
    plan = eng.plan(wps, VEL, DT)
    flights = {}
    for mode in (False, True):
        fleet = eng.fleet(plan, from_plan=mode)
        flights[mode] = _fly(eng, fleet, [K1, K2], sel, lanes)
        _assert_shape("E", flights[mode]["shapes"], pmode=0, poly=mode, threads=128, grid=S, n_tiles=n_tiles, passes=2, pitch=B,
                      lds_below=_pad_lds(3))
    fleet = eng.fleet(plan, from_plan=True)
    unlogged = _fly(eng, fleet, [K1 + K2], sel, lanes, log=False)
    _assert_shape("E", unlogged["shapes"], pmode=0, grid=n_tiles, n_tiles=n_tiles, passes=1)
    ref = fut.result()
    _check_plan("E", plan, ref)
    _check_flight("E row-fed", flights[False], ref)
    _check_flight("E plan-fed", flights[True], ref)
    _check_flight("E unlogged", unlogged, ref, log=False)


def test_full_config4_at_world_one_four_passes(eng, pool, c4):
    """Case F: all 262 144 missions of config 4 on one GPU, rows-free, plan-fed -- 4 096 tiles, four full persistent passes --
    as the bench's world-1 chunking flies them: two logged launches of 1 000 ticks."""
    from oracle import c_oracle as cc
    B, K = C4_TOTAL, 2000
    S = _simds()
    n_tiles = B // 64
    lanes = _chosen_lanes(B, S, seed=6)
    sel = _sel_ticks(K, [1000])
    fut = pool.submit(cc.fleet, c4, VEL, DT, K, sel, lanes)
    plan = eng.plan(c4, VEL, DT, rows=False)
    fleet = eng.fleet(plan)
    got = _fly(eng, fleet, [1000, 1000], sel, lanes)
    _assert_shape("F", got["shapes"], pmode=0, threads=128, grid=S, n_tiles=n_tiles, passes=4, pitch=B, lds_below=_pad_lds(3))
    ref = fut.result()
    _check_plan("F", plan, ref)
    _check_flight("F", got, ref)


def test_config2_every_lane_agrees(eng, pool):
    """Case G: config 2 -- 4 096 UAVs, m = 8, 10 000 ticks, 64 workgroups (at most one per CU): every lane, the ones the
    controller loses included, agrees with the oracle (the older test compared the SET of lost lanes)."""
    from oracle import c_oracle as cc
    from oracle import minsnap_oracle as mo
    B, K = 4096, 10000
    wps = mo.synthetic_missions(B, 8)
    lanes = _chosen_lanes(B, 64, seed=7)
    sel = _sel_ticks(K, [])
    fut = pool.submit(cc.fleet, wps, VEL, DT, K, sel, lanes)
    plan = eng.plan(wps, VEL, DT)
    fleet = eng.fleet(plan)
    got = _fly(eng, fleet, [K], sel, lanes)
    _assert_shape("G", got["shapes"], poly=False, threads=128, lds=2 * 13 * 64 * 8, grid=64, n_tiles=64, passes=1, pitch=B)
    ref = fut.result()
    _check_plan("G", plan, ref)
    _check_flight("G", got, ref)


# ------------------------------------------------------------------------------------------------ rows-free bookkeeping
def _comm(eng):
    from uav_ac import _native as nat
    from uav_ac.fleet import RcclComm
    buf = C.create_string_buffer(nat.COMM_ID_BYTES)
    eng.ctx.call("uavac_comm_unique_id", buf)
    return RcclComm(eng, unique_id=bytes(buf.raw), world=1, rank=0)


def _stretched(wps, f=1.5):
    return wps[:, :1] + f * (wps - wps[:, :1])


def test_rows_free_replan_to_longer_missions_refreshes_its_row_count(eng):
    """A rows-free plan re-planned in place onto waypoints 1.5x as far apart needs more rows: `total_rows` and `plan_counts` say
    so (checked on the host before anything is gathered), and a pipelined gather at world 1 then samples the new rows, which
    agree with the oracle's rows of the new waypoints."""
    import torch
    from oracle import c_oracle as cc
    from oracle import minsnap_oracle as mo
    B, m = 300, 6
    wps = mo.synthetic_missions(B, m)
    wps2 = _stretched(wps)
    want = [cc.plan(w, VEL, DT)[0] for w in wps2]
    n2 = sum(len(t) for t in want)
    plan = eng.plan(wps, VEL, DT, rows=False)
    assert plan.total_rows < n2
    plan.waypoints.copy_(torch.as_tensor(wps2, device=eng.device))
    eng.replan(plan)
    assert plan.total_rows == n2                              # host side, before any row is sampled
    comm = _comm(eng)
    try:
        assert comm.plan_counts(plan) == ([B * m], [n2])
        got, counts = comm.gather_plan(plan, dst=0, parts=True)
        torch.cuda.synchronize()
    finally:
        comm.close()
    assert counts == [n2] and got.traj.shape[0] == n2 and eng.take_flags() == [0, 0, 0, 0]
    ro = got.row_offsets.cpu().numpy()
    rows = got.traj.cpu().numpy()
    assert max(col_err(rows[ro[b]:ro[b + 1]], want[b]) for b in range(B)) <= 1e-8


@pytest.mark.parametrize("parts", [None, True])
def test_undersized_root_buffer_is_refused_not_overrun(eng, parts):
    """The root's row buffer sized from row counts taken BEFORE the waypoints grew: the gather is refused (UavacError, flag 2)
    and nothing is written past the buffer.  The buffer is a prefix of a larger allocation whose tail -- longer than the growth
    -- holds a sentinel: a sampler without a capacity would write into that tail (memory this test owns), never elsewhere."""
    import torch
    from uav_ac import _native as nat
    from oracle import minsnap_oracle as mo
    B, m = 300, 6
    wps = mo.synthetic_missions(B, m)
    plan = eng.plan(wps, VEL, DT, rows=False)
    comm = _comm(eng)
    try:
        stale = comm.plan_counts(plan)
        n1 = stale[1][0]
        plan.waypoints.copy_(torch.as_tensor(_stretched(wps), device=eng.device))
        eng.replan(plan)
        n2 = plan.total_rows
        assert n2 > n1
        big = torch.full((n1 + 2 * (n2 - n1) + 64, 11), SENTINEL, dtype=torch.float64, device=eng.device)
        with pytest.raises(nat.UavacError):
            comm.gather_finish(comm.gather_plan_begin(plan, dst=0, traj=big[:n1], parts=parts, known_counts=stale))
        torch.cuda.synchronize()
    finally:
        comm.close()
    assert bool((big[n1:] == SENTINEL).all()), "rows were written past the buffer"
    assert eng.take_flags() == [0, 0, 0, 0]                  # (gather_finish took flag 2)
    # the same refusal straight from the sampler, and the new entry's argument check
    small = eng.plan_from_parts(plan.coeffs, plan.times, plan.seg_rows, m, VEL, DT, total_rows=n1, traj=big[:n1])
    assert eng.take_flags()[2] == 1 and small.traj.shape[0] == n1
    assert bool((big[n1:] == SENTINEL).all())
    with pytest.raises(nat.UavacError) as e:
        eng.ctx.call("uavac_minsnap_sample_capped_dev", C.c_void_p(plan.coeffs.data_ptr()), C.c_void_p(plan.seg_rows.data_ptr()),
                     C.c_void_p(small.row_offsets.data_ptr()), B, m, DT, C.c_void_p(big.data_ptr()), -1, None, None)
    assert e.value.code == nat.EINVAL


def test_rows_free_ragged_batch_gets_its_rows(eng):
    """`Engine.sample_rows` on a rows-free RAGGED batch: the rows and first headings of the batch planned with rows, bit for bit."""
    import torch
    from oracle import minsnap_oracle as mo
    rng = np.random.default_rng(9)
    missions = [w[:int(rng.integers(2, 10))] for w in mo.synthetic_missions(257, 8)]
    full = eng.plan_ragged(missions, VEL, DT)
    free = eng.plan_ragged(missions, VEL, DT, rows=False)
    assert free.traj is None
    eng.sample_rows(free)
    torch.cuda.synchronize()
    assert free.total_rows == full.total_rows
    assert torch.equal(free.traj, full.traj) and torch.equal(free.first_yaw, full.first_yaw)
    assert eng.take_flags() == [0, 0, 0, 0]
