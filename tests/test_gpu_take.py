"""Missions of a plan selected, reordered and merged on the GPU (`uavac_minsnap_take_offsets_dev` / `uavac_minsnap_take_dev`,
csrc/minsnap_take.hip), through the C ABI and `Engine.take`, `Engine.concat`, `Engine.put`.  Every comparison is exact: a take copies.

What is compared with what:
  * the taken arrays against `uav_ac.scoring.take_parts` of the plan's own arrays, from the middle of sentinel-filled buffers;
  * the sampled rows of a taken batch against the rows of the missions it took, bit for bit in all 11 columns;
  * `Engine.audit` of a taken batch against the audit's columns, `Engine.separation` of a group taken alone against the group inside
    its batch with the partners renumbered;
  * `put` against both sources, mission by mission, in the parts and in the sampled rows;
  * a taken batch flown plan-fed against the same flown row-fed from its sampled rows and against the lanes it took of the whole batch.
All cases use synthetic_missions(96, 8) at velocity 3.0 and dt 0.01 -- the stagger tests' missions -- as a uniform plan and as a ragged
batch of 1 .. 8 segments per mission (`wps[b][:2 + b % 8]`)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VEL, DT, B, M = 3.0, 0.01, 96, 8
PAD, SENT_F, SENT_I = 96, -7777.25, -7777
CUBOIDS = np.array([[11.13, 12.37, 6.21, 7.43, -20.0, 20.0], [3.17, 21.29, 1.61, 15.83, -4.613, -4.087],
                    [22.31, 25.87, 11.19, 14.57, -9.011, -2.203], [1.09, 4.91, -1.27, 2.33, -5.897, -3.511]])
INDEXES = dict(reversed=np.arange(B)[::-1], first=np.array([0]), last=np.array([B - 1]), duplicates=np.array([5, 5, 90, 0, 5, 33, 90]),
               n300=(7 * np.arange(300)) % B)                # n300: past one 256-thread workgroup of the counting kernel


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    return Engine("cuda:0")


_CACHE = {}


def case(eng):
    """Computed once and left unchanged: the missions, the uniform plan with rows, the ragged batch rows-free and with rows."""
    if not _CACHE:
        from oracle import minsnap_oracle as mo
        wps = mo.synthetic_missions(B, M)
        cut = [wps[b][:2 + b % 8] for b in range(B)]
        _CACHE.update(wps=wps, cut=cut, uniform=eng.plan(wps, VEL, DT), ragged=eng.plan_ragged(cut, VEL, DT, rows=False),
                      ragged_rows=eng.plan_ragged(cut, VEL, DT, rows=True))
    return _CACHE


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _i32(eng, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(eng.device)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64 if a.dtype == np.float64 else a.dtype),
                                                                        b.view(np.int64 if b.dtype == np.float64 else b.dtype))


def host_parts(plan):
    """(coeffs (S, 8, 3), times (S,), seg_rows (S,), seg offsets or m, first_yaw (B,)) of a plan as NumPy."""
    ragged = hasattr(plan, "seg_offsets")
    return (plan.coeffs.cpu().numpy().reshape(-1, 8, 3), plan.times.cpu().numpy().reshape(-1), plan.seg_rows.cpu().numpy().reshape(-1),
            plan.seg_offsets_host if ragged else plan.m, plan.first_yaw.cpu().numpy())


def take_abi(eng, plan, idx, with_times=True, with_yaw=True):
    """Both calls of the C ABI on a plan, every output the middle of a larger sentinel-filled buffer: nothing outside may be written,
    and everything inside must be.  -> (seg_offsets, coeffs (S', 8, 3), times | None, seg_rows, first_yaw | None) as NumPy."""
    import torch
    ragged = hasattr(plan, "seg_offsets")
    m = plan.max_m if ragged else plan.m
    so_in = plan.seg_offsets if ragged else None
    index, n = _i32(eng, idx), len(idx)
    so = torch.full((PAD + n + 1 + PAD,), SENT_I, dtype=torch.int64, device=eng.device)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_take_offsets_dev", _p(so_in), plan.B, m, _p(index), n, _p(so[PAD:]))
    so_h = so.cpu().numpy()
    assert (so_h[:PAD] == SENT_I).all() and (so_h[PAD + n + 1:] == SENT_I).all()
    so_h = so_h[PAD:PAD + n + 1].copy()
    S = int(so_h[-1])
    assert so_h[0] == 0 and (np.diff(so_h) >= 1).all() and (np.diff(so_h) <= m).all()      # (what sizes the buffers below)
    co = torch.full((PAD + 24 * S + PAD,), SENT_F, dtype=torch.float64, device=eng.device)
    tm = torch.full((PAD + S + PAD,), SENT_F, dtype=torch.float64, device=eng.device) if with_times else None
    sr = torch.full((PAD + S + PAD,), SENT_I, dtype=torch.int32, device=eng.device)
    fy = torch.full((PAD + n + PAD,), SENT_F, dtype=torch.float64, device=eng.device) if with_yaw else None
    eng.ctx.call("uavac_minsnap_take_dev", _p(plan.coeffs), _p(plan.times) if with_times else None, _p(plan.seg_rows), _p(so_in), plan.B, m,
                 _p(plan.first_yaw) if with_yaw else None, _p(index), n, _p(so[PAD:]), _p(co[PAD:]), _p(tm[PAD:]) if with_times else None,
                 _p(sr[PAD:]), _p(fy[PAD:]) if with_yaw else None)
    torch.cuda.synchronize()
    out = []
    for buf, width, sent in ((co, 24 * S, SENT_F), (tm, S, SENT_F), (sr, S, SENT_I), (fy, n, SENT_F)):
        if buf is None:
            out.append(None)
            continue
        h = buf.cpu().numpy()
        assert (h[:PAD] == sent).all() and (h[PAD + width:] == sent).all() and not (h[PAD:PAD + width] == sent).any()
        out.append(h[PAD:PAD + width].copy())
    return so_h, out[0].reshape(S, 8, 3), out[1], out[2], out[3]


# ------------------------------------------------------------------------------------------------ 1: the arrays, through the C ABI
@pytest.mark.parametrize("which", ["uniform", "ragged"])
def test_the_taken_arrays_equal_take_parts(eng, which):
    from uav_ac.scoring import take_parts
    plan = case(eng)[which]
    co_in, tm_in, sr_in, how, fy_in = host_parts(plan)
    if which == "ragged":
        assert sorted(set(np.diff(how).tolist())) == list(range(1, 9))
    for name, idx in INDEXES.items():
        want = take_parts(co_in, tm_in, sr_in, how, idx)
        so, co, tm, sr, fy = take_abi(eng, plan, idx)
        assert np.array_equal(so, want[3]) and so.dtype == np.int64, name
        assert same_bits(co, want[0]) and same_bits(tm, want[1]) and same_bits(sr, want[2]) and same_bits(fy, fy_in[idx]), name
    # durations and first headings are optional: without them the other outputs are the same
    idx = INDEXES["n300"]
    want = take_parts(co_in, tm_in, sr_in, how, idx)
    for with_times, with_yaw in ((False, True), (True, False), (False, False)):
        so, co, tm, sr, fy = take_abi(eng, plan, idx, with_times, with_yaw)
        assert np.array_equal(so, want[3]) and same_bits(co, want[0]) and same_bits(sr, want[2])
        assert (tm is None) == (not with_times) and (fy is None) == (not with_yaw)
        assert (tm is None or same_bits(tm, want[1])) and (fy is None or same_bits(fy, fy_in[idx]))
    assert eng.take_flags() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 2: bad inputs
def test_indices_out_of_range_are_clamped_and_flagged_and_invalid_arguments_refused(eng):
    import torch
    from uav_ac import _native as nat
    from uav_ac.scoring import take_parts
    k = case(eng)
    for plan in (k["uniform"], k["ragged"]):
        co_in, tm_in, sr_in, how, fy_in = host_parts(plan)
        eng.take_flags()
        so, co, tm, sr, fy = take_abi(eng, plan, np.array([-1, B, 2 ** 31 - 1, 5]))
        flags = eng.take_flags()
        assert flags[0] == 1 and flags[1:] == [0, 0, 0]
        clamped = np.array([0, B - 1, B - 1, 5])
        want = take_parts(co_in, tm_in, sr_in, how, clamped)
        assert np.array_equal(so, want[3]) and same_bits(co, want[0]) and same_bits(tm, want[1]) and same_bits(sr, want[2])
        assert same_bits(fy, fy_in[clamped])
    # Engine.take: a device tensor goes through unread (clamped, flagged), the same numbers on the host are refused
    plan = k["uniform"]
    got = eng.take(plan, torch.tensor([-1, B, 5], device=eng.device))
    assert eng.take_flags()[0] == 1 and torch.equal(got.coeffs.reshape(3, -1), plan.coeffs.reshape(B, -1)[[0, B - 1, 5]])
    for bad in ([-1, B, 5], [], np.zeros(B, dtype=bool), np.ones(B - 1, dtype=bool), [0.5]):
        with pytest.raises(ValueError):
            eng.take(plan, bad)
    # the header's EINVAL cases: nothing is enqueued, no flag is raised
    n = 4
    index = _i32(eng, [0, 1, 2, 3])
    so = torch.zeros((n + 1,), dtype=torch.int64, device=eng.device)
    for args in ((None, B, M, None, n, _p(so)), (None, B, M, _p(index), n, None), (None, 0, M, _p(index), n, _p(so)),
                 (None, B, M, _p(index), 0, _p(so)), (None, B, 0, _p(index), n, _p(so)), (None, B, nat.MAX_SEGMENTS + 1, _p(index), n, _p(so))):
        with pytest.raises(nat.UavacError) as exc:
            eng.ctx.call("uavac_minsnap_take_offsets_dev", *args)
        assert exc.value.code == nat.EINVAL
    eng.ctx.call("uavac_minsnap_take_offsets_dev", None, B, M, _p(index), n, _p(so))
    buf = torch.zeros((n * M * 24,), dtype=torch.float64, device=eng.device)
    ibuf = torch.zeros((n * M,), dtype=torch.int32, device=eng.device)
    co, tm, sr, fy = _p(plan.coeffs), _p(plan.times), _p(plan.seg_rows), _p(plan.first_yaw)
    ix, o, b, i = _p(index), _p(so), _p(buf), _p(ibuf)
    for args in ((None, tm, sr, None, B, M, fy, ix, n, o, b, b, i, b), (co, tm, None, None, B, M, fy, ix, n, o, b, b, i, b),
                 (co, tm, sr, None, B, M, fy, None, n, o, b, b, i, b), (co, tm, sr, None, B, M, fy, ix, n, None, b, b, i, b),
                 (co, tm, sr, None, B, M, fy, ix, n, o, None, b, i, b), (co, tm, sr, None, B, M, fy, ix, n, o, b, b, None, b),
                 (co, tm, sr, None, 0, M, fy, ix, n, o, b, b, i, b), (co, tm, sr, None, B, M, fy, ix, 0, o, b, b, i, b),
                 (co, tm, sr, None, B, 0, fy, ix, n, o, b, b, i, b), (co, tm, sr, None, B, nat.MAX_SEGMENTS + 1, fy, ix, n, o, b, b, i, b),
                 (co, None, sr, None, B, M, fy, ix, n, o, b, b, i, b), (co, tm, sr, None, B, M, fy, ix, n, o, b, None, i, b),
                 (co, tm, sr, None, B, M, None, ix, n, o, b, b, i, b), (co, tm, sr, None, B, M, fy, ix, n, o, b, b, i, None)):
        with pytest.raises(nat.UavacError) as exc:
            eng.ctx.call("uavac_minsnap_take_dev", *args)
        assert exc.value.code == nat.EINVAL
    torch.cuda.synchronize()
    assert not buf.any() and not ibuf.any() and eng.take_flags() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 3: the rows
@pytest.mark.parametrize("which", ["uniform", "ragged"])
def test_the_rows_of_a_taken_batch_are_the_rows_of_the_missions_it_took(eng, which):
    import torch
    from uav_ac.scoring import take_rows
    k = case(eng)
    plan = k[which]
    rowed = k["uniform"] if which == "uniform" else k["ragged_rows"]
    idx = INDEXES["n300"][:130]                                              # n > B, every mission, duplicates
    got = eng.take(plan, idx, rows=True)
    want, want_ro = take_rows(rowed.traj.cpu().numpy(), rowed.row_offsets.cpu().numpy(), idx)
    assert got.B == len(idx) and got.max_m == M and got.free_times and got.waypoints is None and got.velocity == VEL and got.dt == DT
    assert np.array_equal(got.row_offsets.cpu().numpy(), want_ro) and got.total_rows == int(want_ro[-1])
    assert np.array_equal(got.seg_offsets.cpu().numpy(), got.seg_offsets_host)
    traj = got.traj.cpu().numpy()
    for c in range(11):
        assert same_bits(traj[:, c], want[:, c]), c
    for i in (0, 57, len(idx) - 1):
        assert same_bits(got.mission(i), rowed.mission(int(idx[i])))
    at = torch.as_tensor(idx).to(eng.device)
    assert torch.equal(got.first_yaw, rowed.first_yaw[at]) and torch.equal(eng.first_yaw(got), rowed.first_yaw[at])
    assert torch.equal(got.status, plan.status[at]) and got.velocities is None
    assert torch.equal(got.start_positions, torch.as_tensor(np.stack([k["wps"][b][0] for b in idx])).to(eng.device))
    # a mask selects its True entries in ascending order; a device tensor of indices gives the same batch
    mask = np.zeros(B, dtype=bool)
    mask[[3, 64, 95]] = True
    a, b = eng.take(plan, torch.as_tensor(~mask).to(eng.device)), eng.take(plan, np.flatnonzero(~mask))
    assert a.B == B - 3 and torch.equal(a.coeffs, b.coeffs) and torch.equal(a.seg_rows, b.seg_rows) and torch.equal(a.times, b.times)
    assert torch.equal(a.row_offsets, b.row_offsets) and np.array_equal(a.seg_offsets_host, b.seg_offsets_host)
    # the plan itself is left as it is
    assert plan.B == B and (plan.traj is None) == (which == "ragged")
    assert eng.take_flags() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 4: the audits follow
def test_the_audits_of_a_taken_batch_follow_the_missions(eng):
    import torch
    k = case(eng)
    idx = np.array([95, 7, 7, 0, 40, 41, 13, 88, 2])
    at = torch.as_tensor(idx).to(eng.device)
    for plan in (k["uniform"], k["ragged"]):
        whole, part = eng.audit(plan, CUBOIDS), eng.audit(eng.take(plan, idx), CUBOIDS)
        assert same_bits(part.block.cpu().numpy(), whole.block[:, at].cpu().numpy())
        assert torch.equal(part.hit_rows, whole.hit_rows[:, at]) and torch.equal(part.first_hit, whole.first_hit[:, at])
        assert int(whole.hit_rows.sum()) > 0
        # a group taken alone is audited as inside its batch, the partners renumbered
        inside = eng.separation(plan, 0.5, 32)
        alone = eng.separation(eng.take(plan, np.arange(32, 64)), 0.5)
        assert same_bits(alone.min_distance.cpu().numpy(), inside.min_distance[32:64].cpu().numpy())
        want = inside.block[:, 32:64].clone()
        want[0] = torch.where(want[0] >= 0, want[0] - 32, want[0])
        assert torch.equal(alone.block, want)
    assert int(eng.separation(k["uniform"], 0.5, 32).conflicts[32:64].sum()) > 0          # (there is something to find in that group)


# ------------------------------------------------------------------------------------------------ 5: concat and put
def parts_equal(a, b):
    import torch
    return (torch.equal(a.coeffs.reshape(-1, 8, 3), b.coeffs.reshape(-1, 8, 3)) and torch.equal(a.times.reshape(-1), b.times.reshape(-1))
            and torch.equal(a.seg_rows.reshape(-1), b.seg_rows.reshape(-1)) and torch.equal(a.row_offsets, b.row_offsets)
            and torch.equal(a.first_yaw, b.first_yaw))


def test_concat_and_put(eng):
    import torch
    from uav_ac.scoring import take_rows
    k = case(eng)
    uniform, ragged = k["uniform"], k["ragged"]
    both = eng.concat([uniform, ragged])
    so_u = np.arange(B + 1) * M
    assert both.B == 2 * B and both.max_m == M and both.traj is None and both.velocity == VEL and both.velocities is None
    assert np.array_equal(both.seg_offsets_host, np.concatenate([so_u[:-1], ragged.seg_offsets_host + B * M]))
    assert np.array_equal(both.seg_offsets.cpu().numpy(), both.seg_offsets_host)
    assert torch.equal(both.coeffs, torch.cat([uniform.coeffs.reshape(-1, 8, 3), ragged.coeffs]))
    assert torch.equal(both.times, torch.cat([uniform.times.reshape(-1), ragged.times]))
    assert torch.equal(both.seg_rows, torch.cat([uniform.seg_rows.reshape(-1), ragged.seg_rows]))
    assert torch.equal(both.row_offsets, torch.cat([uniform.row_offsets, ragged.row_offsets[1:] + uniform.row_offsets[-1]]))
    assert torch.equal(both.first_yaw, torch.cat([uniform.first_yaw, ragged.first_yaw]))
    assert both.total_rows == uniform.total_rows + int(ragged.row_offsets[-1])
    with pytest.raises(ValueError):
        eng.concat([uniform, eng.plan(k["wps"][:2], VEL, 0.02, rows=False)])
    # put: the missions that the stagger leaves unresolved in groups of 32, re-planned slower
    idx = np.flatnonzero(eng.stagger(uniform, 0.5, 32).steps.cpu().numpy() == -1)
    assert len(idx) == 6
    other = eng.plan_ragged([k["wps"][b] for b in idx], 2.0, DT, rows=True)
    for index in (idx, torch.as_tensor(idx).to(eng.device), torch.as_tensor(np.isin(np.arange(B), idx)).to(eng.device)):
        out = eng.put(uniform, index, other, rows=True)
        assert out.B == B and out.max_m == M and np.isnan(out.velocity) and out.dt == DT
        assert out.velocities.cpu().numpy().tolist() == [2.0 if b in idx else VEL for b in range(B)]
        source = np.arange(B)
        source[idx] = B + np.arange(len(idx))
        co_u, tm_u, sr_u, _, fy_u = host_parts(uniform)
        co_o, tm_o, sr_o, so_o, fy_o = host_parts(other)
        co, tm, sr = out.coeffs.cpu().numpy(), out.times.cpu().numpy(), out.seg_rows.cpu().numpy()
        for b in range(B):
            s0, s1 = out.seg_offsets_host[b:b + 2]
            if b in idx:
                i = int(np.flatnonzero(idx == b)[0])
                o0, o1 = so_o[i:i + 2]
                want = co_o[o0:o1], tm_o[o0:o1], sr_o[o0:o1], fy_o[i]
            else:
                want = co_u[b * M:(b + 1) * M], tm_u[b * M:(b + 1) * M], sr_u[b * M:(b + 1) * M], fy_u[b]
            assert same_bits(co[s0:s1], want[0]) and same_bits(tm[s0:s1], want[1]) and same_bits(sr[s0:s1], want[2]), b
            assert same_bits(out.first_yaw[b:b + 1].cpu().numpy(), np.array([want[3]])), b
        rows_both = np.concatenate([uniform.traj.cpu().numpy(), other.traj.cpu().numpy()])
        ro_both = np.concatenate([uniform.row_offsets.cpu().numpy(), other.row_offsets.cpu().numpy()[1:] + uniform.total_rows])
        want_rows, want_ro = take_rows(rows_both, ro_both, source)
        assert np.array_equal(out.row_offsets.cpu().numpy(), want_ro)
        got_rows = out.traj.cpu().numpy()
        for c in range(11):
            assert same_bits(got_rows[:, c], want_rows[:, c]), c
    assert not same_bits(other.mission(0), uniform.mission(int(idx[0])))      # (the slower plan is another plan)
    # putting back what was taken gives the plan back
    for plan in (uniform, ragged):
        back = eng.put(plan, idx, eng.take(plan, idx))
        assert back.B == B and back.velocity == VEL and back.velocities is None and parts_equal(back, plan)
        assert np.array_equal(back.seg_offsets_host, so_u if plan is uniform else plan.seg_offsets_host)
    for bad, other_plan in (([1, 1, 2, 3, 4, 5], other), (idx[:-1], other), ([0, 1, 2, 3, 4, B], other)):
        with pytest.raises(ValueError):
            eng.put(uniform, bad, other_plan)
    assert eng.take_flags() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 6: flying it
def test_a_taken_batch_flies_plan_fed_as_row_fed_and_as_the_lanes_it_took(eng):
    import torch
    k = case(eng)
    ragged = k["ragged"]
    idx = INDEXES["n300"][:130]
    taken = eng.take(ragged, idx)
    assert taken.traj is None
    fed = eng.fleet(taken)
    rowed = eng.fleet(eng.take(ragged, idx, rows=True), from_plan=False)
    assert fed.from_plan and not rowed.from_plan
    K = 300
    slog, _ = fed.rollout(K, state_log=True)
    slog_r, _ = rowed.rollout(K, state_log=True)
    # (the vehicles' state is rows 0-25; rows 26-29 are the yaw scan that only a plan-fed fleet carries)
    assert torch.equal(fed.state[:26], rowed.state[:26]) and torch.equal(fed.istate, rowed.istate) and torch.equal(slog, slog_r)
    # the rollout's lanes are independent: the same flight as the lanes `idx` of the whole batch
    whole = eng.fleet(ragged)
    assert whole.from_plan
    slog_w, _ = whole.rollout(K, state_log=True)
    at = torch.as_tensor(idx).to(eng.device)
    assert torch.equal(slog, slog_w[:, :, at]) and torch.equal(fed.state, whole.state[:, at]) and torch.equal(fed.istate, whole.istate[:, at])
    assert bool(torch.isfinite(slog).all()) and eng.take_flags() == [0, 0, 0, 0]
