"""`uav_ac.plans`, the part that needs no GPU: the one view of a plan's segments (`segments`) on a uniform Plan and on a ragged batch, and
`Engine.concat` of the two on CPU tensors -- plumbing only when both parts carry their first headings, so no kernel runs -- against the
NumPy concatenation of their arrays, exactly."""
import numpy as np

COUNTS = (1, 4, 2)


def cpu_engine():
    import torch
    from uav_ac.engine import Engine
    eng = object.__new__(Engine)                             # (no context: concat of parts with first headings needs the device and torch only)
    eng._torch, eng.device = torch, torch.device("cpu")
    return eng


def arrays(S, B, rng):
    """Per-segment and per-mission arrays of a plan of S segments in B missions, hand-made: (coeffs (S, 8, 3), times (S,), seg_rows (S,),
    first_yaw (B,), status (B,))."""
    return (rng.standard_normal((S, 8, 3)), rng.uniform(0.5, 2.0, S), rng.integers(1, 9, S).astype(np.int32),
            rng.uniform(-3.0, 3.0, B), rng.integers(0, 2, B).astype(np.int32))


def row_offsets(seg_rows, so):
    return np.concatenate([[0], np.cumsum([seg_rows[so[b]:so[b + 1]].sum() for b in range(len(so) - 1)])]).astype(np.int64)


def uniform_plan():
    """A uniform Plan, B = 2, m = 3, one cruise speed, with first headings."""
    import torch
    from uav_ac.plans import Plan
    co, tm, sr, fy, st = arrays(6, 2, np.random.default_rng(1))
    ro = row_offsets(sr, np.arange(3) * 3)
    plan = Plan(2, 3, 3.0, 0.05, waypoints=None, times=torch.as_tensor(tm.reshape(2, 3)), seg_rows=torch.as_tensor(sr.reshape(2, 3)),
                row_offsets=torch.as_tensor(ro), coeffs=torch.as_tensor(co.reshape(2, 24, 3)), status=torch.as_tensor(st), traj=None,
                total_rows=int(ro[-1]), first_yaw=torch.as_tensor(fy))
    return plan, dict(coeffs=co, times=tm, seg_rows=sr, row_offsets=ro, first_yaw=fy, status=st)


def ragged_batch():
    """A RaggedBatch with COUNTS segments, one cruise speed per mission, with first headings."""
    import torch
    from uav_ac.plans import RaggedBatch
    so = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64)
    co, tm, sr, fy, st = arrays(7, 3, np.random.default_rng(2))
    ro = row_offsets(sr, so)
    vel = np.array([1.5, 2.5, 3.5])
    batch = RaggedBatch(3, 4, float("nan"), 0.05, seg_offsets=torch.as_tensor(so), seg_offsets_host=so, waypoints=None,
                        times=torch.as_tensor(tm), seg_rows=torch.as_tensor(sr), row_offsets=torch.as_tensor(ro), coeffs=torch.as_tensor(co),
                        status=torch.as_tensor(st), traj=None, total_rows=int(ro[-1]), first_yaw=torch.as_tensor(fy),
                        velocities=torch.as_tensor(vel))
    return batch, dict(coeffs=co, times=tm, seg_rows=sr, row_offsets=ro, first_yaw=fy, status=st, seg_offsets=so, velocities=vel)


def test_segments_of_a_uniform_plan():
    from uav_ac.plans import Segments, segments
    plan, _ = uniform_plan()
    s = segments(plan)
    assert isinstance(s, Segments) and s._fields == ("ragged", "B", "m", "S", "so", "so_host")
    assert s.ragged is False and s.so is None and (s.B, s.m, s.S) == (2, 3, 6)
    assert s.so_host.dtype == np.int64 and np.array_equal(s.so_host, np.arange(3) * 3)
    assert not hasattr(plan, "seg_offsets")                  # (how the fleet and the tests tell the two kinds apart)


def test_segments_of_a_ragged_batch():
    from uav_ac.plans import segments
    batch, parts = ragged_batch()
    s = segments(batch)
    assert s.ragged is True and (s.B, s.m, s.S) == (3, 4, 7)
    assert s.so is batch.seg_offsets and s.so_host is batch.seg_offsets_host and np.array_equal(s.so_host, parts["seg_offsets"])


def test_concat_of_a_uniform_plan_and_a_ragged_batch_is_the_numpy_concatenation():
    import torch
    from uav_ac.plans import RaggedBatch
    eng = cpu_engine()
    (plan, a), (batch, b) = uniform_plan(), ragged_batch()
    c = eng.concat([plan, batch])
    assert isinstance(c, RaggedBatch) and c.B == 5 and c.max_m == 4 and c.dt == 0.05
    assert c.free_times is True and c.waypoints is None and c.traj is None and c.hit is None
    for name in ("coeffs", "times", "seg_rows", "first_yaw", "status"):
        got, want = getattr(c, name).numpy(), np.concatenate([a[name], b[name]])
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), name
    so = np.concatenate([np.arange(3) * 3, b["seg_offsets"][1:] + 6])                        # the ragged part's offsets, moved up by 6
    assert c.seg_offsets.dtype == torch.int64 and np.array_equal(c.seg_offsets.numpy(), so)
    assert c.seg_offsets_host.dtype == np.int64 and np.array_equal(c.seg_offsets_host, so)
    assert np.array_equal(c.row_offsets.numpy(), np.concatenate([a["row_offsets"], b["row_offsets"][1:] + a["row_offsets"][-1]]))
    assert c.total_rows == int(a["row_offsets"][-1] + b["row_offsets"][-1])
    # one part has a speed per mission: no common speed, and the part that had one scalar gets it filled in
    assert np.isnan(c.velocity) and np.array_equal(c.velocities.numpy(), np.concatenate([[3.0, 3.0], b["velocities"]]))
    # the parts are left as they are
    assert plan.velocity == 3.0 and plan.velocities is None and not hasattr(plan, "seg_offsets")
    assert np.array_equal(batch.seg_offsets_host, b["seg_offsets"]) and np.array_equal(batch.seg_offsets.numpy(), b["seg_offsets"])
