"""What a per-mission plan kernel makes of a ragged batch whose segment offsets are malformed (csrc/mission_walk.h `mission_of`): a
mission that claims n segments is the clamp(n, 1, max_m) segments from seg_offsets[b] on, whatever n is.  Checked on the three kernels
that walk a mission with a group of lanes -- `uavac_minsnap_audit_dev`, `uavac_minsnap_first_yaw_dev`, `uavac_minsnap_cost_dev` --
through the C ABI: every mission's outputs equal, bit for bit, the outputs of the same call on that mission ALONE, a uniform batch of one
mission of clamp(n, 1, max_m) segments that starts at seg_offsets[b].

The malformed missions (one claims 0 segments, one max_m + 2) sit in the middle of the batch with real segments behind them, so every
address even an unclamped kernel would read lies inside the buffers: a wrong clamp shows as a wrong value and cannot fault."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_M, DT = 4, 0.01
CLAIMED = (3, 0, 4, MAX_M + 2, 2, 4)                         # segments per mission as the offsets state them
CUBS = np.array([[-0.5, 0.5, -9.0, 9.0, -9.0, 9.0], [0.0, 9.0, 0.0, 9.0, -9.0, 9.0]])


def _p(t):
    return C.c_void_p(t.data_ptr())


def bits(a):
    return a.view(np.int64) if a.dtype.kind == "f" else a


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    e = Engine("cuda:0")
    yield e
    e.ctx.set_option("audit_lanes", 16)


@pytest.fixture(scope="module")
def batch(eng):
    import torch
    rng = np.random.default_rng(20261019)
    so = np.concatenate([[0], np.cumsum(CLAIMED)]).astype(np.int64)
    S = int(so[-1])
    on = lambda a: torch.as_tensor(a).to(eng.device)         # noqa: E731
    return dict(so=so, coeffs=on(rng.uniform(-1.0, 1.0, (S, 24))), seg_rows=on(rng.integers(3, 40, S).astype(np.int32)),
                times=on(rng.uniform(0.5, 2.0, S)), seg_offsets=on(so), cubs=on(CUBS))


def calls(eng, k, B, m, first, seg_offsets):
    """The three calls on B missions of (at most) m segments from segment `first` on -> audit (8, B), hits (2, B), first hit (2, B),
    first_yaw (B,), cost (B,) as NumPy."""
    import torch
    dev = dict(device=eng.device)
    audit = torch.full((8, B), -1.0, dtype=torch.float64, **dev)
    hits, first_hit = torch.full((2, B), -7, dtype=torch.int32, **dev), torch.full((2, B), -7, dtype=torch.int32, **dev)
    yaw, cost = torch.full((B,), -1.0, dtype=torch.float64, **dev), torch.full((B,), -1.0, dtype=torch.float64, **dev)
    co, rows, times = k["coeffs"][first:], k["seg_rows"][first:], k["times"][first:]
    so = None if seg_offsets is None else _p(seg_offsets)
    eng._bind_stream()
    eng.ctx.call("uavac_minsnap_audit_dev", _p(co), _p(rows), so, B, m, DT, _p(k["cubs"]), 2, _p(audit), _p(hits), _p(first_hit))
    eng.ctx.call("uavac_minsnap_first_yaw_dev", _p(co), _p(rows), so, B, m, DT, _p(yaw))
    eng.ctx.call("uavac_minsnap_cost_dev", _p(co), _p(times), so, B, m, _p(cost))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (audit, hits, first_hit, yaw, cost)]


@pytest.mark.parametrize("lanes", (16, 64))
def test_a_malformed_mission_is_its_clamped_segments_alone(eng, batch, lanes):
    eng.ctx.set_option("audit_lanes", lanes)
    B, so = len(CLAIMED), batch["so"]
    whole = calls(eng, batch, B, MAX_M, 0, batch["seg_offsets"])
    seg_rows = batch["seg_rows"].cpu().numpy()
    for b, n in enumerate(CLAIMED):
        m = min(max(n, 1), MAX_M)
        alone = calls(eng, batch, 1, m, int(so[b]), None)
        for name, got, want in zip(("audit", "hit_rows", "first_hit", "first_yaw", "cost"), whole, alone):
            assert np.array_equal(bits(got[..., b]), bits(want[..., 0])), (name, b, got[..., b], want[..., 0])
        assert whole[0][0, b] == seg_rows[so[b]:so[b] + m].sum()                       # the rows of the clamped segments, no others
    assert np.isfinite(whole[0]).all() and np.isfinite(whole[4]).all() and (whole[4] > 0).all()
    assert (whole[1] > 0).any() and (whole[3] != 0).all()                              # somebody is inside a cuboid, everybody has a heading
