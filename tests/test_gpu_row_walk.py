"""The corners of the shared row walk (csrc/row_walk.h) for the three kernels built on it -- the plan audit, the plan demand and the
slowdown need (`uavac_minsnap_audit_dev`, `uavac_minsnap_demand_dev`, `uavac_minsnap_need_dev`) -- from ONE small ragged batch whose
row totals sit on both sides of both group widths: fewer rows than 16 lanes, between 16 and 64, more than 64, and two-segment missions
whose first segment ends before the 16th row, so that a lane's first row already lies in the second segment (the walk starts with no
segment loaded and seeks forward before its first load).

Everything is exact (no tolerance; floats by value, NaN equal to NaN), against the NumPy specifications on the product's own rows and
jerk: `audit_from_rows` of tests/test_gpu_plan_audit.py, `scoring.demand_from_rows`, `scoring.need_from_rows`.  At 16 and at 64 lanes
per mission; as one call, as five calls of one mission, and split 2 + 3; with two cuboids and with none; into sentinel-padded outputs
(the _abi helpers of the three kernels' own test files).
"""
import numpy as np
import pytest

from test_gpu_demand import G, NAMES, demand_abi
from test_gpu_need import need_abi
from test_gpu_plan_audit import audit_abi, audit_from_rows

pytestmark = pytest.mark.gpu

VEL, DT = 3.0, 0.01                                          # a first / last segment of length d has ceil(1.5 d / (VEL DT)) = ~50 d rows
MISSIONS = (
    np.array([[1.0, 1.0, -3.0], [1.12, 1.16, -3.0]]),                                   # 0.2 m: ~10 rows
    np.array([[2.0, 1.0, -3.0], [2.6, 1.5, -3.2]]),                                     # 0.81 m: ~41 rows
    np.array([[3.0, 2.0, -3.0], [4.2, 2.9, -3.1], [5.0, 3.6, -2.8]]),                   # 1.50 m + 1.10 m: ~76 + ~56 rows
    np.array([[6.0, 3.0, -3.0], [6.1, 3.14, -3.02], [7.7, 4.3, -3.3]]),                 # 0.17 m + 2.00 m: ~9 + ~100 rows
    np.array([[8.0, 5.0, -3.0], [8.06, 5.08, -3.0], [8.4, 5.4, -3.1]]),                 # 0.10 m + 0.48 m: ~5 + ~24 rows
)
CUBS = np.array([[3.5, 4.5, 2.3, 3.2, -3.5, -2.5],           # mission 2 passes through it
                 [7.0, 9.0, 3.9, 5.5, -3.4, -2.9]])          # mission 3 ends in it, mission 4 starts in it
SPLITS = ((0, 5), (0, 1, 2, 3, 4, 5), (0, 2, 5))             # one call; five calls of B = 1; 2 + 3


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    e = Engine("cuda:0")
    e.take_flags()
    yield e
    e.ctx.set_option("audit_lanes", 16)


@pytest.fixture(scope="module")
def batch(eng):
    """Computed once and left unchanged: the rows-free ragged batch, its rows and jerk on the host, and what NumPy makes of them."""
    from uav_ac.scoring import demand_from_rows, need_from_rows
    free = eng.plan_ragged(MISSIONS, VEL, DT, rows=False)
    sampled = eng.sample_rows(eng.plan_ragged(MISSIONS, VEL, DT, rows=False))
    rows, ro = sampled.traj.cpu().numpy(), sampled.row_offsets.cpu().numpy()
    jerk = []
    for b, w in enumerate(MISSIONS):                         # the jerk sampler takes uniform plans: mission b alone has the same rows
        alone = eng.plan(w[None], VEL, DT)
        assert np.array_equal(alone.traj.cpu().numpy(), rows[ro[b]:ro[b + 1]]), b
        jerk.append(eng.sample_derivatives(alone)[0].cpu().numpy())
    jerk = np.concatenate(jerk)
    assert free.traj is None and eng.take_flags() == [0, 0, 0, 0]

    def demand_spec(cubs):
        d = demand_from_rows(rows, jerk, ro, G, cubs)
        return tuple(d[k] for k in NAMES)
    want = {"audit": {2: audit_from_rows(rows, ro, CUBS), 0: audit_from_rows(rows, ro, None)},
            "demand": {2: demand_spec(CUBS), 0: demand_spec(None)}, "need": need_from_rows(rows, ro, None)}
    return dict(free=free, ro=ro, seg_rows=free.seg_rows.cpu().numpy(), so=np.asarray(free.seg_offsets_host), want=want)


def same(got, want):
    return all(g.shape == w.shape and np.array_equal(g, w, equal_nan=g.dtype.kind == "f") for g, w in zip(got, want))


def in_calls(eng, free, cuts, one_call):
    """`one_call(coeffs, seg_rows, seg_offsets, B, m)` -> arrays (rows, B), once per run of missions cuts[i] .. cuts[i + 1], joined."""
    import torch
    so, got = free.seg_offsets_host, []
    for b0, b1 in zip(cuts[:-1], cuts[1:]):
        part = torch.as_tensor(so[b0:b1 + 1] - so[b0]).to(eng.device)
        got.append(one_call(free.coeffs[int(so[b0]):], free.seg_rows[int(so[b0]):], part, b1 - b0, free.max_m))
    return tuple(np.concatenate(x, axis=1) for x in zip(*got))


def test_the_batch_has_the_corners(batch):
    total, seg_rows, so = np.diff(batch["ro"]), batch["seg_rows"], batch["so"]
    segments = np.diff(so)
    assert segments.tolist() == [1, 1, 2, 2, 2]
    assert all(int(seg_rows[so[b]:so[b + 1]].sum()) == int(total[b]) for b in range(5))
    assert 0 < total[0] < 16 and 17 <= total[1] <= 63 and total[2] > 64 and total[3] > 64 and 17 <= total[4] <= 63
    first = seg_rows[so[:-1]]
    assert 16 < first[2] and 0 < first[3] < 16 and 0 < first[4] < 16           # a lane of 16 starts in the second segment of missions 3 and 4
    a, d = batch["want"]["audit"][2], batch["want"]["demand"][2]
    assert np.isfinite(a[0]).all() and np.isfinite(d[0]).all() and np.isfinite(batch["want"]["need"]).all()
    hit = a[1] > 0
    assert hit.tolist() == [[False, False, True, False, False], [False, False, False, True, True]]
    assert a[2][1, 4] == 0 and a[2][1, 3] > first[3]          # mission 4 starts inside; mission 3 enters in its second segment
    assert np.array_equal(d[2] == 0.0, hit)


@pytest.mark.parametrize("lanes", (16, 64))
def test_audit_demand_and_need_equal_numpy_on_the_rows_whole_alone_and_split(eng, batch, lanes):
    free, want = batch["free"], batch["want"]
    eng.ctx.set_option("audit_lanes", lanes)
    try:
        for cuts in SPLITS:
            for n, cubs in ((2, CUBS), (0, None)):
                got = in_calls(eng, free, cuts, lambda c, s, o, B, m: audit_abi(eng, c, s, o, B, m, DT, cubs))
                assert same(got, want["audit"][n]), ("audit", lanes, cuts, n)
                got = in_calls(eng, free, cuts, lambda c, s, o, B, m: demand_abi(eng, c, s, o, B, m, DT, cubs))
                assert same(got, want["demand"][n]), ("demand", lanes, cuts, n)
            got = in_calls(eng, free, cuts, lambda c, s, o, B, m: (need_abi(eng, c, s, o, B, m),))
            assert same(got, (want["need"],)), ("need", lanes, cuts)
    finally:
        eng.ctx.set_option("audit_lanes", 16)
    assert eng.take_flags() == [0, 0, 0, 0]
