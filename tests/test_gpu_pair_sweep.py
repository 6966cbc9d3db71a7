"""The two sources of the pair sweep (csrc/pair_sweep.h) tied together through the contract they share: a PLAN walked on its groups'
clocks and a FLIGHT read from a state log give the same audit and the same conflict list, bit for bit, when the log holds exactly the
plan's sampled rows -- tick k of column b = mission b's row clamp(k - start_b, 0, n_b - 1), which is where the plan's clock puts it.

The batch: 192 missions of two segments (52 .. 70 rows each at velocity 3 and dt 0.05) in groups [0, 63, 127, 192] -- one tile less than
full, a full tile, one more than full; the second and third 64-mission windows each span two groups -- with start rows 0 .. 5.  The log
has K = max(start + rows) ticks at pitch 208; its rows 3 - 12 and its columns past the batch are NaN: they are never read.

Where the two clocks differ: a plan's group is compared up to ITS horizon, a log up to K for every group.  Past a group's horizon
everybody holds their last row, so the minimum (strict <, lowest row), the conflict bits, the first row inside and `compared` cannot
change, but a pair that is still inside when its group's horizon ends before K would go on counting ticks in the log (`last_row`,
`rows_inside`).  The radius 0.3 is chosen so that no pair does -- 46 entries, 42 missions with a conflict and 150 without, by the NumPy
rule on the oracle's rows --, and the test asserts that on the product's rows before it compares anything."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, M, VEL, DT, RADIUS, PITCH = 192, 2, 3.0, 0.05, 0.3, 208
GO = np.array([0, 63, 127, 192])


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    e = Engine("cuda:0")
    yield e
    e.ctx.set_option("separation_split", 0)
    e.ctx.set_option("conflict_slots", 0)


@pytest.fixture(scope="module")
def case(eng):
    """Computed once and left unchanged: the plan, its start rows, and the log of its sampled rows on the device."""
    import torch
    from oracle import minsnap_oracle as mo
    from uav_ac.scoring import conflicts_from_rows, separation_from_rows
    plan = eng.plan(mo.synthetic_missions(B, M), VEL, DT)
    rows, ro = plan.traj.cpu().numpy(), plan.row_offsets.cpu().numpy()
    n = np.diff(ro)
    assert 20 <= n.min() and n.max() <= 70, (n.min(), n.max())
    start = np.random.default_rng(20260807).integers(0, 6, B).astype(np.int32)
    K = int((start + n).max())
    log = np.full((K, 13, PITCH), np.nan)
    for b in range(B):
        at = np.clip(np.arange(K) - start[b], 0, n[b] - 1)
        log[:, 0:3, b] = rows[ro[b] + at, 0:3]
    # the NumPy rule on these rows: some missions have a conflict and some have none, and no pair is inside at the last row of a group
    # whose horizon ends before K (see the module's docstring)
    conf = separation_from_rows(rows, ro, RADIUS, GO, start)[1][2]
    assert (conf > 0).any() and (conf == 0).any(), (int((conf > 0).sum()), int((conf == 0).sum()))
    off, _, pi = conflicts_from_rows(rows, ro, RADIUS, GO, start)
    owner = np.repeat(np.arange(B), np.diff(off))
    horizon = np.array([(start + n)[GO[g]:GO[g + 1]].max() for g in range(len(GO) - 1)])[np.searchsorted(GO, owner, side="right") - 1]
    assert not ((pi[2] == horizon - 1) & (horizon < K)).any()
    dev = torch.as_tensor(log).to(eng.device)
    return dict(plan=plan, start=start, log=dev[:, :, :B], held=dev)


def audit_bytes(a):
    return a.min_distance.cpu().numpy().tobytes(), a.block.cpu().numpy().tobytes()


def list_bytes(c):
    return c.offsets.cpu().numpy().tobytes(), c.min_distance.cpu().numpy().tobytes(), c.block.cpu().numpy().tobytes()


def test_flown_audit_equals_plan_audit_at_every_split(eng, case):
    seen = []
    try:
        for split in (0, 1, 3):
            eng.ctx.set_option("separation_split", split)
            planned = eng.separation(case["plan"], RADIUS, GO, case["start"])
            flown = eng.flown_separation(case["log"], RADIUS, GO)
            for name in ("min_distance", "partner", "row", "conflicts", "first_conflict", "compared"):
                p, f = getattr(planned, name).cpu().numpy(), getattr(flown, name).cpu().numpy()
                assert p.dtype == f.dtype and np.array_equal(p, f), (split, name, np.flatnonzero(p != f)[:8])
            seen += [audit_bytes(planned), audit_bytes(flown)]
    finally:
        eng.ctx.set_option("separation_split", 0)
    assert all(s == seen[0] for s in seen)
    conflicts = planned.conflicts.cpu().numpy()
    assert (conflicts > 0).any() and (conflicts == 0).any() and (planned.compared.cpu().numpy() == np.repeat(np.diff(GO) - 1, np.diff(GO))).all()


def test_flown_list_equals_plan_list_at_every_shape(eng, case):
    seen = []
    try:
        for split, slots in ((0, 0), (0, 1), (1, 1), (3, 1)):
            eng.ctx.set_option("separation_split", split)
            eng.ctx.set_option("conflict_slots", slots)
            planned = eng.conflicts(case["plan"], RADIUS, GO, case["start"])
            flown = eng.flown_conflicts(case["log"], RADIUS, GO)
            assert planned.total == flown.total > 0, (split, slots, planned.total, flown.total)
            po, fo = planned.offsets.cpu().numpy(), flown.offsets.cpu().numpy()
            assert np.array_equal(po, fo), (split, slots, np.flatnonzero(po != fo)[:8])
            pb, fb = planned.block.cpu().numpy(), flown.block.cpu().numpy()
            assert np.array_equal(pb, fb), (split, slots, np.argwhere(pb != fb)[:8])
            seen += [list_bytes(planned), list_bytes(flown)]
    finally:
        eng.ctx.set_option("separation_split", 0)
        eng.ctx.set_option("conflict_slots", 0)
    assert all(s == seen[0] for s in seen)
