"""Per-UAV tracking scores of a scored rollout, read back and judged the way upstream's acceptance test does.

The scored rollouts (`Fleet.rollout(K, score=True)`, include/uavac.h uavac_control_rollout_scored_dev) accumulate, per UAV, over
the periods of `inner_per_outer` ticks that start with an outer update: how many of the mission's rows were scored, the next
row to score, the sum, sum of squares, maximum and last of e = |position - target row xyz| at the end of each period.  Upstream
checks one UAV from a full log (tests/integration/test_mujoco_trajectory_tracking.py:26-36): mean tracking error < 0.5 m, final
distance to the goal < 0.5 m, no collision.  `summarize` turns a score block into those quantities for every UAV at once and
`acceptance` applies upstream's three assertions.  Pure torch: works on device and on CPU tensors alike.
"""
from __future__ import annotations

from . import _native as nat

# score rows (include/uavac.h): callers read 0-5; 6-10 carry a period a launch ended inside of
COUNT, NEXT_ROW, SUM, SUMSQ, MAX, LAST = range(6)


def summarize(score, istate, nrows) -> dict:
    """score [SCORE_ROWS][B] f64, istate [ISTATE_ROWS][B] i32, nrows (B,) rows per mission -> dict of (B,) tensors:
    rows_scored, complete (next_row == nrows), mean_error, rms_error, max_error (NaN where nothing was scored), final_error
    (the last period's error once complete, NaN before), collided (the sticky obstacle flag, or a ground contact after take-off,
    as uav_ac.main.fly_mission counts it)."""
    import torch
    if score.dim() != 2 or score.shape[0] != nat.SCORE_ROWS:
        raise ValueError(f"score must be [{nat.SCORE_ROWS}][B], got {tuple(score.shape)}")
    B = score.shape[1]
    if istate.shape[-1] != B:
        raise ValueError("istate and score hold different batch sizes")
    s = score.to(torch.float64)
    nrows = torch.as_tensor(nrows, device=s.device).to(torch.float64).reshape(-1)
    if nrows.numel() != B:
        raise ValueError("one row count per UAV")
    count = s[COUNT]
    nan = torch.full_like(count, float("nan"))
    scored = count > 0
    safe = torch.where(scored, count, torch.ones_like(count))
    complete = (s[NEXT_ROW] == nrows) & (nrows > 0)
    ist = istate.to(s.device)
    collided = (ist[2] != 0) | ((ist[3] & nat.GROUND_HIT_AFTER_TAKEOFF) != 0)
    return {
        "rows_scored": count.to(torch.int64),
        "complete": complete,
        "mean_error": torch.where(scored, s[SUM] / safe, nan),
        "rms_error": torch.where(scored, torch.sqrt(s[SUMSQ] / safe), nan),
        "max_error": torch.where(scored, s[MAX], nan),
        "final_error": torch.where(complete, s[LAST], nan),
        "collided": collided,
    }


def acceptance(summary: dict, mean_tol: float = 0.5, final_tol: float = 0.5) -> dict:
    """Upstream's three assertions per UAV (test_mujoco_trajectory_tracking.py:26-36) -> dict of (B,) bool tensors:
    mean_ok (mean tracking error < mean_tol), final_ok (complete and final distance < final_tol), no_collision, and passed
    (all three).  A NaN error fails its assertion."""
    mean_ok = summary["mean_error"] < mean_tol
    final_ok = summary["complete"] & (summary["final_error"] < final_tol)
    no_collision = ~summary["collided"]
    return {"mean_ok": mean_ok, "final_ok": final_ok, "no_collision": no_collision, "passed": mean_ok & final_ok & no_collision}
