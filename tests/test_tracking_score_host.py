"""Host side of the per-UAV tracking scores (no GPU): uav_ac.scoring on hand-made score / istate blocks, and the score layout the
Python binding and include/uavac.h agree on."""
import math
import os
import re

import numpy as np
import pytest

from conftest import REPO


def _block(rows):
    """score [SCORE_ROWS][B] from a list of per-UAV (count, next_row, sum, sumsq, max, last) tuples (rows 6-10 left 0)."""
    import torch
    from uav_ac import _native as nat
    s = torch.zeros((nat.SCORE_ROWS, len(rows)), dtype=torch.float64)
    for b, r in enumerate(rows):
        s[:6, b] = torch.tensor(r, dtype=torch.float64)
    return s


def test_score_rows_match_the_header():
    from uav_ac import _native as nat
    text = open(os.path.join(REPO, "include", "uavac.h")).read()
    assert int(re.search(r"#define UAVAC_SCORE_ROWS (\d+)", text).group(1)) == nat.SCORE_ROWS == 11
    for name in ("uavac_control_rollout_scored_dev", "uavac_control_rollout_plan_scored_dev",
                 "uavac_control_rollout_plan_ragged_scored_dev"):
        assert name in nat.exported_symbols()
        assert re.search(r"\b" + name + r"\s*\(", text)


def test_summarize_complete_incomplete_and_fresh():
    import torch
    from uav_ac.scoring import summarize
    # UAV 0: 4 rows, all scored (errors 0.1 0.2 0.3 0.4); UAV 1: 3 of 5 rows scored; UAV 2: fresh; UAV 3: no rows at all
    e0 = [0.1, 0.2, 0.3, 0.4]
    e1 = [0.5, 0.25, 1.0]
    score = _block([(4, 4, sum(e0), sum(x * x for x in e0), max(e0), e0[-1]),
                    (3, 3, sum(e1), sum(x * x for x in e1), max(e1), e1[-1]),
                    (0, 0, 0, 0, 0, 0),
                    (0, 0, 0, 0, 0, 0)])
    istate = torch.zeros((4, 4), dtype=torch.int32)
    out = summarize(score, istate, torch.tensor([4, 5, 7, 0]))
    assert out["rows_scored"].tolist() == [4, 3, 0, 0]
    assert out["complete"].tolist() == [True, False, False, False]
    assert math.isclose(float(out["mean_error"][0]), np.mean(e0), rel_tol=1e-15)
    assert math.isclose(float(out["rms_error"][0]), math.sqrt(np.mean(np.square(e0))), rel_tol=1e-15)
    assert float(out["max_error"][0]) == 0.4 and float(out["final_error"][0]) == 0.4
    assert math.isclose(float(out["mean_error"][1]), np.mean(e1), rel_tol=1e-15)
    assert float(out["max_error"][1]) == 1.0
    assert math.isnan(float(out["final_error"][1]))          # not complete: no final error
    for k in ("mean_error", "rms_error", "max_error", "final_error"):
        assert math.isnan(float(out[k][2])) and math.isnan(float(out[k][3]))
    assert not bool(out["collided"].any())


def test_collisions_obstacle_flag_and_ground_bit():
    import torch
    from uav_ac import _native as nat
    from uav_ac.scoring import acceptance, summarize
    B = 5
    score = _block([(3, 3, 0.3, 0.03, 0.1, 0.1)] * B)
    istate = torch.zeros((nat.ISTATE_ROWS, B), dtype=torch.int32)
    istate[2, 1] = 1                                                  # obstacle hit (sticky flag)
    istate[3, 2] = nat.GROUND_HIT_AFTER_TAKEOFF                       # ground contact after take-off: bit 4
    istate[3, 3] = nat.GROUND_IN_CONTACT | nat.GROUND_TAKEN_OFF       # resting / airborne bookkeeping: no collision
    istate[3, 4] = nat.GROUND_TAKEN_OFF | nat.GROUND_HIT_AFTER_TAKEOFF
    s = summarize(score, istate, torch.full((B,), 3))
    assert s["collided"].tolist() == [False, True, True, False, True]
    a = acceptance(s)
    assert a["passed"].tolist() == [True, False, False, True, False]
    assert a["mean_ok"].all() and a["final_ok"].all()


def test_acceptance_tolerances_and_nan():
    import torch
    from uav_ac.scoring import acceptance, summarize
    score = _block([(2, 2, 0.8, 0.5, 0.6, 0.6),      # mean 0.4, final 0.6: mean passes, final fails at 0.5
                    (2, 2, 1.2, 0.8, 0.7, 0.3),      # mean 0.6, final 0.3
                    (1, 1, 0.1, 0.01, 0.1, 0.1)])    # incomplete (2 rows): NaN final -> fails
    s = summarize(score, torch.zeros((4, 3), dtype=torch.int32), torch.tensor([2, 2, 2]))
    a = acceptance(s)
    assert a["mean_ok"].tolist() == [True, False, True]
    assert a["final_ok"].tolist() == [False, True, False]
    assert a["passed"].tolist() == [False, False, False]
    a = acceptance(s, mean_tol=1.0, final_tol=1.0)
    assert a["passed"].tolist() == [True, True, False]


def test_summarize_refuses_bad_shapes():
    import torch
    from uav_ac.scoring import summarize
    with pytest.raises(ValueError):
        summarize(torch.zeros((6, 3), dtype=torch.float64), torch.zeros((4, 3), dtype=torch.int32), torch.ones(3))
    with pytest.raises(ValueError):
        summarize(torch.zeros((11, 3), dtype=torch.float64), torch.zeros((4, 2), dtype=torch.int32), torch.ones(3))
    with pytest.raises(ValueError):
        summarize(torch.zeros((11, 3), dtype=torch.float64), torch.zeros((4, 3), dtype=torch.int32), torch.ones(2))


def test_scored_row_fed_kernels_pass_the_row_prefetch_check():
    """The scored twins' row prefetch is checked like the unscored kernels' (uav_ac/_buildcheck.py): 8 row-fed variants."""
    from conftest import PKG
    from uav_ac import _buildcheck
    if not os.path.exists(os.path.join(PKG, "build", "control_rollout.o")):
        pytest.skip("no object files here (library built elsewhere)")
    assert _buildcheck.check_row_prefetch(scored=True) == 8
    assert _buildcheck.check_row_prefetch() == 16
    names = [n for n, _, _ in _buildcheck.check_rollout_registers()]
    assert sum("scored_control_rollout_kernel" in n for n in names) == 50
