"""What the C ABI refuses, and with which code and text: one table of (entry point, the one defect among otherwise valid arguments,
return code, `uavac_last_error`).  It covers the refusals that csrc/uavac_api.hip words once for several entry points -- the dt and
velocity checks, the n_cuboids range, the pair / layer / flown-pair argument sets, the take and delay shapes, the forms of the plan-fed
rollout -- and every option of `uavac_set_option`.  Every defect (a null, a zero, a negative, a NaN) is refused before the first launch.

Valid arguments are real device buffers: a uniform plan at B = 3, m = 2 (made by `uavac_minsnap_plan_dev`), the same waypoints as a ragged
batch of 1, 2 and 2 segments, a state log of K = 2 ticks, G = 2 groups with group_offsets = [0, 1, 3], one cuboid.  SIG gives every entry
point's parameters in order as `name` or `name=key`: the valid value is the fixture's buffer or number of that key, and a row of TABLE
replaces one parameter by name.  ("option:NAME" in a row sets that option for the call and puts it back to 0 after it.)

The test ends with one valid plan on the ctx that took all the refusals and compares its coefficients, bit for bit, with a fresh ctx's:
the refusals left nothing behind.  The options' accepted values are their start values for the same reason."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, EINVAL, ENONFINITE = 0, -1, -2
NAN = float("nan")
B, M, K = 3, 2, 2
VEL, DT, CAP = 2.0, 0.05, 4096

PLAN = "coeffs seg_rows seg_offsets=none B m dt"
PAIR = PLAN + " group_offsets G start_rows radius"
FLOWN = "state_log K B pitch group_offsets G radius"
ROLL = "state istate B K state_log=roll_log cmd_log=none aabbs=none n_obs"
SIG = {
    "uavac_minsnap_row_counts_dev": "wp B m velocity dt times seg_rows row_offsets",
    "uavac_minsnap_row_counts_ragged_dev": "wp=wp_r seg_offsets B m velocity dt times=times_r seg_rows=seg_rows_r row_offsets=row_offsets_r",
    "uavac_minsnap_plan_dev": "wp B m velocity dt times seg_rows row_offsets coeffs status traj cap yaw first_yaw",
    "uavac_minsnap_obstacle_round_dev": "wp=wp_r seg_offsets B m velocity dt aabb=cuboids active overflow touched wp_out "
                                        "seg_offsets_out counters times=times_r seg_rows=seg_rows_r row_offsets=row_offsets_r "
                                        "coeffs=coeffs_r hit",
    "uavac_minsnap_row_counts_v_dev": "wp B m velocities dt times seg_rows row_offsets",
    "uavac_minsnap_row_counts_ragged_v_dev": "wp=wp_r seg_offsets B m velocities dt times=times_r seg_rows=seg_rows_r "
                                             "row_offsets=row_offsets_r",
    "uavac_minsnap_plan_v_dev": "wp B m velocities dt times seg_rows row_offsets coeffs status traj cap yaw first_yaw",
    "uavac_minsnap_plan_bc_dev": "wp B m velocities dt bc times seg_rows row_offsets coeffs status traj cap yaw first_yaw",
    "uavac_minsnap_retime_dev": "wp seg_offsets=none B m velocities dt limits margin max_passes times seg_rows row_offsets coeffs status "
                                "first_yaw audit factors_total converged passes",
    "uavac_minsnap_row_counts_t_dev": "times seg_offsets=none B m dt seg_rows row_offsets",
    "uavac_minsnap_plan_t_dev": "wp seg_offsets=none B m times dt seg_rows row_offsets coeffs status traj cap yaw first_yaw",
    "uavac_minsnap_sample_dev": "coeffs times seg_rows row_offsets B m dt traj",
    "uavac_minsnap_sample_yaw_dev": "coeffs times seg_rows row_offsets B m dt traj yaw",
    "uavac_minsnap_sample_hits_dev": "coeffs times seg_rows row_offsets B m dt traj aabb=cuboids hit",
    "uavac_minsnap_sample_derivs_dev": "coeffs seg_rows row_offsets B m dt traj yaw first_yaw jerk snap",
    "uavac_minsnap_sample_capped_dev": "coeffs seg_rows row_offsets B m dt traj cap yaw first_yaw",
    "uavac_minsnap_sample_ragged_dev": "coeffs=coeffs_r seg_rows=seg_rows_r seg_offsets row_offsets=row_offsets_r B m total_segments dt traj "
                                       "cap aabb=none hit=none first_yaw",
    "uavac_minsnap_sample": "coeffs=coeffs_h times=times_h B m dt row_offsets=row_offsets_h traj=traj_h",
    "uavac_minsnap_first_yaw_dev": PLAN + " first_yaw",
    "uavac_minsnap_audit_dev": PLAN + " cuboids n_cuboids audit hit_rows first_hit",
    "uavac_minsnap_separation_dev": PAIR + " sep isep",
    "uavac_minsnap_conflict_offsets_dev": PAIR + " pair_offsets",
    "uavac_minsnap_conflicts_dev": PAIR + " pair_offsets capacity pair_d pair_i",
    "uavac_minsnap_stagger_dev": PAIR + " step max_steps istag",
    "uavac_minsnap_layer_dev": PAIR + " delta_x delta_y delta_z max_steps ilayer offsets",
    "uavac_minsnap_layer_obs_dev": PAIR + " delta_x delta_y delta_z max_steps cuboids n_cuboids ilayer offsets",
    "uavac_minsnap_delay_offsets_dev": "seg_offsets=none B m start_rows out_seg_offsets",
    "uavac_minsnap_delay_dev": "coeffs times seg_rows seg_offsets=none B m dt start_rows out_seg_offsets out_coeffs out_times out_seg_rows",
    "uavac_minsnap_take_offsets_dev": "seg_offsets=none B m index n out_seg_offsets",
    "uavac_minsnap_take_dev": "coeffs times seg_rows seg_offsets=none B m first_yaw index n out_seg_offsets out_coeffs out_times out_seg_rows "
                              "out_first_yaw",
    "uavac_flown_separation_dev": FLOWN + " sep isep",
    "uavac_flown_conflict_offsets_dev": FLOWN + " pair_offsets",
    "uavac_flown_conflicts_dev": FLOWN + " pair_offsets capacity pair_d pair_i",
    "uavac_flown_audit_dev": "state_log K B pitch cuboids n_cuboids audit first_bad hit_ticks first_hit clearance clearance_tick",
    "uavac_control_rollout_dev": "V traj row_offsets " + ROLL,
    "uavac_control_rollout_scored_dev": "V traj row_offsets " + ROLL + " score",
    "uavac_control_rollout_plan_dev": "V coeffs seg_rows row_offsets yaw first_yaw m dt " + ROLL,
    "uavac_control_rollout_plan_scored_dev": "V coeffs seg_rows row_offsets yaw first_yaw m dt " + ROLL + " score",
    "uavac_control_rollout_plan_ragged_dev": "V coeffs=coeffs_r seg_rows=seg_rows_r seg_offsets row_offsets=row_offsets_r first_yaw m dt " + ROLL,
    "uavac_control_rollout_plan_ragged_scored_dev": "V coeffs=coeffs_r seg_rows=seg_rows_r seg_offsets row_offsets=row_offsets_r first_yaw m dt "
                                                    + ROLL + " score",
    "uavac_set_option": "name value",
}

DT_ONE = "dt must be finite and > 0"
NULL = "null pointer"
N_CUB = "n_cuboids must be in [0, UAVAC_AUDIT_MAX_CUBOIDS]"
M_RANGE = "m must be in [1, UAVAC_MAX_SEGMENTS]"
M_DELAY = "m must be in [1, UAVAC_MAX_SEGMENTS - 1]: a delayed mission needs one more segment"
RADIUS = "radius must be finite and >= 0"
G_MIN = "G must be >= 1 when group_offsets are given"
BAD = "bad size or null pointer"
PITCH_OPT = "option log_pitch is smaller than B"

TABLE = [
    # ---- velocity and dt in one pair of refusals
    ("uavac_minsnap_row_counts_dev", {"velocity": NAN}, ENONFINITE, "non-finite velocity or dt"),
    ("uavac_minsnap_row_counts_dev", {"dt": NAN}, ENONFINITE, "non-finite velocity or dt"),
    ("uavac_minsnap_row_counts_dev", {"velocity": 0.0}, EINVAL, "velocity and dt must be > 0"),
    ("uavac_minsnap_row_counts_dev", {"dt": -0.05}, EINVAL, "velocity and dt must be > 0"),
    ("uavac_minsnap_row_counts_ragged_dev", {"velocity": NAN}, ENONFINITE, "non-finite velocity or dt"),
    ("uavac_minsnap_row_counts_ragged_dev", {"dt": 0.0}, EINVAL, "velocity and dt must be > 0"),
    ("uavac_minsnap_plan_dev", {"dt": NAN}, ENONFINITE, "non-finite velocity or dt"),
    ("uavac_minsnap_plan_dev", {"velocity": -2.0}, EINVAL, "velocity and dt must be > 0"),
    ("uavac_minsnap_obstacle_round_dev", {"velocity": NAN}, ENONFINITE, "non-finite velocity or dt"),
    ("uavac_minsnap_obstacle_round_dev", {"dt": 0.0}, EINVAL, "velocity and dt must be > 0"),
    # ---- dt in two refusals
    ("uavac_minsnap_row_counts_v_dev", {"dt": NAN}, ENONFINITE, "non-finite dt"),
    ("uavac_minsnap_row_counts_v_dev", {"dt": 0.0}, EINVAL, "dt must be > 0"),
    ("uavac_minsnap_row_counts_ragged_v_dev", {"dt": NAN}, ENONFINITE, "non-finite dt"),
    ("uavac_minsnap_row_counts_ragged_v_dev", {"dt": -0.05}, EINVAL, "dt must be > 0"),
    ("uavac_minsnap_plan_v_dev", {"dt": NAN}, ENONFINITE, "non-finite dt"),
    ("uavac_minsnap_plan_v_dev", {"dt": 0.0}, EINVAL, "dt must be > 0"),
    ("uavac_minsnap_plan_bc_dev", {"dt": NAN}, ENONFINITE, "non-finite dt"),
    ("uavac_minsnap_plan_bc_dev", {"dt": 0.0}, EINVAL, "dt must be > 0"),
    ("uavac_minsnap_retime_dev", {"dt": NAN}, ENONFINITE, "non-finite dt"),
    ("uavac_minsnap_retime_dev", {"dt": 0.0}, EINVAL, "dt must be > 0"),
    ("uavac_minsnap_row_counts_t_dev", {"dt": NAN}, ENONFINITE, "non-finite dt"),
    ("uavac_minsnap_row_counts_t_dev", {"dt": 0.0}, EINVAL, "dt must be > 0"),
    ("uavac_minsnap_plan_t_dev", {"dt": NAN}, ENONFINITE, "non-finite dt"),
    ("uavac_minsnap_plan_t_dev", {"dt": -0.05}, EINVAL, "dt must be > 0"),
    # ---- dt in one refusal
    ("uavac_minsnap_sample_dev", {"dt": NAN}, EINVAL, DT_ONE),
    ("uavac_minsnap_sample_dev", {"dt": 0.0}, EINVAL, DT_ONE),
    ("uavac_minsnap_sample_yaw_dev", {"dt": NAN}, EINVAL, DT_ONE),
    ("uavac_minsnap_sample_hits_dev", {"dt": 0.0}, EINVAL, DT_ONE),
    ("uavac_minsnap_sample_derivs_dev", {"dt": NAN}, EINVAL, DT_ONE),
    ("uavac_minsnap_sample_capped_dev", {"dt": -0.05}, EINVAL, DT_ONE),
    ("uavac_minsnap_sample_ragged_dev", {"dt": NAN}, EINVAL, DT_ONE),
    ("uavac_minsnap_sample", {"dt": NAN}, EINVAL, DT_ONE),
    ("uavac_minsnap_sample", {"dt": 0.0}, EINVAL, DT_ONE),
    ("uavac_minsnap_first_yaw_dev", {"dt": NAN}, EINVAL, DT_ONE),
    ("uavac_minsnap_first_yaw_dev", {"dt": 0.0}, EINVAL, DT_ONE),
    ("uavac_minsnap_audit_dev", {"dt": NAN}, EINVAL, DT_ONE),
    ("uavac_minsnap_audit_dev", {"dt": 0.0}, EINVAL, DT_ONE),
    ("uavac_minsnap_delay_dev", {"dt": NAN}, EINVAL, DT_ONE),
    ("uavac_minsnap_delay_dev", {"dt": 0.0}, EINVAL, DT_ONE),
    # ---- the n_cuboids range
    ("uavac_minsnap_audit_dev", {"n_cuboids": -1}, EINVAL, N_CUB),
    ("uavac_minsnap_audit_dev", {"n_cuboids": 17}, EINVAL, N_CUB),
    ("uavac_minsnap_layer_obs_dev", {"n_cuboids": -1}, EINVAL, N_CUB),
    ("uavac_minsnap_layer_obs_dev", {"n_cuboids": 17}, EINVAL, N_CUB),
    ("uavac_flown_audit_dev", {"n_cuboids": -1}, EINVAL, N_CUB),
    ("uavac_flown_audit_dev", {"n_cuboids": 17}, EINVAL, N_CUB),
    # ---- the pair calls' argument set, in its order, through the separation audit; then one of each through the others
    ("uavac_minsnap_separation_dev", {"coeffs": None}, EINVAL, "null waypoint pointer"),
    ("uavac_minsnap_separation_dev", {"B": 0}, EINVAL, "B must be >= 1"),
    ("uavac_minsnap_separation_dev", {"m": 0}, EINVAL, M_RANGE),
    ("uavac_minsnap_separation_dev", {"m": 65}, EINVAL, M_RANGE),
    ("uavac_minsnap_separation_dev", {"seg_rows": None}, EINVAL, NULL),
    ("uavac_minsnap_separation_dev", {"sep": None}, EINVAL, NULL),
    ("uavac_minsnap_separation_dev", {"isep": None}, EINVAL, NULL),
    ("uavac_minsnap_separation_dev", {"dt": NAN}, EINVAL, DT_ONE),
    ("uavac_minsnap_separation_dev", {"dt": 0.0}, EINVAL, DT_ONE),
    ("uavac_minsnap_separation_dev", {"radius": NAN}, EINVAL, RADIUS),
    ("uavac_minsnap_separation_dev", {"radius": -1.0}, EINVAL, RADIUS),
    ("uavac_minsnap_separation_dev", {"G": 0}, EINVAL, G_MIN),
    ("uavac_minsnap_conflict_offsets_dev", {"pair_offsets": None}, EINVAL, NULL),
    ("uavac_minsnap_conflict_offsets_dev", {"dt": NAN}, EINVAL, DT_ONE),
    ("uavac_minsnap_conflict_offsets_dev", {"G": 0}, EINVAL, G_MIN),
    ("uavac_minsnap_conflicts_dev", {"pair_offsets": None}, EINVAL, NULL),
    ("uavac_minsnap_conflicts_dev", {"dt": 0.0}, EINVAL, DT_ONE),
    ("uavac_minsnap_conflicts_dev", {"radius": NAN}, EINVAL, RADIUS),
    ("uavac_minsnap_conflicts_dev", {"capacity": -1}, EINVAL, "capacity must be >= 0"),
    ("uavac_minsnap_conflicts_dev", {"pair_d": None}, EINVAL, "pair_d and pair_i are required when capacity > 0"),
    ("uavac_minsnap_stagger_dev", {"istag": None}, EINVAL, NULL),
    ("uavac_minsnap_stagger_dev", {"dt": NAN}, EINVAL, DT_ONE),
    ("uavac_minsnap_stagger_dev", {"radius": -1.0}, EINVAL, RADIUS),
    ("uavac_minsnap_stagger_dev", {"step": 0}, EINVAL, "step must be >= 1"),
    ("uavac_minsnap_stagger_dev", {"max_steps": -1}, EINVAL, "max_steps must be in [0, UAVAC_STAGGER_MAX_STEPS]"),
    # ---- the layer calls' argument set
    ("uavac_minsnap_layer_dev", {"coeffs": None}, EINVAL, "null waypoint pointer"),
    ("uavac_minsnap_layer_dev", {"ilayer": None}, EINVAL, NULL),
    ("uavac_minsnap_layer_dev", {"offsets": None}, EINVAL, NULL),
    ("uavac_minsnap_layer_dev", {"dt": NAN}, EINVAL, DT_ONE),
    ("uavac_minsnap_layer_dev", {"G": 0}, EINVAL, G_MIN),
    ("uavac_minsnap_layer_dev", {"delta_z": NAN}, EINVAL, "delta must be finite"),
    ("uavac_minsnap_layer_dev", {"max_steps": -1}, EINVAL, "max_steps must be in [0, UAVAC_LAYER_MAX_STEPS]"),
    ("uavac_minsnap_layer_obs_dev", {"offsets": None}, EINVAL, NULL),
    ("uavac_minsnap_layer_obs_dev", {"dt": 0.0}, EINVAL, DT_ONE),
    ("uavac_minsnap_layer_obs_dev", {"delta_x": NAN}, EINVAL, "delta must be finite"),
    ("uavac_minsnap_layer_obs_dev", {"max_steps": 1024}, EINVAL, "max_steps must be in [0, UAVAC_LAYER_MAX_STEPS]"),
    ("uavac_minsnap_layer_obs_dev", {"cuboids": None}, EINVAL, "cuboids must be given when n_cuboids > 0"),
    # ---- the flown pair calls' argument set, in its order; the flown audit shares the log's shape
    ("uavac_flown_separation_dev", {"state_log": None}, EINVAL, NULL),
    ("uavac_flown_separation_dev", {"sep": None}, EINVAL, NULL),
    ("uavac_flown_separation_dev", {"K": 0}, EINVAL, "K must be >= 1"),
    ("uavac_flown_separation_dev", {"B": 0}, EINVAL, "B must be >= 1"),
    ("uavac_flown_separation_dev", {"pitch": 2}, EINVAL, "pitch must be >= B"),
    ("uavac_flown_separation_dev", {"radius": NAN}, EINVAL, RADIUS),
    ("uavac_flown_separation_dev", {"G": 0}, EINVAL, G_MIN),
    ("uavac_flown_conflict_offsets_dev", {"pair_offsets": None}, EINVAL, NULL),
    ("uavac_flown_conflict_offsets_dev", {"K": 0}, EINVAL, "K must be >= 1"),
    ("uavac_flown_conflict_offsets_dev", {"pitch": 2}, EINVAL, "pitch must be >= B"),
    ("uavac_flown_conflicts_dev", {"state_log": None}, EINVAL, NULL),
    ("uavac_flown_conflicts_dev", {"B": 0}, EINVAL, "B must be >= 1"),
    ("uavac_flown_conflicts_dev", {"radius": -1.0}, EINVAL, RADIUS),
    ("uavac_flown_conflicts_dev", {"capacity": -1}, EINVAL, "capacity must be >= 0"),
    ("uavac_flown_audit_dev", {"first_bad": None}, EINVAL, NULL),
    ("uavac_flown_audit_dev", {"K": 0}, EINVAL, "K must be >= 1"),
    ("uavac_flown_audit_dev", {"B": 0}, EINVAL, "B must be >= 1"),
    ("uavac_flown_audit_dev", {"pitch": 2}, EINVAL, "pitch must be >= B"),
    # ---- take and delay shapes
    ("uavac_minsnap_take_offsets_dev", {"index": None}, EINVAL, NULL),
    ("uavac_minsnap_take_offsets_dev", {"B": 0}, EINVAL, "B must be >= 1"),
    ("uavac_minsnap_take_offsets_dev", {"n": 0}, EINVAL, "n must be >= 1"),
    ("uavac_minsnap_take_offsets_dev", {"m": 0}, EINVAL, M_RANGE),
    ("uavac_minsnap_take_offsets_dev", {"m": 65}, EINVAL, M_RANGE),
    ("uavac_minsnap_take_dev", {"out_coeffs": None}, EINVAL, NULL),
    ("uavac_minsnap_take_dev", {"B": 0}, EINVAL, "B must be >= 1"),
    ("uavac_minsnap_take_dev", {"n": -1}, EINVAL, "n must be >= 1"),
    ("uavac_minsnap_take_dev", {"m": 0}, EINVAL, M_RANGE),
    ("uavac_minsnap_take_dev", {"out_times": None}, EINVAL, "times and out_times go together: both or none"),
    ("uavac_minsnap_delay_offsets_dev", {"start_rows": None}, EINVAL, NULL),
    ("uavac_minsnap_delay_offsets_dev", {"B": 0}, EINVAL, "B must be >= 1"),
    ("uavac_minsnap_delay_offsets_dev", {"m": 0}, EINVAL, M_DELAY),
    ("uavac_minsnap_delay_offsets_dev", {"m": 64}, EINVAL, M_DELAY),
    ("uavac_minsnap_delay_dev", {"out_seg_rows": None}, EINVAL, NULL),
    ("uavac_minsnap_delay_dev", {"B": 0}, EINVAL, "B must be >= 1"),
    ("uavac_minsnap_delay_dev", {"m": 64}, EINVAL, M_DELAY),
    ("uavac_minsnap_delay_dev", {"out_times": None}, EINVAL, "times and out_times go together: both or none"),
    # ---- the rollout's forms
    ("uavac_control_rollout_dev", {"V": None}, EINVAL, "null vehicle"),
    ("uavac_control_rollout_dev", {"traj": None}, EINVAL, BAD),
    ("uavac_control_rollout_dev", {"K": -1}, EINVAL, BAD),
    ("uavac_control_rollout_dev", {"option:log_pitch": 2}, EINVAL, PITCH_OPT),
    ("uavac_control_rollout_scored_dev", {"score": None}, EINVAL, "null score"),
    ("uavac_control_rollout_scored_dev", {"cmd_log": "cmd_log"}, EINVAL, "no scores together with a command log"),
    ("uavac_control_rollout_scored_dev", {"B": 0}, EINVAL, BAD),
    ("uavac_control_rollout_plan_dev", {"V": None}, EINVAL, "null vehicle"),
    ("uavac_control_rollout_plan_dev", {"coeffs": None}, EINVAL, "null waypoint pointer"),
    ("uavac_control_rollout_plan_dev", {"B": 0}, EINVAL, "B must be >= 1"),
    ("uavac_control_rollout_plan_dev", {"m": 65}, EINVAL, M_RANGE),
    ("uavac_control_rollout_plan_dev", {"seg_rows": None}, EINVAL, BAD),
    ("uavac_control_rollout_plan_dev", {"K": -1}, EINVAL, BAD),
    ("uavac_control_rollout_plan_dev", {"n_obs": -1}, EINVAL, BAD),
    ("uavac_control_rollout_plan_dev", {"yaw": None, "first_yaw": None}, EINVAL, "need the dense yaw column or the missions' first headings"),
    ("uavac_control_rollout_plan_dev", {"dt": NAN}, EINVAL, DT_ONE),
    ("uavac_control_rollout_plan_dev", {"dt": 0.0}, EINVAL, DT_ONE),
    ("uavac_control_rollout_plan_dev", {"option:log_pitch": 2}, EINVAL, PITCH_OPT),
    ("uavac_control_rollout_plan_scored_dev", {"score": None}, EINVAL, "null score"),
    ("uavac_control_rollout_plan_scored_dev", {"cmd_log": "cmd_log"}, EINVAL, "no scores together with a command log"),
    ("uavac_control_rollout_plan_scored_dev", {"dt": NAN}, EINVAL, DT_ONE),
    ("uavac_control_rollout_plan_scored_dev", {"option:log_pitch": 2}, EINVAL, PITCH_OPT),
    ("uavac_control_rollout_plan_ragged_dev", {"coeffs": None}, EINVAL, "null waypoint pointer"),
    ("uavac_control_rollout_plan_ragged_dev", {"seg_offsets": None}, EINVAL, BAD),
    ("uavac_control_rollout_plan_ragged_dev", {"first_yaw": None}, EINVAL, BAD),
    ("uavac_control_rollout_plan_ragged_dev", {"state": None}, EINVAL, BAD),
    ("uavac_control_rollout_plan_ragged_dev", {"dt": NAN}, EINVAL, DT_ONE),
    ("uavac_control_rollout_plan_ragged_dev", {"dt": -0.05}, EINVAL, DT_ONE),
    ("uavac_control_rollout_plan_ragged_dev", {"option:log_pitch": 2}, EINVAL, PITCH_OPT),
    ("uavac_control_rollout_plan_ragged_scored_dev", {"score": None}, EINVAL, "null score"),
    ("uavac_control_rollout_plan_ragged_scored_dev", {"cmd_log": "cmd_log"}, EINVAL, "no scores together with a command log"),
    ("uavac_control_rollout_plan_ragged_scored_dev", {"first_yaw": None}, EINVAL, BAD),
    ("uavac_control_rollout_plan_ragged_scored_dev", {"dt": 0.0}, EINVAL, DT_ONE),
    # ---- every option: its start value is taken; a value it does not take, where there is one (the others clamp or test for zero)
    ("uavac_set_option", {"name": b"yaw_group", "value": 8}, OK, None),
    ("uavac_set_option", {"name": b"yaw_group", "value": 2}, EINVAL, "yaw_group is 1, 4, 8 or 16"),
    ("uavac_set_option", {"name": b"audit_lanes", "value": 16}, OK, None),
    ("uavac_set_option", {"name": b"audit_lanes", "value": 32}, EINVAL, "audit_lanes is 16 or 64"),
    ("uavac_set_option", {"name": b"separation_split", "value": 0}, OK, None),
    ("uavac_set_option", {"name": b"separation_split", "value": 65}, EINVAL, "separation_split is 0 (automatic) or 1 .. UAVAC_SEP_MAX_SPLIT"),
    ("uavac_set_option", {"name": b"conflict_slots", "value": 0}, OK, None),
    ("uavac_set_option", {"name": b"conflict_slots", "value": -1}, EINVAL, "conflict_slots is 0 (automatic) or 1 .. 64"),
    ("uavac_set_option", {"name": b"flown_audit_split", "value": 0}, OK, None),
    ("uavac_set_option", {"name": b"flown_audit_split", "value": 65}, EINVAL,
     "flown_audit_split is 0 (automatic) or 1 .. UAVAC_FLOWN_AUDIT_MAX_SPLIT"),
    ("uavac_set_option", {"name": b"timeopt_chunk", "value": 0}, OK, None),
    ("uavac_set_option", {"name": b"timeopt_chunk", "value": -1}, EINVAL, "timeopt_chunk is 0 (automatic) or a number of missions"),
    ("uavac_set_option", {"name": b"sampler_waves", "value": 4}, OK, None),
    ("uavac_set_option", {"name": b"sampler_waves", "value": 3}, EINVAL, "sampler_waves is 1, 2, 4, 8 or 16"),
    ("uavac_set_option", {"name": b"sampler_group", "value": 1}, OK, None),
    ("uavac_set_option", {"name": b"sampler_group", "value": 0}, EINVAL, "sampler_group is 1 .. 64"),
    ("uavac_set_option", {"name": b"sampler_group", "value": 65}, EINVAL, "sampler_group is 1 .. 64"),
    ("uavac_set_option", {"name": b"rollout_align", "value": 1}, OK, None),
    ("uavac_set_option", {"name": b"log_pitch", "value": 0}, OK, None),
    ("uavac_set_option", {"name": b"log_pitch", "value": -1}, EINVAL, "log_pitch is 0 (= B) or a number of doubles >= B"),
    ("uavac_set_option", {"name": b"late_handover", "value": -1}, OK, None),
    ("uavac_set_option", {"name": b"solve_order", "value": 1}, OK, None),
    ("uavac_set_option", {"name": b"solve_order", "value": 2}, EINVAL, "solve_order is 0 (one-ended), 1 (two-ended) or -1 (by the launch)"),
    ("uavac_set_option", {"name": b"solve_order", "value": -2}, EINVAL, "solve_order is 0 (one-ended), 1 (two-ended) or -1 (by the launch)"),
    ("uavac_set_option", {"name": b"solve_park", "value": -1}, OK, None),
    ("uavac_set_option", {"name": b"solve_keep", "value": -1}, OK, None),
    ("uavac_set_option", {"name": b"solve_lanes", "value": -1}, OK, None),
    ("uavac_set_option", {"name": b"solve_lanes", "value": 0}, EINVAL, "solve_lanes is -1, 64, 32 or 16"),
    ("uavac_set_option", {"name": b"solve_lanes", "value": 8}, EINVAL, "solve_lanes is -1, 64, 32 or 16"),
    ("uavac_set_option", {"name": b"coeff_dma", "value": -1}, OK, None),
    ("uavac_set_option", {"name": b"idle_waves", "value": -1}, OK, None),
    ("uavac_set_option", {"name": b"cu_balance", "value": 1}, OK, None),
    ("uavac_set_option", {"name": b"lds_pad", "value": 0}, OK, None),
    ("uavac_set_option", {"name": b"lds_pad", "value": -8}, EINVAL, "lds_pad is 0 .. 122880 bytes"),
    ("uavac_set_option", {"name": b"lds_pad", "value": 122881}, EINVAL, "lds_pad is 0 .. 122880 bytes"),
    ("uavac_set_option", {"name": b"no_such_option", "value": 1}, EINVAL, "unknown option"),
    ("uavac_set_option", {"name": b"", "value": 1}, EINVAL, "unknown option"),
]

WAYPOINTS = np.array([[[0.0, 0.0, -1.0], [1.5, 0.5, -1.5], [2.5, 2.0, -1.0]],
                      [[0.5, 2.5, -2.0], [1.0, 1.0, -1.2], [2.0, 0.2, -2.2]],
                      [[3.0, 3.0, -1.0], [2.0, 2.2, -2.0], [0.4, 1.6, -1.4]]])


def _plan(ctx, dev, torch):
    """The valid plan of the fixture and of the tail: -> the arrays `uavac_minsnap_plan_dev` filled."""
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    p = dict(wp=torch.as_tensor(WAYPOINTS).to(dev), times=f64(B, M), seg_rows=torch.zeros(B, M, dtype=torch.int32, device=dev),
             row_offsets=torch.zeros(B + 1, dtype=torch.int64, device=dev), coeffs=f64(B, 8 * M, 3),
             status=torch.zeros(B, dtype=torch.int32, device=dev), traj=f64(CAP, 11), yaw=f64(CAP), first_yaw=f64(B))
    ctx.call("uavac_minsnap_plan_dev", p["wp"].data_ptr(), B, M, VEL, DT, p["times"].data_ptr(), p["seg_rows"].data_ptr(),
             p["row_offsets"].data_ptr(), p["coeffs"].data_ptr(), p["status"].data_ptr(), p["traj"].data_ptr(), CAP, p["yaw"].data_ptr(),
             p["first_yaw"].data_ptr())
    torch.cuda.synchronize()
    return p


def _context(torch):
    from uav_ac import _native as N
    ctx = N.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    return ctx


@pytest.fixture(scope="module")
def world():
    import torch
    from uav_ac import _native as N
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    ctx = _context(torch)
    ns = _plan(ctx, dev, torch)
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    i64 = lambda *s: torch.zeros(s, dtype=torch.int64, device=dev)
    # the ragged batch of 1, 2 and 2 segments: the uniform plan's missions, the first cut to its first segment
    seg_offsets = torch.as_tensor(np.array([0, 1, 3, 5], dtype=np.int64)).to(dev)
    wp_r = torch.as_tensor(np.concatenate([WAYPOINTS[0, :2], WAYPOINTS[1], WAYPOINTS[2]])).to(dev)
    ns.update(seg_offsets=seg_offsets, wp_r=wp_r, times_r=f64(5), seg_rows_r=i32(5), row_offsets_r=i64(B + 1), coeffs_r=f64(5, 8, 3))
    ctx.call("uavac_minsnap_row_counts_ragged_dev", wp_r.data_ptr(), seg_offsets.data_ptr(), B, M, VEL, DT, ns["times_r"].data_ptr(),
             ns["seg_rows_r"].data_ptr(), ns["row_offsets_r"].data_ptr())
    ctx.call("uavac_minsnap_solve_ragged_dev", wp_r.data_ptr(), ns["times_r"].data_ptr(), seg_offsets.data_ptr(), B, M,
             ns["coeffs_r"].data_ptr(), None)
    V = N.Vehicle.default()
    ns.update(V=V, state=f64(N.STATE_ROWS, B), istate=i32(N.ISTATE_ROWS, B), positions=ns["wp"][:, 0].contiguous())
    ctx.call("uavac_state_init_dev", C.byref(V), ns["positions"].data_ptr(), B, 1, ns["state"].data_ptr(), ns["istate"].data_ptr())
    torch.cuda.synchronize()
    state_log = f64(K, 13, B)
    state_log[:, 3] = 1.0                                   # a log of resting vehicles: unit quaternions at the first waypoints
    state_log[:, :3] = ns["wp"][:, 0].T
    ns.update(
        none=None, B=B, m=M, K=K, n=2, G=2, pitch=B, velocity=VEL, dt=DT, cap=CAP, total_segments=5, radius=1.0, capacity=8, step=1,
        max_steps=4, delta_x=0.0, delta_y=0.0, delta_z=1.0, n_cuboids=1, n_obs=0, margin=0.1, max_passes=2,
        velocities=torch.full((B,), VEL, dtype=torch.float64, device=dev), bc=f64(B, 6, 3), limits=(C.c_double * 4)(3.0, 3.0, 2.0, 12.0),
        passes=C.c_int(0), audit=f64(8, B), factors_total=f64(B), converged=i32(B), jerk=f64(CAP, 3), snap=f64(CAP, 3), hit=i32(B * 64),
        cuboids=torch.as_tensor(np.array([[0.9, 1.1, 0.9, 1.1, -1.3, -1.1]])).to(dev), hit_rows=i32(1, B), first_hit=i32(1, B),
        group_offsets=torch.as_tensor(np.array([0, 1, 3], dtype=np.int64)).to(dev), start_rows=i32(B), sep=f64(B), isep=i32(5, B),
        pair_offsets=i64(B + 1), pair_d=f64(8), pair_i=i32(5, 8), istag=i32(3, B), ilayer=i32(4, B), offsets=f64(B, 3),
        out_seg_offsets=i64(B + 1), out_coeffs=f64(B * (M + 1), 8, 3), out_times=f64(B * (M + 1)), out_seg_rows=i32(B * (M + 1)),
        out_first_yaw=f64(B), index=torch.as_tensor(np.array([2, 0], dtype=np.int32)).to(dev),
        active=i32(B), overflow=i32(B), touched=i32(B), wp_out=f64(B * 65, 3), seg_offsets_out=i64(B + 1), counters=i32(4),
        state_log=state_log, first_bad=i32(B), hit_ticks=i32(1, B), clearance=f64(1, B), clearance_tick=i32(1, B),
        roll_log=f64(K, 13, B), cmd_log=f64(K, 12, B), score=f64(11, B),
        coeffs_h=ns["coeffs"].cpu().numpy(), times_h=ns["times"].cpu().numpy(), row_offsets_h=ns["row_offsets"].cpu().numpy())
    ns["traj_h"] = np.zeros((int(ns["row_offsets_h"][-1]), 11))
    torch.cuda.synchronize()
    yield ctx, ns, torch
    ctx.close()


def _arg(v):
    if v is None or isinstance(v, (int, float, bytes)):
        return v
    if isinstance(v, np.ndarray):
        return v.ctypes.data_as(C.c_void_p)
    if isinstance(v, C.Structure):
        return C.byref(v)
    if isinstance(v, (C.Array, C._SimpleCData)):
        return C.cast(C.pointer(v), C.c_void_p)
    return C.c_void_p(v.data_ptr())


def test_sig_and_table_agree():
    """Every row names an entry point of SIG and parameters of that entry point; every entry point of SIG has a row."""
    for entry, defect, _, _ in TABLE:
        params = [p.split("=")[0] for p in SIG[entry].split()]
        assert all(k.startswith("option:") or k in params for k in defect), (entry, defect)
    assert {row[0] for row in TABLE} == set(SIG)


def test_refusals_then_a_valid_plan(world):
    ctx, ns, torch = world
    from uav_ac import _native as N
    lib = N.lib()
    wrong = []
    for entry, defect, want_rc, want_text in TABLE:
        values = {}
        for p in SIG[entry].split():
            name, _, key = p.partition("=")
            values[name] = ns[key or name] if entry != "uavac_set_option" else None
        options = {k[7:]: v for k, v in defect.items() if k.startswith("option:")}
        for name, v in defect.items():
            if not name.startswith("option:"):
                values[name] = ns[v] if isinstance(v, str) else v
        for name, v in options.items():
            ctx.set_option(name, v)
        rc = getattr(lib, entry)(ctx._h, *[_arg(v) for v in values.values()])
        text = lib.uavac_last_error(ctx._h).decode()
        for name in options:
            ctx.set_option(name, 0)
        if rc != want_rc or (want_text is not None and text != want_text):
            wrong.append((entry, defect, rc, text))
    assert not wrong, wrong
    # nothing was left behind: the same plan from this ctx and from one that has refused nothing
    torch.cuda.synchronize()
    after = _plan(ctx, ns["wp"].device, torch)
    fresh_ctx = _context(torch)
    fresh = _plan(fresh_ctx, ns["wp"].device, torch)
    fresh_ctx.close()
    for name in ("coeffs", "times", "seg_rows", "row_offsets", "first_yaw"):
        assert after[name].cpu().numpy().tobytes() == fresh[name].cpu().numpy().tobytes(), name
    assert after["coeffs"].cpu().numpy().tobytes() == ns["coeffs"].cpu().numpy().tobytes()
    flags = (C.c_int32 * 4)()
    ctx.call("uavac_take_flags", flags)
    assert list(flags) == [0, 0, 0, 0]
