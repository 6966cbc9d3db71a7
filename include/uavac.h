/*
 * uavac.h -- C ABI of libuavac.so: batched minimum-snap planning and cascaded
 * control + 6-DoF rollout for fleets of independent quadrotors on AMD MI355X
 * (gfx950).  Hand-written HIP kernels behind plain pointers and sizes.
 *
 * The reference (Mdhvince/UAV-Autonomous-control) has no FFI layer: its boundary
 * is a set of Python classes.  Each entry point below names the reference
 * interface it replaces (paths relative to the upstream repository root); the
 * Python binding a maintainer adds on the reference side is in INTEGRATION.md.
 *
 * Conventions
 *   - all floating point is IEEE fp64; NED world frame, FRD body frame;
 *   - every function returns UAVAC_OK (0) or a negative UAVAC_E* code; the text
 *     of the last failure is available from uavac_last_error(ctx);
 *   - a ctx owns one HIP stream (or borrows the caller's, see
 *     uavac_set_stream) and is not thread-safe; distinct ctxs are independent;
 *   - functions with the _dev suffix take DEVICE pointers, enqueue on the ctx
 *     stream and return without synchronising; the un-suffixed twins take HOST
 *     pointers, stage through device scratch and are synchronous on return;
 *   - nothing here ever falls back to a CPU path: without a usable GPU
 *     uavac_create fails with UAVAC_EHIP.
 */
#ifndef UAVAC_H
#define UAVAC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UAVAC_VERSION 310 /* 0.3.1: rows-free planning chain (uavac_minsnap_plan_dev with traj = NULL), uavac_minsnap_first_yaw_dev;
                             0.3.0: plan gather, log pitch, row offsets from row counts; 0.2.0: ground-plane fields, istate has 4 rows */

#define UAVAC_OK 0
#define UAVAC_EINVAL (-1)    /* bad shape / size / null pointer                    */
#define UAVAC_ENONFINITE (-2)/* non-finite waypoint, velocity or dt                */
#define UAVAC_EHIP (-3)      /* HIP runtime error (text in uavac_last_error)       */
#define UAVAC_ESINGULAR (-4) /* a mission's knot system is singular (e.g. repeated waypoint) */
#define UAVAC_ENOMEM (-5)
#define UAVAC_ECOMM (-6)     /* RCCL error (text in uavac_last_error)              */
#define UAVAC_ETOOLCHAIN (-7)/* uavac_create's self-check (first context of a process): the atan2 of the device math library this build
                                linked no longer has the bits its sampler's heading() reproduces -- heading() (csrc/minsnap_yaw.h) must
                                be re-derived for that library; rebuilding alone reproduces the failure (text on stderr) */

#define UAVAC_MAX_SEGMENTS 64   /* m, segments per mission                          */
#define UAVAC_TRAJ_COLS 11      /* x y z vx vy vz ax ay az yaw spline_id: minimum_snap.py:122-123 */
#define UAVAC_STATE_ROWS 30     /* see uavac_control_* below                        */
#define UAVAC_ISTATE_ROWS 4
#define UAVAC_CMD_COLS 12
#define UAVAC_SCORE_ROWS 11     /* tracking scores of the scored rollouts, see uavac_control_rollout_scored_dev */

typedef struct uavac_ctx uavac_ctx;

/* Vehicle constants, limits and controller gains.
 * Replaces the attributes of uav_ac/quadrotor/quad.py:11-86 (Quad.__init__) that the
 * controller reads, with the values models/lab_course.xml:3,9-13,100,116 provides. */
typedef struct uavac_vehicle {
    double g;               /* gravity [m/s^2]                      quad.py:39  */
    double dt;              /* inner (dynamics / motor) step [s]    quad.py:40  */
    double dt_outer;        /* CascadedController.dt = dt * inner_per_outer  main.py:97-98 */
    double mass;
    double inertia[3];      /* diagonal body inertia                */
    double arm;             /* roll/pitch lever arm of each rotor   */
    double kf;              /* rotor speed^2 -> thrust coefficient  */
    double kappa;           /* rotor reaction torque / thrust       */
    double min_thrust, max_thrust;      /* per rotor [N]             */
    double tau_rise, tau_fall;          /* motor time constants [s]  */
    double max_ascent, max_descent, max_speed_xy, max_horiz_accel, max_tilt; /* flight_limits */
    double kp_xy, kd_xy, kp_z, kd_z, ki_z;                /* quad.py:65-67 */
    double kp_roll, kp_pitch, kp_yaw, kp_p, kp_q, kp_r;   /* quad.py:68-73 */
    int32_t inner_per_outer;            /* config.ini:2 `frequency`  */
    int32_t ground;                     /* 0: free flight (default).  1: a horizontal ground plane the body can rest on
                                         * and take off from -- the on-ground start of the reference's scene
                                         * (lab_course.xml:34,98: plane at z = 0, body box of half height 0.02 m
                                         * starting 1 mm above it).  BUILD-DEFINED contact, not MuJoCo's solver: a
                                         * normal acceleration toward the critically damped reference
                                         * -2 vz / tc - r / tc^2 (r = penetration of the body's lowest point) whenever
                                         * that pushes up harder than free flight does; no friction, no contact
                                         * torque.  Contact FORCES are therefore not comparable with MuJoCo's. */
    double ground_z;                    /* NED z of the plane (0 = the reference scene)                      */
    double ground_clearance;            /* body centre above its lowest point (half height of geom "body") */
    double ground_timeconst;            /* tc: MuJoCo's default solref time constant, 0.02 s               */
} uavac_vehicle;
/* Ground bookkeeping bits in istate row 3 (only touched when V->ground != 0), after
 * MujocoSimulation._record_collisions (mujoco_sim.py:220-230): */
#define UAVAC_GROUND_IN_CONTACT 1     /* the body touches the plane after this tick (`has_collision`)      */
#define UAVAC_GROUND_TAKEN_OFF 2      /* sticky: height >= UAVAC_TAKEOFF_HEIGHT has been reached            */
#define UAVAC_GROUND_HIT_AFTER_TAKEOFF 4 /* sticky: contact after take-off (`collision_detected`)            */
#define UAVAC_TAKEOFF_HEIGHT 0.1      /* TAKEOFF_HEIGHT, mujoco_sim.py:17                                   */

/* ---- context ------------------------------------------------------------------ */
int uavac_version(void);
/* device_id < 0: use the current HIP device. */
int uavac_create(uavac_ctx **out, int device_id);
void uavac_destroy(uavac_ctx *ctx);
const char *uavac_last_error(const uavac_ctx *ctx);
/* Borrow a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream).  NULL is a
 * valid handle: HIP's legacy default stream (what torch uses unless told otherwise).
 * uavac_reset_stream goes back to the ctx-owned (non-blocking) stream. */
int uavac_set_stream(uavac_ctx *ctx, void *hip_stream);
int uavac_reset_stream(uavac_ctx *ctx);
int uavac_synchronize(uavac_ctx *ctx);
/* The HIP device the ctx was created for.  Every entry point makes that device current for its own
 * duration and restores the caller's: a ctx for GPU 1 works while GPU 0 is the thread's device. */
int uavac_device(const uavac_ctx *ctx);
/* Name and template arguments <compute waves, store waves, state log, command log, obstacle test,
 * plan-fed> of the rollout kernel the ctx launched last ("" before the first): what a profile of
 * the same call will show.  Diagnostics for benchmarks; the string lives in the ctx. */
const char *uavac_last_rollout_kernel(const uavac_ctx *ctx);
/* Vector registers per lane of that kernel in the loaded code object (hipFuncGetAttributes; 0 = unknown).  The rollout
 * kernels must stay within 256: two wavefronts of the kernel share a SIMD (compute + store wave), and at 258 a launch ran
 * 1.96 ms instead of 1.27 ms.  __graft_entry__.build() refuses a build that crosses the line; this is the same number seen
 * from the running process. */
int uavac_last_rollout_vgprs(const uavac_ctx *ctx);
/* Shape of that launch, out[6] = grid (workgroups), threads per workgroup, dynamic LDS bytes per workgroup (the cu_balance /
 * lds_pad pad included), log pitch (doubles between log rows), 64-UAV tiles, persistent passes (tiles walked per workgroup,
 * rounded up).  All 0 before the first rollout.  Read-only diagnostics: tests prove which launch form they reached with it. */
int uavac_last_rollout_launch(const uavac_ctx *ctx, int64_t out[6]);
/* Name and template arguments of the coefficient-solve kernel the ctx launched last -- "minsnap_solve_tw_kernel<ragged, parked
 * in LDS, missions per wave, blocks kept in registers>", "minsnap_solve_bt_kernel<...>" (the one-ended form) or
 * "minsnap_solve_kernel" (banded) -- and of the sampler kernel launched last: "minsnap_sample_stream_kernel<waves, hits,
 * derivatives, ragged>" or "minsnap_sample_kernel<hits, derivatives, yaw chunks per store[, ragged]>".  "" before the first.
 * Read-only diagnostics like uavac_last_rollout_kernel: tests prove which form they reached with them. */
const char *uavac_last_solve_kernel(const uavac_ctx *ctx);
const char *uavac_last_sample_kernel(const uavac_ctx *ctx);
/* Shape of that sampler launch, out[5] = grid, threads per workgroup, dynamic LDS bytes, missions per workgroup (the
 * "sampler_group" after it shrank to fit LDS), address phase of the chunk grid (0 .. 63; -1 for the one-wave form). */
int uavac_last_sample_launch(const uavac_ctx *ctx, int64_t out[5]);
/* "libuavac <version>; gfx950; HIP <x.y.z>; <compiler version>" of the build (static string). */
const char *uavac_build_info(void);
/* Which physical GPU the ctx runs on: "uuid=<32 hex digits>;pci=<domain:bus:device.function>;name=<gcnArchName>" into buf
 * (NUL-terminated, truncated to n bytes).  The multi-GPU bench gathers one per rank: eight ranks must name eight devices. */
int uavac_device_identity(uavac_ctx *ctx, char *buf, int n);
/* The shader clock the chip holds while other work runs: enqueues ONE wavefront on the ctx's stream that stamps
 * s_memtime (shader cycles) and s_memrealtime (100 MHz) , sleeps until `window_us` of real time have passed and stamps again;
 * stamps [4] (DEVICE memory, int64) = {cycles0, real0, cycles1, real1}.  Clock = (cycles1 - cycles0) / (real1 - real0) x 100 MHz
 * (MI355X_MICROARCH.md, DVFS give-back (6)).  Bind the ctx to a side stream (uavac_set_stream) to run it BESIDE the kernels of
 * interest; it holds one wave slot and issues nothing but s_sleep.  1 <= window_us <= 1 000 000. */
int uavac_clock_probe_dev(uavac_ctx *ctx, int window_us, int64_t *stamps);
/* Tuning knobs; results never depend on them (tested bit for bit).  "rollout_align": 1 (default) =
 * precede a rollout launch that writes a log by an empty kernel of the same workgroup shape (one
 * compute + one store wave), which makes the hardware place one wave of each kind on every SIMD
 * whatever ran before; 0 = do not.  "yaw_group": 1, 4, 8 (default) or 16 = how
 * many 64-row chunks of the sampler's dense yaw column are written together.  "late_handover": -1
 * (default: chosen per launch), 0, 1 = when the compute wave hands a tick's log values to the store
 * wave.  "lds_pad": extra LDS bytes per rollout workgroup (caps the workgroups a CU takes; 0).
 * "cu_balance": 1 (default) = a logged rollout that needs two or three workgroups on every CU sizes their LDS so
 * that no CU takes more of them than its even share (the dispatcher otherwise gives some CUs three and
 * some one where two each would do), 0 = off.
 * "solve_order" is NOT a tuning knob -- it selects the elimination order of the coefficient solve and with
 * it the rounding: 1 (default) = two-ended, two lanes per mission that meet at the middle knot
 * (csrc/minsnap_solve_tw.hip); 0 = one-ended (csrc/minsnap_solve_bt.hip, rounds 1-4), kept as the
 * cross-check; the two agree to ~5e-14 relative on the coefficients.  -1 (opt-in) = the launcher picks the faster of the two by
 * (m, B) -- one-ended for uniform batches of m <= 8 from 48 missions per SIMD on -- at the price that a mission's last bits then
 * depend on the size of the batch it is planned in (the default keeps a shard's coefficients equal to the whole job's).
 * "idle_waves": -1 (default: chosen per launch), 0, 1 = a placeholder wave between the compute and the
 * store wave of every rollout workgroup, which lets two workgroups on a CU occupy all four SIMDs
 * (16 385 .. 32 768 UAVs).  "coeff_dma": -1 (default: chosen per launch), 0, 1, 2 = the plan-fed rollout's mode: 0 the compute
 * wave evaluates target rows and reloads a segment's coefficients through registers on the spot; 1 the same with the
 * coefficients arriving by LDS-DMA an outer tick ahead; 2 the second (store) wave owns the cursor and evaluates the rows in
 * its idle time (kernels that have one; inner_per_outer >= 7).  Same bits in every mode.  "solve_park": -1 (default: chosen per launch), 0, 1 = the coefficient solve parks its forward sweep in the HBM
 * workspace / in LDS (when (m - 1) x 14 KB fit; same bits); "solve_lanes": -1 (default: chosen per launch), 64, 32, 16 = lanes
 * of a wavefront of the solve that carry (half of) a mission -- the two-ended solve gives a mission two lanes: 32, 16, 8 missions
 * per wavefront -- (fewer = more wavefronts for the same batch; same bits); "solve_keep": -1
 * (default: chosen per launch), 0, 1 = the solve of a uniform batch keeps the first five knots' blocks of its forward sweep in
 * registers instead of the workspace (same bits).  "sampler_waves": 4 (default), 2, 8, 16 = wavefronts per workgroup of the
 * chunk-streaming sampler, "sampler_group": 1 (default) .. 64 = consecutive missions per workgroup;
 * "sampler_waves" 1 = the one-wave-per-mission sampler (same rows bit for bit; faster into some row
 * buffers, slower into most: DESIGN K2).  "audit_lanes": 16 (default) or 64 = lanes per mission of uavac_minsnap_audit_dev.
 * "timeopt_chunk": 0 (default: sized from UAVAC_TIMEOPT_SCRATCH_BYTES) or the missions per chunk of uavac_minsnap_optimize_times_dev
 * (same results).  "separation_split": 0 (default: sized from B and G) or 1 .. UAVAC_SEP_MAX_SPLIT = workgroups that share the partners
 * of one window of 64 missions in uavac_minsnap_separation_dev and uavac_flown_separation_dev (same results).  "flown_audit_split": 0
 * (default: sized from B and K) or 1 .. UAVAC_FLOWN_AUDIT_MAX_SPLIT = workgroups that share the ticks of one window of 64 vehicles in
 * uavac_flown_audit_dev (same results).  "conflict_slots": 0 (default: 64) or 1 .. 64 = j-tile slots per mission and discovery round
 * of the conflict lists (uavac_minsnap_conflict_offsets_dev, uavac_minsnap_conflicts_dev, uavac_flown_conflict_offsets_dev,
 * uavac_flown_conflicts_dev, and the two cross calls uavac_minsnap_conflict_against_offsets_dev, uavac_minsnap_conflicts_against_dev;
 * same results, less scratch, more rounds).  "search_block": 0 (default: 64), 64, 128 or 256 = missions per
 * block of uavac_minsnap_stagger_wide_dev and uavac_minsnap_layer_wide_dev (same results).
 * Defaults from the environment (UAVAC_ROLLOUT_ALIGN, UAVAC_YAW_GROUP, UAVAC_SAMPLER_WAVES, UAVAC_SAMPLER_GROUP) at uavac_create.
 * ONE option is not a tuning knob but part of the log layout: "log_pitch" = P doubles per log row,
 * 0 (default) = B.  With P >= B the rollouts write state_log [K][13][P] and cmd_log [K][12][P]
 * (columns B .. P-1 are never touched).  Rows of a multiple of 16 doubles start on 128-byte lines
 * whatever B is: B = 65 534 with P = 65 536 streams like B = 65 536, with P = B at half that rate. */
int uavac_set_option(uavac_ctx *ctx, const char *name, int value);
/* The _dev planning entry points report data-dependent failures through sticky device-side flags
 * instead of synchronising: flags[0] non-finite segment duration, flags[1] singular knot system,
 * flags[2] trajectory buffer too small (uavac_minsnap_plan_dev), flags[3] a mission with more than
 * 2^31-1 rows.  This call synchronises the stream, returns them and clears them.  The host-pointer
 * twins clear the flags on entry and turn them into UAVAC_E* return codes themselves. */
int uavac_take_flags(uavac_ctx *ctx, int32_t flags[4]);
/* Fill *V with the laboratory vehicle (lab_course.xml) and the gains of quad.py:42-73. */
void uavac_vehicle_default(uavac_vehicle *V);

/* ---- planning -----------------------------------------------------------------
 * Batched drop-in for uav_ac/planning/minimum_snap.py MinimumSnap._generate_trajectory
 * (:97-124) on B independent missions of m segments each (obstacles=None path).
 *
 *   wp          [B][m+1][3]  waypoints
 *   times       [B][m]       segment durations            (_generate_time_per_spline :311-321)
 *   seg_rows    [B][m] i32   rows sampled per segment = len(np.arange(0, T, dt))    (:104)
 *   row_offsets [B+1]  i64   exclusive prefix sum of the per-mission row totals
 *   coeffs      [B][8m][3]   polynomial coefficients, ascending powers, per spline  (:153)
 *   traj        [row_offsets[B]][11]  rows of all missions back to back (:122-123)
 */
int uavac_minsnap_row_counts_dev(uavac_ctx *ctx, const double *wp, int B, int m, double velocity,
                                 double dt, double *times, int32_t *seg_rows, int64_t *row_offsets);
/* Solves the joint minimum-snap QP of _compute_spline_parameters (:138-153) per mission.
 * status [B] i32 (may be NULL): 0 ok, 1 singular system. */
int uavac_minsnap_solve_dev(uavac_ctx *ctx, const double *wp, const double *times, int B, int m,
                            double *coeffs, int32_t *status);
/* The same QP through the other device solver: wave-per-mission banded LU with partial pivoting in LDS
 * (uavac_minsnap_solve_dev is the lane-per-mission block-Thomas recurrence).  Kept as an independent,
 * pivoted cross-check; ~50x slower. */
int uavac_minsnap_solve_banded_dev(uavac_ctx *ctx, const double *wp, const double *times, int B, int m,
                                   double *coeffs, int32_t *status);
/* Sampler (:100-119) + yaw scan (_calculate_yaws :126-136). */
int uavac_minsnap_sample_dev(uavac_ctx *ctx, const double *coeffs, const double *times,
                             const int32_t *seg_rows, const int64_t *row_offsets, int B, int m,
                             double dt, double *traj);
/* uavac_minsnap_sample_dev that also writes the yaw column on its own: yaw[row_offsets[B]]
 * (yaw[i] == traj[i][9]); input of uavac_control_rollout_plan_dev. */
int uavac_minsnap_sample_yaw_dev(uavac_ctx *ctx, const double *coeffs, const double *times,
                                 const int32_t *seg_rows, const int64_t *row_offsets, int B, int m,
                                 double dt, double *traj, double *yaw);
/* Sampler that also reports, per mission and spline, whether any sampled position lies inside the cuboid
 * aabb[6] = xmin xmax ymin ymax zmin zmax (device pointer; inclusive test of is_collision_cuboid :327-357):
 * hit [B][m] i32 (0/1).  This is the collision scan of _generate_collision_free_trajectory (:81-87), fused
 * into the sampling pass; the midpoint insertion that follows (:91-92) is host logic. */
int uavac_minsnap_sample_hits_dev(uavac_ctx *ctx, const double *coeffs, const double *times,
                                  const int32_t *seg_rows, const int64_t *row_offsets, int B, int m,
                                  double dt, double *traj, const double *aabb, int32_t *hit);

/* The sampler with every optional output: yaw [rows] (or NULL) as above; first_yaw [B] (or NULL) =
 * the heading of each mission's first row that has one (what the rows before it take; 0 when no
 * row has one) -- all a plan-fed rollout needs to scan the yaw itself; jerk / snap [rows][3] (or
 * NULL) = polynom(8, 3, t) @ coeffs and polynom(8, 4, t) @ coeffs, the two samples the reference
 * evaluates in comments only (minimum_snap.py:111-112,118-119).  They are separate arrays: the
 * (N, 11) row layout of get_trajectory() never changes. */
int uavac_minsnap_sample_derivs_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows,
                                    const int64_t *row_offsets, int B, int m, double dt, double *traj,
                                    double *yaw, double *first_yaw, double *jerk, double *snap);
/* uavac_minsnap_sample_derivs_dev (rows, optional yaw column, optional first headings) into a row buffer of
 * traj_capacity_rows rows (yaw, when given, as many values): when row_offsets[B] exceeds it the launch writes nothing and
 * raises flag 2 (uavac_take_flags), like uavac_minsnap_plan_dev.  row_offsets may point into a larger table (a sub-range of
 * missions whose offsets stay absolute): the capacity is then that of the whole buffer.  UAVAC_EINVAL for a negative
 * capacity.  The form every caller should use whose buffer was sized from a row count it did not just read. */
int uavac_minsnap_sample_capped_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows,
                                    const int64_t *row_offsets, int B, int m, double dt, double *traj,
                                    int64_t traj_capacity_rows, double *yaw, double *first_yaw);
/* The whole planning chain of MinimumSnap.get_trajectory() (obstacles=None; minimum_snap.py:59-61,
 * 97-124) enqueued by ONE call: times + row counts, row offsets, coefficient solve, sampler (+ yaw
 * column when yaw != NULL, + the missions' first headings when first_yaw != NULL) -- four kernel
 * launches back to back, no host code in between.  The row
 * buffer must have been sized by the caller: traj holds traj_capacity_rows rows (yaw as many
 * values); when the plan needs more it is refused AS A WHOLE and flag 2 is raised (uavac_take_flags):
 * times, seg_rows, row_offsets, coeffs, status, traj, yaw and first_yaw all keep what they held, so the
 * previous plan stays consistent and flyable (times / row counts / offsets are computed into ctx scratch
 * and copied into the caller's arrays by a device-side commit only when the rows fit).
 * Typical use: size the buffers once with uavac_minsnap_row_counts_dev, then re-plan in place.
 *
 * ROWS-FREE form: traj == NULL (then yaw must be NULL and traj_capacity_rows is ignored).  The chain is times + row counts,
 * row offsets, coefficient solve and -- when first_yaw != NULL -- uavac_minsnap_first_yaw_dev: everything a plan-fed rollout
 * (uavac_control_rollout_plan_dev with yaw == NULL) and uavac_gather_plan_dev need, and not one of the 88-byte rows.  For ranks
 * of a multi-GPU job whose trajectories are sampled where they are wanted (the root of the final gather re-samples them from
 * the gathered plan, bit-identical): sampling them on the peer as well was the same work done twice.  Nothing can be refused,
 * so times / seg_rows / row_offsets are written in place. */
int uavac_minsnap_plan_dev(uavac_ctx *ctx, const double *wp, int B, int m, double velocity, double dt,
                           double *times, int32_t *seg_rows, int64_t *row_offsets, double *coeffs,
                           int32_t *status, double *traj, int64_t traj_capacity_rows, double *yaw,
                           double *first_yaw);

/* first_yaw [B] of a solved plan WITHOUT sampling its rows: the heading of each mission's first sample with |v_xy| >= 1e-3
 * (MinimumSnap._calculate_yaws, minimum_snap.py:126-136: the rows before it take that heading; 0 when no sample has one) --
 * bit for bit what the sampler writes into first_yaw, from coeffs [B][8m][3] and seg_rows [B][m] alone.  Sixteen lanes per
 * mission (four missions per wavefront) walk the rows sixteen at a time from row 0 and stop at the first step that holds a valid
 * one.  seg_offsets [B+1] (device) != NULL: a ragged batch (coeffs [S][8][3], seg_rows [S] back to back, m = the largest
 * segment count); NULL: uniform. */
int uavac_minsnap_first_yaw_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets,
                                int B, int m, double dt, double *first_yaw);

/* PLAN AUDIT: what the sampled rows of a solved plan would show, per mission, WITHOUT sampling them -- whether a plan (a rows-free
 * one in particular) is flyable before it is flown.  The control law clips the target climb rate, the target horizontal velocity
 * and the horizontal acceleration command (max_ascent / max_descent, max_speed_xy, max_horiz_accel of uavac_vehicle); the planner
 * knows none of these limits, and the obstacle loop does not re-check earlier cuboids (uavac_minsnap_obstacle_waypoints).  One
 * kernel walks every mission's rows with the sampler's own arithmetic -- exactly the rows the sampler would write, row r of
 * segment s at t = (r - first row of s) * dt -- and stores none of them.  seg_offsets as in uavac_minsnap_first_yaw_dev: NULL =
 * uniform batch (coeffs [B][8m][3], seg_rows [B][m]); otherwise ragged (arrays back to back, m = the largest segment count,
 * segment counts clamped to 1 .. m as the sampler clamps them).
 *   audit [UAVAC_AUDIT_ROWS][B] f64 (SoA like the score block), maxima over the mission's rows:
 *     0 the mission's row total (exact as a double)      4 peak horizontal acceleration sqrt(ax^2 + ay^2)
 *     1 peak horizontal speed sqrt(vx^2 + vy^2)           5 peak upward acceleration   max(-az)   (NED)
 *     2 peak climb rate   max(-vz)   (NED)                6 peak downward acceleration max(az)
 *     3 peak descent rate max(vz)                         7 peak speed sqrt(vx^2 + vy^2 + vz^2)
 *   cuboids  [n_cuboids][6]  xmin xmax ymin ymax zmin zmax, 0 <= n_cuboids <= UAVAC_AUDIT_MAX_CUBOIDS
 *   hit_rows  [n_cuboids][B] i32: how many of the mission's samples lie inside cuboid c (inclusive test of is_collision_cuboid,
 *             minimum_snap.py:327-357, on the very positions the sampler stores)
 *   first_hit [n_cuboids][B] i32: mission-local index of the first such row, -1 when there is none
 * n_cuboids == 0: cuboids, hit_rows and first_hit must all be NULL.
 * ROUNDING is part of the contract: the squares are separately rounded products and sums (no fused multiply-add), the maximum
 * is taken of the squares, one correctly rounded sqrt comes last -- a peak equals np.sqrt(vx * vx + vy * vy).max() (row 7:
 * vx * vx + vy * vy + vz * vz, left to right) over the sampler's rows bit for bit, whatever the launch shape or the batch split
 * (option "audit_lanes": 16 (default) or 64 lanes of a wavefront per mission; a tuning knob, same results).
 * A mission with ANY non-finite sample -- a singular knot system writes NaN coefficients -- reports NaN in rows 1-7, no hits and
 * first_hit -1 (so does a mission without rows): a singular plan never looks feasible.
 * UAVAC_EINVAL before anything is enqueued: n_cuboids outside 0 .. UAVAC_AUDIT_MAX_CUBOIDS, a NULL where a pointer is required
 * (or a pointer where n_cuboids == 0 requires NULL), B < 1, m outside 1 .. UAVAC_MAX_SEGMENTS, dt not positive and finite. */
#define UAVAC_AUDIT_ROWS 8
#define UAVAC_AUDIT_MAX_CUBOIDS 16
int uavac_minsnap_audit_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                            double dt, const double *cuboids, int n_cuboids, double *audit, int32_t *hit_rows, int32_t *first_hit);

/* PLAN DEMAND: what a solved plan ASKS OF THE VEHICLE, per mission, WITHOUT sampling its rows -- the plan-side counterpart of
 * uavac_flown_audit_dev's bank_x / bank_y / body_rate / clearance.  The control law clips the bank command (csrc/control_law.h: bxc =
 * clamp(acx / acc_z, +-max_tilt)), which on a perfectly tracked plan is |ax| / |a - g e3|: it depends on the vertical acceleration of
 * the same row, binds long before max_horiz_accel does, and the law divides by g - az, which a fast plan drives through zero.
 * uavac_minsnap_audit_dev reports none of this.  One kernel walks the rows as the plan audit does (csrc/minsnap_demand.hip) and stores
 * none of them.  coeffs / seg_rows / seg_offsets / B / m / dt as in uavac_minsnap_audit_dev (seg_offsets NULL = uniform, otherwise
 * ragged and clamped); g: the gravitational acceleration (uavac_vehicle.g), m/s^2.
 * PER ROW, from the sampler's position p and acceleration a (the values uavac_minsnap_sample_dev writes) and the jerk j that
 * uavac_minsnap_sample_derivs_dev writes, bit for bit; every product, sum, quotient and fmax is ONE rounded operation (no fused
 * multiply-add), in exactly this order:
 *     fz  = g - az                                        (NED: hover has fz = g)
 *     n2  = (ax * ax + ay * ay) + fz * fz                 specific thrust, squared
 *     bx2 = n2 > 0 ? (ax * ax) / n2 : 0                   by2 likewise with ay
 *     jj  = (jx * jx + jy * jy) + jz * jz
 *     jf  = (jx * ax + jy * ay) - jz * fz
 *     w2  = n2 > 0 ? fmax(jj - (jf * jf) / n2, 0) / n2 : 0      the roll / pitch rate the curve demands, squared (no yaw rate)
 *     inverted = fz <= 0                                  the row asks for thrust downward
 *     per cuboid: ex = px < xmin ? xmin - px : (px > xmax ? px - xmax : 0), ey, ez likewise; d2 = (ex * ex + ey * ey) + ez * ez
 * The maxima and minima are taken of these SQUARES and one correctly rounded sqrt comes last.
 *   demand  [UAVAC_DEMAND_ROWS][B] f64:   0 the mission's row total      3 sqrt(max bx2)  the bank about x the plan demands
 *                                          1 sqrt(max n2)  m/s^2          4 sqrt(max by2)
 *                                          2 sqrt(min n2)                 5 sqrt(max w2)   rad/s
 *   idemand [UAVAC_IDEMAND_ROWS][B] i32:  0 the number of inverted rows, 1 the mission-local index of the first one (-1: none)
 *   cuboids [n_cuboids][6] xmin xmax ymin ymax zmin zmax, 0 <= n_cuboids <= UAVAC_AUDIT_MAX_CUBOIDS
 *   clearance     [n_cuboids][B] f64 = sqrt(min d2): 0 when a sample lies inside the cuboid or on a face
 *   clearance_row [n_cuboids][B] i32: the mission-local index of the FIRST row that attains it
 * n_cuboids == 0: cuboids, clearance and clearance_row must all be NULL.
 * The reductions are max, min, integer add and the lexicographic minimum of (d2, row): exact and order-free, so the outputs depend
 * neither on the launch shape nor on the batch split (option "audit_lanes": 16 or 64 lanes per mission, same results).  They equal
 * what NumPy computes from the sampled rows and jerk, bit for bit (uav_ac/scoring.py demand_from_rows).
 * A mission with ANY non-finite sample (position, velocity, acceleration or jerk), and a mission without rows, reports NaN in rows
 * 1-5, clearance NaN, every index -1 and 0 inverted rows: a singular plan never looks feasible.
 * UAVAC_EINVAL before anything is enqueued: n_cuboids outside 0 .. UAVAC_AUDIT_MAX_CUBOIDS, a NULL where a pointer is required (or
 * a pointer where n_cuboids == 0 requires NULL), B < 1, m outside 1 .. UAVAC_MAX_SEGMENTS, dt or g not positive and finite. */
#define UAVAC_DEMAND_ROWS 6
#define UAVAC_IDEMAND_ROWS 2
int uavac_minsnap_demand_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                             double dt, double g, const double *cuboids, int n_cuboids, double *demand, int32_t *idemand,
                             double *clearance, int32_t *clearance_row);

/* SEPARATION AUDIT: the fleet's audit against itself.  For every mission of a GROUP of missions that share an airspace: the closest
 * approach to any other mission of the group, to which one and when; how many others come inside a protection radius and when the
 * first one does -- from coefficients and row counts alone (csrc/minsnap_separation.hip, csrc/fleet_clock.h): no row is written, nothing is read back,
 * everything is enqueued on the ctx stream.  coeffs / seg_rows / seg_offsets / B / m / dt as in uavac_minsnap_audit_dev (seg_offsets
 * NULL = uniform, otherwise ragged and clamped).
 * CLOCK.  The missions of a group share one row clock k = 0, 1, ....  Mission b has N_b rows -- exactly the rows the sampler writes,
 * walked as the plan audit walks them -- and start row S_b = start_rows[b] (i32, device; NULL: all 0).  At clock row k it stands at
 * its own row clamp(k - S_b, 0, N_b - 1): before its start it waits on its first row, after its end it holds its last row (what the
 * rollout flies once the cursor stops: the repeated last-row periods of the scored twins).  The group's horizon is H_g = max over
 * its missions of S_b + N_b, and every pair is compared at every k in [0, H_g).
 * GROUPS.  group_offsets [G+1] i64 (device), non-decreasing, group_offsets[0] = 0, group_offsets[G] = B: group g holds missions
 * [group_offsets[g], group_offsets[g+1]); NULL (G is ignored) = one group of all B.  Missions of different groups are never compared.
 * EXCLUDED MISSIONS.  A mission with no rows, or with any coefficient of its (clamped) segments not finite -- a singular knot system
 * writes NaN coefficients --, is excluded: nobody is compared with it, and it reports sep NaN, partner -1, row -1, conflicts 0, first
 * conflict -1, compared 0.  Everybody else reports in `compared` how many partners it WAS compared with, so a skipped neighbour is
 * visible: a mission is clear iff conflicts == 0 and compared == its group's size - 1.  Finite coefficients whose samples overflow
 * are outside the contract.
 * OUTPUTS per mission b (structure of arrays, like the audit block):
 *   sep  [B] f64: the minimum distance to any compared partner over [0, H_g); +inf when no partner was compared (a group of one, or
 *        all the others excluded)
 *   isep [UAVAC_SEP_ROWS][B] i32:  0 the partner's batch index      1 the clock row of the minimum      (both -1 when sep is +inf or NaN)
 *        2 conflicts = the number of partners j with min_k d^2(b, j, k) < r^2      3 the first clock row at which any partner is
 *        inside the radius (-1: none)      4 compared
 * ROUNDING AND TIES are part of the contract, as for the plan audit.  Positions come from the sampler's own fma chain, t = (double)(int)(r
 * - first row of the segment) * dt.  The distance is formed without contraction: dx = xi - xj, ..., d^2 = (dx * dx + dy * dy) + dz * dz
 * with separately rounded products and sums; the minimum is taken of the squares and one correctly rounded sqrt comes last; r^2 =
 * radius * radius is rounded once; inside means d^2 < r^2, strictly.  The minimum is the lexicographic minimum of (d^2, clock row,
 * partner index): the lowest row first, then the lowest partner -- an exact reduction that does not depend on order.  Every output
 * is therefore bit for bit what NumPy gives on the sampled rows with the same clamped indexing (uav_ac.scoring.separation_from_rows),
 * whatever the launch shape or what else is in the batch: a group audited alone gives the same numbers with the partner indices
 * shifted.  (Option "separation_split": 0 = automatic (default), 1 .. UAVAC_SEP_MAX_SPLIT = workgroups that share the partners of one
 * window of 64 missions; a tuning knob, same results.)  Cost: pairs x horizon -- about 13 fp64 operations per pair and clock row.
 * BAD INPUTS.  A negative start_rows[b] cannot be refused by the host: it is clamped to 0 and raises sticky flag 0 (uavac_take_flags),
 * like a bad segment count; so does one above 2^29 (clamped to 2^29), and a mission of more than 2^29 rows, which is excluded.
 * UAVAC_EINVAL before anything is enqueued: no context, a NULL required pointer (coeffs, seg_rows, sep, isep), B < 1, m outside 1 ..
 * UAVAC_MAX_SEGMENTS, dt not positive and finite, radius negative or not finite, G < 1 when group_offsets != NULL. */
#define UAVAC_SEP_ROWS 5
#define UAVAC_SEP_MAX_SPLIT 64
int uavac_minsnap_separation_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                 double dt, const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, double *sep,
                                 int32_t *isep);

/* CONFLICT LIST: the separation audit's conflict graph in CSR form -- not one partner and a count per mission, but every pair inside
 * the radius, with when and how near (csrc/minsnap_conflicts.hip).  From coefficients and row counts alone: no row is written, nothing
 * is read back, everything is enqueued on the ctx stream, scratch comes from the ctx arena (UAVAC_ENOMEM with a message when it cannot
 * be had).  coeffs / seg_rows / seg_offsets / B / m / dt / group_offsets / G / start_rows / radius exactly as in
 * uavac_minsnap_separation_dev, and CLOCK, GROUPS, EXCLUDED MISSIONS, ROUNDING and BAD INPUTS are the ones stated there.
 * THE LIST.  Mission i lists every partner j of its group with d^2(i, j, k) < r^2 -- strictly -- at some clock row k in [0, H_g).  An
 * excluded mission is nobody's partner and lists nothing.  The entries of mission i are [pair_offsets[i], pair_offsets[i + 1]), its
 * partners in ascending batch index; pair_offsets [B + 1] i64 is the exclusive prefix sum of the audit's `conflicts`.  Per entry e:
 *   pair_d [E] f64: the pair's minimum distance over [0, H_g): the minimum of the squares, then one correctly rounded sqrt
 *   pair_i [UAVAC_CONF_ROWS][capacity] i32:  0 the partner j      1 the first clock row inside      2 the last clock row inside
 *        3 the number of clock rows inside (less than last - first + 1 when the pair parts and meets again)      4 the clock row of the
 *        pair's minimum, the lowest one on a tie
 * Two calls, in the order counts -> offsets -> allocate -> fill that uavac_minsnap_delay_offsets_dev / uavac_minsnap_delay_dev have:
 *   uavac_minsnap_conflict_offsets_dev  pair_offsets [B + 1].  The caller reads pair_offsets[B], the number of entries E, to size the
 *                                       buffers.
 *   uavac_minsnap_conflicts_dev         pair_d and pair_i for buffers of `capacity` entries (the row stride of pair_i).  It repeats the
 *                                       discovery and relies on nothing the first call left behind.
 * WHAT THE RESULT GUARANTEES, on the same inputs:  diff(pair_offsets) == isep[2] of the audit.  The minimum of row 1 over a mission's
 * entries == isep[3].  For a mission with conflicts > 0 the audit's (sep, row, partner) is the lexicographic minimum of (pair_d, row 4,
 * partner) over its entries.  d^2 is bit-symmetric -- (xi - xj)^2 == (xj - xi)^2 --, so the entries (i -> j) and (j -> i) agree in
 * pair_d and in rows 1 .. 4.  Every output is bit for bit what NumPy gives on the sampled rows (uav_ac.scoring.conflicts_from_rows),
 * whatever the launch shape (options "separation_split" and "conflict_slots") or what else is in the batch: a group listed alone gives
 * the same records with the partner indices shifted.
 * BOUNDS are part of the contract.  Mission i writes nothing outside its slice, and nothing is written at or beyond `capacity` (or below
 * 0).  Entries of a slice that lie at or beyond `capacity` are dropped and raise sticky flag 2 (a buffer that is too small).  The plan
 * may have changed between the two calls: a mission that now has more or fewer partners than its slice holds fills what fits in
 * ascending partner order -- entries of the slice beyond its partners are left as they were -- and raises sticky flag 0.  capacity == 0
 * with pair_d == pair_i == NULL is allowed (pair_offsets[B] == 0: nothing to fill).
 * UAVAC_EINVAL before anything is enqueued: everything uavac_minsnap_separation_dev refuses (required pointers: coeffs, seg_rows,
 * pair_offsets), capacity < 0, pair_d or pair_i NULL with capacity > 0.
 * Cost: each call about one audit (pairs x horizon); the fill adds entries x horizon. */
#define UAVAC_CONF_ROWS 5
int uavac_minsnap_conflict_offsets_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B,
                                       int m, double dt, const int64_t *group_offsets, int G, const int32_t *start_rows, double radius,
                                       int64_t *pair_offsets);
int uavac_minsnap_conflicts_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                double dt, const int64_t *group_offsets, int G, const int32_t *start_rows, double radius,
                                const int64_t *pair_offsets, int64_t capacity, double *pair_d, int32_t *pair_i);

/* STAGGER: the call that acts on the separation audit's verdict -- prioritised deconfliction by start delay.  Within a group the
 * missions are taken in ascending batch index, which is the priority (the lowest index is never delayed), and each one is granted the
 * smallest start delay that keeps it outside the protection radius of every mission decided before it -- from coefficients and row
 * counts alone (csrc/minsnap_stagger.hip, csrc/fleet_search.h): no row is written, nothing is read back, everything is enqueued on the ctx stream, scratch
 * comes from the ctx arena.  coeffs / seg_rows / seg_offsets / B / m / dt / group_offsets / G / start_rows / radius exactly as in
 * uavac_minsnap_separation_dev, and CLOCK, GROUPS, EXCLUDED MISSIONS and ROUNDING are the ones stated there: mission b with start s
 * stands at its own row clamp(k - s, 0, N_b - 1); d^2 = (dx * dx + dy * dy) + dz * dz without contraction; r^2 = radius * radius
 * rounded once; inside means d^2 < r^2, strictly.  start_rows[b] is the BASE start S_b (NULL: all 0), clamped to 0 .. 2^29.
 * THE RULE.  Per group, the included missions in ascending batch index.  Mission i examines the candidates q = 0, 1, ..., max_steps in
 * that order; candidate q has start s = S_i + q * step.  A candidate is CLEAR iff for every included mission j < i of the group, at
 * its granted start T_j, and every clock row k in [0, max(s + N_i, T_j + N_j)) the two are not inside the radius (past that row both
 * hold their last rows, so any longer horizon gives the same answer; before min(s, T_j) both wait on their first rows).  The first
 * clear candidate is granted: T_i = s, steps = q.  If none is clear the mission is UNRESOLVED: steps = -1, T_i = S_i -- it stays where
 * it was and remains a partner for every later mission.
 * OUTPUT istag [UAVAC_STAGGER_ROWS][B] i32 (device), per mission b:  0 the granted start row T_b      1 steps, the candidate index
 * granted; -1 = unresolved; -2 = not examined (an excluded mission, or a group above UAVAC_STAGGER_MAX_GROUP)      2 earlier = the
 * number of missions it was checked against: the included missions before it in its group, so a skipped neighbour is visible like
 * `compared` in the audit.  A mission that was not examined reports its clamped base start, -2 and 0, and nobody is checked against
 * an excluded one.
 * Every output is an integer decided by comparisons of d^2 with r^2 on the audit's arithmetic, so it is exactly what NumPy gives on
 * the sampled rows (uav_ac.scoring.stagger_from_rows), whatever else is in the batch: a group staggered alone gives the same numbers.
 * WHAT THE RESULT GUARANTEES.  uavac_minsnap_separation_dev on the same plan, groups and radius with start_rows = istag[0] finds no
 * pair of RESOLVED missions (steps >= 0) inside the radius; in a group all of whose missions are resolved, conflicts == 0 everywhere.
 * WHAT IT IS NOT.  A greedy answer in priority order, not a minimum of the total delay; a later mission never moves an earlier one.
 * Two missions that share a first or last waypoint can never be resolved by waiting: they wait on, or hold, the same point.  To FLY
 * the granted starts make them part of the plan (uavac_minsnap_delay_dev below): the rollout's cursor has no start row and needs none.
 * Cost: about 13 fp64 operations per (mission, candidate lane, earlier partner, clock row); 64 candidates ride in the lanes of one
 * pass, so a mission that is clear at q = 0 costs one pass over its earlier partners; one workgroup per group, the missions of a
 * group one after the other.
 * BAD INPUTS.  As in the audit a start_rows[b] outside 0 .. 2^29 is clamped and raises sticky flag 0, and a mission of more than 2^29
 * rows is excluded and raises it.  A group of more than UAVAC_STAGGER_MAX_GROUP missions (its offsets are on the device) cannot be
 * refused by the host: all of its missions report their base start, -2 and 0, flag 0 is raised, the other groups are unaffected.
 * UAVAC_EINVAL before anything is enqueued: everything uavac_minsnap_separation_dev refuses (no context, a NULL required pointer --
 * coeffs, seg_rows, istag --, B < 1, m outside 1 .. UAVAC_MAX_SEGMENTS, dt not positive and finite, radius negative or not finite,
 * G < 1 when group_offsets != NULL), step < 1, max_steps outside 0 .. UAVAC_STAGGER_MAX_STEPS, (long long)step * max_steps > 2^29,
 * group_offsets == NULL with B > UAVAC_STAGGER_MAX_GROUP. */
#define UAVAC_STAGGER_ROWS 3
#define UAVAC_STAGGER_MAX_STEPS 1023
#define UAVAC_STAGGER_MAX_GROUP 256
int uavac_minsnap_stagger_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                              double dt, const int64_t *group_offsets, int G, const int32_t *start_rows, double radius,
                              int step, int max_steps, int32_t *istag);

/* STAGGER FOR GROUPS OF ANY SIZE: uavac_minsnap_stagger_dev's rule without UAVAC_STAGGER_MAX_GROUP (csrc/minsnap_stagger_wide.hip,
 * csrc/fleet_wide.h).  Every argument means what it means there, and istag [UAVAC_STAGGER_ROWS][B] holds the same integers: on a batch
 * whose groups all fit the narrow call the two calls' outputs are equal, and for any group sizes they are exactly what NumPy gives on
 * the sampled rows (uav_ac.scoring.stagger_from_rows(..., max_group = group_cap)).
 * group_cap >= 1 is the caller's bound on the largest group: a group above it (its offsets are on the device) is not examined -- base
 * start, -2 and 0 for all of its missions, sticky flag 0 --, as a group above UAVAC_STAGGER_MAX_GROUP is there.  group_offsets == NULL
 * means one group of all B.
 * HOW.  A group is cut into blocks of 64, 128 or 256 consecutive missions (option "search_block"; same results).  Per block two
 * launches: a SEED kernel, parallel over the whole chip, computes for every candidate of the block's missions whether it meets a
 * mission of an earlier block at its granted start -- one bit per (mission, candidate) in scratch --, then the narrow call's search
 * decides the block with one workgroup per group, its candidates' "met somebody" bits starting from the seed.  A candidate is clear
 * iff no partner decided before it is inside the radius at any clock row; an OR does not care how it is split, so the outputs depend
 * neither on the block size nor on the launch shape.  2 ceil(min(group_cap, B) / block) launches (the pre-pass, a search per block, a
 * seed per block but the first) and two memsets on the ctx stream, no host read; a launch for a block that no group has costs an empty launch, so give the smallest group_cap you can.
 * Scratch from the ctx arena: 8 + 8 (max_steps / 64 + 1) bytes per mission and 8 per group; UAVAC_ENOMEM when it does not fit.
 * UAVAC_EINVAL before anything is enqueued: everything uavac_minsnap_stagger_dev refuses but its group limit, group_cap < 1,
 * group_offsets == NULL with B > group_cap. */
int uavac_minsnap_stagger_wide_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                   double dt, const int64_t *group_offsets, int G, int group_cap, const int32_t *start_rows,
                                   double radius, int step, int max_steps, int32_t *istag);

/* DELAY AS A PLAN TRANSFORM: how start rows -- istag[0] of uavac_minsnap_stagger_dev, or any start_rows of the separation audit -- are
 * flown.  Mission b of the input (coeffs / times / seg_rows / seg_offsets / B / m / dt as in uavac_minsnap_audit_dev: seg_offsets NULL =
 * uniform, otherwise ragged with segment counts clamped to 1 .. m) has m_b segments and start row S_b = start_rows[b] (i32, device,
 * required).  The output is a RAGGED plan (csrc/minsnap_delay.hip):
 *   S_b == 0: the mission's m_b segments, copied as they are.
 *   S_b  > 0: m_b + 1 segments: a HOLD segment first -- c0 = c0 of the mission's first segment bit for bit, c1 .. c7 = 0, seg_rows = S_b,
 *             duration (double)S_b * dt -- then its own segments unchanged.
 * The sampler therefore writes S_b hold rows -- the position c0, velocity and acceleration 0, spline id 0 -- followed by the mission's
 * original rows bit for bit with their spline ids moved up by one.  A hold row is below MIN_HORIZONTAL_SPEED_FOR_YAW, so its yaw is
 * the mission's first heading, as for every leading row without a heading: first_yaw [B] of the delayed plan is the input's, and every
 * original row keeps its yaw.  (A hold row is NOT row 0 repeated: a solved mission's row 0 carries velocities of rounding size; only
 * its position is exactly c0.)  That position is what the separation audit's clock means by "waits on its first row":
 * uavac_minsnap_separation_dev on the delayed plan gives, bit for bit, what it gives on the input with start_rows.  A plan that starts
 * in motion (uavac_minsnap_plan_bc_dev) is accepted: its hold stands still and its first own row moves, which is the clock's meaning too.
 * Two calls, in the order row counts -> offsets -> allocate -> sample has everywhere here; everything is enqueued on the ctx stream and
 * the library reads nothing back:
 *   uavac_minsnap_delay_offsets_dev  out_seg_offsets [B+1] i64 = exclusive prefix sum of m_b + (S_b > 0).  The caller reads
 *                                    out_seg_offsets[B], the delayed plan's segment total, to size the buffers.
 *   uavac_minsnap_delay_dev          out_coeffs [S'][8][3], out_seg_rows [S'] and -- iff times != NULL -- out_times [S'], S' = that total.
 * Row offsets of the result: uavac_minsnap_row_offsets_ragged_dev(out_seg_rows, out_seg_offsets, B, m + 1).
 * BAD INPUTS follow the separation audit: a start row below 0 or above 2^29 is clamped and raises sticky flag 0 (uavac_take_flags).
 * UAVAC_EINVAL before anything is enqueued: no context, a NULL required pointer (start_rows and out_seg_offsets; for the second call
 * also coeffs, seg_rows, out_coeffs, out_seg_rows), B < 1, m outside 1 .. UAVAC_MAX_SEGMENTS - 1 (a delayed mission needs one more
 * segment), dt not positive and finite, times == NULL xor out_times == NULL. */
int uavac_minsnap_delay_offsets_dev(uavac_ctx *ctx, const int64_t *seg_offsets, int B, int m, const int32_t *start_rows,
                                    int64_t *out_seg_offsets);
int uavac_minsnap_delay_dev(uavac_ctx *ctx, const double *coeffs, const double *times, const int32_t *seg_rows, const int64_t *seg_offsets,
                            int B, int m, double dt, const int32_t *start_rows, const int64_t *out_seg_offsets, double *out_coeffs,
                            double *out_times, int32_t *out_seg_rows);

/* LAYER: prioritised deconfliction by OFFSET -- the second lever on the separation audit's verdict.  uavac_minsnap_stagger_dev makes a
 * mission wait; this call moves it, by whole steps of `delta` (metres; NED, so delta_z < 0 is one flight level UP; any direction is
 * allowed, a lateral offset is the same code).  From coefficients and row counts alone (csrc/minsnap_layer.hip, csrc/fleet_search.h): no row is written,
 * nothing is read back, everything is enqueued on the ctx stream, scratch comes from the ctx arena.  coeffs / seg_rows / seg_offsets /
 * B / m / dt / group_offsets / G / start_rows / radius exactly as in uavac_minsnap_stagger_dev, and CLOCK, GROUPS, EXCLUDED MISSIONS,
 * the priority (ascending batch index; the lowest index is never moved) and the group limit are the ones stated there.  start_rows[b]
 * are FIXED starts here (NULL: all 0; clamped to 0 .. 2^29) -- istag[0] of a stagger call, for instance: nobody is delayed by this call.
 * CANDIDATES.  Mission i examines the layers q = 0, 1, ..., max_steps in that order.  Layer q is the mission with the offset o_a =
 * fl((double)q * delta_a) added to c0 of EVERY one of its segments on the axes a = x, y, z: c0'_a = fl(c0_a + o_a) -- the product and
 * the sum are rounded one after the other, never as one fma.  Layer 0 is the mission as it is, bit for bit: nothing is added.
 * Positions are the sampler's fma chain on those coefficients (only its last fma per axis sees c0), partners j < i stand on their
 * GRANTED layers, the distance and the comparison are the audit's: d^2 = (dx * dx + dy * dy) + dz * dz without contraction, inside
 * means d^2 < r^2 strictly.  A candidate is CLEAR iff for every included mission j < i of the group and every clock row k in [0,
 * max(S_i + N_i, S_j + N_j)) the two are not inside the radius.  The first clear candidate is granted; a mission with none is
 * UNRESOLVED: steps = -1, it stays on layer 0 and remains a partner for every later mission.
 * OUTPUTS (device).  ilayer [UAVAC_LAYER_ROWS][B] i32, per mission b:  0 the granted layer (0 when unresolved or not examined)      1
 * steps, the candidate index granted; -1 = unresolved; -2 = not examined (an excluded mission, or a group above UAVAC_LAYER_MAX_GROUP)
 * 2 earlier = the included missions before it in its group.  offsets [B][3] f64: fl((double)layer * delta_a) of the granted layer,
 * ready for uavac_minsnap_shift_dev.  Every output is decided by comparisons of d^2 with r^2, so it is exactly what NumPy gives on the
 * sampled rows of the shifted plans (uav_ac.scoring.layer_from_rows), whatever else is in the batch.
 * WHAT THE RESULT GUARANTEES.  uavac_minsnap_separation_dev on the SHIFTED plan (uavac_minsnap_shift_dev with `offsets`), same groups,
 * radius and start_rows, finds no pair of RESOLVED missions inside the radius: the search evaluated exactly those coefficients.
 * WHAT IT IS NOT.  A greedy answer in priority order, not a minimum of the total displacement.  It knows nothing about obstacles unless
 * obstacles are given (uavac_minsnap_layer_obs_dev below): a layer can move a mission into a cuboid, so uavac_minsnap_audit_dev has to
 * be run again on the shifted plan.  An all-zero delta is
 * legal (every steps is then 0, -1 or -2); a delta so large that q * delta or a position overflows is outside the contract.
 * Cost: as stagger's, about 13 fp64 operations per (mission, candidate lane, earlier partner, clock row); 64 layers ride in the lanes of
 * one pass.
 * BAD INPUTS.  As in stagger: a start_rows[b] outside 0 .. 2^29 is clamped and raises sticky flag 0, a mission of more than 2^29 rows
 * is excluded and raises it, a group above UAVAC_LAYER_MAX_GROUP given on the device reports 0 / -2 / 0 for all of its missions and
 * raises it.  UAVAC_EINVAL before anything is enqueued: everything uavac_minsnap_separation_dev refuses (required pointers: coeffs,
 * seg_rows, ilayer, offsets), a delta that is not finite, max_steps outside 0 .. UAVAC_LAYER_MAX_STEPS, group_offsets == NULL with
 * B > UAVAC_LAYER_MAX_GROUP. */
#define UAVAC_LAYER_ROWS 3
#define UAVAC_LAYER_MAX_STEPS 1023
#define UAVAC_LAYER_MAX_GROUP 256
int uavac_minsnap_layer_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                            double dt, const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, double delta_x,
                            double delta_y, double delta_z, int max_steps, int32_t *ilayer, double *offsets);

/* LAYER WITH OBSTACLES: the same search, which also refuses every layer that puts the mission into a cuboid (csrc/minsnap_layer_obs.hip).
 * Every argument of uavac_minsnap_layer_dev means what it means there -- the clock, the groups, the excluded missions (judged on layer
 * 0), the clamped starts, the group limit, the rounding of the candidates and the distance arithmetic are that call's --, plus cuboids
 * [n_cuboids][6] f64 (device): xmin xmax ymin ymax zmin zmax as in uavac_minsnap_audit_dev, 0 <= n_cuboids <= UAVAC_AUDIT_MAX_CUBOIDS
 * (cuboids may be NULL with n_cuboids = 0).  The differences, and only these:
 * BLOCKED CANDIDATES.  Candidate layer q of mission i is BLOCKED when any of the mission's own rows 0 .. N_i - 1 on that layer -- the
 * positions the sampler writes for the plan shifted by fl(q * delta), bit for bit -- lies inside any cuboid by the audit's inclusive
 * test (x >= xmin && x <= xmax && ...: a NaN bound or an inverted box contains nothing).  Those rows cover the mission's whole shared
 * clock: before its start it holds row 0, after its end row N_i - 1.  The cuboid test comes first: a blocked candidate is never
 * compared with partners, and one that is both blocked and in conflict counts as blocked.
 * EVERY INCLUDED MISSION IS EXAMINED, the first of its group too (earlier = 0, no partners): it gets the lowest layer that no cuboid
 * blocks.  "The lowest index is never moved" becomes "is moved only by a cuboid".
 * UNRESOLVED: no layer 0 .. max_steps is both unblocked and clear: steps = -1, layer 0, and it remains a partner for later missions.
 * OUTPUTS (device).  ilayer [UAVAC_LAYER_OBS_ROWS][B] i32: rows 0-2 as uavac_minsnap_layer_dev's; row 3 blocked = how many of the
 * candidates q = 0 .. steps - 1 (0 .. max_steps when unresolved) a cuboid refused, 0 for a mission that was not examined.  steps = -1
 * with blocked = max_steps + 1 says that EVERY layer hits a cuboid: such a mission needs a new plan around the obstacle, not an offset.
 * offsets [B][3] as there.  With n_cuboids = 0 rows 0-2 and the offsets equal uavac_minsnap_layer_dev's, bit for bit, and row 3 is 0.
 * Exactly what NumPy gives on the sampled rows of the shifted plans (uav_ac.scoring.layer_obstacles_from_rows).
 * WHAT THE RESULT GUARANTEES.  On the plan shifted by `offsets`, uavac_minsnap_audit_dev with the same cuboids counts no row of a
 * RESOLVED mission inside any of them, and uavac_minsnap_separation_dev finds no pair of resolved missions inside the radius.  An
 * unresolved or unexamined mission stays where it was, wherever that is.  Still greedy in priority order.
 * Cost: the search's, plus per round of 64 candidates one pass over the mission's own rows (a position and 6 n_cuboids comparisons
 * per row and lane): measured at 65 536 missions in groups of 64, 1.26 x the search without obstacles with 4 cuboids, 1.8 x with 16.
 * UAVAC_EINVAL before anything is enqueued: everything uavac_minsnap_layer_dev refuses, n_cuboids outside 0 .. UAVAC_AUDIT_MAX_CUBOIDS,
 * cuboids == NULL with n_cuboids > 0. */
#define UAVAC_LAYER_OBS_ROWS 4
int uavac_minsnap_layer_obs_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                double dt, const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, double delta_x,
                                double delta_y, double delta_z, int max_steps, const double *cuboids, int n_cuboids, int32_t *ilayer,
                                double *offsets);

/* LAYER FOR GROUPS OF ANY SIZE: uavac_minsnap_layer_obs_dev's rule without UAVAC_LAYER_MAX_GROUP (csrc/minsnap_layer_wide.hip,
 * csrc/fleet_wide.h), by the decomposition of uavac_minsnap_stagger_wide_dev: per block of 64, 128 or 256 missions (option
 * "search_block"; same results) a seed kernel marks the candidate layers that meet a mission of an earlier block on its granted
 * layer, then the narrow call's search decides the block.  The cuboids are the search's business alone: a blocked candidate is
 * refused whatever its seed bit says, and `blocked` counts the refusals only.  Every argument means what it means in
 * uavac_minsnap_layer_obs_dev, ilayer is [UAVAC_LAYER_OBS_ROWS][B] and offsets [B][3] as there, and on a batch whose groups all fit the
 * narrow call the outputs are equal bit for bit; with n_cuboids = 0 (cuboids may be NULL) rows 0-2 and the offsets are
 * uavac_minsnap_layer_dev's and row 3 is 0.  For any group sizes: exactly what NumPy gives on the sampled rows of the shifted plans
 * (uav_ac.scoring.layer_obstacles_from_rows(..., max_group = group_cap)).
 * group_cap, the launches, the scratch and UAVAC_ENOMEM as in uavac_minsnap_stagger_wide_dev; a group above group_cap reports 0 / -2 /
 * 0 / 0 for all of its missions and raises sticky flag 0.
 * UAVAC_EINVAL before anything is enqueued: everything uavac_minsnap_layer_obs_dev refuses but its group limit, group_cap < 1,
 * group_offsets == NULL with B > group_cap. */
int uavac_minsnap_layer_wide_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                 double dt, const int64_t *group_offsets, int G, int group_cap, const int32_t *start_rows, double radius,
                                 double delta_x, double delta_y, double delta_z, int max_steps, const double *cuboids, int n_cuboids,
                                 int32_t *ilayer, double *offsets);

/* AGAINST COMMITTED TRAFFIC THAT NEVER MOVES: the audit and the two searches for new missions that are fitted around missions which
 * have already been granted a start and a layer, or are in the air (csrc/minsnap_separation_against.hip,
 * csrc/minsnap_stagger_against.hip, csrc/minsnap_layer_against.hip, csrc/fleet_against.h).  From coefficients and row counts alone:
 * no row is written, nothing is read back, everything is enqueued on the ctx stream, scratch comes from the ctx arena.
 * THE TRAFFIC is a second plan with its own arguments, in every one of the three calls the seven behind G: t_coeffs / t_seg_rows /
 * t_seg_offsets / Bt / mt like coeffs / seg_rows / seg_offsets / B / m of uavac_minsnap_separation_dev (t_seg_offsets NULL = uniform
 * with mt segments each, otherwise ragged with segment counts clamped to 1 .. mt), t_group_offsets [G + 1] i64 or NULL, t_start_rows
 * [Bt] i32 or NULL = all 0.  It shares dt and G with the plan.
 * CLOCK.  One row clock per group for both sides: a mission of the plan with start s and a traffic mission with start t_start_rows[j]
 * stand at their own rows clamp(k - start, 0, N - 1) -- each waits on its first row before its start and holds its last row after
 * its end.  The horizon covers both sides: H_g = max(S + N) over the included missions of the plan's group g AND of the traffic's.
 * GROUPS.  Group g of the plan meets group g of the traffic and nobody else's.  group_offsets and t_group_offsets are both NULL -- one
 * group each: all B against all Bt -- or both given, G + 1 entries each, ascending from 0 to B and from 0 to Bt; a group of either side
 * may be empty.  Offsets are clamped to the batch they index, as everywhere.
 * EXCLUDED MISSIONS, on either side: no rows, a coefficient that is not finite, or more than 2^29 rows.  Excluded traffic is
 * nobody's partner and is counted nowhere.  A TRAFFIC MISSION STANDS AS PLANNED at its start row: it has no candidate and no layer,
 * is never examined and never written -- no call writes to any of the traffic's arrays or has an output row for it.
 * ROUNDING is uavac_minsnap_separation_dev's: positions by the sampler's fma chain, d^2 = (dx * dx + dy * dy) + dz * dz without
 * contraction, r^2 = radius * radius rounded once, inside means d^2 < r^2 strictly.
 * BAD INPUTS.  Start rows of either side outside 0 .. 2^29 are clamped and raise sticky flag 0 (uavac_take_flags), and so does a
 * mission of more than 2^29 rows, which is excluded.  UAVAC_EINVAL before anything is enqueued: what the call without traffic
 * refuses (below, per call), then a NULL t_coeffs or t_seg_rows, Bt < 1, mt outside 1 .. UAVAC_MAX_SEGMENTS, offsets given on one
 * side only (group_offsets == NULL xor t_group_offsets == NULL).
 *
 * uavac_minsnap_separation_against_dev: THE CROSS AUDIT.  For every mission of the plan the closest approach to any included traffic
 * mission of its group on the shared clock.  Missions of the plan are never compared with each other.  sep [B] f64 and isep
 * [UAVAC_SEP_ROWS][B] i32 have the layout of uavac_minsnap_separation_dev with these meanings: sep the minimum distance; row 0 partner
 * = the TRAFFIC batch index (0 .. Bt - 1); 1 the clock row of the minimum; 2 conflicts = the number of traffic missions that come
 * inside the radius; 3 the first clock row with one inside (-1: none); 4 compared = the included traffic missions of the group.  The
 * same arithmetic and ties: the lexicographic minimum of (d^2, row, partner), one correctly rounded sqrt last, strict <.  A mission
 * whose group has no included traffic reports +inf, -1, -1, 0, -1, 0; an excluded mission of the plan NaN, -1, -1, 0, -1, 0.  Bit for
 * bit what NumPy gives on the sampled rows (uav_ac.scoring.separation_against_rows), whatever the launch shape (option
 * "separation_split").  Refuses what uavac_minsnap_separation_dev refuses (required pointers: coeffs, seg_rows, sep, isep).  Scratch:
 * that call's, plus 8 bytes per traffic mission.  Cost: plan missions x traffic missions of the group x horizon.
 *
 * uavac_minsnap_stagger_against_dev: uavac_minsnap_stagger_wide_dev's rule and outputs -- group_cap, start_rows (the BASE starts),
 * step, max_steps and istag [UAVAC_STAGGER_ROWS][B] mean what they mean there, and group_cap bounds the PLAN's missions of a group
 * -- with ONE MORE CLAUSE IN "CLEAR": candidate q of mission i is clear iff it is outside the radius of every included mission j < i
 * of its group at its granted start T_j AND of every included traffic mission of its group at that mission's start, at every clock
 * row below the horizon, which covers the traffic's ends too.  earlier (row 2) counts the included traffic of the group PLUS the
 * included plan missions before it.  The first included mission of a group is examined whenever its group has included traffic (in
 * uavac_minsnap_stagger_wide_dev it never is).  A group without included traffic gives exactly that call's answers.  Exactly what
 * NumPy gives on the sampled rows (uav_ac.scoring.stagger_against_rows(..., max_group = group_cap)), whatever the block size.
 * WHAT THE RESULT GUARANTEES: uavac_minsnap_separation_against_dev with start_rows = istag[0] reports conflicts == 0 for every
 * RESOLVED mission, and uavac_minsnap_separation_dev on the plan alone finds no pair of resolved missions inside the radius.  Two
 * traffic missions that conflict with each other stay as they are: this call decides nothing about them.
 * HOW.  The traffic is a virtual earlier block of the block-wise search (csrc/fleet_wide.h): behind the two pre-passes and the
 * memsets one small kernel fills every group's carry with the traffic's count and horizon, and ONE seed kernel over all B missions,
 * parallel over the chip, ORs into the seed words what the traffic does to every candidate 0 .. max_steps; then the seed / search
 * launches per block as there, unchanged.  Three launches more than that call.  Refuses what uavac_minsnap_stagger_wide_dev refuses.
 * Scratch: that call's, plus 8 bytes per traffic mission; UAVAC_ENOMEM with a message when it does not fit.  Cost: the seed is
 * missions x (max_steps / 64 + 1) rounds x traffic of the group x horizon, a round ending early once all its candidates are hit.
 *
 * uavac_minsnap_layer_against_dev: the same extension of uavac_minsnap_layer_wide_dev -- the cuboid policy: every included mission
 * is examined, a blocked candidate is refused before anybody is compared; ilayer is [UAVAC_LAYER_OBS_ROWS][B], offsets [B][3], cuboids
 * may be NULL with n_cuboids = 0.  start_rows are FIXED starts.  A traffic mission is compared AS IT IS, on no layer: a caller who has
 * layered the traffic passes the shifted plan (uavac_minsnap_shift_dev).  earlier counts the included traffic plus the included plan
 * missions before it; a group without included traffic gives exactly uavac_minsnap_layer_wide_dev's answers.  Exactly what NumPy
 * gives (uav_ac.scoring.layer_against_rows(..., max_group = group_cap)).  Refuses what uavac_minsnap_layer_wide_dev refuses.  Launches,
 * scratch and UAVAC_ENOMEM as in uavac_minsnap_stagger_against_dev.
 *
 * uavac_minsnap_conflict_against_offsets_dev, uavac_minsnap_conflicts_against_dev: THE CROSS CONFLICT LIST, the cross audit's conflict
 * graph in CSR form (csrc/minsnap_conflicts_against.hip).  What uavac_minsnap_conflict_offsets_dev / uavac_minsnap_conflicts_dev are to
 * uavac_minsnap_separation_dev, these two are to the cross audit: the same two calls in the same order (offsets -> read pair_offsets[B]
 * -> allocate -> fill), pair_offsets [B + 1] i64, pair_d [capacity] f64 and pair_i [UAVAC_CONF_ROWS][capacity] i32 with the rows of
 * CONFLICT LIST above.  Everything in this block applies -- clock, groups, excluded missions, rounding, bad inputs and their flags --
 * and so does the conflict list's contract:
 *   THE LIST.  Mission i of the PLAN lists every included traffic mission j of its group with d^2(i, j, k) < r^2 -- strictly -- at some
 *   clock row k in [0, H_g), H_g over both sides, in ascending j; row 0, the partner, is the TRAFFIC batch index (0 .. Bt - 1).
 *   Missions of the plan are never compared with each other.  An excluded plan mission lists nothing, excluded traffic is listed by
 *   nobody, a group without included traffic lists nothing.
 *   The fill repeats the discovery and relies on nothing the offsets call left behind.
 *   BOUNDS.  An entry is written only inside the mission's slice, at or above 0 and below `capacity`.  Sticky flag 2 is raised when the
 *   buffers end inside a slice; sticky flag 0 when a slice holds another number of entries than the mission has partners (what fits is
 *   filled in ascending partner order, the rest of the slice is left as it was).  capacity == 0 with pair_d == pair_i == NULL is allowed.
 *   Neither call writes to any array of either plan.
 * WHAT THE RESULT GUARANTEES, on the same inputs as uavac_minsnap_separation_against_dev: diff(pair_offsets) == isep[2], the cross
 * audit's conflicts.  The minimum of row 1 over a mission's entries == isep[3], its first_conflict.  For a mission with an entry the
 * audit's (sep, row, partner) is the lexicographic minimum of (pair_d, row 4, partner) over its entries.  d^2 is bit-symmetric, so the
 * list of the traffic against the plan (sides and groups swapped) is the transpose of this one, bit for bit
 * (uav_ac.scoring.conflicts_transposed).  Every output is bit for bit what NumPy gives on the sampled rows
 * (uav_ac.scoring.conflicts_against_rows), whatever the launch shape (options "separation_split" and "conflict_slots") or what else is
 * in either batch: a group of both sides listed alone gives the same records with the partner indices shifted.
 * UAVAC_EINVAL before anything is enqueued: what uavac_minsnap_separation_against_dev refuses for the two plans (required pointers:
 * coeffs, seg_rows, pair_offsets; then the traffic's list above), then capacity < 0, pair_d or pair_i NULL with capacity > 0.
 * Rounds: the discovery is repeated over the tile slots until ceil(Bt / 64) j-tiles, the most a traffic group can have, are covered.
 * Scratch: the plan-side list's, plus 8 bytes per traffic mission.  Cost: each call about one cross audit; the fill adds entries x
 * horizon. */
int uavac_minsnap_conflict_against_offsets_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B,
                                               int m, double dt, const int64_t *group_offsets, int G, const double *t_coeffs,
                                               const int32_t *t_seg_rows, const int64_t *t_seg_offsets, int Bt, int mt,
                                               const int64_t *t_group_offsets, const int32_t *t_start_rows, const int32_t *start_rows,
                                               double radius, int64_t *pair_offsets);
int uavac_minsnap_conflicts_against_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B,
                                        int m, double dt, const int64_t *group_offsets, int G, const double *t_coeffs,
                                        const int32_t *t_seg_rows, const int64_t *t_seg_offsets, int Bt, int mt,
                                        const int64_t *t_group_offsets, const int32_t *t_start_rows, const int32_t *start_rows, double radius,
                                        const int64_t *pair_offsets, int64_t capacity, double *pair_d, int32_t *pair_i);
int uavac_minsnap_separation_against_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B,
                                         int m, double dt, const int64_t *group_offsets, int G, const double *t_coeffs,
                                         const int32_t *t_seg_rows, const int64_t *t_seg_offsets, int Bt, int mt,
                                         const int64_t *t_group_offsets, const int32_t *t_start_rows, const int32_t *start_rows,
                                         double radius, double *sep, int32_t *isep);
int uavac_minsnap_stagger_against_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                      double dt, const int64_t *group_offsets, int G, const double *t_coeffs, const int32_t *t_seg_rows,
                                      const int64_t *t_seg_offsets, int Bt, int mt, const int64_t *t_group_offsets,
                                      const int32_t *t_start_rows, int group_cap, const int32_t *start_rows, double radius, int step,
                                      int max_steps, int32_t *istag);
int uavac_minsnap_layer_against_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                    double dt, const int64_t *group_offsets, int G, const double *t_coeffs, const int32_t *t_seg_rows,
                                    const int64_t *t_seg_offsets, int Bt, int mt, const int64_t *t_group_offsets,
                                    const int32_t *t_start_rows, int group_cap, const int32_t *start_rows, double radius, double delta_x,
                                    double delta_y, double delta_z, int max_steps, const double *cuboids, int n_cuboids, int32_t *ilayer,
                                    double *offsets);

/* OFFSET AS A PLAN TRANSFORM: how the granted layers are flown and audited.  out_coeffs = coeffs (the same layout: [B][8 m][3] uniform
 * with seg_offsets == NULL, or [total_segments][8][3] ragged with seg_offsets [B+1]; total_segments is ignored for a uniform batch)
 * with c0'[a] = fl(c0[a] + offsets[b][a]) in every segment of mission b; c1 .. c7 are copied bit for bit, and so is every segment of a
 * mission whose three offsets are all +-0 (a -0.0 stays -0.0).  offsets [B][3] f64 (device), e.g. the output of uavac_minsnap_layer_dev;
 * non-finite offsets pass through, and the mission then counts as excluded downstream like any non-finite plan.  Durations, row
 * counts, offsets tables and first headings of the shifted plan are the input's.  The sampled rows of the shifted plan differ from the
 * input's in columns 0-2 only.  out_coeffs may be coeffs itself (in place).  One kernel on the ctx stream; nothing is read back.
 * The obstacle audit has to be re-run on the shifted plan.
 * UAVAC_EINVAL before anything is enqueued: no context, a NULL pointer (coeffs, offsets, out_coeffs), B < 1, m outside 1 ..
 * UAVAC_MAX_SEGMENTS, seg_offsets != NULL with total_segments outside 1 .. B * m. */
int uavac_minsnap_shift_dev(uavac_ctx *ctx, const double *coeffs, const int64_t *seg_offsets, int B, int m, int64_t total_segments,
                            const double *offsets, double *out_coeffs);

/* TAKE: a gather of missions -- how missions of a plan are selected, reordered and merged on the device (csrc/minsnap_take.hip).  The
 * input is a plan as uavac_minsnap_delay_dev takes it (coeffs / times / seg_rows / seg_offsets / B / m: seg_offsets NULL = uniform,
 * otherwise ragged with segment counts clamped to 1 .. m; times may be NULL), optionally first_yaw [B] f64, and index [n] i32 (device,
 * required): duplicates and any order are allowed, n may exceed B.  The output is a RAGGED plan of n missions: mission i of the result
 * is mission index[i] of the input, every bit of it -- its m_index[i] segments' 24 coefficients, row counts and (iff times != NULL)
 * durations, and (iff first_yaw != NULL) its first heading.  Nothing is computed, so the sampled rows of output mission i are the rows
 * of input mission index[i] bit for bit, and so is everything that is computed per mission (uavac_minsnap_audit_dev, a plan-fed
 * rollout's lane); what is computed per group (uavac_minsnap_separation_dev, stagger, layer) of a taken group is the group's with the
 * partners renumbered, whatever else was in the batch.  uav_ac.scoring.take_parts is the construction in NumPy.
 * Two calls, in the order offsets -> allocate -> fill that uavac_minsnap_delay_dev has; everything is enqueued on the ctx stream and
 * the library reads nothing back:
 *   uavac_minsnap_take_offsets_dev  out_seg_offsets [n+1] i64 = exclusive prefix sum of m_index[i].  The caller reads out_seg_offsets[n],
 *                                   the result's segment total (at most n * m), to size the buffers.
 *   uavac_minsnap_take_dev          out_coeffs [S'][8][3], out_seg_rows [S'], -- iff times != NULL -- out_times [S'], S' = that total, and
 *                                   -- iff first_yaw != NULL -- out_first_yaw [n].
 * Row offsets of the result: uavac_minsnap_row_offsets_ragged_dev(out_seg_rows, out_seg_offsets, n, m).  The outputs must not overlap
 * the inputs.
 * BAD INPUTS.  An index[i] outside 0 .. B - 1 cannot be refused without a read-back: it is clamped into that range and raises sticky
 * flag 0 (uavac_take_flags), like a bad start row.  UAVAC_EINVAL before anything is enqueued: no context, a NULL required pointer (index
 * and out_seg_offsets; for the second call also coeffs, seg_rows, out_coeffs, out_seg_rows), B < 1, n < 1, m outside 1 ..
 * UAVAC_MAX_SEGMENTS, times == NULL xor out_times == NULL, first_yaw == NULL xor out_first_yaw == NULL.
 * Cost: one read and one write of what is taken -- 200 bytes per segment with durations -- by one thread per 16 bytes of coefficients. */
int uavac_minsnap_take_offsets_dev(uavac_ctx *ctx, const int64_t *seg_offsets, int B, int m, const int32_t *index, int n,
                                   int64_t *out_seg_offsets);
int uavac_minsnap_take_dev(uavac_ctx *ctx, const double *coeffs, const double *times, const int32_t *seg_rows, const int64_t *seg_offsets,
                           int B, int m, const double *first_yaw, const int32_t *index, int n, const int64_t *out_seg_offsets,
                           double *out_coeffs, double *out_times, int32_t *out_seg_rows, double *out_first_yaw);

/* ORDER: priorities into a within-group order -- what a priority other than the batch index needs.  The searches
 * (uavac_minsnap_stagger_dev, uavac_minsnap_layer_dev, uavac_minsnap_layer_obs_dev) take the missions of a group in ascending batch
 * index; with this call the plan is reordered within its groups (uavac_minsnap_take_dev with index = order), the search runs on it
 * unchanged, and its per-mission answers are gathered back with rank.  priority [B] f64 (device); group_offsets [G + 1] i64 / G as in
 * uavac_minsnap_separation_dev, clamped to the batch in the same way (NULL: one group of all B); order, rank [B] i32 (device).
 * THE RULE.  Within each group the missions are sorted by the total order "a before b" iff  p_a is a number and p_b is NaN,  or
 * p_a < p_b,  or  (p_a == p_b or both are NaN) and a < b.  So a LOWER priority goes first, -0.0 ties with +0.0, NaN comes after +inf,
 * and ties go to the lower batch index: priority[b] = b is the identity.
 * OUTPUTS.  order[g0 + k] = the mission in slot k of its group [g0, g1); rank is the inverse permutation, rank[order[s]] = s.  A mission
 * that no group holds keeps its place: order[b] = rank[b] = b.  With offsets that follow the contract (ascending from 0 to B) order is
 * a permutation of 0 .. B - 1 that maps every group onto itself, so the same group_offsets describe the reordered batch.  No write
 * leaves [B], whatever the offsets hold; with offsets that do not ascend the contents of order and rank are unspecified.
 * Every comparison is exact, so there is no rounding and the result does not depend on the launch shape: it is what NumPy gives
 * (uav_ac.scoring.priority_order).  Any group size is accepted -- the limits of the searches are theirs.
 * Cost: a counting rank, a mission's slot is the number of missions of its group that come before it: the sum of g^2 comparisons over
 * the groups, one thread per mission, the priorities through LDS tiles.  One kernel on the ctx stream; nothing is read back.
 * UAVAC_EINVAL before anything is enqueued: no context, a NULL priority / order / rank, B < 1, G < 1 when group_offsets != NULL. */
int uavac_fleet_order_dev(uavac_ctx *ctx, const double *priority, const int64_t *group_offsets, int G, int B, int32_t *order,
                          int32_t *rank);

/* ENVELOPE: every mission's SWEPT BOX, per mission, WITHOUT sampling its rows -- what the split of a fleet into independent airspaces
 * (uavac_fleet_airspaces_dev below) starts from.  One kernel walks every mission's rows as the plan audit does
 * (csrc/minsnap_envelope.hip) and stores none of them.  coeffs / seg_rows / seg_offsets / B / m / dt as in uavac_minsnap_audit_dev
 * (seg_offsets NULL = uniform, otherwise ragged with segment counts clamped to 1 .. m).
 *   reach [B][3] f64 (device) or NULL: an offset per mission whose plan is covered as well, e.g. fl(max_steps * delta) of a layer search
 *   env   [B][6] f64 (device): lo x, lo y, lo z, hi x, hi y, hi z -- the minimum and the maximum, per axis, of the positions the sampler
 *         writes for the mission and, with reach, of the positions it writes for the mission shifted by reach[b]
 *         (uavac_minsnap_shift_dev) too: the hull of both.
 * ROUNDING is part of the contract.  Positions by the sampler's fma chain, hence the bits of the rows; the shifted side from c0' =
 * fl(c0 + reach[b][a]) in every segment -- a rounded sum of its own, then the same chain: the two roundings of uavac_minsnap_shift_dev,
 * which also leaves a mission alone whose three reach components are all +-0.  Minimum and maximum are exact and independent of order,
 * so the result does not depend on the launch shape (option "audit_lanes": 16 or 64 lanes per mission, same results); -0.0 and +0.0
 * are the same number here: the contract is equality as numbers, NaN in the same places (uav_ac.scoring.envelope_from_rows on the
 * sampled rows).  A mission without rows, or with ANY position that is not finite on either side, reports NaN in all six.
 * WHY A BOX IS ENOUGH.  Rounded subtraction, multiplication and addition are monotone, the chain ends per axis with fma(p, t, c0), which
 * is monotone in c0, and a layer's coefficient fl(c0 + fl(q * delta_a)) is monotone in q: every row of every layer q = 0 .. max_steps
 * lies, per axis, between the mission's rows on layer 0 and on layer max_steps, inside the box with reach = fl(max_steps * delta).  Hold
 * rows and the rows a mission waits on before its start are its own first and last rows.  So if fl(lo_i - hi_j) >= radius on some axis,
 * every d^2 a search can compute for the pair is >= radius * radius, whatever the starts and the granted layers: never inside.
 * Exactly env [B][6] is written, nothing is read back, one kernel on the ctx stream.
 * UAVAC_EINVAL before anything is enqueued: no context, a NULL coeffs / seg_rows / env, B < 1, m outside 1 .. UAVAC_MAX_SEGMENTS, dt not
 * positive and finite. */
int uavac_minsnap_envelope_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                               double dt, const double *reach, double *env);

/* AIRSPACES: a fleet split into groups of missions that can never meet.  The prioritised searches (uavac_minsnap_stagger_dev,
 * uavac_minsnap_layer_dev and their _obs / _wide forms) cost the square of a group's size, and `group_offsets` is the only lever on it;
 * this call computes the finest split that changes no answer.  A mission's greedy decision depends only on earlier missions that can
 * come inside the radius of it; those are all in its connected component of the graph below; so the unchanged search, run per
 * component on the missions in their original relative order, gives every mission the start / steps / layer / blocked that the search
 * over the whole group gives (`earlier` becomes the count within the component).  csrc/fleet_airspaces.hip;
 * uav_ac.scoring.airspaces_from_envelopes states the rule in NumPy, round for round.
 *   env [B][6] f64 (device): the boxes of uavac_minsnap_envelope_dev.  group_offsets [G + 1] i64 / G as in uavac_fleet_order_dev,
 *   clamped to the batch in the same way (NULL: one group of all B); a mission that no group holds is linked to nobody.
 *   labels [B] i32 (device), info [2] i32 (device).
 * THE LINK.  Missions i != j of the same group are linked iff on all three axes fl(lo_i - hi_j) < radius and fl(lo_j - hi_i) < radius:
 * one rounded subtraction each, nothing contracted, strictly less -- a gap of exactly the radius is no link, radius 0 links boxes that
 * overlap by more than a face, and a box with a NaN links to nobody.
 * ONE ROUND, on whole arrays (double-buffered, so it is reproducible):  m[i] = min(lab[i], min of lab[j] over the linked j);
 * lab'[i] = m[m[i]].  The first round starts from lab[i] = i; with resume = 1 from `labels` as given (the output of an earlier call
 * on the same boxes; a value outside 0 .. B - 1 is read as the nearest index).  The call enqueues at most `rounds` rounds, and a round
 * whose predecessor changed nothing exits at once: no workgroup waits for another, there is no grid-wide barrier.
 *   info[0] = how many rounds of this call changed a label;  info[1] = 1 iff the last round that ran changed nothing.
 * With info[1] = 1 the labels are FINAL: labels[b] is the lowest batch index of b's component -- unique, so it depends neither on the
 * launch shape nor on how the rounds were split over calls.  With info[1] = 0 they describe a FINER partition than the components:
 * call again with resume = 1, and NEVER hand such labels to a search -- its answers would not be the group's.
 * Cost per round: the sum of g^2 box tests over the groups, one lane per mission, the partners through LDS tiles; two launches per
 * round and two more per call; scratch (B + rounds words) from the ctx arena.  Exactly labels [B] and info [2] are written.
 * UAVAC_EINVAL before anything is enqueued: no context, a NULL env / labels / info, B < 1, G < 1 when group_offsets != NULL, radius
 * negative or not finite, rounds < 1, resume outside {0, 1}.  UAVAC_ENOMEM / UAVAC_EHIP when the scratch cannot be had. */
int uavac_fleet_airspaces_dev(uavac_ctx *ctx, const double *env, const int64_t *group_offsets, int G, int B, double radius, int rounds,
                              int resume, int32_t *labels, int32_t *info);

/* FLOWN SEPARATION: the separation audit of a FLIGHT.  uavac_minsnap_separation_dev speaks about plans; the vehicles track them with an
 * error.  This call reads the positions in a rollout's state log and reports, in the same terms and with the same exactness, how close
 * the vehicles came (csrc/flown_separation.hip): nothing is read back, everything is enqueued on the ctx stream, scratch from the arena.
 *   state_log [K][13][pitch] f64 (device) as the rollouts write it: positions are rows 0-2; pitch >= B doubles per row (option
 *             "log_pitch"); columns B .. pitch - 1 are never read.  The CLOCK is the tick k = 0 .. K - 1 (the log's first index: clock row
 *             of the plan = k / inner_per_outer).
 *   group_offsets, G, radius, sep [B], isep [UAVAC_SEP_ROWS][B] exactly as in uavac_minsnap_separation_dev.
 * For vehicle i, a partner j != i of its group and tick k: dx = xi - xj, ..., d^2 = (dx * dx + dy * dy) + dz * dz without contraction;
 * r^2 = radius * radius rounded once; inside means d^2 < r^2, strictly.  A pair-tick is VALID iff its d^2 is not NaN.
 *   sep       one correctly rounded sqrt of the lexicographic minimum of (d^2, tick, partner) over the valid pair-ticks
 *   isep  0   that partner      1 that tick      2 conflicts = the partners with some valid pair-tick inside the radius
 *         3   the first tick with anybody inside (-1: none)      4 compared = the partners with at least one valid pair-tick
 * With no valid pair-tick at all -- a group of one, or a vehicle whose log is NaN throughout --: sep = +inf and -1 / -1 / 0 / -1 / 0.
 * `compared` makes a vehicle whose log holds NaN visible: uav_ac.scoring.separation_ok applies unchanged.  Positions that are
 * infinite, or whose differences overflow, are outside the contract (they do not fault).
 * Every reduction is a lexicographic minimum, an integer sum over disjoint partners, an OR or an integer minimum, so every output is bit
 * for bit what NumPy gives on the log (uav_ac.scoring.separation_from_log) whatever the launch shape (option "separation_split" applies
 * as it does to the plan audit), the pitch, or what else is in the batch: a group audited alone gives the same numbers with the partner
 * indices shifted.  Cost: pairs x ticks, about 13 fp64 operations per pair-tick; the log's positions are read once per j-tile of 64.
 * UAVAC_EINVAL before anything is enqueued: no context, NULL state_log, sep or isep, K < 1, B < 1, pitch < B, radius negative or not
 * finite, G < 1 when group_offsets != NULL. */
int uavac_flown_separation_dev(uavac_ctx *ctx, const double *state_log, int K, int B, int64_t pitch, const int64_t *group_offsets, int G,
                               double radius, double *sep, int32_t *isep);

/* FLOWN CONFLICT LIST: the flown separation audit's conflict graph in CSR form -- not one partner and a count per vehicle, but every
 * pair a flight brought inside the radius, with when and how near (csrc/flown_conflicts.hip).  What uavac_minsnap_conflicts_dev is to
 * uavac_minsnap_separation_dev, this is to uavac_flown_separation_dev: nothing is read back, no log leaves the device, everything is
 * enqueued on the ctx stream, scratch comes from the ctx arena (UAVAC_ENOMEM with a message when it cannot be had).
 * state_log / K / B / pitch / group_offsets / G / radius exactly as in uavac_flown_separation_dev, and so are the log's layout
 * [K][13][pitch], the CLOCK (the tick k = 0 .. K - 1), the columns B .. pitch - 1 that are never read, d^2 = (dx * dx + dy * dy) + dz * dz
 * without contraction, r^2 = radius * radius rounded once, inside meaning d^2 < r^2, strictly, and a pair-tick being VALID iff its d^2
 * is not NaN.
 * THE LIST.  Vehicle i lists every partner j != i of its group that has a valid pair-tick inside the radius.  The entries of vehicle i
 * are [pair_offsets[i], pair_offsets[i + 1]), its partners in ascending batch index; pair_offsets [B + 1] i64 is the exclusive prefix
 * sum of the flown audit's `conflicts`.  Per entry e:
 *   pair_d [E] f64: one correctly rounded sqrt of the minimum d^2 over the pair's valid pair-ticks
 *   pair_i [UAVAC_CONF_ROWS][capacity] i32:  0 the partner j      1 the first tick inside      2 the last tick inside
 *        3 the number of ticks inside (less than last - first + 1 when the pair parts and meets again; a NaN tick in the middle of an
 *        incursion is not inside and is not counted)      4 the tick of the pair's minimum, the lowest one on a tie
 * UAVAC_CONF_ROWS and the rows are those of the plan's list, with ticks where it has clock rows (clock row of the plan = tick /
 * inner_per_outer).  Two calls, in the order counts -> offsets -> allocate -> fill that the plan's list has:
 *   uavac_flown_conflict_offsets_dev  pair_offsets [B + 1].  The caller reads pair_offsets[B], the number of entries E, to size the
 *                                     buffers.
 *   uavac_flown_conflicts_dev         pair_d and pair_i for buffers of `capacity` entries (the row stride of pair_i).  It repeats the
 *                                     discovery and relies on nothing the first call left in the arena.
 * WHAT THE RESULT GUARANTEES, on the same inputs as uavac_flown_separation_dev:  diff(pair_offsets) == isep[2].  The minimum of row 1
 * over a vehicle's entries == isep[3].  For a vehicle with conflicts > 0 the audit's (sep, tick, partner) is the lexicographic minimum
 * of (pair_d, row 4, partner) over its entries.  d^2 is bit-symmetric, so the entries (i -> j) and (j -> i) agree in pair_d and in rows
 * 1 .. 4.  Every output is bit for bit what NumPy gives on the log (uav_ac.scoring.conflicts_from_log), whatever the pitch, the launch
 * shape (options "separation_split" and "conflict_slots") or what else is in the batch: a group listed alone gives the same records
 * with the partner indices shifted.
 * BOUNDS are part of the contract, and they are those of uavac_minsnap_conflicts_dev.  Vehicle i writes nothing outside its slice, and
 * nothing is written at or beyond `capacity` (or below 0).  Entries of a slice that lie at or beyond `capacity` are dropped and raise
 * sticky flag 2.  The log or the radius may have changed between the two calls: a vehicle that now has more or fewer partners than its
 * slice holds fills what fits in ascending partner order -- entries of the slice beyond its partners are left as they were -- and
 * raises sticky flag 0.  capacity == 0 with pair_d == pair_i == NULL is allowed (pair_offsets[B] == 0: nothing to fill).
 * UAVAC_EINVAL before anything is enqueued: everything uavac_flown_separation_dev refuses (required pointers: state_log,
 * pair_offsets), capacity < 0, pair_d or pair_i NULL with capacity > 0.
 * Cost: each call about one flown audit (pairs x ticks); the fill adds entries x ticks, each entry reading its two columns of the log
 * (lanes across consecutive entries, which share their owner's column and their group's span of a log row). */
int uavac_flown_conflict_offsets_dev(uavac_ctx *ctx, const double *state_log, int K, int B, int64_t pitch, const int64_t *group_offsets,
                                     int G, double radius, int64_t *pair_offsets);
int uavac_flown_conflicts_dev(uavac_ctx *ctx, const double *state_log, int K, int B, int64_t pitch, const int64_t *group_offsets, int G,
                              double radius, const int64_t *pair_offsets, int64_t capacity, double *pair_d, int32_t *pair_i);

/* FLOWN AUDIT: the plan audit of a FLIGHT.  uavac_minsnap_audit_dev says what a plan's rows would show against the flight limits and the
 * cuboids; the vehicles track the plan with an error, and uavac_minsnap_layer_obs_dev deliberately puts missions next to cuboids.  This
 * call reads a rollout's state log once and reports, per vehicle, what it DID (csrc/flown_audit.hip): nothing is read back, everything is
 * enqueued on the ctx stream, scratch from the arena.
 *   state_log [K][13][pitch] f64 (device) as the rollouts write it and as uavac_flown_separation_dev takes it; its rows are
 *             x y z | q0 q1 q2 q3 | vx vy vz | p q r (NED; the quaternion scalar first: row 3 is 1 at identity, uavac_state_init_dev);
 *             columns B .. pitch - 1 are never read.  The clock is the tick k = 0 .. K - 1.
 *   cuboids   [n_cuboids][6] f64 (device): xmin xmax ymin ymax zmin zmax, 0 <= n_cuboids <= UAVAC_AUDIT_MAX_CUBOIDS.
 *             n_cuboids == 0: cuboids, hit_ticks, first_hit, clearance and clearance_tick must all be NULL.
 * VALID TICK.  Tick k of vehicle b is valid iff all 13 logged values are finite.  Peaks, hits and clearances are taken over the valid
 * ticks only.
 *   audit [UAVAC_FLOWN_AUDIT_ROWS][B] f64 (SoA like the plan audit's block):
 *     0 the number of valid ticks (exact as a double)     4 peak speed sqrt(max((vx * vx + vy * vy) + vz * vz))
 *     1 peak horizontal speed sqrt(max(vx * vx + vy * vy))    5 max |2 * (q1 * q3 + q0 * q2)|
 *     2 peak climb rate   max(-vz)   (NED)                6 max |2 * (q2 * q3 - q0 * q1)|
 *     3 peak descent rate max(vz)                         7 peak body rate sqrt(max((p * p + q * q) + r * r))
 *     Rows 5 and 6 are the rotation-matrix elements R13 and R23 the control law clips its attitude COMMAND to with max_tilt
 *     (csrc/control_law.h); the flown attitude may exceed the command.
 *   first_bad [B] i32: the first invalid tick, -1 when every tick is valid.
 *   hit_ticks [n_cuboids][B] i32: the number of valid ticks whose position lies inside cuboid c -- the inclusive test px >= xmin && px <=
 *             xmax && ... of the rollouts' `collided` and of uavac_minsnap_audit_dev;  first_hit [n_cuboids][B] i32: the first such tick, -1
 *             when there is none.
 *   clearance [n_cuboids][B] f64, clearance_tick [n_cuboids][B] i32: the closest approach to cuboid c and its tick.  Per valid tick
 *             ex = px < xmin ? xmin - px : (px > xmax ? px - xmax : 0.0), ey and ez likewise -- selects, so a NaN bound gives 0 on its
 *             axis and an inverted one whatever the two comparisons give, exactly as np.where does --, d2 = (ex * ex + ey * ey) + ez * ez;
 *             reported is the lexicographic minimum of (d2, tick) over the valid ticks: clearance = sqrt(d2), clearance_tick = that tick.
 *             For a proper box (xmin <= xmax, ...) clearance == 0 iff hit_ticks > 0.
 * ROUNDING is part of the contract, as for the plan audit: every product and every sum is separately rounded (no fused multiply-add), a
 * maximum is taken of the squares, and one correctly rounded sqrt comes last.  The maximum of -0.0 and +0.0 is +0.0 (rows 2 and 3 of a
 * vehicle that never climbs or never sinks).
 * NO VALID TICK (a vehicle whose log is NaN throughout): row 0 is 0, rows 1-7 are NaN, first_bad 0, hit_ticks 0, first_hit -1, clearance
 * NaN, clearance_tick -1 -- such a vehicle never looks clean (uav_ac.scoring.flight_feasibility).
 * Every reduction is a maximum, an integer sum, an integer minimum or a lexicographic minimum, so every output is bit for bit what
 * NumPy gives on the log (uav_ac.scoring.audit_from_log) whatever the launch shape, the pitch, or what else is in the batch.  (Option
 * "flown_audit_split": 0 = automatic (default), 1 .. UAVAC_FLOWN_AUDIT_MAX_SPLIT = workgroups that share the ticks of one window of 64
 * vehicles; a tuning knob, same results.)  Cost: one read of the log, K x 13 x B x 8 bytes, and about 30 fp64 operations per cuboid and tick.
 * UAVAC_EINVAL before anything is enqueued: no context, NULL state_log, audit or first_bad, K < 1, B < 1, pitch < B, n_cuboids outside
 * 0 .. UAVAC_AUDIT_MAX_CUBOIDS, a NULL among cuboids / hit_ticks / first_hit / clearance / clearance_tick with n_cuboids > 0 or a
 * pointer among them with n_cuboids == 0. */
#define UAVAC_FLOWN_AUDIT_ROWS 8
#define UAVAC_FLOWN_AUDIT_MAX_SPLIT 64
int uavac_flown_audit_dev(uavac_ctx *ctx, const double *state_log, int K, int B, int64_t pitch, const double *cuboids, int n_cuboids,
                          double *audit, int32_t *first_bad, int32_t *hit_ticks, int32_t *first_hit, double *clearance,
                          int32_t *clearance_tick);

/* ONE CRUISE SPEED PER MISSION: the _v twins of uavac_minsnap_row_counts_dev, uavac_minsnap_row_counts_ragged_dev and
 * uavac_minsnap_plan_dev (both of its forms: rows with a capacity and flag 2 and the same all-or-nothing commit, and rows-free with
 * traj == NULL) take velocities [B] (device) where those take `velocity` -- what a fleet of MinimumSnap(path, obstacles, velocity,
 * dt) objects with different speeds is (minimum_snap.py:13-57: every object carries its own).  Everything downstream works from
 * times / seg_rows / coeffs alone and has no such twin: solve, samplers, first headings, audit, plan-fed rollouts, plan gathers.
 * CONTRACT: mission b's durations, row counts, coefficients, rows and first heading are bit for bit what the scalar entry point
 * gives that mission at velocity = velocities[b]: the same kernel with the same arithmetic (norm nested in fused multiply-adds, one
 * IEEE division, the factor 1.5 on the first and last segment, ceil(T / dt)).  A velocities[b] that is not positive and finite
 * cannot be refused by the host: it raises sticky flag 0 like a non-finite duration, its mission gets 0 rows (its durations are
 * whatever the division gives, its coefficients accordingly: do not fly it), and the other missions are unaffected. */
int uavac_minsnap_row_counts_v_dev(uavac_ctx *ctx, const double *wp, int B, int m, const double *velocities,
                                   double dt, double *times, int32_t *seg_rows, int64_t *row_offsets);
int uavac_minsnap_row_counts_ragged_v_dev(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B,
                                          int max_m, const double *velocities, double dt, double *times,
                                          int32_t *seg_rows, int64_t *row_offsets);
int uavac_minsnap_plan_v_dev(uavac_ctx *ctx, const double *wp, int B, int m, const double *velocities, double dt,
                             double *times, int32_t *seg_rows, int64_t *row_offsets, double *coeffs,
                             int32_t *status, double *traj, int64_t traj_capacity_rows, double *yaw,
                             double *first_yaw);

/* MISSIONS THAT START AND END IN MOTION.  uavac_minsnap_solve_dev pins velocity, acceleration and jerk to zero at the first and last
 * waypoint (MinimumSnap._generate_start_and_goal_constraints, minimum_snap.py:200-223); these two take them per mission:
 *   bc [B][6][3] f64 (device): rows 0-2 = velocity, acceleration, jerk at the FIRST waypoint, rows 3-5 = the same at the LAST one;
 *                              columns x y z (NED, SI units: m/s, m/s^2, m/s^3).
 * The same QP with those six right-hand sides: the optimum of the reference's dense KKT system with b[2m : 2m+3] = bc rows 0-2 and
 * b[2m+3 : 2m+6] = bc rows 3-5.  One lane per mission, one-ended block-Thomas recurrence (csrc/minsnap_solve_bc.hip); the boundary
 * values touch the right-hand side of the first and last interior knot and the coefficients of the first and last segment only.
 * BIT-EXACT by construction: a mission's coeffs[1] == v0, coeffs[2] == 0.5 * a0, coeffs[3] == j0 * (1.0 / 6.0) (rows of its first
 * segment, per column).  With bc all zero the result is the rest-to-rest optimum, rounded as the one-ended elimination rounds it
 * (within 1e-12 of uavac_minsnap_solve_dev relative to the largest coefficient, not bit-equal to it).
 * status [B] (may be NULL) and sticky flag 1 as for uavac_minsnap_solve_dev: a singular knot system gives status 1 and NaN
 * coefficients.  A NON-FINITE value in mission b's bc cannot be refused without a sync: mission b's coefficients come out
 * non-finite (its status stays 0: the pivots do not depend on bc -- the plan audit reports such a mission as NaN), the other
 * missions are unaffected.
 * uavac_minsnap_solve_bc_dev: seg_offsets == NULL: a uniform batch (wp [B][m+1][3], times [B][m], coeffs [B][8m][3]); otherwise the
 * ragged layout of uavac_minsnap_solve_ragged_dev with m = the largest segment count.  Mission b of a ragged call equals a uniform
 * call on it alone, and any split of a batch the whole, bit for bit.  UAVAC_EINVAL as for uavac_minsnap_solve_dev, and for bc == NULL.
 * uavac_minsnap_plan_bc_dev: uavac_minsnap_plan_v_dev with this solve in the solve's place -- both forms, rows with a capacity,
 * flag 2 and the all-or-nothing commit (a refused plan keeps its coefficients), and rows-free with traj == NULL; velocities [B] is
 * always a device array.  Durations, row counts and offsets do not depend on bc: same kernels, same bits as the _v chain.
 * CONTRACT: everything downstream reads only times / seg_rows / coeffs and is unchanged -- samplers, first headings, audit,
 * plan-fed rollouts, plan gathers.  Row 0 of a mission then carries velocity v0, and its yaw is the heading of v0 where
 * |v0_xy| >= 1e-3. */
int uavac_minsnap_solve_bc_dev(uavac_ctx *ctx, const double *wp, const double *times, const int64_t *seg_offsets, int B, int m,
                               const double *bc, double *coeffs, int32_t *status);
int uavac_minsnap_plan_bc_dev(uavac_ctx *ctx, const double *wp, int B, int m, const double *velocities, double dt,
                              const double *bc, double *times, int32_t *seg_rows, int64_t *row_offsets, double *coeffs,
                              int32_t *status, double *traj, int64_t traj_capacity_rows, double *yaw, double *first_yaw);

/* RETIMING FACTORS: by how much each mission of an audited plan must be slowed down to stay inside the limits the control law
 * clips its targets to.  Scaling every segment duration of a mission by k > 1 -- planning it at velocity / k -- leaves the
 * minimum-snap curve where it is (p'(t) = p(t / k)): velocity peaks scale by 1 / k, acceleration peaks by 1 / k^2.
 *   audit      [UAVAC_AUDIT_ROWS][B]  of uavac_minsnap_audit_dev (rows 1-4 are read)
 *   limits     [4] HOST: max_speed_xy, max_ascent, max_descent, max_horiz_accel (uavac_vehicle)
 *   velocities [B] in/out, factors [B] out, counters [2] i32 (device; ADDED to, not cleared: zero them first)
 * Per mission, every step ONE rounded IEEE operation, nothing contracted (part of the contract: uav_ac.scoring.retime_factors, a
 * NumPy restatement, gives the same bits):
 *   r = max(speed_xy / limits[0], ascent / limits[1], descent / limits[2], sqrt(accel_xy / limits[3]))
 *   any of the four peaks NaN (a singular plan, a mission without rows): factors[b] = NaN, velocity untouched, counters[1] += 1;
 *   r <= 1: factors[b] = 1.0, velocity untouched bit for bit;
 *   else    k = r / (1 - margin), factors[b] = k, velocities[b] = velocities[b] / k, counters[0] += 1.
 * The audit's peaks are maxima over SAMPLES, and the slower plan is sampled elsewhere on the curve: `margin` must exceed the
 * relative gap between sampled and continuous peaks (about 1e-4 for 3 m legs at 3 m/s and dt = 0.01; more for a coarser dt) for
 * one pass to suffice.  UAVAC_EINVAL before anything is enqueued: a limit that is not positive and finite, margin outside [0, 1),
 * B < 1, a NULL pointer. */
int uavac_minsnap_retime_factors_dev(uavac_ctx *ctx, const double *audit, int B, const double limits[4], double margin,
                                     double *velocities, double *factors, int32_t *counters);
/* THE LOOP that slows down exactly the missions that need it, by exactly the factor they need.  Pointers are DEVICE pointers
 * except limits and passes; unlike the other _dev calls this one SYNCHRONISES: once per pass the host reads the two counters
 * (like the obstacle loop reads its four).  seg_offsets == NULL: uniform batch, wp [B][m+1][3]; otherwise ragged (arrays back to
 * back, m = the largest segment count).  Each pass: the rows-free chain at the current velocities (times + row counts, offsets,
 * coefficient solve, first headings when first_yaw != NULL), uavac_minsnap_audit_dev without cuboids, the factors above.  It
 * stops when no mission was slowed down, or after max_passes retimings -- the pass after the last retiming only judges:
 * max_passes = 0 audits the plan at the given velocities and changes none.  No row is sampled anywhere; sample once afterwards
 * with the samplers.  On return times, seg_rows, row_offsets, coeffs, status (may be NULL), first_yaw (may be NULL) and audit
 * [UAVAC_AUDIT_ROWS][B] describe the plan AT THE RETURNED velocities [B] (in/out); factors_total [B] = the product of the
 * mission's factors in pass order (1.0 when it was never touched, NaN when a peak was NaN), one rounded multiplication per pass;
 * converged [B] i32 = 1 iff the mission's last audit asked for no retiming (a NaN mission: 0); *passes = retimings done.
 * The sticky flags are left to the caller (uavac_take_flags).  UAVAC_EINVAL as for the factors, and for max_passes < 0. */
int uavac_minsnap_retime_dev(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B, int m, double *velocities,
                             double dt, const double limits[4], double margin, int max_passes, double *times,
                             int32_t *seg_rows, int64_t *row_offsets, double *coeffs, int32_t *status, double *first_yaw,
                             double *audit, double *factors_total, int32_t *converged, int *passes);

/* RETIMING TO THE TILT AND THRUST LIMITS AS WELL.  The four limits above are the ones the control law clips its TARGETS to; it also clips
 * the bank command to max_tilt (csrc/control_law.h), and the rotors give between min_thrust and max_thrust.  uavac_minsnap_demand_dev
 * reports what a plan asks of these; the three calls below act on it.  Slowing a mission by k > 1 leaves its curve in place and divides
 * its accelerations by u = k^2.
 *   demand_limits [4] HOST: g (uavac_vehicle.g), max_tilt, Fmax = 4 max_thrust / mass, Fmin = 4 min_thrust / mass (specific thrust, m/s^2)
 * The host forms t2 = max_tilt * max_tilt, D = Fmax * Fmax - g * g and E = g * g - Fmin * Fmin once, each product and difference ONE
 * rounded operation.
 *
 * uavac_minsnap_need_dev (csrc/minsnap_need.hip): need [UAVAC_NEED_ROWS][B] f64, per mission the slowdown FACTOR each limit asks for on
 * its own -- 0 tilt, 1 upright, 2 thrust_max, 3 thrust_min -- from coefficients and row counts alone; coeffs / seg_rows / seg_offsets /
 * B / m / dt as in uavac_minsnap_audit_dev.  Stream-ordered, no sync.  PER ROW, from the sampler's acceleration a (the values
 * uavac_minsnap_sample_dev writes, bit for bit); every product, sum, difference, fmax and sqrt is ONE rounded operation (no fused
 * multiply-add), in exactly this order (tau = max_tilt):
 *     xx = ax * ax; yy = ay * ay; h = xx + yy; A = h + az * az; gz = g * az
 *     q  = fmax(fmax(xx - t2 * h, yy - t2 * h), 0)
 *     T  = q > 0 ? tau * az + sqrt(q) : -inf              tilt:       u >= T / (tau g)
 *     U  = az                                             upright:    u >= U / g   (non-strict, see below)
 *     H  = sqrt(gz * gz + A * D) - gz                     thrust max: u >= H / D
 *     d  = gz * gz - A * E
 *     Lo = (az > 0 && d >= 0) ? gz + sqrt(d) : -inf       thrust min: u >= Lo / E  (the admissible interval that reaches to infinity;
 *                                                         a second one at faster timing lies beyond a thrust reversal and is not used)
 * Division by a positive constant is monotone under rounding, so the maxima are taken of these NUMERATORS (fmax from -inf) and each is
 * divided once per mission:
 *     need[0] = sqrt(fmax(max T / (tau * g), 0))    need[1] = sqrt(fmax(max U / g, 0))
 *     need[2] = sqrt(fmax(max H / D, 0))            need[3] = sqrt(fmax(max Lo / E, 0))
 * The reductions are maxima: exact and order-free, so the outputs depend neither on the launch shape nor on the batch split (option
 * "audit_lanes": 16 or 64 lanes per mission, same results).  They equal what NumPy computes from the sampled rows, bit for bit
 * (uav_ac/scoring.py need_from_rows).  Hover gives 0, 0, 0, 0.  A mission with ANY non-finite sample (position, velocity or
 * acceleration), and a mission without rows, reports NaN in all four: a singular plan never looks feasible.
 * KNOWN EDGE: a row in exact free fall (az == g) with min_thrust = 0 gives need[1] = 1 and is not slowed, although
 * uavac_minsnap_demand_dev counts it as inverted; with Fmin > 0 the thrust_min term covers it (u = g / (g - Fmin) > 1).
 * The body rate (no closed form) and the cuboid clearance (slowing down moves no curve) are not retimed to.
 *
 * uavac_minsnap_retime_demand_factors_dev: uavac_minsnap_retime_factors_dev with the need block beside the audit block.  With r_audit
 * the four-term maximum formed exactly as there,
 *     r = fmax(r_audit, fmax(fmax(need[0], need[1]), fmax(need[2], need[3])))
 * a NaN among the four peaks OR the four needs: factors[b] = NaN, velocity untouched, counters[1] += 1; r <= 1: factors[b] = 1.0,
 * velocity untouched bit for bit; else k = r / (1 - margin), factors[b] = k, velocities[b] = velocities[b] / k, counters[0] += 1.
 *   binding [B] i32: the index of the FIRST term that attains r, in the order 0 speed_xy, 1 ascent, 2 descent, 3 accel_xy, 4 tilt,
 *   5 upright, 6 thrust_max, 7 thrust_min; -1 for a NaN mission.  Written for every mission, also where r <= 1 (the nearest limit).
 *
 * uavac_minsnap_retime_demand_dev: THE LOOP of uavac_minsnap_retime_dev with demand_limits as a further input, need
 * [UAVAC_NEED_ROWS][B] and binding [B] as further outputs (both describe the plan at the returned velocities, like audit), and one more
 * launch per pass: the need kernel after the audit.  One counter read per pass, as there.
 *
 * UAVAC_EINVAL before anything is enqueued: g or max_tilt not positive and finite; Fmax not finite or <= g (the vehicle cannot hover);
 * Fmin < 0 or >= g; and every refusal of the call each of the three mirrors (uavac_minsnap_audit_dev, uavac_minsnap_retime_factors_dev,
 * uavac_minsnap_retime_dev). */
#define UAVAC_NEED_ROWS 4
int uavac_minsnap_need_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                           double dt, const double demand_limits[4], double *need);
int uavac_minsnap_retime_demand_factors_dev(uavac_ctx *ctx, const double *audit, const double *need, int B, const double limits[4],
                                            const double demand_limits[4], double margin, double *velocities, double *factors,
                                            int32_t *binding, int32_t *counters);
int uavac_minsnap_retime_demand_dev(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B, int m, double *velocities,
                                    double dt, const double limits[4], const double demand_limits[4], double margin, int max_passes,
                                    double *times, int32_t *seg_rows, int64_t *row_offsets, double *coeffs, int32_t *status,
                                    double *first_yaw, double *audit, double *need, double *factors_total, int32_t *binding,
                                    int32_t *converged, int *passes);

/* PLANS FROM GIVEN DURATIONS, THE SNAP COST, AND OPTIMISED SEGMENT TIMES (csrc/minsnap_timeopt.hip).  Every chain above takes its
 * durations from upstream's rule T_s = |leg_s| / velocity [* 1.5 on the first and last leg] (minimum_snap.py:311-321); these four take
 * them as they are given, measure a plan, and divide a mission's total time between its legs so that the snap cost falls -- the second
 * half of the minimum-snap method (Mellinger & Kumar 2011).  Rest to rest only (no bc).  Throughout, seg_offsets == NULL: a uniform
 * batch (wp [B][m+1][3], times [B][m], coeffs [B][8m][3]); otherwise the ragged layout of uavac_minsnap_solve_ragged_dev with m = the
 * largest segment count.  Mission b of a ragged call equals a uniform call on it alone, and any split of a batch the whole, bit for bit.
 *
 * uavac_minsnap_row_counts_t_dev: seg_rows = ceil(T / dt) in fp64 -- the single IEEE division and ceil of uavac_minsnap_row_counts_dev,
 * so seg_rows == len(np.arange(0, T, dt)) -- and row_offsets [B+1] by the same scan.  A duration that is not positive and finite
 * raises sticky flag 0 and leaves its MISSION without rows (what a bad per-mission speed does); the other missions are unaffected.
 *
 * uavac_minsnap_plan_t_dev: the planning chain of uavac_minsnap_plan_v_dev with `times` an INPUT (never written) -- both forms: rows
 * with a capacity, flag 2 and the all-or-nothing commit (a refused plan keeps seg_rows, row_offsets, coeffs, rows and first_yaw), and
 * rows-free with traj == NULL.  Same kernels downstream of the durations: given the durations of a velocity chain it reproduces that
 * chain bit for bit.  A ragged batch has no dense yaw column (yaw must be NULL), like uavac_minsnap_sample_ragged_dev.
 *
 * uavac_minsnap_cost_dev: cost [B] f64, J_b = sum over the mission's segments and the three axes of the integral of snap^2 over
 * [0, T_s] -- upstream's c^T H c (_create_snap_cost_matrix, no 1/2).  ROUNDING (part of the contract): not computed from H, whose
 * T^(r+c-7) terms of both signs cancel, but by the four-point Gauss-Legendre rule, exact for the degree-6 integrand and a sum of
 * non-negative terms: half = 0.5 T; nodes x = -0.8611363115940526, -0.3399810435848563, +0.3399810435848563, +0.8611363115940526 in
 * that order with weights w = 0.3478548451374538, 0.6521451548625461, 0.6521451548625461, 0.3478548451374538; t = half + half * x;
 * snap per axis by Horner on (840 c7, 360 c6, 120 c5, 24 c4); q = (sx sx + sy sy) + sz sz; seg += (half * w) * q.  Nothing is
 * contracted.  Sixteen lanes per mission: lane l adds its segments l, l + 16, ... in that order, the sixteen sums meet in a fixed xor
 * tree (distances 8, 4, 2, 1) -- the result depends neither on the launch shape nor on the batch split.  A non-finite coefficient or
 * duration anywhere in a mission gives NaN for that mission alone.
 *
 * uavac_minsnap_optimize_times_dev: times [.] in/out, cost_before / cost_after [B] f64, accepted [B] i32; every pointer a DEVICE
 * pointer.  NO HOST SYNCHRONISATION: the iteration count is fixed, a mission with nothing left to gain idles, the whole loop is
 * enqueued on the ctx stream (the ctx's scratch grows on the first call of a size, as everywhere).  Per mission with m >= 2 segments:
 * T = the durations, total = sum(T0) in index order, J = cost(solve(T)), alpha = UAVAC_TIMEOPT_ALPHA0.  A mission with one segment,
 * with a first cost that is not finite or with a duration that is not positive and finite is returned bit for bit, accepted = 0.
 * Each of `iterations` iterations:
 *   probes      h = UAVAC_TIMEOPT_PROBE_STEP * total / m; for i = 0 .. m-1: g_i = +1 at i, -1 / (m - 1) elsewhere,
 *               d_i = (J(T + h g_i) - J) / h
 *   direction   G_k = d_k - (sum_{i != k} d_i) / (m - 1), D = -G; max|D| zero or a d_i not finite: the mission sits this iteration
 *               out, unchanged; otherwise D is scaled so that max|D| = min(T)
 *   candidates  j = 0 .. UAVAC_TIMEOPT_CANDIDATES-1: a_j = alpha 2^-j, Tc = T + a_j D; dropped when min(Tc) <
 *               UAVAC_TIMEOPT_FLOOR * min(T0), else Tc *= total / sum(Tc), solved and costed
 *   selection   the candidate with the smallest cost STRICTLY below J (the lowest j on a tie; a NaN is never accepted) becomes T and
 *               J, accepted += 1, alpha = min(UAVAC_TIMEOPT_ALPHA_MAX, 2 a_j); none: alpha *= 2^-UAVAC_TIMEOPT_CANDIDATES
 * So cost_after <= cost_before, sum(T) is kept (to rounding) and min(T) >= UAVAC_TIMEOPT_FLOOR * min(T0).  cost_after is bit for bit
 * uavac_minsnap_cost_dev of uavac_minsnap_solve_dev at the returned durations.  The m probes of all missions go through the solve as
 * ONE batch, the candidates as a second; the batch is walked in chunks of missions sized from UAVAC_TIMEOPT_SCRATCH_BYTES of scratch
 * (option "timeopt_chunk": missions per chunk, 0 = automatic; a tuning knob, same results).  The promise is a lower snap cost, not
 * feasibility: audit the new plan (and against the cuboids again -- the curve passes the same waypoints, not the same points between).
 * UAVAC_EINVAL before anything is enqueued: iterations < 0, B < 1, m outside 1 .. UAVAC_MAX_SEGMENTS, a NULL pointer (seg_offsets,
 * status, traj, yaw and first_yaw may be NULL), dt not positive and finite. */
#define UAVAC_TIMEOPT_PROBE_STEP 1.0e-6
#define UAVAC_TIMEOPT_CANDIDATES 6
#define UAVAC_TIMEOPT_ALPHA0 0.25
#define UAVAC_TIMEOPT_ALPHA_MAX 0.5
#define UAVAC_TIMEOPT_FLOOR 0.2
#define UAVAC_TIMEOPT_SCRATCH_BYTES (256ull << 20)
int uavac_minsnap_row_counts_t_dev(uavac_ctx *ctx, const double *times, const int64_t *seg_offsets, int B, int m, double dt,
                                   int32_t *seg_rows, int64_t *row_offsets);
int uavac_minsnap_plan_t_dev(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B, int m, const double *times,
                             double dt, int32_t *seg_rows, int64_t *row_offsets, double *coeffs, int32_t *status, double *traj,
                             int64_t traj_capacity_rows, double *yaw, double *first_yaw);
int uavac_minsnap_cost_dev(uavac_ctx *ctx, const double *coeffs, const double *times, const int64_t *seg_offsets, int B, int m,
                           double *cost);
int uavac_minsnap_optimize_times_dev(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B, int m, double *times,
                                     int iterations, double *cost_before, double *cost_after, int32_t *accepted);

/* row_offsets [B+1] from per-segment row counts that exist already -- the second half of
 * uavac_minsnap_row_counts_dev on its own, for a plan whose seg_rows [B][m] came from elsewhere (the
 * peers' plans after uavac_gather_plan_dev): exclusive prefix sum of the per-mission totals
 * (sum of len(np.arange(0, T, dt)) over the mission's splines, minimum_snap.py:104). */
int uavac_minsnap_row_offsets_dev(uavac_ctx *ctx, const int32_t *seg_rows, int B, int m, int64_t *row_offsets);
/* The same for a ragged batch (seg_rows [S] back to back, mission b's at seg_offsets[b] .. seg_offsets[b+1]). */
int uavac_minsnap_row_offsets_ragged_dev(uavac_ctx *ctx, const int32_t *seg_rows, const int64_t *seg_offsets, int B,
                                         int max_m, int64_t *row_offsets);

/* Ragged batches: missions with different numbers of waypoints in one call -- what a fleet of MinimumSnap objects with
 * paths of different lengths is (minimum_snap.py:13-57 takes any path), and what the obstacle loop (:63-95) produces as
 * soon as one mission has received a midpoint.  Mission b has m_b = seg_offsets[b+1] - seg_offsets[b] segments
 * (1 <= m_b <= max_m <= UAVAC_MAX_SEGMENTS; seg_offsets [B+1] i64, device, seg_offsets[0] = 0) and m_b + 1 waypoints.
 * Everything per-segment lies back to back in mission order: wp [S + B][3] (mission b starts at waypoint
 * seg_offsets[b] + b), times / seg_rows / hit [S], coeffs [S][8][3], S = seg_offsets[B] = total_segments.
 * Same kernels, same arithmetic: mission b's outputs equal those of a uniform call on it alone, bit for bit.
 * A segment count outside 1 .. max_m raises sticky flag 0 (uavac_take_flags) and is clamped.  The sampler takes the
 * capacity of the row buffer like uavac_minsnap_plan_dev (flag 2 and nothing written when it is too small; < 0: not
 * checked), an optional cuboid + hit flags (both or neither) and optional first_yaw [B]. */
/* The same on HOST buffers, the whole chain in one call (seg_offsets on the host; validated: 1 .. UAVAC_MAX_SEGMENTS
 * segments each): times [S] and coeffs [S][8][3] optional (NULL), row_offsets [B+1] always; traj NULL (or
 * traj_capacity_rows < row_offsets[B]: UAVAC_EINVAL after everything else was produced) skips the rows -- call once with
 * traj = NULL to learn row_offsets[B], allocate, call again. */
int uavac_minsnap_plan_ragged(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B, double velocity,
                              double dt, double *times, int64_t *row_offsets, double *coeffs, double *traj,
                              int64_t traj_capacity_rows);
int uavac_minsnap_row_counts_ragged_dev(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B,
                                        int max_m, double velocity, double dt, double *times,
                                        int32_t *seg_rows, int64_t *row_offsets);
int uavac_minsnap_solve_ragged_dev(uavac_ctx *ctx, const double *wp, const double *times,
                                   const int64_t *seg_offsets, int B, int max_m, double *coeffs,
                                   int32_t *status);
int uavac_minsnap_sample_ragged_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows,
                                    const int64_t *seg_offsets, const int64_t *row_offsets, int B, int max_m,
                                    int64_t total_segments, double dt, double *traj,
                                    int64_t traj_capacity_rows, const double *aabb, int32_t *hit,
                                    double *first_yaw);
/* ONE ROUND of the obstacle loop of MinimumSnap._generate_collision_free_trajectory (minimum_snap.py:81-93) for B ragged
 * missions against one cuboid aabb[6], entirely on the device (no rows are stored: inside the loop only the hit flags
 * matter; sample the final waypoints once with uavac_minsnap_*_ragged_dev afterwards):
 *   - the missions with active[b] != 0 are planned (durations, row counts, coefficient solve) -- the others are left alone;
 *   - every spline of an active mission with a sample inside the cuboid (inclusive test, is_collision_cuboid :327-357,
 *     on the very positions the sampler would store) gets the midpoint of its two waypoints inserted before its end
 *     waypoint (insert_midpoints_at_indexes :359-391): wp_out / seg_offsets_out are the waypoint arrays of the next round
 *     (all B missions; untouched ones are copied), laid out like wp / seg_offsets;
 *   - an active mission without a hit is clean for this cuboid: active[b] = 0; one that would outgrow UAVAC_MAX_SEGMENTS is
 *     left as it is: active[b] = 0, overflow[b] = 1; a mission that received midpoints: touched[b] = 1, stays active;
 *   - counters [4] i32 (device): missions still active, missions that outgrew UAVAC_MAX_SEGMENTS in this round, the largest segment
 *     count after the round (a valid max_m for the next one), the segment total of the batch after the round.
 * max_m >= every mission's segment count, <= UAVAC_MAX_SEGMENTS.  SCRATCH (device, caller-owned, sizes TRUSTED -- the call
 * cannot check them; S_cap >= the segment total before the round): times [S_cap], seg_rows [S_cap] i32, row_offsets [B+1],
 * coeffs [S_cap][8][3], hit [S_cap] i32.  They are scratch in the strict sense: what they hold after the call is valid only
 * for the missions that were active IN THIS ROUND (waves without an active mission skip the solve while the segment offsets
 * move from round to round): do not sample from them -- plan the final waypoints with uavac_minsnap_*_ragged_dev.  wp_out
 * holds S_cap_next + B waypoints with S_cap_next >= the segment total after the round (at most twice the one before, and
 * never more than B * UAVAC_MAX_SEGMENTS).  A singular knot system (repeated waypoint) raises sticky flag 1; its mission's
 * positions are NaN, inside no cuboid: it leaves the loop as if collision-free -- check uavac_take_flags. */
int uavac_minsnap_obstacle_round_dev(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B, int max_m,
                                     double velocity, double dt, const double *aabb, int32_t *active, int32_t *overflow,
                                     int32_t *touched, double *wp_out, int64_t *seg_offsets_out, int32_t *counters,
                                     double *times, int32_t *seg_rows, int64_t *row_offsets, double *coeffs, int32_t *hit);

/* The whole obstacle loop on HOST buffers: MinimumSnap(path_b, obstacles, velocity, dt) up to the final waypoint list, for B
 * ragged missions (wp [S + B][3], seg_offsets [B+1] as above) against n_cuboids cuboids [n_cuboids][6] visited in order
 * (minimum_snap.py:72-93: earlier ones are not re-checked).  Unlike the reference's, the loop is bounded: at most
 * max_iterations + 1 rounds per obstacle; a mission that runs out, or would outgrow UAVAC_MAX_SEGMENTS, keeps the waypoints
 * it has and is reported in converged [B] (0; may be NULL).  recheck_passes > 0 sweeps the missions that received midpoints
 * over the obstacle list again (beyond the reference).  Output: the final waypoints wp_out [seg_offsets_out[B] + B][3]
 * (wp_capacity rows available; B * (UAVAC_MAX_SEGMENTS + 1) always suffice; UAVAC_EINVAL with seg_offsets_out filled in when
 * it is too small) -- sample them with uavac_minsnap_plan_ragged to get get_trajectory()'s rows.  UAVAC_ESINGULAR (outputs
 * complete): some mission has a repeated waypoint; its collision scan was void. */
int uavac_minsnap_obstacle_waypoints(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B, double velocity,
                                     double dt, const double *cuboids, int n_cuboids, int max_iterations, int recheck_passes,
                                     double *wp_out, int64_t wp_capacity, int64_t *seg_offsets_out, int32_t *converged);

/* MinimumSnap._calculate_yaws (minimum_snap.py:126-136) on its own, for B independent velocity
 * sequences of any length: sequence b = rows [offsets[b], offsets[b+1]) of velocities[.][3] (only
 * vx, vy are read); yaws[offsets[B]].  Headings of rows with |v_xy| >= 1e-3, np.unwrap over those,
 * hold-last-valid, leading rows take the first valid heading, all zeros when none is valid. */
int uavac_yaw_scan_dev(uavac_ctx *ctx, const double *velocities, const int64_t *offsets, int B,
                       double *yaws);
/* Host twin for one sequence: velocities [n][3] -> yaws [n]. */
int uavac_yaw_scan(uavac_ctx *ctx, const double *velocities, int64_t n, double *yaws);

/* Host-pointer twins (synchronous).  They stage through device scratch and a pinned ping-pong
 * buffer that the ctx keeps between calls (no allocation per call once warm). */
int uavac_minsnap_row_counts(uavac_ctx *ctx, const double *wp, int B, int m, double velocity,
                             double dt, double *times, int32_t *seg_rows, int64_t *row_offsets);
int uavac_minsnap_solve(uavac_ctx *ctx, const double *wp, int B, int m, double velocity,
                        double *coeffs, double *times);
int uavac_minsnap_sample(uavac_ctx *ctx, const double *coeffs, const double *times, int B, int m,
                         double dt, const int64_t *row_offsets, double *traj);

/* ---- control ------------------------------------------------------------------
 * Batched drop-in for one tick of uav_ac/main.py TrajectoryController.step (:37-61)
 * [CascadedController: uav_ac/control/controller.py:26-168; rotor allocation and motor
 * lag: uav_ac/quadrotor/quad.py:88-122] followed by MujocoSimulation.step
 * (uav_ac/simulation/mujoco_sim.py:144-151) restricted to free flight (rotor wrench
 * :232-251 + semi-implicit Euler free-body step; no contacts).
 *
 * State is struct-of-arrays over the batch (lane b = UAV b):
 *   state  [30][B] f64: rows 0-12  X = x y z | q0 q1 q2 q3 | vx vy vz | p q r   (quad.py:75-80)
 *                       rows 13-16 omega, rows 17-20 omega_command               (quad.py:83-86)
 *                       row  21    altitude integral error                       (controller.py:20)
 *                       row  22    thrust_cmd, rows 23-25 pqr_cmd                (main.py:26-27)
 *                       rows 26-29 the yaw scan a plan-fed rollout carries when it is given no dense yaw column:
 *                                  the row it stands before, heading seen (0/1), last heading, unwrap sum
 *                                  (minimum_snap.py:126-136; zero after uavac_state_init, maintained by the kernel)
 *   istate [4][B]  i32: trajectory_index, inner_step (main.py:24-25), collided (sticky obstacle flag),
 *                       ground bookkeeping bits (UAVAC_GROUND_*; stays 0 in free flight)
 *   traj / row_offsets: as produced by uavac_minsnap_sample (UAV b follows mission b).
 */
/* X = [position, identity attitude, rest]; rotors at hover speed if hover != 0, else 0;
 * controller memory cleared (TrajectoryController.reset, main.py:29-35).
 * positions [B][3] may be NULL (origin). */
int uavac_state_init_dev(uavac_ctx *ctx, const uavac_vehicle *V, const double *positions, int B,
                         int hover, double *state, int32_t *istate);
/* K ticks fused in one launch.  state_log [K][13][B] (X after every tick) or NULL;
 * cmd_log [K][12][B] (thrust_cmd, pqr_cmd, omega_command, omega after the controller part
 * of every tick) or NULL; aabbs [n_obs][6] = xmin xmax ymin ymax zmin zmax (inclusive test of
 * minimum_snap.py:327-357, evaluated on the position after every tick) or NULL.
 * Any B is accepted; the logs stream at full rate when their rows start on 128-byte lines: B a
 * multiple of 16, or uavac_set_option(ctx, "log_pitch", P) with P >= B a multiple of 16 -- the logs
 * are then [K][13][P] and [K][12][P]. */
int uavac_control_rollout_dev(uavac_ctx *ctx, const uavac_vehicle *V, const double *traj,
                              const int64_t *row_offsets, double *state, int32_t *istate, int B,
                              int K, double *state_log, double *cmd_log, const double *aabbs,
                              int n_obs);
/* The same rollout fed by the plan instead of the sampled rows: the target row of every outer tick is
 * evaluated inside the kernel from the coefficients of the UAV's current segment (bit-identical to
 * the sampler's rows).  The yaw -- the one column that is a scan over all earlier rows -- comes
 * either from the dense yaw column uavac_minsnap_sample_yaw_dev writes (yaw [row_offsets[B]]), or,
 * with yaw == NULL, from the scan the vehicle carries itself in state rows 26-29 (it visits its rows
 * in order), seeded with first_yaw [B] from the sampler; bit-identical either way, and in the second
 * form no yaw byte is read or written.  coeffs [B][8m][3], seg_rows [B][m], row_offsets [B+1], dt
 * as given to the sampler.  Same results as uavac_control_rollout_dev on the sampled trajectory,
 * without its HBM read traffic (80 B per UAV and outer tick, fetched as 128-byte lines).  A cursor
 * (istate row 0) that the caller moved is honoured: the carried scan is rebuilt from row 0 at launch. */
int uavac_control_rollout_plan_dev(uavac_ctx *ctx, const uavac_vehicle *V, const double *coeffs,
                                   const int32_t *seg_rows, const int64_t *row_offsets,
                                   const double *yaw, const double *first_yaw, int m, double dt,
                                   double *state, int32_t *istate, int B, int K, double *state_log,
                                   double *cmd_log, const double *aabbs, int n_obs);

/* The same for a ragged batch (uavac_minsnap_*_ragged_dev): coeffs [S][8][3] and seg_rows [S] back to back, mission b's
 * segments at seg_offsets[b] .. seg_offsets[b+1]; the vehicles scan the yaw themselves from first_yaw [B]. */
int uavac_control_rollout_plan_ragged_dev(uavac_ctx *ctx, const uavac_vehicle *V, const double *coeffs,
                                          const int32_t *seg_rows, const int64_t *seg_offsets,
                                          const int64_t *row_offsets, const double *first_yaw, int max_m,
                                          double dt, double *state, int32_t *istate, int B, int K,
                                          double *state_log, double *cmd_log, const double *aabbs, int n_obs);

/* Scored twins: the same flight (state, istate, state_log and the obstacle flag bit for bit what the unscored twin gives) while
 * the kernel accumulates per-UAV tracking scores on the side, without a log.  The arguments are the twin's plus
 * score [UAVAC_SCORE_ROWS][B] f64 (device memory) last.  score == NULL or cmd_log != NULL: UAVAC_EINVAL (scores are never
 * accumulated together with a command log).
 * A PERIOD is the inner_per_outer = F ticks that start with an outer update (a tick with istate[1] % F == 0 on a mission that
 * has rows) and end after the dynamics step of its F-th tick; the outer update reads row r = the cursor.  At its end
 * e = sqrt(dx*dx + dy*dy + dz*dz), d = position - row r's x y z (upstream's tracking_errors entry,
 * tests/integration/test_mujoco_trajectory_tracking.py:26-36).  The period is SCORED only if r >= next_row; then, left to right
 * one period after another: count += 1, next_row = r + 1, sum += e, sumsq += e*e, max = max(max, e), last = e.  From a fresh
 * score (all zeros) rows 0 .. N-1 are scored once each and the repeated last-row periods after the cursor stops are not:
 * sum / count is upstream's np.mean(tracking_errors), and once next_row == N, last is the distance to the final row at the end
 * of its period (upstream's goal-distance check, the final row standing in for goal_position).
 *   score rows: 0 count   1 next_row   2 sum of e   3 sum of e*e   4 max e   5 last e
 *               6 pending row + 1 (0: none)   7 istate[1] when the scored launch that left it pending ended
 *               8-10 the pending target x y z
 * All zeros is a fresh start.  Callers read rows 0-5; rows 6-10 carry a period a launch ends inside of into the next scored
 * launch, which resumes it only if row 7 == inner and inner % F != 0 (no tick, scored or not, ran in between), and drops it
 * otherwise (an unscored launch or uavac_control_step_dev inside a period drops that period): a scored flight split into
 * launches at any tick gives the same score bits as one launch. */
int uavac_control_rollout_scored_dev(uavac_ctx *ctx, const uavac_vehicle *V, const double *traj,
                                     const int64_t *row_offsets, double *state, int32_t *istate, int B,
                                     int K, double *state_log, double *cmd_log, const double *aabbs,
                                     int n_obs, double *score);
int uavac_control_rollout_plan_scored_dev(uavac_ctx *ctx, const uavac_vehicle *V, const double *coeffs,
                                          const int32_t *seg_rows, const int64_t *row_offsets,
                                          const double *yaw, const double *first_yaw, int m, double dt,
                                          double *state, int32_t *istate, int B, int K, double *state_log,
                                          double *cmd_log, const double *aabbs, int n_obs, double *score);
int uavac_control_rollout_plan_ragged_scored_dev(uavac_ctx *ctx, const uavac_vehicle *V, const double *coeffs,
                                                 const int32_t *seg_rows, const int64_t *seg_offsets,
                                                 const int64_t *row_offsets, const double *first_yaw, int max_m,
                                                 double dt, double *state, int32_t *istate, int B, int K,
                                                 double *state_log, double *cmd_log, const double *aabbs, int n_obs,
                                                 double *score);
/* One tick (K = 1, no logs): the literal drop-in of tc.step() + simulation.step(). */
int uavac_control_step_dev(uavac_ctx *ctx, const uavac_vehicle *V, const double *traj,
                           const int64_t *row_offsets, double *state, int32_t *istate, int B);

/* Host-pointer twins (synchronous). */
int uavac_state_init(uavac_ctx *ctx, const uavac_vehicle *V, const double *positions, int B,
                     int hover, double *state, int32_t *istate);
int uavac_control_rollout(uavac_ctx *ctx, const uavac_vehicle *V, const double *traj,
                          const int64_t *row_offsets, double *state, int32_t *istate, int B, int K,
                          double *state_log, double *cmd_log, const double *aabbs, int n_obs);

/* The two halves of a tick on their own, for callers that own the simulation loop the way
 * uav_ac/main.py does (controller callback + external physics):
 *   uavac_controller_tick = TrajectoryController.step (main.py:37-61): outer loop every
 *       inner_per_outer-th call, body-rate loop, allocation, motor lag; X is read, not advanced;
 *   uavac_dynamics_step   = MujocoSimulation.step in free flight (mujoco_sim.py:144-151,232-251):
 *       advances X from the current rotor speeds; aabbs/istate optional (sticky flag in istate row 2). */
int uavac_controller_tick_dev(uavac_ctx *ctx, const uavac_vehicle *V, const double *traj,
                              const int64_t *row_offsets, double *state, int32_t *istate, int B);
int uavac_dynamics_step_dev(uavac_ctx *ctx, const uavac_vehicle *V, double *state, int32_t *istate,
                            int B, const double *aabbs, int n_obs);
int uavac_controller_tick(uavac_ctx *ctx, const uavac_vehicle *V, const double *traj,
                          const int64_t *row_offsets, double *state, int32_t *istate, int B);
int uavac_dynamics_step(uavac_ctx *ctx, const uavac_vehicle *V, double *state, int32_t *istate, int B,
                        const double *aabbs, int n_obs);

/* ---- resident tick-by-tick session ----------------------------------------------
 * For callers that own the loop like uav_ac/main.py:113-118 does -- `tc.step(); simulation.step()`
 * once per inner tick, with host code reading and writing quad.X / quad.omega in between.  The
 * trajectory rows of the B UAVs are uploaded once at creation; the state lives in pinned host memory
 * that is mapped into the device and that the tick kernels read and write IN PLACE:
 * uavac_pilot_state() -> [30][B] f64, uavac_pilot_istate() -> [4][B] i32 (layouts above), valid until
 * uavac_pilot_destroy.  uavac_pilot_tick runs the controller half (uavac_controller_tick), the
 * vehicle half (uavac_dynamics_step) or both on that state and returns when the results are
 * visible to the host: one kernel launch (or two) and one stream synchronisation per call, no
 * copies, no allocation.  The host may edit the state between calls (that is what the reference's
 * tests do to quad.X). */
typedef struct uavac_pilot uavac_pilot;
#define UAVAC_PILOT_CONTROLLER 1
#define UAVAC_PILOT_DYNAMICS 2
int uavac_pilot_create(uavac_ctx *ctx, const double *traj, const int64_t *row_offsets, int B,
                       uavac_pilot **out);                 /* traj / row_offsets: HOST pointers */
void uavac_pilot_destroy(uavac_pilot *pilot);
double *uavac_pilot_state(uavac_pilot *pilot);
int32_t *uavac_pilot_istate(uavac_pilot *pilot);
int uavac_pilot_set_obstacles(uavac_pilot *pilot, const double *aabbs, int n_obs);   /* HOST [n_obs][6] */
int uavac_pilot_tick(uavac_pilot *pilot, const uavac_vehicle *V, int what);

/* ---- per-function probes ------------------------------------------------------
 * One stage of the control law at a time on small array-of-struct batches (host pointers,
 * synchronous).  They run the very __device__ functions the fused rollout inlines, so the
 * reference's unit-level known answers (tests/unit/control/test_controller.py,
 * tests/unit/quadrotor/test_quad.py) can be replayed against the HIP path, and they back the
 * single-UAV facade classes.  mask selects which optional inputs override computed values.
 *
 * outer: in [B][41] = X(13) | R(9) | target row(11) | integral | thrust_in | bxy_in(2) |
 *                     euler_in(phi,theta,psi) | q_cmd_in
 *        out[B][21] = R(9) [Quad.R, quad.py:129-155] | phi theta psi [quad.py:189-213] |
 *                     thrust, integral' [altitude, controller.py:26-56] | bxy(2) [lateral :58-97] |
 *                     p_c q_c [roll_pitch_controller :132-154] | pqr_cmd(3) [reduced_attitude :99-113]
 * inner: in [B][24] = X(13) | pqr_cmd(3) | thrust_cmd | omega(4) | moment_in(3)
 *        out[B][15] = moment(3) [body_rate_controller :115-130] | rotor forces(4)
 *                     [_allocate_rotor_forces, quad.py:105-122] | omega_command(4), omega'(4)
 *                     [set_propeller_speed, quad.py:88-103] */
#define UAVAC_PROBE_OUTER_IN 41
#define UAVAC_PROBE_OUTER_OUT 21
#define UAVAC_PROBE_INNER_IN 24
#define UAVAC_PROBE_INNER_OUT 15
#define UAVAC_PROBE_USE_R 1       /* altitude / roll_pitch take the given rot_mat                */
#define UAVAC_PROBE_USE_THRUST 2  /* lateral takes thrust_in instead of altitude's result        */
#define UAVAC_PROBE_USE_BXY 4     /* roll_pitch takes bxy_in instead of lateral's result         */
#define UAVAC_PROBE_USE_EULER 8   /* yaw_controller takes euler_in (duck-typed quad)             */
#define UAVAC_PROBE_USE_QCMD 16   /* yaw_controller takes q_cmd_in instead of roll_pitch's q_c   */
#define UAVAC_PROBE_USE_MOMENT 1  /* (inner) allocation takes moment_in instead of body_rate's   */
int uavac_probe_outer(uavac_ctx *ctx, const uavac_vehicle *V, const double *in, int B, int mask, double *out);
int uavac_probe_inner(uavac_ctx *ctx, const uavac_vehicle *V, const double *in, int B, int mask, double *out);
/* The sampler's heading of a velocity sample (csrc/minsnap_yaw.h: the device library's atan2 with the instruction count cut)
 * beside the library's own atan2(y, x) on the same operands; DEVICE pointers, n values each, asynchronous.  They must agree bit
 * for bit (np.arctan2 in MinimumSnap._calculate_yaws, minimum_snap.py:131, is matched to <= 1e-5 by either). */
int uavac_probe_heading_dev(uavac_ctx *ctx, const double *y, const double *x, int64_t n, double *heading, double *library);

/* ---------------------------------------------------------------------------------------------
 * RRT* planner -- replaces uav_ac/planning/rrt.py.
 *
 * B independent planning problems, one wavefront each, all sharing step (= max_distance),
 * max_iter and the obstacle list.  Random numbers stay on the host: samples[B][max_iter][3] holds,
 * per iteration, the node RRTStar._generate_random_node (rrt.py:118-127) returned (NumPy's legacy
 * global generator, one uniform() for the goal bias then three for the coordinates).
 * With cap = max_iter + 1, per problem:
 *   nodes       [cap][3]  `all_nodes` in insertion order (entry 0 = round(start, 2)); rows past
 *                          counts[0] are zero
 *   canon       [cap]     first entry with bit-identical coordinates = the dict key of the entry
 *   parent      [cap]     indexed by key: key of tree[key] at the end of run(), -1 = no such key
 *   best_parent [cap]     the same for `best_tree` (stored at the last improvement)
 *   best_path   [cap][3]  `best_path`, start -> goal, counts[4] rows
 *   counts      [6]       n_nodes, iterations begun, status, entries when best_tree was stored,
 *                          best_path rows, dynamic_it_counter
 *   best_cost             path_cost(best_path) (rrt.py:84-91); +inf without a path
 * status: UAVAC_RRT_OK, or what the reference raises -- UAVAC_RRT_NO_PATH ("No path found",
 * rrt.py:72-73), UAVAC_RRT_COST_INCREASED (:55-56), UAVAC_RRT_KEY_ERROR (a dict lookup failed).
 * Per-problem failures are reported in counts, not in the return value. */
#define UAVAC_RRT_OK 0
#define UAVAC_RRT_NO_PATH 1
#define UAVAC_RRT_COST_INCREASED 2
#define UAVAC_RRT_KEY_ERROR 3
int uavac_rrt_star_dev(uavac_ctx *ctx, const double *start, const double *goal, int B, double step,
                       int max_iter, const double *samples, const double *cuboids, int n_obs,
                       double *nodes, int32_t *canon, int32_t *parent, int32_t *best_parent,
                       double *best_path, int32_t *counts, double *best_cost);
int uavac_rrt_star(uavac_ctx *ctx, const double *start, const double *goal, int B, double step,
                   int max_iter, const double *samples, const double *cuboids, int n_obs,
                   double *nodes, int32_t *canon, int32_t *parent, int32_t *best_parent,
                   double *best_path, int32_t *counts, double *best_cost);
/* E candidate edges p0[e] -> p1[e] against n_obs cuboids [xmin xmax ymin ymax zmin zmax]:
 * hit[e] = 1 when the segment crosses any of them (RRTStar._is_valid_connection is False),
 * slab test of RRTStar._segment_intersects_cuboid (rrt.py:231-274). */
int uavac_rrt_segment_hits_dev(uavac_ctx *ctx, const double *p0, const double *p1, int E,
                               const double *cuboids, int n_obs, int32_t *hit);
int uavac_rrt_segment_hits(uavac_ctx *ctx, const double *p0, const double *p1, int E,
                           const double *cuboids, int n_obs, int32_t *hit);
/* out[e] = np.linalg.norm(p1[e] - p0[e]) as _find_nearest_node / _find_valid_neighbors /
 * _cost_to_come / path_cost take it (rrt.py:84-91,129-173).  p1 is [E][3], or one point [3] for
 * every edge when p1_is_single != 0. */
int uavac_rrt_edge_lengths_dev(uavac_ctx *ctx, const double *p0, const double *p1,
                               int p1_is_single, int E, double *out);
int uavac_rrt_edge_lengths(uavac_ctx *ctx, const double *p0, const double *p1, int p1_is_single,
                           int E, double *out);
/* The nodes RRTStar._generate_random_node (rrt.py:118-127) returns in n consecutive calls after
 * np.random.seed(seeds[b]) -- NumPy's legacy MT19937 stream reproduced on the GPU, bit for bit --
 * for B problems: samples[B][n][3] (what uavac_rrt_star takes); consumed[B][n] (or NULL) = doubles
 * of the stream used up to and including draw i.  limits_lw / limits_up are HOST pointers to 3
 * doubles (the space limits shared by the batch); goals[B][3] must already be rounded to 0.01. */
int uavac_rrt_draw_nodes_dev(uavac_ctx *ctx, const uint32_t *seeds, const double *goals, int B, int n,
                             const double *limits_lw, const double *limits_up, double epsilon,
                             double *samples, int64_t *consumed);
/* RRTStar.simplify_path (rrt.py:93-116) for B paths at once: paths[B][cap][3] with lens[B] waypoints
 * each (e.g. best_path / counts[4] of uavac_rrt_star) -> out_paths[B][cap][3], out_lens[B]: from
 * each kept waypoint the farthest one with a clear direct connection is kept next. */
int uavac_rrt_simplify_dev(uavac_ctx *ctx, const double *paths, const int32_t *lens, int B, int cap,
                           const double *cuboids, int n_obs, double *out_paths, int32_t *out_lens);
int uavac_rrt_simplify(uavac_ctx *ctx, const double *paths, const int32_t *lens, int B, int cap,
                       const double *cuboids, int n_obs, double *out_paths, int32_t *out_lens);
/* RRTStar.path_cost (rrt.py:84-91): the edge lengths of the polyline path[n][3] summed in path
 * order (also the accumulation of _cost_to_come, :163-173, on the node -> start chain). */
int uavac_rrt_path_cost_dev(uavac_ctx *ctx, const double *path, int n, double *cost);
int uavac_rrt_path_cost(uavac_ctx *ctx, const double *path, int n, double *cost);
/* RRTStar._adapt_random_node_position (rrt.py:140-148) for E (sample, nearest node) pairs:
 * out[e] = sample[e] when within step of nearest[e], else the rounded point at step from it. */
int uavac_rrt_steer_dev(uavac_ctx *ctx, const double *sample, const double *nearest, int E,
                        double step, double *out);
int uavac_rrt_steer(uavac_ctx *ctx, const double *sample, const double *nearest, int E, double step,
                    double *out);

/* ---------------------------------------------------------------------------------------------
 * Multi-GPU.  One process per GPU, one ctx per process; missions are sharded by
 * contiguous index blocks and every entry point above works on its own shard -- nothing is
 * exchanged while planning or flying.  The ONE exchange of the path is the final gather of the
 * ragged row blocks (trajectories, or any [n][row_elems] f64 block) to a root rank over RCCL:
 * ncclGroupStart + ncclRecv per peer on the root / ncclSend on the peers + ncclGroupEnd
 * (rccl.h:700,722,923), i.e. every peer uses its own direct xGMI link into the root at once.
 * (No reference counterpart: upstream plans and flies one mission per process, main.py:87-120.)
 *
 * nccl_comm is an ncclComm_t (passed as void* so that this header does not need rccl.h): either the
 * caller's own communicator or one made by uavac_comm_init_rank.  Bootstrap: rank 0 calls
 * uavac_comm_unique_id and hands the 128 bytes to the other ranks by any side channel (environment,
 * file, torch.distributed store); then every rank calls uavac_comm_init_rank (collective). */
#define UAVAC_COMM_ID_BYTES 128
int uavac_comm_unique_id(uavac_ctx *ctx, char id[UAVAC_COMM_ID_BYTES]);
int uavac_comm_init_rank(uavac_ctx *ctx, const char id[UAVAC_COMM_ID_BYTES], int world, int rank,
                         void **nccl_comm);
int uavac_comm_destroy(uavac_ctx *ctx, void *nccl_comm);
int uavac_comm_abort(uavac_ctx *ctx, void *nccl_comm);      /* after a failure or a timeout */
int uavac_comm_shape(uavac_ctx *ctx, void *nccl_comm, int *world, int *rank);
/* Every rank contributes its row count; counts [world] (HOST) receives all of them
 * (ncclAllGather of one int64 per rank; synchronous). */
int uavac_gather_counts(uavac_ctx *ctx, void *nccl_comm, int64_t n_rows, int64_t *counts);
/* Gather: rank r's rows [counts[r]][row_elems] (device) land at row offset sum(counts[:r]) of out
 * (device, root only: [sum(counts)][row_elems]; ignored elsewhere).  counts is the HOST array of
 * uavac_gather_counts.  Enqueued on the ctx stream; uavac_comm_finish synchronises the stream and
 * reports asynchronous RCCL errors. */
int uavac_gather_rows_dev(uavac_ctx *ctx, void *nccl_comm, const double *rows, int64_t n_rows,
                          int row_elems, const int64_t *counts, int root, double *out);
/* Gather of the PLAN instead of the rows.  The rows of a mission are a deterministic, bit-reproducible function of its
 * coefficients and per-segment row counts (uavac_minsnap_sample_dev), 204 B per segment against ~10 KB of rows: the peers
 * send coeffs [n_segments][8][3], times [n_segments] (optional: NULL on every rank or on none) and seg_rows [n_segments]
 * to the root in ONE grouped launch (three ncclSend per peer / three ncclRecv per peer on the root), the root then calls
 * uavac_minsnap_row_offsets_dev + uavac_minsnap_sample_dev on the gathered plan and holds the very rows the peers hold,
 * written at its own HBM rate instead of arriving at the rate of its xGMI links (BASELINE config 4: 0.4 GB instead of
 * 20.8 GB through the root's seven links).  seg_counts is the HOST array of uavac_gather_counts(n_segments); rank r's block
 * lands at segment offset sum(seg_counts[:r]) of the *_out arrays (device, root only).  Enqueued on the ctx stream;
 * uavac_comm_finish synchronises.  (No reference counterpart, like the row gather.) */
int uavac_gather_plan_dev(uavac_ctx *ctx, void *nccl_comm, const double *coeffs, const double *times,
                          const int32_t *seg_rows, int64_t n_segments, const int64_t *seg_counts, int root,
                          double *coeffs_out, double *times_out, int32_t *seg_rows_out);
/* One PART of uavac_gather_plan_dev, for a gather that is PIPELINED with the root's re-sampling: segments
 * [part_first[r], part_first[r] + part_counts[r]) of rank r's block travel and land on the root where the gather of the whole
 * blocks puts them (segment offset sum(seg_counts[:r]) + part_first[r] of the *_out arrays).  The pointers are those of the rank's
 * WHOLE block / of the root's whole output arrays; an array travels when its pointer is non-NULL, on every rank alike (the root:
 * when its *_out pointer is non-NULL) -- e.g. first times + seg_rows of the whole blocks (12 B per segment: the root can then lay
 * out every mission's rows), then the coefficients (192 B per segment) in a few parts, each of which the root samples while the
 * next one arrives.  seg_counts / part_first / part_counts [world] are HOST arrays, the same on every rank.  Enqueued on the ctx
 * stream like the other gathers; RCCL executes the operations of one communicator in the order they were issued, whatever
 * streams they were issued on.  (No reference counterpart.) */
int uavac_gather_plan_part_dev(uavac_ctx *ctx, void *nccl_comm, const double *coeffs, const double *times,
                               const int32_t *seg_rows, const int64_t *seg_counts, const int64_t *part_first,
                               const int64_t *part_counts, int root, double *coeffs_out, double *times_out,
                               int32_t *seg_rows_out);
/* NCCL_VERSION_CODE of the rccl.h this library was built with, and ncclGetVersion() of the RCCL the process has
 * mapped (in a Python process: the one bundled with torch).  uavac_comm_init_rank refuses a different major version
 * or a runtime older than 2.10; only entry points stable since then are used, so the minor versions may differ. */
int uavac_comm_versions(int *built_with, int *runtime);
int uavac_comm_finish(uavac_ctx *ctx, void *nccl_comm);
/* Self-test of the transport on a single GPU: src [n] -> dst [n] through ncclSend + ncclRecv with
 * this rank as its own peer, grouped exactly like the gather (enqueued; then uavac_comm_finish). */
int uavac_comm_loopback_dev(uavac_ctx *ctx, void *nccl_comm, const double *src, double *dst, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* UAVAC_H */
