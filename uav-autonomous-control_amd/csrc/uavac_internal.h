// Internal declarations shared by the libuavac.so translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>

#include "uavac.h"

struct uavac_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;    // == own_stream unless borrowed
    int32_t *d_flags = nullptr;      // [4] device-side error flags (0: non-finite input, 1: singular system)
    int32_t *d_totals = nullptr;     // scratch for the row-count scan
    size_t totals_cap = 0;
    double *d_ws = nullptr;          // block-Thomas workspace [m-1][28][B]
    size_t ws_cap = 0;               // in doubles
    char *d_plan = nullptr;          // uavac_minsnap_plan_dev: times / seg_rows / row_offsets before they are committed
    size_t plan_cap = 0;             // in bytes
    // Device scratch of the host-pointer twins and small internal temporaries: one arena, grown on demand and kept,
    // laid out anew by every Scratch (uavac_scratch.h) that commits.  Reuse across calls is ordered by the ctx stream.
    char *d_arena = nullptr;
    size_t arena_cap = 0;
    bool scratch_live = false;       // a committed Scratch holds pieces of the arena: a second one must not lay it out again
    // Pinned host staging (hipHostMalloc) of the host-pointer twins: two halves used as a ping-pong pipeline.
    char *h_pin = nullptr;
    size_t pin_cap = 0;
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    std::string err;
    int sampler_waves = 4;           // tuning: wavefronts per workgroup of the sampler: 2, 4, 8, 16 (minsnap_sample_stream.hip); 1 = one wave per mission (minsnap_sample.hip)
    int sampler_group = 1;           // tuning: consecutive missions per workgroup of the streaming sampler
    int yaw_group = 8;               // tuning: chunks of the sampler's dense yaw column that leave together (1, 4, 8, 16)
    int audit_lanes = 16;            // tuning: lanes of a wavefront that walk one mission in the plan audit: 16 or 64 (minsnap_audit.hip; same results)
    int separation_split = 0;        // tuning: workgroups that share the j-tiles of one window of the separation audits (minsnap_separation.hip, flown_separation.hip; same results); 0 = sized from the batch
    int search_block = 0;            // tuning: missions per block of the block-wise prioritised search (fleet_wide.h; same results): 64, 128, 256; 0 = the default there
    int conflict_slots = 0;          // tuning: j-tile slots per mission and round of the conflict list's discovery (minsnap_conflicts.hip; same results); 0 = 64
    int flown_audit_split = 0;       // tuning: workgroups that share the ticks of one window of the flown audit (flown_audit.hip; same results); 0 = sized from the batch
    int timeopt_chunk = 0;          // tuning: missions per chunk of the duration optimisation (minsnap_timeopt.hip; same results); 0 = sized from UAVAC_TIMEOPT_SCRATCH_BYTES
    int rollout_align = 1;          // tuning: launch the 2-wave aligner kernel before a logged launch of shape 1
    int late_handover = -1;          // tuning: -1 = the launcher picks per launch; 0 / 1 = slab handed over at the end of the tick / a third of a tick later
    int coeff_dma = -1;              // tuning: -1 = the launcher picks per launch; 0 / 1 / 2 = the plan-fed rollout's PMODE (control_rollout.hip)
    int solve_order = 1;             // which elimination order solves: 1 = two-ended, two lanes per mission (minsnap_solve_tw.hip; the default), 0 = one-ended (minsnap_solve_bt.hip: other rounding, kept as the cross-check)
    int solve_park = -1;             // tuning: where the block-Thomas solve parks its forward sweep: -1 = the launcher picks, 0 = HBM workspace, 1 = LDS (when it fits)
    int solve_lanes = -1;            // tuning: lanes per wave of the block-Thomas solve that carry a mission (64 / 32 / 16; -1 = the launcher picks)
    int solve_keep = -1;             // tuning: the solve of a uniform batch keeps its first five knots' parked blocks in registers: -1 = the launcher picks, 0 / 1
    int idle_waves = -1;             // tuning: placeholder wave between compute and store wave (0 / 1); -1 = the launcher picks
    int cu_balance = 1;              // tuning: a logged rollout below a full chip asks for as much LDS per workgroup as keeps a CU from taking more workgroups than its even share (0: off)
    int lds_pad = 0;                 // tuning: extra dynamic LDS per rollout workgroup (bytes): caps the workgroups a CU takes
    int log_pitch = 0;               // doubles per row of the rollout's logs; 0 = B (option "log_pitch")
    int n_simds = 1024;              // SIMDs of the device (4 per CU): the logged rollout launches one workgroup per SIMD at most
    std::string last_rollout;        // name and template arguments of the rollout kernel launched last (diagnostics)
    int last_rollout_vgprs = 0;      // ... and its vector registers per lane (hipFuncGetAttributes); 0 = unknown
    int64_t last_rollout_launch[6] = {0, 0, 0, 0, 0, 0};   // ... and its shape: grid, threads, dynamic LDS, log pitch, tiles, passes
    int launch_rc = UAVAC_OK;        // set by a rollout launcher that had to give up before the launch (text in err)
    std::string last_solve;          // name and template arguments of the coefficient-solve kernel launched last (diagnostics)
    std::string last_sample;         // ... and of the sampler kernel launched last
    int64_t last_sample_launch[5] = {0, 0, 0, 0, 0};   // ... and its shape: grid, threads, dynamic LDS, missions per workgroup, address phase
};

// Every entry point that launches, allocates or copies runs with the ctx's device current and puts the caller's
// device back on return: a ctx created for GPU 1 must work while GPU 0 is the thread's current device.
struct uavac_device_guard {
    int prev = -1;
    bool switched = false;
    explicit uavac_device_guard(const uavac_ctx *ctx) {
        if (ctx && hipGetDevice(&prev) == hipSuccess && prev != ctx->device) switched = hipSetDevice(ctx->device) == hipSuccess;
    }
    ~uavac_device_guard() {
        if (switched) (void)hipSetDevice(prev);
    }
    uavac_device_guard(const uavac_device_guard &) = delete;
    uavac_device_guard &operator=(const uavac_device_guard &) = delete;
};
#define UAVAC_ENTER(ctx)                \
    if (!(ctx)) return UAVAC_EINVAL;    \
    uavac_device_guard uavac_guard_(ctx)

#define UAVAC_HIP(ctx, call)                                                                     \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                      \
            return UAVAC_EHIP;                                                                   \
        }                                                                                        \
    } while (0)

static inline int uavac_fail(uavac_ctx *ctx, int code, const char *msg) {
    if (ctx) ctx->err = msg;
    return code;
}

constexpr int kLogRows = 13;   // rows of the rollout's state log per tick ([K][13][pitch] f64; positions: rows 0-2), for every kernel that reads one

// blockIdx -> tile such that the blocks of one XCD own a contiguous range of tiles; a bijection on [0, n) for every
// n.  Workgroups go to the chip's 8 XCDs round-robin (blockIdx % 8); when consecutive tiles are consecutive in memory,
// this gives every XCD's L2 one contiguous span to stream to HBM instead of every eighth piece.  Store-only probes:
// the sampler's write pattern 5.6 -> 6.7 TB/s, the rollout's log 5.4 -> 6.3 TB/s (tools/sampler_store_probe.hip,
// tools/log_layout_probe.hip).
#ifdef __HIPCC__
// Workgroup barrier that orders LDS traffic only.  __syncthreads() is also a release/acquire fence for GLOBAL memory:
// the compiler puts `s_waitcnt vmcnt(0)` in front of it, so a wave that has stores (or a prefetch) in flight waits
// for their completion -- a full HBM round trip -- at every barrier.  The kernels here hand data over through LDS
// and never read back what they store to HBM, so they wait for LDS (lgkmcnt) alone and leave vector-memory
// operations in flight across the barrier.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
// Same for a workgroup that is a single wavefront: LDS operations of one wave execute in order, so only the
// compiler needs to be told not to move memory accesses across this point.
__device__ __forceinline__ void lds_wave_fence() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

__device__ __forceinline__ int xcd_contiguous(int block, int n) {
    const int x = block & 7, q = n >> 3, r = n & 7;
    return x * q + (x < r ? x : r) + (block >> 3);
}
#endif

// uavac_create's self-check (control_probe.hip): the sampler's heading() against the device library's atan2, which the rollout's
// yaw scan uses, on 2^16 + 144 operand pairs; *mismatches = pairs whose bits differ.
int uavac_heading_selfcheck(uavac_ctx *ctx, int *mismatches);

// "Grow this ctx buffer if it is too small", for every buffer the ctx owns: `cap` and `need` are in the buffer's own unit, `bytes`
// is what `need` takes.  The old block is freed after the ctx stream has drained (nothing enqueued may still use it); what it
// held is lost.  `pinned`: page-locked host memory instead of device memory.
template <class T>
int uavac_grow(uavac_ctx *ctx, T *&buf, size_t &cap, size_t need, size_t bytes, bool pinned = false) {
    if (need <= cap) return UAVAC_OK;
    UAVAC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (buf) UAVAC_HIP(ctx, pinned ? hipHostFree(buf) : hipFree(buf));
    buf = nullptr;
    cap = 0;
    void *p = nullptr;
    UAVAC_HIP(ctx, pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes));
    buf = static_cast<T *>(p);
    cap = need;
    return UAVAC_OK;
}
// Device scratch arena (uavac_api.hip): room for `bytes` in total, with headroom when it has to grow.  Scratch::commit
// (uavac_scratch.h) is its one caller.
int uavac_arena_reserve(uavac_ctx *ctx, size_t bytes);
// Pinned staging: at least `bytes` of page-locked host memory in ctx->h_pin.
int uavac_pin_reserve(uavac_ctx *ctx, size_t bytes);
// Pageable host buffer <-> device through the pinned ping-pong buffer, ordered on the ctx stream (uavac_api.hip).
// h2d returns once the source has been read; d2h once the destination holds the data.
int uavac_h2d(uavac_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int uavac_d2h(uavac_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);

// Kernel-side view of uavac_vehicle with the per-call constants hoisted on the host.
struct VehK {
    double g, dt, dt_outer, mass, inv_mass;
    double I[3], inv_I[3];
    double arm, inv_arm, kappa, inv_kappa, kf, inv_kf;
    double min_thrust, max_thrust, c_min, c_max;
    double resp_rise, resp_fall;     // 1 - exp(-dt/tau): quad.py:102
    double max_ascent, max_descent, max_speed_xy, max_horiz_accel, max_tilt;
    double kp_xy, kd_xy, kp_z, kd_z, ki_z, kp_roll, kp_pitch, kp_yaw;
    double ikp[3];                   // I * kp_pqr: controller.py:128
    double hover_omega;
    double ground_zc, ground_k, ground_b, ground_z;   // contact starts at pz > ground_zc = ground_z - clearance; 1/tc^2, 2/tc
    // the non-inline fp64 literals of the per-tick path (control_law.h): smallest normal, the large-angle threshold on
    // (|w| dt / 2)^2, the Taylor coefficients of cos and sinc, 3/8 and the threshold of the renormalisation series.  They
    // travel with the vehicle constants so that the rollout can put them into vector registers ONCE, ahead of its tick loop
    double lit_tiny, lit_h2_small, lit_c8, lit_c6, lit_c4, lit_s9, lit_s7, lit_s5, lit_s3, lit_375, lit_e_small;
    int F;
    int ground;
};

VehK uavac_make_vehk(const uavac_vehicle &V);
int uavac_check_vehicle(uavac_ctx *ctx, const uavac_vehicle *V);

// launchers
// seg_offsets (device, [B+1]) != NULL: ragged batch -- mission b has seg_offsets[b+1] - seg_offsets[b] segments (1 .. m,
// m = the batch's maximum); waypoints, times, row counts, coefficients and hit flags lie back to back
int uavac_launch_row_counts(uavac_ctx *ctx, const double *wp, int B, int m, double velocity, double dt,
                            double *times, int32_t *seg_rows, int64_t *row_offsets, const int64_t *seg_offsets = nullptr);
// the same with a cruise speed per mission, velocities [B] (device): a value that is not positive and finite raises flag 0 and
// leaves its mission without rows
int uavac_launch_row_counts_v(uavac_ctx *ctx, const double *wp, int B, int m, const double *velocities, double dt,
                              double *times, int32_t *seg_rows, int64_t *row_offsets, const int64_t *seg_offsets = nullptr);
// The coefficient solve (minsnap_solve.hip): hands over to the two-ended or the one-ended block-Thomas launcher by ctx->solve_order.
// guard_rows (device, may be NULL): the launch does nothing when *guard_rows > guard_capacity (a refused planning chain)
int uavac_launch_coeff_solve(uavac_ctx *ctx, const double *wp, const double *times, int B, int m, double *coeffs,
                             int32_t *status, const int64_t *seg_offsets = nullptr, const int64_t *guard_rows = nullptr,
                             int64_t guard_capacity = 0, const int32_t *active = nullptr);
// its two forms: two lanes per mission (minsnap_solve_tw.hip), one lane per mission (minsnap_solve_bt.hip); what the two launchers
// share on the host side is in minsnap_solve_launch.h, the device pieces of both kernels in minsnap_kkt.h
int uavac_launch_solve_tw(uavac_ctx *ctx, const double *wp, const double *times, int B, int m, double *coeffs,
                          int32_t *status, const int64_t *seg_offsets, const int64_t *guard_rows, int64_t guard_capacity,
                          const int32_t *active);
int uavac_launch_solve_bt(uavac_ctx *ctx, const double *wp, const double *times, int B, int m, double *coeffs,
                          int32_t *status, const int64_t *seg_offsets, const int64_t *guard_rows, int64_t guard_capacity,
                          const int32_t *active);
// the solve with boundary derivatives (minsnap_solve_bc.hip): bc [B][6][3] (device) = (v, a, j) at the first and at the last waypoint
int uavac_launch_solve_bc(uavac_ctx *ctx, const double *wp, const double *times, int B, int m, const double *bc, double *coeffs,
                          int32_t *status, const int64_t *seg_offsets, const int64_t *guard_rows, int64_t guard_capacity);
// One round of the obstacle loop on the device (minsnap_obstacles.hip): collision scan of the active missions' splines
// (no rows stored) + midpoint insertion into the next waypoint arrays
int uavac_launch_obstacle_scan_and_insert(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, const double *coeffs,
                                          const int32_t *seg_rows, int B, int max_m, double dt, const double *aabb,
                                          int32_t *active, int32_t *overflow, int32_t *touched, int32_t *hit, double *wp_out,
                                          int64_t *seg_offsets_out, int32_t *counters);
// row_offsets [B+1] from per-segment row counts that exist already (minsnap_solve.hip)
int uavac_launch_row_offsets(uavac_ctx *ctx, const int32_t *seg_rows, int B, int m, int64_t *row_offsets,
                             const int64_t *seg_offsets = nullptr);
// exclusive prefix sum of ctx->d_totals [B] (filled by the caller's kernel together with the tile sums) -> out [B+1] i64
int uavac_launch_totals_scan(uavac_ctx *ctx, int B, int64_t *out);
int uavac_ensure_totals(uavac_ctx *ctx, int B, int32_t **totals, int64_t **tile_sums);
// times / seg_rows / row_offsets from scratch into the caller's arrays unless row_offsets_s[B] > capacity_rows
int uavac_launch_plan_commit(uavac_ctx *ctx, const double *times_s, const int32_t *seg_rows_s, const int64_t *row_offsets_s,
                             int B, int m, int64_t capacity_rows, double *times, int32_t *seg_rows, int64_t *row_offsets);
// the pivoted banded-LU form of the coefficient solve: the cross-check behind uavac_minsnap_solve_banded_dev
int uavac_launch_solve_banded(uavac_ctx *ctx, const double *wp, const double *times, int B, int m, double *coeffs,
                              int32_t *status);
// Optional outputs / inputs of the sampler (minsnap_sample.hip)
struct SampleExtras {
    const double *aabb = nullptr;    // [6] cuboid of the collision scan, with
    int32_t *hit = nullptr;          // [B][m] hit flags
    double *yaw_dense = nullptr;     // [rows] the yaw column on its own
    double *first_yaw = nullptr;     // [B] heading of each mission's first row that has one (0 when none has)
    double *jerk = nullptr;          // [rows][3]
    double *snap = nullptr;          // [rows][3]
    int64_t capacity_rows = -1;      // rows the trajectory buffer holds; < 0: not checked
    const int64_t *seg_offsets = nullptr;   // [B+1] ragged batch (see uavac_launch_row_counts); m is then the maximum
    int64_t total_segments = -1;            // ... and its number of segments (sizes the hit flags)
};
int uavac_launch_sample(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *row_offsets,
                        int B, int m, double dt, double *traj, const SampleExtras &x);
// the same rows from workgroups of `waves` (4, 8, 16) wavefronts that stream the 64-row chunks of `group` consecutive missions
// in address order (minsnap_sample_stream.hip)
int uavac_launch_sample_stream(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *row_offsets, int B,
                               int m, double dt, double *traj, const SampleExtras &x, int waves, int group);
int uavac_launch_yaw_scan(uavac_ctx *ctx, const double *velocities, const int64_t *offsets, int B, double *yaws);
// first_yaw [B] without the rows (minsnap_first_yaw.hip): what the sampler writes there, from the coefficients and row counts alone
int uavac_launch_first_yaw(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                           double dt, double *first_yaw);
// what a plan's rows would show, per mission, without the rows (minsnap_audit.hip): audit [UAVAC_AUDIT_ROWS][B], and per cuboid
// hit_rows / first_hit [n_cuboids][B]
int uavac_launch_audit(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                       double dt, const double *cuboids, int n_cuboids, double *audit, int32_t *hit_rows, int32_t *first_hit);
// what a plan asks of the vehicle, per mission, without the rows (minsnap_demand.hip): demand [UAVAC_DEMAND_ROWS][B], idemand
// [UAVAC_IDEMAND_ROWS][B], and per cuboid clearance / clearance_row [n_cuboids][B]
int uavac_launch_demand(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                        double g, const double *cuboids, int n_cuboids, double *demand, int32_t *idemand, double *clearance,
                        int32_t *clearance_row);
// the fleet's audit against itself (minsnap_separation.hip): sep [B], isep [UAVAC_SEP_ROWS][B]; scratch from the ctx arena
int uavac_launch_separation(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                            const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, double *sep, int32_t *isep);
// the audit's conflict graph in CSR form (minsnap_conflicts.hip): pair_offsets [B + 1], then pair_d [capacity] and pair_i
// [UAVAC_CONF_ROWS][capacity]; scratch from the ctx arena
int uavac_launch_conflict_offsets(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                  double dt, const int64_t *group_offsets, int G, const int32_t *start_rows, double radius,
                                  int64_t *pair_offsets);
int uavac_launch_conflicts(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                           const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, const int64_t *pair_offsets,
                           int64_t capacity, double *pair_d, int32_t *pair_i);
// the call that acts on it (minsnap_stagger.hip): start delays by priority, istag [UAVAC_STAGGER_ROWS][B]; scratch from the ctx arena
int uavac_launch_stagger(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                         const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, int step, int max_steps,
                         int32_t *istag);
// the delays as part of the plan (minsnap_delay.hip): out_seg_offsets [B+1] = prefix sum of m_b + (S_b > 0); then the delayed plan's
// coefficients, durations (times / out_times may both be NULL) and row counts, a leading hold segment for every mission with S_b > 0
int uavac_launch_delay_offsets(uavac_ctx *ctx, const int64_t *seg_offsets, int B, int m, const int32_t *start_rows, int64_t *out_seg_offsets);
int uavac_launch_delay(uavac_ctx *ctx, const double *coeffs, const double *times, const int32_t *seg_rows, const int64_t *seg_offsets, int B,
                       int m, double dt, const int32_t *start_rows, const int64_t *out_seg_offsets, double *out_coeffs, double *out_times,
                       int32_t *out_seg_rows);
// deconfliction by offset layers at fixed starts (minsnap_layer.hip): ilayer [UAVAC_LAYER_ROWS][B], offsets [B][3]; scratch from the ctx
// arena; and the offsets as part of the plan: out_coeffs = coeffs with offsets[b] added to c0 of every segment of mission b
int uavac_launch_layer(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                       const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, double delta_x, double delta_y,
                       double delta_z, int max_steps, int32_t *ilayer, double *offsets);
// the two searches for groups of any size up to group_cap (minsnap_stagger_wide.hip, minsnap_layer_wide.hip: the block-wise form of
// fleet_wide.h); outputs as uavac_launch_stagger's and uavac_launch_layer_obs's; scratch, the seed words included, from the ctx arena
int uavac_launch_stagger_wide(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                              const int64_t *group_offsets, int G, int group_cap, const int32_t *start_rows, double radius, int step,
                              int max_steps, int32_t *istag);
int uavac_launch_layer_wide(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                            const int64_t *group_offsets, int G, int group_cap, const int32_t *start_rows, double radius, double delta_x,
                            double delta_y, double delta_z, int max_steps, const double *cuboids, int n_cuboids, int32_t *ilayer,
                            double *offsets);
// the same two searches and the audit AGAINST TRAFFIC, a second plan (t_*) that never moves (minsnap_stagger_against.hip,
// minsnap_layer_against.hip: fleet_against.h; minsnap_separation_against.hip); outputs as the wide searches' and the audit's
int uavac_launch_stagger_against(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                                 const int64_t *group_offsets, int G, int group_cap, const int32_t *start_rows, const double *t_coeffs,
                                 const int32_t *t_seg_rows, const int64_t *t_seg_offsets, int Bt, int mt, const int64_t *t_group_offsets,
                                 const int32_t *t_start_rows, double radius, int step, int max_steps, int32_t *istag);
int uavac_launch_layer_against(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                               const int64_t *group_offsets, int G, int group_cap, const int32_t *start_rows, const double *t_coeffs,
                               const int32_t *t_seg_rows, const int64_t *t_seg_offsets, int Bt, int mt, const int64_t *t_group_offsets,
                               const int32_t *t_start_rows, double radius, double delta_x, double delta_y, double delta_z, int max_steps,
                               const double *cuboids, int n_cuboids, int32_t *ilayer, double *offsets);
int uavac_launch_separation_against(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                    double dt, const int64_t *group_offsets, int G, const int32_t *start_rows, const double *t_coeffs,
                                    const int32_t *t_seg_rows, const int64_t *t_seg_offsets, int Bt, int mt, const int64_t *t_group_offsets,
                                    const int32_t *t_start_rows, double radius, double *sep, int32_t *isep);
// the cross audit's conflict graph in CSR form (minsnap_conflicts_against.hip): pair_offsets [B + 1], then pair_d [capacity] and pair_i
// [UAVAC_CONF_ROWS][capacity] with TRAFFIC batch indices as partners; scratch from the ctx arena
int uavac_launch_conflict_against_offsets(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B,
                                          int m, double dt, const int64_t *group_offsets, int G, const int32_t *start_rows,
                                          const double *t_coeffs, const int32_t *t_seg_rows, const int64_t *t_seg_offsets, int Bt, int mt,
                                          const int64_t *t_group_offsets, const int32_t *t_start_rows, double radius, int64_t *pair_offsets);
int uavac_launch_conflicts_against(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                   double dt, const int64_t *group_offsets, int G, const int32_t *start_rows, const double *t_coeffs,
                                   const int32_t *t_seg_rows, const int64_t *t_seg_offsets, int Bt, int mt, const int64_t *t_group_offsets,
                                   const int32_t *t_start_rows, double radius, const int64_t *pair_offsets, int64_t capacity, double *pair_d,
                                   int32_t *pair_i);
int uavac_launch_shift(uavac_ctx *ctx, const double *coeffs, const int64_t *seg_offsets, int B, int m, int64_t total_segments,
                       const double *offsets, double *out_coeffs);
// the same search, refusing every layer on which a row of the mission's own lies inside a cuboid (minsnap_layer_obs.hip): cuboids
// [n_cuboids][6] (may be NULL with n_cuboids = 0), ilayer [UAVAC_LAYER_OBS_ROWS][B]
int uavac_launch_layer_obs(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                           const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, double delta_x, double delta_y,
                           double delta_z, int max_steps, const double *cuboids, int n_cuboids, int32_t *ilayer, double *offsets);
// the separation the fleet flew (flown_separation.hip): the audit's outputs from the positions of a state log [K][13][pitch]
int uavac_launch_flown_separation(uavac_ctx *ctx, const double *state_log, int K, int B, int64_t pitch, const int64_t *group_offsets, int G,
                                  double radius, double *sep, int32_t *isep);
// that audit's conflict graph in CSR form (flown_conflicts.hip): pair_offsets [B + 1], then pair_d [capacity] and pair_i
// [UAVAC_CONF_ROWS][capacity] with ticks where the plan's list has clock rows; scratch from the ctx arena
int uavac_launch_flown_conflict_offsets(uavac_ctx *ctx, const double *state_log, int K, int B, int64_t pitch, const int64_t *group_offsets,
                                        int G, double radius, int64_t *pair_offsets);
int uavac_launch_flown_conflicts(uavac_ctx *ctx, const double *state_log, int K, int B, int64_t pitch, const int64_t *group_offsets, int G,
                                 double radius, const int64_t *pair_offsets, int64_t capacity, double *pair_d, int32_t *pair_i);
// what the vehicles did against the flight limits and the cuboids (flown_audit.hip): audit [UAVAC_FLOWN_AUDIT_ROWS][B], first_bad [B],
// and per cuboid hit_ticks / first_hit / clearance / clearance_tick [n_cuboids][B], from a state log [K][13][pitch]; scratch from the arena
int uavac_launch_flown_audit(uavac_ctx *ctx, const double *state_log, int K, int B, int64_t pitch, const double *cuboids, int n_cuboids,
                             double *audit, int32_t *first_bad, int32_t *hit_ticks, int32_t *first_hit, double *clearance,
                             int32_t *clearance_tick);
// Retiming factors from an audit block (minsnap_retime.hip): factors [B], counters [2] += {missions slowed down, missions with a
// NaN peak}; apply != 0 divides the velocities of the missions over a limit by their factor.  The loop's extras (each may be NULL):
// factors_total [B] *= the factor applied (NaN for a NaN mission), converged [B] = 1 where the factor is 1.0, else 0.
struct RetimeLimits {
    double speed_xy, ascent, descent, horiz_accel;
};
int uavac_launch_retime_factors(uavac_ctx *ctx, const double *audit, int B, const RetimeLimits &limits, double margin, int apply,
                                double *velocities, double *factors, int32_t *counters, double *factors_total, int32_t *converged);
// The slowdown factors the vehicle's tilt and thrust limits ask for, per mission, without the rows (minsnap_need.hip): need
// [UAVAC_NEED_ROWS][B].  The constants are formed once on the host (uavac_api.hip need_limits), each ONE rounded operation.
struct NeedLimits {
    double g, tau;       // gravitational acceleration, max_tilt
    double t2;           // tau * tau
    double tg;           // tau * g
    double D;            // Fmax * Fmax - g * g   (> 0: the vehicle can hover)
    double E;            // g * g - Fmin * Fmin   (> 0)
};
int uavac_launch_need(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                      const NeedLimits &limits, double *need);
// The retiming factors with the need block's four terms beside the audit's four (minsnap_retime.hip); binding [B] = the first term
// that attains the maximum (0 .. 7, -1 for a NaN mission).  Everything else as uavac_launch_retime_factors.
int uavac_launch_retime_demand_factors(uavac_ctx *ctx, const double *audit, const double *need, int B, const RetimeLimits &limits,
                                       double margin, int apply, double *velocities, double *factors, int32_t *binding, int32_t *counters,
                                       double *factors_total, int32_t *converged);
// Plans from given durations, the snap cost and the optimisation of the durations (minsnap_timeopt.hip); seg_offsets as above.
// seg_rows = ceil(times / dt) and row_offsets [B+1]; a duration that is not positive and finite raises flag 0 and leaves its mission
// without rows
int uavac_launch_row_counts_t(uavac_ctx *ctx, const double *times, const int64_t *seg_offsets, int B, int m, double dt,
                              int32_t *seg_rows, int64_t *row_offsets);
// seg_rows / row_offsets from scratch into the caller's arrays unless row_offsets_s[B] > capacity_rows (uavac_launch_plan_commit
// without the durations, which are an input there)
int uavac_launch_plan_t_commit(uavac_ctx *ctx, const int32_t *seg_rows_s, const int64_t *row_offsets_s, const int64_t *seg_offsets, int B,
                               int m, int64_t capacity_rows, int32_t *seg_rows, int64_t *row_offsets);
// cost [B] = integral of snap^2 over every mission
int uavac_launch_cost(uavac_ctx *ctx, const double *coeffs, const double *times, const int64_t *seg_offsets, int B, int m, double *cost);
// the whole optimisation loop, enqueued: times [.] in/out, cost_before / cost_after [B], accepted [B]
int uavac_launch_optimize_times(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B, int m, double *times, int iterations,
                                double *cost_before, double *cost_after, int32_t *accepted);
// out [n] = value (minsnap_retime.hip)
int uavac_launch_fill_f64(uavac_ctx *ctx, double *out, size_t n, double value);
int uavac_launch_state_init(uavac_ctx *ctx, const VehK &V, const double *positions, int B, int hover, double *state,
                            int32_t *istate);
// What the rollout needs to evaluate target rows itself instead of reading them (control_rollout.hip, POLY)
struct PlanRef {
    const double *coeffs = nullptr;      // [B][8m][3]
    const int32_t *seg_rows = nullptr;   // [B][m]
    const double *yaw = nullptr;         // [row_offsets[B]] dense yaw column of the sampler, or NULL: the rollout scans the yaw
    const double *first_yaw = nullptr;   // [B] (with yaw == NULL) heading the rows before a mission's first heading take
    double dt = 0.0;
    int m = 0;
    const int64_t *seg_offsets = nullptr;   // [B+1] ragged batch: coeffs [S][8][3], seg_rows [S] back to back, m = the maximum
};
int uavac_launch_rollout(uavac_ctx *ctx, const VehK &V, const double *traj, const int64_t *row_offsets, double *state,
                         int32_t *istate, int B, int K, double *state_log, double *cmd_log, const double *aabbs,
                         int n_obs, const PlanRef *plan = nullptr, double *score = nullptr);
// missions of a plan selected, reordered and merged (minsnap_take.hip): out_seg_offsets [n+1] = prefix sum of the segment counts of
// the missions index[i] (clamped into 0 .. B - 1, flag 0); then their coefficients, durations (times / out_times may both be NULL), row
// counts and first headings (first_yaw / out_first_yaw may both be NULL), output mission i = input mission index[i]
int uavac_launch_take_offsets(uavac_ctx *ctx, const int64_t *seg_offsets, int B, int m, const int32_t *index, int n, int64_t *out_seg_offsets);
int uavac_launch_take(uavac_ctx *ctx, const double *coeffs, const double *times, const int32_t *seg_rows, const int64_t *seg_offsets, int B,
                      int m, const double *first_yaw, const int32_t *index, int n, const int64_t *out_seg_offsets, double *out_coeffs,
                      double *out_times, int32_t *out_seg_rows, double *out_first_yaw);
// priorities into a within-group order (minsnap_take.hip): order [B] = the mission in every slot, rank [B] its inverse
int uavac_launch_fleet_order(uavac_ctx *ctx, const double *priority, const int64_t *group_offsets, int G, int B, int32_t *order,
                             int32_t *rank);
// a mission's swept box without the rows (minsnap_envelope.hip): env [B][6] = lo x y z, hi x y z over the sampler's positions and, with
// reach [B][3] (device, may be NULL), over those of the plan with c0' = fl(c0 + reach[b]) as well
int uavac_launch_envelope(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                          double dt, const double *reach, double *env);
// the connected components of "boxes nearer than the radius", per group (fleet_airspaces.hip): labels [B] = the lowest batch index of
// the mission's component once converged, info [2] = {rounds that changed a label, converged}; scratch from the ctx arena
int uavac_launch_fleet_airspaces(uavac_ctx *ctx, const double *env, const int64_t *group_offsets, int G, int B, double radius, int rounds,
                                 int resume, int32_t *labels, int32_t *info);
