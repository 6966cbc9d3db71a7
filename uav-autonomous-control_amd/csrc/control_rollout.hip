// Fused cascaded controller + rotor allocation + motor lag + NED 6-DoF free-body step (gfx950).
//
// One lane per UAV, K ticks per launch, all controller / vehicle state in registers.
// Per tick (upstream paths):
//   every F-th tick: TrajectoryController._update_outer_loop      uav_ac/main.py:47-61
//       Quad.R / quat_to_rot                                      uav_ac/quadrotor/quad.py:129-155
//       CascadedController.altitude                               uav_ac/control/controller.py:26-56
//       CascadedController.lateral                                :58-97
//       CascadedController.roll_pitch_controller / yaw_controller :132-168 (Euler angles quad.py:189-213)
//   every tick:  CascadedController.body_rate_controller          controller.py:115-130
//                Quad._allocate_rotor_forces / set_propeller_speed quad.py:88-122
//                MujocoSimulation._apply_rotor_forces + mj_step    uav_ac/simulation/mujoco_sim.py:144-151,232-251
//                (free joint, Euler integrator, no contacts; restated in NED/FRD)
//
// HBM traffic per UAV tick: 104 B of state log (13 f64, coalesced) + one 88 B trajectory row every F ticks.
//
// Workgroup = one compute wave + (when a log is requested) one STORE wave.
//   Measured on MI355X at B = 65 536, per 1 000 ticks: arithmetic alone 0.76 ms; the 6.8 GB log stream alone,
//   in this [K][13][B] pattern, 1.25-1.4 ms (tools/store_wave_probe.hip; a contiguous fill reaches 6.5 TB/s).
//   A wave that issues a vector store stalls until the CU's store path has taken it, so with the stores in
//   the compute waves a tick costs arithmetic + store time (1.74-1.8 ms), and neither start-time stagger,
//   nor spreading the stores through the tick, nor removing the compiler's per-tick vmcnt(0) changes that
//   much: the storing wave itself is what blocks.  Here the compute wave never stores: each tick it drops
//   its 13 (+12) log values into an LDS slab (ds_write, non-blocking), one workgroup barrier hands the slab
//   to the store wave, and that wave streams it to HBM while the compute wave is already in the next tick
//   (two slabs, ping-pong): 1.66 ms, i.e. the store stream (slowed ~25 % by the concurrent arithmetic) now
//   sets the pace and the arithmetic hides under it.

#include "control_law.h"
#include "minsnap_eval.h"
#include "minsnap_yaw.h"

#include <atomic>
#include <cmath>
#include <cstdlib>
#include <string>

namespace {

using namespace uavac_dev;

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ---- trajectory-row prefetch with a hand-placed wait ------------------------------------------------
// On gfx950 loads and stores share one in-order counter (vmcnt).  A row load the compiler knows to be in
// flight across ticks makes it put `s_waitcnt vmcnt(0)` at every join of the tick loop (its registers are
// loop-carried).  Issued from inline asm the load is invisible to that pass; the registers are touched by
// nothing until row_wait(), which every later read is data-dependent on.
// The operands are output-only ("=&v").  What makes that right is not the constraint but the BUILD CHECK: uav_ac/_buildcheck.py
// (run by __graft_entry__.build() and by the CPU tests) disassembles every row-fed variant and fails the build unless both issue
// sites load into the same twenty registers and no instruction reads or writes one of them between the loads and an
// `s_waitcnt vmcnt(0)` -- i.e. unless the loads land in the very registers row_wait() hands on.  (An output-only operand MAY be
// given a register of its own and copied into the carried one before the data has arrived; it happened once, NOTES R4-4, and
// the check is what catches it.  The "+v" form, which ties the destination to the carried register by construction, was measured
// in round 5: +1.5 % on every row-fed tick -- the twenty registers then stay live through the outer block -- and +2.7 % with an
// empty block in front to end their live range, tools/r05_asm_ab.sh; so the check carries the guarantee instead.)
struct RowRegs { u32x4 q[5]; };          // columns 0..9 of a row (x y z vx vy vz ax ay az yaw): 80 bytes

__device__ __forceinline__ void row_issue(RowRegs &r, const double *p) {
    asm volatile("global_load_dwordx4 %0, %5, off\n\t"
                 "global_load_dwordx4 %1, %5, off offset:16\n\t"
                 "global_load_dwordx4 %2, %5, off offset:32\n\t"
                 "global_load_dwordx4 %3, %5, off offset:48\n\t"
                 "global_load_dwordx4 %4, %5, off offset:64"
                 : "=&v"(r.q[0]), "=&v"(r.q[1]), "=&v"(r.q[2]), "=&v"(r.q[3]), "=&v"(r.q[4])
                 : "v"(p)
                 : "memory");
}
__device__ __forceinline__ void row_wait(RowRegs &r) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(r.q[0]), "+v"(r.q[1]), "+v"(r.q[2]), "+v"(r.q[3]), "+v"(r.q[4])::"memory");
}
template <class T> __device__ __forceinline__ void settle(T &x) { asm volatile("" : "+v"(x)); }

// Plan-fed rollout: the 24 coefficients of a lane's NEXT segment travel from HBM straight into the lane's column of the wave's
// LDS tile (LDS-DMA, global_load_lds_dwordx4: no registers, nothing to wait for here) -- issued when the cursor enters the
// segment, needed one outer tick (F ticks) later.  Loaded through registers on the spot they cost the whole load latency at
// every segment change of any lane of the wave (44 % of the outer ticks), and that latency grows with the chip's load: 1.1 k
// cycles at 8 192 UAVs, 2.3 k at 32 768, 3 k at 49 152 (NOTES R4-3, profiles/r04_tick_stamps_*.jsonl) -- it was the half-full chip's longer tick.
// Tile layout [12][64][2] doubles (minsnap_eval.h, STRIDE 0): instruction p moves doubles 2p, 2p + 1 of every active lane; lane l
// lands at M0 + offset + 16 l, and the instruction offset counts for the GLOBAL address and for the LDS address alike, so M0
// advances by 1024 - 16 per instruction.  Masked-off lanes keep their column (tools/scratch/ldsdma_gather_probe.hip).
// Like the row prefetch the loads are invisible to the compiler's vmcnt bookkeeping; `plan_loads_wait` covers them.
__device__ __forceinline__ void coeffs_dma(const double *src, unsigned tile_lds_bytes) {
    // M0 is a register the compiler reserves for itself: it takes no clobber for it ("inline asm clobber list contains reserved
    // registers: m0"), so the block saves it in a scalar register of its own and puts it back -- whatever the compiler keeps
    // there survives.  (The DMA instructions read M0 when they issue; the value may change behind them.)
    unsigned saved_m0;
    asm volatile("s_mov_b32 %0, m0\n\t"
                 "s_mov_b32 m0, %2\n\ts_nop 1\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                 "s_add_u32 m0, m0, 0x3f0\n\ts_nop 1\n\tglobal_load_lds_dwordx4 %1, off offset:16\n\t"
                 "s_add_u32 m0, m0, 0x3f0\n\ts_nop 1\n\tglobal_load_lds_dwordx4 %1, off offset:32\n\t"
                 "s_add_u32 m0, m0, 0x3f0\n\ts_nop 1\n\tglobal_load_lds_dwordx4 %1, off offset:48\n\t"
                 "s_add_u32 m0, m0, 0x3f0\n\ts_nop 1\n\tglobal_load_lds_dwordx4 %1, off offset:64\n\t"
                 "s_add_u32 m0, m0, 0x3f0\n\ts_nop 1\n\tglobal_load_lds_dwordx4 %1, off offset:80\n\t"
                 "s_add_u32 m0, m0, 0x3f0\n\ts_nop 1\n\tglobal_load_lds_dwordx4 %1, off offset:96\n\t"
                 "s_add_u32 m0, m0, 0x3f0\n\ts_nop 1\n\tglobal_load_lds_dwordx4 %1, off offset:112\n\t"
                 "s_add_u32 m0, m0, 0x3f0\n\ts_nop 1\n\tglobal_load_lds_dwordx4 %1, off offset:128\n\t"
                 "s_add_u32 m0, m0, 0x3f0\n\ts_nop 1\n\tglobal_load_lds_dwordx4 %1, off offset:144\n\t"
                 "s_add_u32 m0, m0, 0x3f0\n\ts_nop 1\n\tglobal_load_lds_dwordx4 %1, off offset:160\n\t"
                 "s_add_u32 m0, m0, 0x3f0\n\ts_nop 1\n\tglobal_load_lds_dwordx4 %1, off offset:176\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(saved_m0) : "v"(src), "s"(tile_lds_bytes) : "memory", "scc");
}
// the row count of the segment AFTER the one just entered: needed a whole segment later
// ("+v": the load lands IN the loop-carried register; an output-only operand may get a register of its own and be copied
// into the carried one right away, before the data has arrived)
__device__ __forceinline__ void seg_rows_issue(int &r, const int32_t *p) {
    asm volatile("global_load_dword %0, %1, off" : "+v"(r) : "v"(p) : "memory");
}
__device__ __forceinline__ void plan_loads_wait(int &r) { asm volatile("s_waitcnt vmcnt(0)" : "+v"(r)::"memory"); }
template <int N> __device__ __forceinline__ void store_wave_loads_wait(int &r) { asm volatile("s_waitcnt vmcnt(%1)" : "+v"(r) : "n"(N) : "memory"); }

__device__ __forceinline__ double row_col(const RowRegs &r, int c) {      // c is a compile-time constant
    const u32x4 q = r.q[c >> 1];
    u32x2 h;
    if (c & 1) { h.x = q.z; h.y = q.w; } else { h.x = q.x; h.y = q.y; }
    return __builtin_bit_cast(double, h);
}

// A store whose address is a wave-uniform 64-bit base in SGPRs plus a 32-bit byte offset per lane.  The store wave issues
// 13 (+12) of these per tick; with the lane folded into a 64-bit VGPR pointer every one of them needed a 64-bit vector
// add first, and those adds queue behind the compute wave's fp64 instructions on the SIMD's single vector issue port
// (each waits up to one fp64 instruction, ~7 cycles).  In this form the row addresses advance with scalar adds and the
// store wave issues no vector-ALU instruction per store.
__device__ __forceinline__ void store_uniform_base(double *base, unsigned lane_bytes, double v) {
    asm volatile("global_store_dwordx2 %0, %1, %2" : : "v"(lane_bytes), "v"(v), "s"(base) : "memory");
}

// The constants only the outer loop needs (gains, flight limits) are re-read from the kernel-argument
// segment inside the outer block instead of living in SGPRs across the whole tick loop: the per-tick path
// alone needs ~50 SGPRs of constants, both sets together overflow the 102 available and the overflow
// would be paid in v_readlane on every tick.  VehK is the kernel's first argument => offset 0.
__device__ __forceinline__ VehK outer_constants() {
    typedef const __attribute__((address_space(4))) VehK *kptr;
    kptr vp = (kptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(vp));                 // opaque: the scalar loads below stay inside the outer block
    VehK O;
    O.g = vp->g; O.dt_outer = vp->dt_outer; O.mass = vp->mass; O.c_min = vp->c_min; O.c_max = vp->c_max;
    O.max_ascent = vp->max_ascent; O.max_descent = vp->max_descent; O.max_speed_xy = vp->max_speed_xy;
    O.max_horiz_accel = vp->max_horiz_accel; O.max_tilt = vp->max_tilt;
    O.kp_xy = vp->kp_xy; O.kd_xy = vp->kd_xy; O.kp_z = vp->kp_z; O.kd_z = vp->kd_z; O.ki_z = vp->ki_z;
    O.kp_roll = vp->kp_roll; O.kp_pitch = vp->kp_pitch; O.kp_yaw = vp->kp_yaw;
    return O;
}

// CW: compute waves per workgroup (UAVs per workgroup = 64 CW).  LDS slab layout: [2][NR][64 CW] doubles,
// NR = 13 state rows (+ 12 command rows).
// POLY: the target row of an outer tick is not read from the sampled trajectory but evaluated from the 24
// coefficients of the UAV's current segment (the sampler's own function, bit for bit: minsnap_eval.h), with the
// yaw -- the one column that is a scan over all earlier rows -- taken from the sampler's dense yaw array 16 rows at
// a time.  Per UAV and outer tick that is 8 B of yaw plus 192 B of coefficients per ~110 rows instead of an 80-B
// row whose 128-B lines the log stream has evicted from L2 by the next outer tick: HBM read traffic per launch
// drops from 1.3 GB to 0.1 GB at B = 65 536.  Coefficients [24][64] and yaws [16][64] of a compute wave live in LDS.
constexpr int poly_tile_doubles(bool yawscan) { return (24 + (yawscan ? 0 : 16)) * 64; }    // no yaw slots when the kernel scans the yaw

// YAWSCAN (with POLY): the yaw of a target row -- the one column that is a scan over all earlier rows -- is not read from a
// dense column either: the vehicle visits its rows in order, one per outer tick, so it carries the scan itself (has a
// heading been seen, the last one, the running sum of np.unwrap's corrections: state rows 27-29, with row 26 saying
// which row they stand before) and evaluates minimum_snap.py:126-136 for the row at hand with the sampler's own
// functions (minsnap_yaw.h; the sampler sums the corrections in the same left-to-right order).  Rows before a mission's
// first heading take P.first_yaw[b].  A cursor that does not match the carried scan (a caller moved it, another kernel
// advanced it) is caught at launch and the scan is rebuilt from row 0.  No yaw bytes are read or written at all.
// (The heading here is the device library's atan2, the sampler's is uavac_yaw::heading(): the same operations in the same order by
// construction, with the library's version inlined by the compiler.  Both written as heading() the plan-fed kernels need 257-260
// vector registers -- one wave per SIMD -- so the agreement is CHECKED instead: uavac_create() runs both over 2^16 operand pairs
// and every special value and refuses to hand out a context (UAVAC_ETOOLCHAIN) when a single bit differs.)
//
// SCORE: per-UAV tracking scores (include/uavac.h, UAVAC_SCORE_ROWS) accumulated by the compute wave on the side of the flight.
// The 11 values of a lane live in an LDS slot [11][64] of its compute wave (one lane per column: conflict-free ds_read_b64 /
// ds_write_b64), loaded from `score` when a persistent tile starts and written back when it ends -- not in vector registers
// (the plan-fed kernels sit at the 256 limit) and not read-modify-written in global memory inside the tick loop (a load waited
// on in the dependent chain stalls the wave).  The outer update parks its row and target xyz in the slot; the last tick of the
// period measures the distance to it after the free-body step.
constexpr int kScoreRows = UAVAC_SCORE_ROWS;
constexpr int tgt_rows(bool score) { return score ? 11 : 10; }    // TGW tile: the target row (+ its row index when scoring)

// One period ends: e = |position - target xyz| (upstream's tracking_errors entry, test_mujoco_trajectory_tracking.py:26-36),
// scored when its row has not been scored yet.  Written out without contraction: the same operations, in the same order, as the
// numpy statement of the rule in the tests.
__device__ __forceinline__ void score_period_end(double *sc, double px, double py, double pz) {
#pragma clang fp contract(off)
    const double pend = sc[6 * 64];
    if (pend != 0.0) {
        const double dx = px - sc[8 * 64], dy = py - sc[9 * 64], dz = pz - sc[10 * 64];
        const double e = sqrt(dx * dx + dy * dy + dz * dz);
        if (pend - 1.0 >= sc[1 * 64]) {
            const double mx = sc[4 * 64];
            sc[0] = sc[0] + 1.0;
            sc[1 * 64] = pend;
            sc[2 * 64] = sc[2 * 64] + e;
            sc[3 * 64] = sc[3 * 64] + e * e;
            sc[4 * 64] = e > mx ? e : mx;
            sc[5 * 64] = e;
        }
        sc[6 * 64] = 0.0;
    }
}

template <int CW, int SW, bool LOG_STATE, bool LOG_CMD, bool AABB, bool POLY, bool GROUND, bool YAWSCAN, int PMODE = 0>
__global__ void __launch_bounds__((LOG_STATE || LOG_CMD || AABB) ? 64 * CW + 128 : 64 * CW)       // compute [+ placeholder] + store
control_rollout_kernel(const VehK V, const double *__restrict__ traj, const int64_t *__restrict__ row_offsets,
                       double *__restrict__ state, int32_t *__restrict__ istate, int B, int K,
                       double *__restrict__ state_log, double *__restrict__ cmd_log,
                       const double *__restrict__ aabbs, int n_obs, int n_tiles, size_t log_pitch, const PlanRef P,
                       int late_handover, int n_idle) {
    constexpr bool SCORE = false;
    double *const score = nullptr;
#include "control_rollout_body.inc"
}

// The same flight with the tracking scores [UAVAC_SCORE_ROWS][B] (never with a command log: include/uavac.h).  `score` is the
// LAST argument: outer_constants() reads VehK at kernel-argument offset 0.
template <int CW, int SW, bool LOG_STATE, bool LOG_CMD, bool AABB, bool POLY, bool GROUND, bool YAWSCAN, int PMODE = 0>
__global__ void __launch_bounds__((LOG_STATE || LOG_CMD || AABB) ? 64 * CW + 128 : 64 * CW)
scored_control_rollout_kernel(const VehK V, const double *__restrict__ traj, const int64_t *__restrict__ row_offsets,
                              double *__restrict__ state, int32_t *__restrict__ istate, int B, int K,
                              double *__restrict__ state_log, double *__restrict__ cmd_log,
                              const double *__restrict__ aabbs, int n_obs, int n_tiles, size_t log_pitch, const PlanRef P,
                              int late_handover, int n_idle, double *__restrict__ score) {
    static_assert(!LOG_CMD, "no scores together with a command log");
    constexpr bool SCORE = true;
#include "control_rollout_body.inc"
}

__global__ void state_init_kernel(const VehK V, const double *__restrict__ positions, int B, int hover,
                                  double *__restrict__ state, int32_t *__restrict__ istate) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const size_t sB = (size_t)B;
    for (int r = 0; r < UAVAC_STATE_ROWS; ++r) state[r * sB + b] = 0.0;
    if (positions) {
        state[0 * sB + b] = positions[3 * (size_t)b + 0];
        state[1 * sB + b] = positions[3 * (size_t)b + 1];
        state[2 * sB + b] = positions[3 * (size_t)b + 2];
    }
    state[3 * sB + b] = 1.0;
    if (hover) {
        for (int i = 0; i < 4; ++i) { state[(13 + i) * sB + b] = V.hover_omega; state[(17 + i) * sB + b] = V.hover_omega; }
    }
    for (int r = 0; r < UAVAC_ISTATE_ROWS; ++r) istate[r * sB + b] = 0;
}

// Empty kernel with the workgroup shape of the logged rollout (two waves).  Where the dispatcher puts the waves of a
// 2-wave workgroup depends on the shape of the kernel that ran before: after the planning kernels (1-wave
// workgroups) 5-15 % of the SIMDs receive two compute waves and others two store waves, and the launch runs 25 %
// slower (tools/first_launch_bisect.py, profiles/r02_placement_census.txt; it heals by itself over the next two
// launches).  After ANY kernel of 2-wave workgroups the placement is one compute + one store wave on every SIMD.
__global__ void __launch_bounds__(256) rollout_align_kernel() {}

// One compute + one store wave per 64 UAVs, one hand-over per tick.  (Two ticks per hand-over -- the compute wave fills two
// slabs before the barrier, the store wave drains two after it; 2 x 2 slabs + the coefficient tile still fit four workgroups
// per CU once the yaw tile is gone -- is bit-identical and changes nothing: 14.46-14.49 ms per bench step against
// 14.49-14.54 (a throw-away probe on the round-2 tree).  The rendezvous is not what couples the stages.)  (Four compute + four store waves per 256 UAVs -- one workgroup per CU, whose
// 8 waves the dispatcher always deals round the 4 SIMDs evenly, so that no aligner is needed -- was measured at 1.65 ms
// per 1 000 ticks against 1.33 ms: the per-tick barrier then couples eight waves; round 3 measured two + two waves per 128 UAVs
// slower at every batch size as well, profiles/r03_rollout_shapes_wide_workgroup.jsonl.  The kernel keeps its CW / SW
// parameters; only <1, 1> is instantiated.)
template <bool LS, bool LC, bool AB, bool POLY, bool GR, bool YS, int PMODE = 0, bool SC = false>
void launch_shape(uavac_ctx *ctx, const VehK &V, const double *traj, const int64_t *row_offsets, double *state,
                  int32_t *istate, int B, int K, double *state_log, double *cmd_log, const double *aabbs, int n_obs,
                  const PlanRef &P, double *score) {
    constexpr int CW = 1, SW = 1;
    constexpr bool WATCH = AB && !LS && !LC;           // obstacles without a log: the second wave only watches
    constexpr bool LOGGING = LS || LC || WATCH;
    constexpr int NU = 64 * CW;
    constexpr int NR = (LS ? 13 : 0) + (LC ? UAVAC_CMD_COLS : 0) + (WATCH ? 3 : 0);
    const int n_tiles = (B + NU - 1) / NU;
    // a placeholder wave between compute and store wave where two workgroups share a CU (more than a quarter, at most half
    // as many tiles as the chip has SIMDs: 257 .. 512 on an MI355X) -- see the kernel, PLACEHOLDER WAVES
    int n_idle = 0;
    if (LOGGING) {
        if (ctx->idle_waves >= 0) n_idle = ctx->idle_waves > 1 ? 1 : ctx->idle_waves;
        else n_idle = (4 * n_tiles > ctx->n_simds && 2 * n_tiles <= ctx->n_simds) ? 1 : 0;
    }
    const int threads = NU + (LOGGING ? 64 * (1 + n_idle) : 0);
    const size_t lds = sizeof(double) * (2 * NR * NU + (POLY ? CW * poly_tile_doubles(YS) : 0) + (PMODE == 2 ? tgt_rows(SC) * NU : 0) +
                                         (SC ? CW * kScoreRows * NU : 0));
    const void *kern;
    if constexpr (SC) kern = (const void *)scored_control_rollout_kernel<CW, SW, LS, LC, AB, POLY, GR, YS, PMODE>;
    else kern = (const void *)control_rollout_kernel<CW, SW, LS, LC, AB, POLY, GR, YS, PMODE>;
    // With a second wave per workgroup the launch holds at most one workgroup per SIMD; a batch with more 64-UAV tiles than
    // the chip has SIMDs is walked by those workgroups pass after pass inside ONE launch (persistent tiles, see the kernel).
    // Round 2 issued one launch per 65 536 columns instead (a single launch with two workgroups per SIMD had been measured
    // at 4.04 ms per 1 000 ticks for B = 131 072 against 3.15 ms for two launches): every launch boundary made all SIMDs
    // wait for the slowest one.  Without a second wave one launch of all tiles is kept (two compute waves per SIMD hide
    // each other's latency).  Results do not depend on the split.
    const int max_wgs = ctx->n_simds / CW;                     // one compute wave per SIMD at most
    const int grid = (LOGGING && n_tiles > max_wgs) ? max_wgs : n_tiles;
    const int cols = grid * NU < B ? grid * NU : B;            // columns in flight at a time
    // Hand the slab over at the end of the tick, or a third of a tick later (after the next tick's motor model)?  Results are the
    // same bit for bit.  Round 5 (tools/half_chip_options.py, profiles/r05_launcher_sweep_m*.jsonl: every size from 12 288 to
    // 65 536 UAVs x hand-over point x PMODE, interleaved): the late hand-over wins or ties at EVERY size with the round-4
    // kernels -- 0.857 against 0.890 ms per 1 000 logged ticks at 32 768 UAVs, 0.852 / 0.883 at 24 576, 1.092 / 1.105 at 57 344 --
    // so it is the default (round 3 had found a window from 20 480 to 40 960 UAVs where the end of the tick was better; that was
    // before the target rows left the compute wave's outer tick).  Option "late_handover" still forces either.
    const int late = ctx->late_handover >= 0 ? ctx->late_handover : 1;
    (void)cols;
    // WORKGROUPS PER CU.  Below a full chip nothing but LDS limits how many of these workgroups a CU takes (registers allow four),
    // and the dispatcher does not deal them evenly: at 512 workgroups on 256 CUs some CUs get three and some one, and the launch ends
    // with its slowest CU.  The workgroup therefore asks for as much LDS as makes k + 1 of them NOT fit a CU, k = the number every CU
    // must take, for k = 2 and 3 (round 5, profiles/r05_cu_balance.jsonl: 32 768 UAVs 0.878 -> 0.849 and 0.869 -> 0.854 ms per 1 000 ticks on two
    // boxes; no effect where k workgroups per CU is what happens anyway).  Option "cu_balance" = 0 switches it off; "lds_pad" > 0
    // overrides it.  (A full chip needs nothing: four workgroups per CU is all its registers hold.)
    size_t pad = (size_t)ctx->lds_pad;
    if (LOGGING && pad == 0 && ctx->cu_balance != 0) {
        const int cus = ctx->n_simds / 4;
        const int k = (grid + cus - 1) / cus;
        // (k = 1 is left alone: measured no gain there, and a workgroup that claims half a CU's LDS could starve beside another
        // kernel on a second stream -- the root of config 4 re-samples its peers' rows while it flies)
        if (k >= 2 && k <= 3) {
            const size_t lds_cu = (size_t)160 * 1024;
            const size_t want = ((lds_cu / (size_t)(k + 1) + 1024) + 1023) & ~(size_t)1023;
            if (want * (size_t)k <= lds_cu && want > lds) pad = want - lds;
        }
    }
    const size_t pitch = (LS || LC) ? (ctx->log_pitch > 0 ? (size_t)ctx->log_pitch : (size_t)B) : (size_t)B;
    if (LOGGING && ctx->rollout_align)
        hipLaunchKernelGGL(rollout_align_kernel, dim3(grid), dim3(threads), 0, ctx->stream);
    if (lds + pad > 64 * 1024) {
        // (an "lds_pad" beyond what a workgroup may have is refused HERE, with the runtime's words, not by a launch that never runs)
        const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds + pad));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            ctx->err = std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize = ") + std::to_string(lds + pad) + "): " + hipGetErrorString(e);
            ctx->launch_rc = UAVAC_EHIP;
            return;
        }
    }
    if constexpr (SC) {
        auto kfn = scored_control_rollout_kernel<CW, SW, LS, LC, AB, POLY, GR, YS, PMODE>;
        hipLaunchKernelGGL(kfn, dim3(grid), dim3(threads), lds + pad, ctx->stream, V, traj, row_offsets, state, istate,
                           B, K, state_log, cmd_log, aabbs, n_obs, n_tiles, pitch, P, late, n_idle, score);
    } else {
        auto kfn = control_rollout_kernel<CW, SW, LS, LC, AB, POLY, GR, YS, PMODE>;
        hipLaunchKernelGGL(kfn, dim3(grid), dim3(threads), lds + pad, ctx->stream, V, traj, row_offsets, state, istate,
                           B, K, state_log, cmd_log, aabbs, n_obs, n_tiles, pitch, P, late, n_idle);
    }
    auto tf = [](bool v) { return v ? "true" : "false"; };
    char name[184];
    snprintf(name, sizeof name, "%scontrol_rollout_kernel<%d, %d, %s, %s, %s, %s, %s, %s, %d>", SC ? "scored_" : "", CW, SW, tf(LS), tf(LC),
             tf(AB), tf(POLY), tf(GR), tf(YS), PMODE);     // the name rocprofv3 prints, argument for argument
    ctx->last_rollout = name;
    const int64_t shape[6] = {grid, threads, (int64_t)(lds + pad), (int64_t)pitch, n_tiles, grid > 0 ? (n_tiles + grid - 1) / grid : 0};
    for (int i = 0; i < 6; ++i) ctx->last_rollout_launch[i] = shape[i];
    // vector registers of that kernel as the loaded code object has them (once per variant): above 256 a SIMD holds ONE
    // wave of it and the launch runs at 0.65x -- a toolchain that crosses the line shows up here and in bench.py's line
    // (one value per kernel variant, the same from every ctx: an atomic, since distinct ctxs may launch from distinct threads)
    static std::atomic<int> vgprs{-1};
    int v = vgprs.load(std::memory_order_relaxed);
    if (v < 0) {
        hipFuncAttributes fa;
        v = hipFuncGetAttributes(&fa, kern) == hipSuccess ? fa.numRegs : 0;
        vgprs.store(v, std::memory_order_relaxed);
    }
    ctx->last_rollout_vgprs = v;
}

template <bool LS, bool LC, bool AB, bool SC = false>
void launch_variant(uavac_ctx *ctx, const VehK &V, const double *traj, const int64_t *row_offsets, double *state,
                    int32_t *istate, int B, int K, double *state_log, double *cmd_log, const double *aabbs, int n_obs,
                    const PlanRef *plan, double *score) {
#define UAVAC_SHAPE_ARGS ctx, V, traj, row_offsets, state, istate, B, K, state_log, cmd_log, aabbs, n_obs
    // Plan-fed kernels, PMODE (see the kernel): who evaluates the target rows, how coefficients reach the LDS tile.  Per 1 000
    // logged ticks, same process and buffers (tools/rollout_ab.py, m = 12), mode 2 / 1 / 0 (= round 3):
    //     16 384 UAVs 0.792 / 0.834 / 0.852 ms     32 768  0.879 / 0.891 / 0.984     49 152  1.011 / 0.997 / 1.055-1.078
    //     65 536      1.297 / 1.27 / 1.25-1.26
    // * up to two workgroups per CU every working wave has a SIMD of its own and the second wave's idle time is free: it
    //   evaluates the rows (2; needs a second wave, and F >= 7 inner ticks per outer tick: the row is evaluated in four pieces,
    //   one to four ticks after the cursor moved);
    // * with three or four workgroups per CU a second wave shares its SIMD with a compute wave: the compute wave evaluates, its
    //   coefficients arrive by LDS-DMA (1) -- also the form of the kernels without a second wave while the chip is not full;
    // * a full chip is bound by its log stream and the twelve DMA instructions per segment change are only in the way: through
    //   registers, on the spot (0).
    // Same bits in every mode.  (Template parameters, not branches: with two forms in one kernel the plan-fed variants need
    // 257-260 vector registers.)  Option "coeff_dma": -1 = as above, 0 / 1 / 2 = that mode where the kernel has it.
    constexpr bool LOGGING = LS || LC || AB;
    const int tiles = (B + 63) / 64, in_flight = (LOGGING && tiles > ctx->n_simds) ? ctx->n_simds : tiles;
    int mode = 0;
    if (plan) {
        if (ctx->coeff_dma >= 0) mode = ctx->coeff_dma > 2 ? 2 : ctx->coeff_dma;
        // (round 5, same sweep: the second wave's rows pay up to 26 624 UAVs -- 0.840 against 0.852 ms at 24 576 -- and lose from
        // 28 672 on -- 0.866 against 0.857 at 32 768: the crossover lies below "two workgroups on every CU")
        else mode = in_flight * 64 >= 60 * ctx->n_simds ? 0 : (in_flight * 64 <= 26 * ctx->n_simds ? 2 : 1);
        if (mode == 2 && (!LOGGING || V.F < 7)) mode = 1;
    }
    // (the scored kernel without a second wave that reads the dense yaw column has no PMODE 0 form: it needs 258 vector registers
    // there, one wave per SIMD; it flies PMODE 1, same bits)
    constexpr bool NO_P0_DENSE = SC && !LOGGING;
#define UAVAC_LAUNCH_MODE(GR_, YS_)                                                                     \
    do {                                                                                                \
        if (mode == 1) launch_shape<LS, LC, AB, true, GR_, YS_, 1, SC>(UAVAC_SHAPE_ARGS, *plan, score);            \
        else if (mode == 2) {                                                                                      \
            if constexpr (LOGGING) launch_shape<LS, LC, AB, true, GR_, YS_, 2, SC>(UAVAC_SHAPE_ARGS, *plan, score); \
        } else if constexpr (NO_P0_DENSE && !YS_) launch_shape<LS, LC, AB, true, GR_, YS_, 1, SC>(UAVAC_SHAPE_ARGS, *plan, score);  \
        else launch_shape<LS, LC, AB, true, GR_, YS_, 0, SC>(UAVAC_SHAPE_ARGS, *plan, score);                      \
    } while (0)
    if (plan && !plan->yaw) {                       // the rollout scans the yaw itself
        if (V.ground) UAVAC_LAUNCH_MODE(true, true); else UAVAC_LAUNCH_MODE(false, true);
    } else if (plan) {
        if (V.ground) UAVAC_LAUNCH_MODE(true, false); else UAVAC_LAUNCH_MODE(false, false);
#undef UAVAC_LAUNCH_MODE
    } else {
        if (V.ground) launch_shape<LS, LC, AB, false, true, false, 0, SC>(UAVAC_SHAPE_ARGS, PlanRef{}, score);
        else launch_shape<LS, LC, AB, false, false, false, 0, SC>(UAVAC_SHAPE_ARGS, PlanRef{}, score);
    }
#undef UAVAC_SHAPE_ARGS
}

void launch_flags(uavac_ctx *ctx, const VehK &V, const double *traj, const int64_t *row_offsets, double *state,
                  int32_t *istate, int B, int K, double *state_log, double *cmd_log, const double *aabbs, int n_obs,
                  const PlanRef *plan, double *score) {
    const bool ls = state_log != nullptr, lc = cmd_log != nullptr, ab = (aabbs != nullptr && n_obs > 0);
#define UAVAC_ARGS ctx, V, traj, row_offsets, state, istate, B, K, state_log, cmd_log, aabbs, n_obs, plan, score
    if (!score) {
        if (ls) {
            if (lc) { if (ab) launch_variant<true, true, true>(UAVAC_ARGS); else launch_variant<true, true, false>(UAVAC_ARGS); }
            else    { if (ab) launch_variant<true, false, true>(UAVAC_ARGS); else launch_variant<true, false, false>(UAVAC_ARGS); }
        } else {
            if (lc) { if (ab) launch_variant<false, true, true>(UAVAC_ARGS); else launch_variant<false, true, false>(UAVAC_ARGS); }
            else    { if (ab) launch_variant<false, false, true>(UAVAC_ARGS); else launch_variant<false, false, false>(UAVAC_ARGS); }
        }
    } else {                                       // scored twins: never with a command log (the entry points refuse one)
        if (ls) { if (ab) launch_variant<true, false, true, true>(UAVAC_ARGS); else launch_variant<true, false, false, true>(UAVAC_ARGS); }
        else    { if (ab) launch_variant<false, false, true, true>(UAVAC_ARGS); else launch_variant<false, false, false, true>(UAVAC_ARGS); }
    }
#undef UAVAC_ARGS
}

}  // namespace

int uavac_launch_state_init(uavac_ctx *ctx, const VehK &V, const double *positions, int B, int hover, double *state,
                            int32_t *istate) {
    hipLaunchKernelGGL(state_init_kernel, dim3((B + 255) / 256), dim3(256), 0, ctx->stream, V, positions, B, hover,
                       state, istate);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}

int uavac_launch_rollout(uavac_ctx *ctx, const VehK &V, const double *traj, const int64_t *row_offsets, double *state,
                         int32_t *istate, int B, int K, double *state_log, double *cmd_log, const double *aabbs,
                         int n_obs, const PlanRef *plan, double *score) {
    // One compute wave + one store wave per workgroup.  (Four compute waves sharing one store wave were
    // measured 15 % slower at B = 65 536: a single wave cannot issue a CU's 52 stores per tick fast enough.
    // Two compute waves with the store wave moving 16 B per lane -- 13 x 1 KB wave stores per tick instead of
    // 26 x 512 B -- were 17 % slower too, 1.47 vs 1.25 ms on the same box: the per-tick barrier then couples
    // two compute waves.  Replacing the per-tick barrier by a ring of 4 slabs with produced / consumed counters in
    // LDS, so that the compute wave may run 4 ticks ahead of a stalled store wave, was slower as well: 1.35 vs
    // 1.26 ms -- the hand-over is not what limits the kernel.)  The log rows want B to be a multiple of 16 (128-B lines): B = 65 534 runs at half
    // the rate of B = 65 536 because every 512-B wave store then straddles two partially written lines.
    ctx->launch_rc = UAVAC_OK;
    launch_flags(ctx, V, traj, row_offsets, state, istate, B, K, state_log, cmd_log, aabbs, n_obs, plan, score);
    if (ctx->launch_rc != UAVAC_OK) return ctx->launch_rc;       // (the text is in ctx->err)
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}
