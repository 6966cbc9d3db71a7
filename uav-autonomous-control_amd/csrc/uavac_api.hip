// C ABI of libuavac.so: context management, argument validation, device-pointer entry points and
// their host-pointer twins (which stage through device scratch).  See include/uavac.h.

#include "uavac_internal.h"
#include "uavac_scratch.h"

#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

namespace {

constexpr size_t kStageChunk = (size_t)256 << 10;     // bytes per half of the pinned ping-pong buffer
// Transfers up to this size go through the ctx's own pinned buffer (no pinning work inside the runtime, no allocation), up
// to four pieces with the DMA of one overlapping the CPU copy of its neighbour; larger ones are handed to hipMemcpyAsync as
// they are: the runtime's pageable path moves them at 50 GB/s aggregate (H2D + D2H of a 4 096-UAV rollout,
// tools/host_path_rate.py), a single-threaded copy through a staging buffer at 27.
constexpr size_t kStageLimit = (size_t)1 << 20;
static_assert(kStageLimit >= 2 * kStageChunk, "the ping-pong needs transfers of more than one piece to overlap anything");
}  // namespace

// Host <-> device copies of the host-pointer twins.  The caller's buffers are pageable; they travel through the ctx's
// pinned staging buffer in kStageChunk pieces, two halves in flight: the DMA of one piece overlaps the CPU copy of the
// next (h2d) or previous (d2h) one.  Ordered on the ctx stream like everything else.
int uavac_h2d(uavac_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes) {
    if (!bytes) return UAVAC_OK;
    if (bytes > kStageLimit) {
        UAVAC_HIP(ctx, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
        return UAVAC_OK;                  // pageable source: the runtime has read it when the call returns
    }
    if (int rc = uavac_pin_reserve(ctx, 2 * kStageChunk)) return rc;
    const char *src = static_cast<const char *>(src_host);
    char *dst = static_cast<char *>(dst_dev);
    size_t i = 0;
    for (size_t off = 0; off < bytes; off += kStageChunk, ++i) {
        const size_t n = (bytes - off < kStageChunk) ? bytes - off : kStageChunk;
        char *half = ctx->h_pin + (i & 1) * kStageChunk;
        if (i >= 2) UAVAC_HIP(ctx, hipEventSynchronize(ctx->pin_ev[i & 1]));     // the DMA that last read this half
        std::memcpy(half, src + off, n);
        UAVAC_HIP(ctx, hipMemcpyAsync(dst + off, half, n, hipMemcpyHostToDevice, ctx->stream));
        UAVAC_HIP(ctx, hipEventRecord(ctx->pin_ev[i & 1], ctx->stream));
    }
    // the halves must not be rewritten by a later call before these DMAs have read them
    UAVAC_HIP(ctx, hipEventSynchronize(ctx->pin_ev[0]));
    if (i > 1) UAVAC_HIP(ctx, hipEventSynchronize(ctx->pin_ev[1]));
    return UAVAC_OK;
}

int uavac_d2h(uavac_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes) {
    if (!bytes) return UAVAC_OK;
    if (bytes > kStageLimit) {
        UAVAC_HIP(ctx, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
        UAVAC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return UAVAC_OK;
    }
    if (int rc = uavac_pin_reserve(ctx, 2 * kStageChunk)) return rc;
    char *dst = static_cast<char *>(dst_host);
    const char *src = static_cast<const char *>(src_dev);
    const size_t n_chunks = (bytes + kStageChunk - 1) / kStageChunk;
    auto len = [&](size_t i) { return (i + 1 < n_chunks) ? kStageChunk : bytes - i * kStageChunk; };
    auto issue = [&](size_t i) -> int {
        UAVAC_HIP(ctx, hipMemcpyAsync(ctx->h_pin + (i & 1) * kStageChunk, src + i * kStageChunk, len(i),
                                      hipMemcpyDeviceToHost, ctx->stream));
        UAVAC_HIP(ctx, hipEventRecord(ctx->pin_ev[i & 1], ctx->stream));
        return UAVAC_OK;
    };
    if (int rc = issue(0)) return rc;
    for (size_t i = 0; i < n_chunks; ++i) {
        if (i + 1 < n_chunks)
            if (int rc = issue(i + 1)) return rc;                        // its half was drained one iteration ago
        UAVAC_HIP(ctx, hipEventSynchronize(ctx->pin_ev[i & 1]));
        std::memcpy(dst + i * kStageChunk, ctx->h_pin + (i & 1) * kStageChunk, len(i));
    }
    return UAVAC_OK;
}

namespace {

bool finite_all(const double *p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

int check_plan_args(uavac_ctx *ctx, const void *wp, int B, int m) {
    if (!ctx) return UAVAC_EINVAL;
    if (!wp) return uavac_fail(ctx, UAVAC_EINVAL, "null waypoint pointer");
    if (B < 1) return uavac_fail(ctx, UAVAC_EINVAL, "B must be >= 1");
    if (m < 1 || m > UAVAC_MAX_SEGMENTS) return uavac_fail(ctx, UAVAC_EINVAL, "m must be in [1, UAVAC_MAX_SEGMENTS]");
    return UAVAC_OK;
}

// The refusals that several entry points word alike, one spelling each.  dt: in one refusal ...
int check_dt_positive(uavac_ctx *ctx, double dt) {
    if (!std::isfinite(dt) || !(dt > 0.0)) return uavac_fail(ctx, UAVAC_EINVAL, "dt must be finite and > 0");
    return UAVAC_OK;
}
// ... in two, where a non-finite value has its own code ...
int check_dt(uavac_ctx *ctx, double dt) {
    if (!std::isfinite(dt)) return uavac_fail(ctx, UAVAC_ENONFINITE, "non-finite dt");
    if (!(dt > 0.0)) return uavac_fail(ctx, UAVAC_EINVAL, "dt must be > 0");
    return UAVAC_OK;
}
// ... and together with the batch's one cruise speed
int check_velocity_dt(uavac_ctx *ctx, double velocity, double dt) {
    if (!std::isfinite(velocity) || !std::isfinite(dt)) return uavac_fail(ctx, UAVAC_ENONFINITE, "non-finite velocity or dt");
    if (!(velocity > 0.0) || !(dt > 0.0)) return uavac_fail(ctx, UAVAC_EINVAL, "velocity and dt must be > 0");
    return UAVAC_OK;
}
int check_n_cuboids(uavac_ctx *ctx, int n_cuboids) {
    if (n_cuboids < 0 || n_cuboids > UAVAC_AUDIT_MAX_CUBOIDS)
        return uavac_fail(ctx, UAVAC_EINVAL, "n_cuboids must be in [0, UAVAC_AUDIT_MAX_CUBOIDS]");
    return UAVAC_OK;
}
// the shapes of the take calls (n missions out of B) and of the delay calls (`delayed`, with n = 1: a delayed mission grows by a segment)
int check_take_shape(uavac_ctx *ctx, int B, int n, int m, bool delayed = false) {
    if (B < 1) return uavac_fail(ctx, UAVAC_EINVAL, "B must be >= 1");
    if (n < 1) return uavac_fail(ctx, UAVAC_EINVAL, "n must be >= 1");
    if (delayed && (m < 1 || m > UAVAC_MAX_SEGMENTS - 1))
        return uavac_fail(ctx, UAVAC_EINVAL, "m must be in [1, UAVAC_MAX_SEGMENTS - 1]: a delayed mission needs one more segment");
    if (m < 1 || m > UAVAC_MAX_SEGMENTS) return uavac_fail(ctx, UAVAC_EINVAL, "m must be in [1, UAVAC_MAX_SEGMENTS]");
    return UAVAC_OK;
}

// The device-side flags are sticky until read: the host twins clear them on entry (so that what an earlier _dev call
// left behind is not reported against valid input) and read-and-clear them on exit.
int clear_flags(uavac_ctx *ctx) {
    UAVAC_HIP(ctx, hipMemsetAsync(ctx->d_flags, 0, 4 * sizeof(int32_t), ctx->stream));
    return UAVAC_OK;
}
int read_flags(uavac_ctx *ctx, int32_t out[4]) {
    UAVAC_HIP(ctx, hipMemcpyAsync(out, ctx->d_flags, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    UAVAC_HIP(ctx, hipMemsetAsync(ctx->d_flags, 0, 4 * sizeof(int32_t), ctx->stream));
    UAVAC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return UAVAC_OK;
}

}  // namespace

int uavac_arena_reserve(uavac_ctx *ctx, size_t bytes) {
    if (bytes <= ctx->arena_cap) return UAVAC_OK;
    size_t want = bytes + bytes / 4;                                 // headroom, so that a slowly growing need does not reallocate every call
    if (want < ((size_t)1 << 20)) want = (size_t)1 << 20;
    if (uavac_grow(ctx, ctx->d_arena, ctx->arena_cap, want, want) == UAVAC_OK) return UAVAC_OK;
    (void)hipGetLastError();
    return uavac_grow(ctx, ctx->d_arena, ctx->arena_cap, bytes, bytes);      // no room for the headroom: the exact size
}

int uavac_pin_reserve(uavac_ctx *ctx, size_t bytes) {
    if (!ctx->pin_ev[0]) {
        UAVAC_HIP(ctx, hipEventCreateWithFlags(&ctx->pin_ev[0], hipEventDisableTiming));
        UAVAC_HIP(ctx, hipEventCreateWithFlags(&ctx->pin_ev[1], hipEventDisableTiming));
    }
    return uavac_grow(ctx, ctx->h_pin, ctx->pin_cap, bytes, bytes, true);
}

VehK uavac_make_vehk(const uavac_vehicle &V) {
    VehK k{};
    k.g = V.g; k.dt = V.dt; k.dt_outer = V.dt_outer; k.mass = V.mass; k.inv_mass = 1.0 / V.mass;
    for (int i = 0; i < 3; ++i) { k.I[i] = V.inertia[i]; k.inv_I[i] = 1.0 / V.inertia[i]; }
    k.arm = V.arm; k.inv_arm = 1.0 / V.arm; k.kappa = V.kappa; k.inv_kappa = 1.0 / V.kappa;
    k.kf = V.kf; k.inv_kf = 1.0 / V.kf;
    k.min_thrust = V.min_thrust; k.max_thrust = V.max_thrust;
    k.c_min = 4.0 * V.min_thrust; k.c_max = 4.0 * V.max_thrust;
    k.resp_rise = 1.0 - std::exp(-V.dt / V.tau_rise);
    k.resp_fall = 1.0 - std::exp(-V.dt / V.tau_fall);
    k.max_ascent = V.max_ascent; k.max_descent = V.max_descent; k.max_speed_xy = V.max_speed_xy;
    k.max_horiz_accel = V.max_horiz_accel; k.max_tilt = V.max_tilt;
    k.kp_xy = V.kp_xy; k.kd_xy = V.kd_xy; k.kp_z = V.kp_z; k.kd_z = V.kd_z; k.ki_z = V.ki_z;
    k.kp_roll = V.kp_roll; k.kp_pitch = V.kp_pitch; k.kp_yaw = V.kp_yaw;
    k.ikp[0] = V.inertia[0] * V.kp_p; k.ikp[1] = V.inertia[1] * V.kp_q; k.ikp[2] = V.inertia[2] * V.kp_r;
    k.hover_omega = std::sqrt(V.mass * V.g / (4.0 * V.kf));
    k.lit_tiny = 2.2250738585072014e-308; k.lit_h2_small = 1.0e-3;
    k.lit_c8 = 1.0 / 40320; k.lit_c6 = -1.0 / 720; k.lit_c4 = 1.0 / 24;
    k.lit_s9 = 1.0 / 362880; k.lit_s7 = -1.0 / 5040; k.lit_s5 = 1.0 / 120; k.lit_s3 = -1.0 / 6;
    k.lit_375 = 0.375; k.lit_e_small = 1.0e-6;
    k.F = V.inner_per_outer;
    k.ground = V.ground ? 1 : 0;
    k.ground_z = V.ground_z;
    k.ground_zc = V.ground_z - V.ground_clearance;
    k.ground_k = k.ground ? 1.0 / (V.ground_timeconst * V.ground_timeconst) : 0.0;
    k.ground_b = k.ground ? 2.0 / V.ground_timeconst : 0.0;
    return k;
}

int uavac_check_vehicle(uavac_ctx *ctx, const uavac_vehicle *V) {
    if (!V) return uavac_fail(ctx, UAVAC_EINVAL, "null vehicle");
    const double pos[] = {V->g, V->dt, V->dt_outer, V->mass, V->inertia[0], V->inertia[1], V->inertia[2], V->arm,
                          V->kf, V->kappa, V->max_thrust, V->tau_rise, V->tau_fall};
    for (double v : pos)
        if (!(v > 0.0) || !std::isfinite(v)) return uavac_fail(ctx, UAVAC_EINVAL, "vehicle constant must be finite and > 0");
    if (!(V->min_thrust >= 0.0) || !(V->max_thrust > V->min_thrust))
        return uavac_fail(ctx, UAVAC_EINVAL, "thrust limits must satisfy 0 <= min < max");
    if (V->inner_per_outer < 1) return uavac_fail(ctx, UAVAC_EINVAL, "inner_per_outer must be >= 1");
    if (V->ground) {
        if (!std::isfinite(V->ground_z) || !(V->ground_clearance >= 0.0) || !std::isfinite(V->ground_clearance) ||
            !(V->ground_timeconst > 0.0) || !std::isfinite(V->ground_timeconst))
            return uavac_fail(ctx, UAVAC_EINVAL, "ground plane needs finite z, clearance >= 0 and time constant > 0");
        if (!(V->ground_timeconst >= 2.0 * V->dt))      // the explicit step of the contact law is stable for dt <= tc / 2
            return uavac_fail(ctx, UAVAC_EINVAL, "ground_timeconst must be at least 2 dt");
    }
    return UAVAC_OK;
}

namespace {

// times + row counts + offsets at one cruise speed for the batch, or at one per mission (velocities [B], device)
int launch_counts(uavac_ctx *ctx, const double *wp, int B, int m, double velocity, double dt, double *times, int32_t *seg_rows,
                         int64_t *row_offsets, const int64_t *seg_offsets = nullptr) {
    return uavac_launch_row_counts(ctx, wp, B, m, velocity, dt, times, seg_rows, row_offsets, seg_offsets);
}
int launch_counts(uavac_ctx *ctx, const double *wp, int B, int m, const double *velocities, double dt, double *times,
                         int32_t *seg_rows, int64_t *row_offsets, const int64_t *seg_offsets = nullptr) {
    return uavac_launch_row_counts_v(ctx, wp, B, m, velocities, dt, times, seg_rows, row_offsets, seg_offsets);
}

// ctx->d_plan: where a chain with a row capacity keeps what it computes before it is committed -- the durations [B m] (`with_times`;
// otherwise they are the caller's input), the row counts [B m] and the row offsets [B + 1], each at a 256-byte boundary
struct PlanScratch {
    double *times;
    int32_t *seg_rows;
    int64_t *row_offsets;
};
int plan_scratch(uavac_ctx *ctx, int B, int m, bool with_times, PlanScratch &p) {
    auto padded = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    const size_t nseg = (size_t)B * m, o_rows = with_times ? padded(nseg * 8) : 0, o_offs = o_rows + padded(nseg * 4);
    const size_t need = o_offs + padded(((size_t)B + 1) * 8);
    if (int rc = uavac_grow(ctx, ctx->d_plan, ctx->plan_cap, need, need)) return rc;
    p = PlanScratch{reinterpret_cast<double *>(ctx->d_plan), reinterpret_cast<int32_t *>(ctx->d_plan + o_rows),
                    reinterpret_cast<int64_t *>(ctx->d_plan + o_offs)};
    return UAVAC_OK;
}

// The planning chain behind uavac_minsnap_plan_dev (Vel = double), uavac_minsnap_plan_v_dev (Vel = const double *) and
// uavac_minsnap_plan_bc_dev (the latter with bc != NULL: the solve with boundary derivatives in the solve's place); the
// arguments have been validated.
template <class Vel>
int plan_chain(uavac_ctx *ctx, const double *wp, int B, int m, Vel velocity, double dt, double *times, int32_t *seg_rows,
                      int64_t *row_offsets, double *coeffs, int32_t *status, double *traj, int64_t traj_capacity_rows, double *yaw,
                      double *first_yaw, const double *bc = nullptr) {
    auto solve = [&](const double *tm, const int64_t *guard_rows, int64_t guard_capacity) {
        return bc ? uavac_launch_solve_bc(ctx, wp, tm, B, m, bc, coeffs, status, nullptr, guard_rows, guard_capacity)
                  : uavac_launch_coeff_solve(ctx, wp, tm, B, m, coeffs, status, nullptr, guard_rows, guard_capacity);
    };
    if (!traj) {
        // Rows-free chain: no row buffer, hence nothing to refuse -- times, row counts and offsets go straight into the caller's
        // arrays; the one value of the sampler a plan-fed rollout needs comes from the first-heading kernel.
        if (yaw) return uavac_fail(ctx, UAVAC_EINVAL, "a dense yaw column needs the rows: traj is NULL");
        if (int rc = launch_counts(ctx, wp, B, m, velocity, dt, times, seg_rows, row_offsets)) return rc;
        if (int rc = solve(times, nullptr, 0)) return rc;
        return first_yaw ? uavac_launch_first_yaw(ctx, coeffs, seg_rows, nullptr, B, m, dt, first_yaw) : UAVAC_OK;
    }
    if (traj_capacity_rows < 0) return uavac_fail(ctx, UAVAC_EINVAL, "negative capacity");
    // The whole chain enqueued from here: nothing returns to the caller (or to an interpreter) between the launches.
    // Times, row counts and offsets go to ctx scratch first; whether the plan fits the caller's row buffer is only known on
    // the device (row_offsets_s[B]), so every later stage reads that one word: the commit kernel copies the three arrays
    // into the caller's only when it fits, the solver and the sampler do nothing when it does not (the sampler raises
    // flag 2).  A refused plan leaves times, seg_rows, row_offsets, coeffs, rows and first_yaw exactly as they were.
    PlanScratch s;
    if (int rc = plan_scratch(ctx, B, m, true, s)) return rc;
    if (int rc = launch_counts(ctx, wp, B, m, velocity, dt, s.times, s.seg_rows, s.row_offsets)) return rc;
    if (int rc = uavac_launch_plan_commit(ctx, s.times, s.seg_rows, s.row_offsets, B, m, traj_capacity_rows, times, seg_rows,
                                          row_offsets)) return rc;
    // (Round 6 tried to hide this solve behind the sampler: the batch cut into 2 / 4 / 8 mission blocks, block i sampled on an
    // auxiliary stream while block i + 1 was being solved.  Bit-identical and SLOWER -- +1.3 % / +13 % / +23 % at 65 536 x 12 --
    // because a solve wave cannot get onto a SIMD the sampler's grid keeps full: commit 53921dc, profiles/r06_plan_blocks_ab*.jsonl.)
    if (int rc = solve(s.times, s.row_offsets + B, traj_capacity_rows)) return rc;
    SampleExtras x;
    x.yaw_dense = yaw;
    x.first_yaw = first_yaw;
    x.capacity_rows = traj_capacity_rows;         // the sampler refuses (flag 2) instead of overrunning the buffer
    return uavac_launch_sample(ctx, coeffs, s.seg_rows, s.row_offsets, B, m, dt, traj, x);
}

// The options of uavac_set_option: where each is kept, which values it takes and what a refusal says.
//   kOneOf   one of the values a[] (zero ends the list: no set here holds it)      kClamp   every value is taken, clamped into a[0] .. a[1]
//   kRange   a[0] <= value <= a[1]                                                kBool    every value is taken: 0 or not
//   kPad8    kRange, rounded down to a multiple of 8                                   kAutoOr  0 (automatic), or kOneOf
enum class Rule { kOneOf, kRange, kClamp, kBool, kPad8, kAutoOr };
struct Option {
    const char *name;
    int uavac_ctx::*field;
    Rule rule;
    int a[5];
    const char *message;
};
constexpr int kIntMax = 0x7fffffff;
const Option kOptions[] = {
    {"yaw_group", &uavac_ctx::yaw_group, Rule::kOneOf, {1, 4, 8, 16}, "yaw_group is 1, 4, 8 or 16"},
    {"audit_lanes", &uavac_ctx::audit_lanes, Rule::kOneOf, {16, 64}, "audit_lanes is 16 or 64"},
    {"separation_split", &uavac_ctx::separation_split, Rule::kRange, {0, UAVAC_SEP_MAX_SPLIT},
     "separation_split is 0 (automatic) or 1 .. UAVAC_SEP_MAX_SPLIT"},
    {"search_block", &uavac_ctx::search_block, Rule::kAutoOr, {64, 128, 256}, "search_block is 0 (default), 64, 128 or 256"},
    {"conflict_slots", &uavac_ctx::conflict_slots, Rule::kRange, {0, 64}, "conflict_slots is 0 (automatic) or 1 .. 64"},
    {"flown_audit_split", &uavac_ctx::flown_audit_split, Rule::kRange, {0, UAVAC_FLOWN_AUDIT_MAX_SPLIT},
     "flown_audit_split is 0 (automatic) or 1 .. UAVAC_FLOWN_AUDIT_MAX_SPLIT"},
    {"timeopt_chunk", &uavac_ctx::timeopt_chunk, Rule::kRange, {0, kIntMax}, "timeopt_chunk is 0 (automatic) or a number of missions"},
    {"sampler_waves", &uavac_ctx::sampler_waves, Rule::kOneOf, {1, 2, 4, 8, 16}, "sampler_waves is 1, 2, 4, 8 or 16"},
    {"sampler_group", &uavac_ctx::sampler_group, Rule::kRange, {1, 64}, "sampler_group is 1 .. 64"},
    {"rollout_align", &uavac_ctx::rollout_align, Rule::kBool, {}, nullptr},
    {"log_pitch", &uavac_ctx::log_pitch, Rule::kRange, {0, kIntMax}, "log_pitch is 0 (= B) or a number of doubles >= B"},
    {"late_handover", &uavac_ctx::late_handover, Rule::kClamp, {-1, 1}, nullptr},
    {"solve_order", &uavac_ctx::solve_order, Rule::kRange, {-1, 1}, "solve_order is 0 (one-ended), 1 (two-ended) or -1 (by the launch)"},
    {"solve_park", &uavac_ctx::solve_park, Rule::kClamp, {-1, 1}, nullptr},
    {"solve_keep", &uavac_ctx::solve_keep, Rule::kClamp, {-1, 1}, nullptr},
    {"solve_lanes", &uavac_ctx::solve_lanes, Rule::kOneOf, {-1, 64, 32, 16}, "solve_lanes is -1, 64, 32 or 16"},
    {"coeff_dma", &uavac_ctx::coeff_dma, Rule::kClamp, {-1, 2}, nullptr},
    {"idle_waves", &uavac_ctx::idle_waves, Rule::kClamp, {-1, 1}, nullptr},
    {"cu_balance", &uavac_ctx::cu_balance, Rule::kBool, {}, nullptr},
    {"lds_pad", &uavac_ctx::lds_pad, Rule::kPad8, {0, 120 * 1024}, "lds_pad is 0 .. 122880 bytes"},
};

const Option *find_option(const char *name) {
    for (const Option &o : kOptions)
        if (!std::strcmp(o.name, name)) return &o;
    return nullptr;
}

// -> false: the option does not take this value (nothing stored)
bool apply_option(uavac_ctx *ctx, const Option &o, int value) {
    bool listed = false;
    for (int v : o.a) listed |= v != 0 && v == value;
    const bool ranged = o.rule == Rule::kRange || o.rule == Rule::kPad8;
    if ((o.rule == Rule::kOneOf && !listed) || (o.rule == Rule::kAutoOr && value != 0 && !listed) || (ranged && (value < o.a[0] || value > o.a[1]))) return false;
    if (o.rule == Rule::kPad8) value &= ~7;
    if (o.rule == Rule::kClamp) value = value < o.a[0] ? o.a[0] : (value > o.a[1] ? o.a[1] : value);
    if (o.rule == Rule::kBool) value = value ? 1 : 0;
    ctx->*o.field = value;
    return true;
}

// an option's start value from the environment; a value the option does not take is ignored
void option_from_env(uavac_ctx *ctx, const char *variable, const char *name) {
    if (const char *e = getenv(variable)) (void)apply_option(ctx, *find_option(name), atoi(e));
}

struct ctx_deleter {
    void operator()(uavac_ctx *ctx) const { uavac_destroy(ctx); }      // (copes with a ctx that was built in part)
};

}  // namespace

extern "C" {

int uavac_version(void) { return UAVAC_VERSION; }

int uavac_create(uavac_ctx **out, int device_id) {
    if (!out) return UAVAC_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return UAVAC_EHIP;   // no CPU fallback, ever
    // whatever has been built when a step below fails is taken down by uavac_destroy
    std::unique_ptr<uavac_ctx, ctx_deleter> owner(new (std::nothrow) uavac_ctx());
    uavac_ctx *ctx = owner.get();
    if (!ctx) return UAVAC_ENOMEM;
    if (device_id >= 0) {
        if (device_id >= ndev) return UAVAC_EHIP;
        ctx->device = device_id;
    } else if (hipGetDevice(&ctx->device) != hipSuccess) return UAVAC_EHIP;
    uavac_device_guard guard(ctx);                // stream and buffers are created on the ctx's device
    {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess || cur != ctx->device) return UAVAC_EHIP;
    }
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) return UAVAC_EHIP;
    ctx->stream = ctx->own_stream;
    if (hipMalloc(&ctx->d_flags, 4 * sizeof(int32_t)) != hipSuccess ||
        hipMemset(ctx->d_flags, 0, 4 * sizeof(int32_t)) != hipSuccess)
        return UAVAC_EHIP;
    option_from_env(ctx, "UAVAC_YAW_GROUP", "yaw_group");
    if (const char *e = getenv("UAVAC_ROLLOUT_ALIGN")) ctx->rollout_align = (e[0] == '0') ? 0 : 1;      // (not the option's rule: "x" is on)
    option_from_env(ctx, "UAVAC_SAMPLER_WAVES", "sampler_waves");
    option_from_env(ctx, "UAVAC_SAMPLER_GROUP", "sampler_group");
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) == hipSuccess && cus > 0)
            ctx->n_simds = 4 * cus;
    }
    // The rollout's yaw scan (device library atan2) and the sampler's (uavac_yaw::heading) must agree bit for bit, or plan-fed and
    // row-fed flights part at np.unwrap's forks.  Both are compiled INTO this library (the device library is linked as bitcode at
    // build time), so the answer is a property of the build: checked on the device by the first context of the process (~0.1 ms)
    // and remembered -- later contexts skip it (round-5 advice).  A failure is not remembered: every uavac_create refuses.
    static std::atomic<int> heading_checked{0};
    if (!getenv("UAVAC_SKIP_SELFCHECK") && heading_checked.load(std::memory_order_acquire) == 0) {
        int bad = -1;
        const int rc = uavac_heading_selfcheck(ctx, &bad);
        if (rc == UAVAC_OK && bad == 0) heading_checked.store(1, std::memory_order_release);
        if (rc != UAVAC_OK || bad != 0) {
            if (rc == UAVAC_OK)
                fprintf(stderr, "libuavac: self-check failed: heading() and the atan2 of the device library this build linked differ on %d of "
                                "65680 operand pairs (built with: %s).  The device library's atan2 has changed: heading() in "
                                "csrc/minsnap_yaw.h (polynomial, operation order) must be re-derived from it -- rebuilding alone "
                                "reproduces this failure\n", bad, uavac_build_info());
            return rc != UAVAC_OK ? rc : UAVAC_ETOOLCHAIN;
        }
    }
    *out = owner.release();
    return UAVAC_OK;
}

void uavac_destroy(uavac_ctx *ctx) {
    if (!ctx) return;
    uavac_device_guard guard(ctx);
    if (ctx->own_stream) (void)hipStreamSynchronize(ctx->own_stream);
    if (ctx->d_flags) (void)hipFree(ctx->d_flags);
    if (ctx->d_totals) (void)hipFree(ctx->d_totals);
    if (ctx->d_ws) (void)hipFree(ctx->d_ws);
    if (ctx->d_plan) (void)hipFree(ctx->d_plan);
    if (ctx->d_arena) (void)hipFree(ctx->d_arena);
    if (ctx->h_pin) (void)hipHostFree(ctx->h_pin);
    for (hipEvent_t e : ctx->pin_ev)
        if (e) (void)hipEventDestroy(e);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

const char *uavac_last_error(const uavac_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int uavac_set_stream(uavac_ctx *ctx, void *hip_stream) {
    if (!ctx) return UAVAC_EINVAL;
    ctx->stream = static_cast<hipStream_t>(hip_stream);      // NULL = HIP's legacy default stream
    return UAVAC_OK;
}

int uavac_reset_stream(uavac_ctx *ctx) {
    if (!ctx) return UAVAC_EINVAL;
    ctx->stream = ctx->own_stream;
    return UAVAC_OK;
}

int uavac_synchronize(uavac_ctx *ctx) {
    UAVAC_ENTER(ctx);
    UAVAC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return UAVAC_OK;
}

int uavac_device(const uavac_ctx *ctx) { return ctx ? ctx->device : UAVAC_EINVAL; }

int uavac_set_option(uavac_ctx *ctx, const char *name, int value) {
    if (!ctx || !name) return UAVAC_EINVAL;
    const Option *o = find_option(name);
    if (!o) return uavac_fail(ctx, UAVAC_EINVAL, "unknown option");
    if (!apply_option(ctx, *o, value)) return uavac_fail(ctx, UAVAC_EINVAL, o->message);
    return UAVAC_OK;
}

const char *uavac_last_rollout_kernel(const uavac_ctx *ctx) { return ctx ? ctx->last_rollout.c_str() : ""; }

const char *uavac_last_solve_kernel(const uavac_ctx *ctx) { return ctx ? ctx->last_solve.c_str() : ""; }

const char *uavac_last_sample_kernel(const uavac_ctx *ctx) { return ctx ? ctx->last_sample.c_str() : ""; }

int uavac_last_sample_launch(const uavac_ctx *ctx, int64_t out[5]) {
    if (!ctx || !out) return UAVAC_EINVAL;
    for (int i = 0; i < 5; ++i) out[i] = ctx->last_sample_launch[i];
    return UAVAC_OK;
}

int uavac_last_rollout_vgprs(const uavac_ctx *ctx) { return ctx ? ctx->last_rollout_vgprs : UAVAC_EINVAL; }

int uavac_last_rollout_launch(const uavac_ctx *ctx, int64_t out[6]) {
    if (!ctx || !out) return UAVAC_EINVAL;
    for (int i = 0; i < 6; ++i) out[i] = ctx->last_rollout_launch[i];
    return UAVAC_OK;
}

#define UAVAC_STR2(x) #x
#define UAVAC_STR(x) UAVAC_STR2(x)
const char *uavac_build_info(void) {
    return "libuavac " UAVAC_STR(UAVAC_VERSION) "; gfx950; HIP " UAVAC_STR(HIP_VERSION_MAJOR) "." UAVAC_STR(HIP_VERSION_MINOR) "."
           UAVAC_STR(HIP_VERSION_PATCH) "; " __VERSION__;
}

int uavac_device_identity(uavac_ctx *ctx, char *buf, int n) {
    UAVAC_ENTER(ctx);
    if (!buf || n < 1) return uavac_fail(ctx, UAVAC_EINVAL, "null buffer");
    hipDeviceProp_t prop;
    UAVAC_HIP(ctx, hipGetDeviceProperties(&prop, ctx->device));
    char uuid[33] = {0}, pci[32] = {0};
    for (int i = 0; i < 16; ++i) snprintf(uuid + 2 * i, 3, "%02x", (unsigned)(unsigned char)prop.uuid.bytes[i]);
    if (hipDeviceGetPCIBusId(pci, (int)sizeof pci, ctx->device) != hipSuccess) pci[0] = 0;
    snprintf(buf, (size_t)n, "uuid=%s;pci=%s;name=%s", uuid, pci, prop.gcnArchName);
    return UAVAC_OK;
}

int uavac_take_flags(uavac_ctx *ctx, int32_t flags[4]) {
    UAVAC_ENTER(ctx);
    if (!flags) return uavac_fail(ctx, UAVAC_EINVAL, "null flags");
    return read_flags(ctx, flags);
}

void uavac_vehicle_default(uavac_vehicle *V) {
    if (!V) return;
    std::memset(V, 0, sizeof(*V));
    V->g = 9.81; V->dt = 0.001; V->inner_per_outer = 10; V->dt_outer = V->dt * V->inner_per_outer;
    V->mass = 0.5; V->inertia[0] = 0.0023; V->inertia[1] = 0.0023; V->inertia[2] = 0.0046;
    V->arm = 0.120208; V->kf = 1.0; V->kappa = 0.016;
    V->min_thrust = 0.1; V->max_thrust = 4.5; V->tau_rise = 0.0125; V->tau_fall = 0.025;
    V->max_ascent = 3.0; V->max_descent = 2.0; V->max_speed_xy = 3.0; V->max_horiz_accel = 12.0; V->max_tilt = 0.7;
    // second_order_gains(tau, zeta) = (1/tau^2, 2 zeta/tau): quad.py:124-127 with the constants of :42-51
    V->kp_xy = 1.0 / (0.25 * 0.25); V->kd_xy = 2.0 * 0.875 / 0.25;
    V->kp_z = 1.0 / (0.2 * 0.2);    V->kd_z = 2.0 * 0.8 / 0.2;
    V->ki_z = 0.1;
    V->kp_roll = 1.0 / 0.07; V->kp_pitch = 1.0 / 0.07; V->kp_yaw = 1.0 / 0.25;
    V->kp_p = 1.0 / 0.008; V->kp_q = 1.0 / 0.008; V->kp_r = 1.0 / 0.09;
    // free flight by default; the plane of lab_course.xml:34 and the body box of :101 when switched on
    V->ground = 0; V->ground_z = 0.0; V->ground_clearance = 0.02; V->ground_timeconst = 0.02;
}

// ------------------------------------------------------------------------------- planning, device
int uavac_minsnap_row_counts_dev(uavac_ctx *ctx, const double *wp, int B, int m, double velocity, double dt,
                                 double *times, int32_t *seg_rows, int64_t *row_offsets) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, wp, B, m)) return rc;
    if (!times || !seg_rows || !row_offsets) return uavac_fail(ctx, UAVAC_EINVAL, "null output pointer");
    if (int rc = check_velocity_dt(ctx, velocity, dt)) return rc;
    return uavac_launch_row_counts(ctx, wp, B, m, velocity, dt, times, seg_rows, row_offsets);
}

int uavac_minsnap_solve_dev(uavac_ctx *ctx, const double *wp, const double *times, int B, int m, double *coeffs,
                            int32_t *status) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, wp, B, m)) return rc;
    if (!times || !coeffs) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    return uavac_launch_coeff_solve(ctx, wp, times, B, m, coeffs, status);
}

int uavac_minsnap_solve_banded_dev(uavac_ctx *ctx, const double *wp, const double *times, int B, int m,
                                   double *coeffs, int32_t *status) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, wp, B, m)) return rc;
    if (!times || !coeffs) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    return uavac_launch_solve_banded(ctx, wp, times, B, m, coeffs, status);
}

static int check_sample_args(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *row_offsets,
                             int B, int m, double dt, const double *traj) {
    if (int rc = check_plan_args(ctx, coeffs, B, m)) return rc;
    if (!seg_rows || !row_offsets || !traj) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_dt_positive(ctx, dt)) return rc;
    return UAVAC_OK;
}

int uavac_minsnap_sample_dev(uavac_ctx *ctx, const double *coeffs, const double *times, const int32_t *seg_rows,
                             const int64_t *row_offsets, int B, int m, double dt, double *traj) {
    (void)times;
    UAVAC_ENTER(ctx);
    if (int rc = check_sample_args(ctx, coeffs, seg_rows, row_offsets, B, m, dt, traj)) return rc;
    return uavac_launch_sample(ctx, coeffs, seg_rows, row_offsets, B, m, dt, traj, SampleExtras{});
}

int uavac_minsnap_sample_yaw_dev(uavac_ctx *ctx, const double *coeffs, const double *times, const int32_t *seg_rows,
                                 const int64_t *row_offsets, int B, int m, double dt, double *traj, double *yaw) {
    (void)times;
    UAVAC_ENTER(ctx);
    if (int rc = check_sample_args(ctx, coeffs, seg_rows, row_offsets, B, m, dt, traj)) return rc;
    if (!yaw) return uavac_fail(ctx, UAVAC_EINVAL, "null yaw");
    SampleExtras x;
    x.yaw_dense = yaw;
    return uavac_launch_sample(ctx, coeffs, seg_rows, row_offsets, B, m, dt, traj, x);
}

int uavac_minsnap_sample_hits_dev(uavac_ctx *ctx, const double *coeffs, const double *times, const int32_t *seg_rows,
                                  const int64_t *row_offsets, int B, int m, double dt, double *traj,
                                  const double *aabb, int32_t *hit) {
    (void)times;
    UAVAC_ENTER(ctx);
    if (int rc = check_sample_args(ctx, coeffs, seg_rows, row_offsets, B, m, dt, traj)) return rc;
    if (!aabb || !hit) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    SampleExtras x;
    x.aabb = aabb;
    x.hit = hit;
    return uavac_launch_sample(ctx, coeffs, seg_rows, row_offsets, B, m, dt, traj, x);
}

int uavac_minsnap_sample_derivs_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows,
                                    const int64_t *row_offsets, int B, int m, double dt, double *traj, double *yaw,
                                    double *first_yaw, double *jerk, double *snap) {
    UAVAC_ENTER(ctx);
    if (int rc = check_sample_args(ctx, coeffs, seg_rows, row_offsets, B, m, dt, traj)) return rc;
    SampleExtras x;
    x.yaw_dense = yaw;
    x.first_yaw = first_yaw;
    x.jerk = jerk;
    x.snap = snap;
    return uavac_launch_sample(ctx, coeffs, seg_rows, row_offsets, B, m, dt, traj, x);
}

int uavac_minsnap_sample_capped_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *row_offsets,
                                    int B, int m, double dt, double *traj, int64_t traj_capacity_rows, double *yaw,
                                    double *first_yaw) {
    UAVAC_ENTER(ctx);
    if (int rc = check_sample_args(ctx, coeffs, seg_rows, row_offsets, B, m, dt, traj)) return rc;
    if (traj_capacity_rows < 0) return uavac_fail(ctx, UAVAC_EINVAL, "negative capacity");
    SampleExtras x;
    x.yaw_dense = yaw;
    x.first_yaw = first_yaw;
    x.capacity_rows = traj_capacity_rows;
    return uavac_launch_sample(ctx, coeffs, seg_rows, row_offsets, B, m, dt, traj, x);
}

// ------------------------------------------------------------------------------- planning, device, ragged batches
int uavac_minsnap_row_counts_ragged_dev(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B, int max_m,
                                        double velocity, double dt, double *times, int32_t *seg_rows, int64_t *row_offsets) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, wp, B, max_m)) return rc;
    if (!seg_offsets || !times || !seg_rows || !row_offsets) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_velocity_dt(ctx, velocity, dt)) return rc;
    return uavac_launch_row_counts(ctx, wp, B, max_m, velocity, dt, times, seg_rows, row_offsets, seg_offsets);
}

int uavac_minsnap_solve_ragged_dev(uavac_ctx *ctx, const double *wp, const double *times, const int64_t *seg_offsets, int B,
                                   int max_m, double *coeffs, int32_t *status) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, wp, B, max_m)) return rc;
    if (!seg_offsets || !times || !coeffs) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    return uavac_launch_coeff_solve(ctx, wp, times, B, max_m, coeffs, status, seg_offsets);
}

int uavac_minsnap_sample_ragged_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets,
                                    const int64_t *row_offsets, int B, int max_m, int64_t total_segments, double dt,
                                    double *traj, int64_t traj_capacity_rows, const double *aabb, int32_t *hit,
                                    double *first_yaw) {
    UAVAC_ENTER(ctx);
    if (int rc = check_sample_args(ctx, coeffs, seg_rows, row_offsets, B, max_m, dt, traj)) return rc;
    if (!seg_offsets) return uavac_fail(ctx, UAVAC_EINVAL, "null seg_offsets");
    if (total_segments < B || total_segments > (int64_t)B * max_m)
        return uavac_fail(ctx, UAVAC_EINVAL, "total_segments must lie in [B, B * max_m]");
    if ((aabb == nullptr) != (hit == nullptr)) return uavac_fail(ctx, UAVAC_EINVAL, "aabb and hit go together");
    SampleExtras x;
    x.aabb = aabb;
    x.hit = hit;
    x.first_yaw = first_yaw;
    x.capacity_rows = traj_capacity_rows;
    x.seg_offsets = seg_offsets;
    x.total_segments = total_segments;
    return uavac_launch_sample(ctx, coeffs, seg_rows, row_offsets, B, max_m, dt, traj, x);
}

int uavac_minsnap_plan_dev(uavac_ctx *ctx, const double *wp, int B, int m, double velocity, double dt, double *times,
                           int32_t *seg_rows, int64_t *row_offsets, double *coeffs, int32_t *status, double *traj,
                           int64_t traj_capacity_rows, double *yaw, double *first_yaw) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, wp, B, m)) return rc;
    if (!times || !seg_rows || !row_offsets || !coeffs) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_velocity_dt(ctx, velocity, dt)) return rc;
    return plan_chain(ctx, wp, B, m, velocity, dt, times, seg_rows, row_offsets, coeffs, status, traj, traj_capacity_rows, yaw, first_yaw);
}

// ---------------------------------------------------------------- planning, device, one cruise speed per mission
int uavac_minsnap_row_counts_v_dev(uavac_ctx *ctx, const double *wp, int B, int m, const double *velocities, double dt,
                                   double *times, int32_t *seg_rows, int64_t *row_offsets) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, wp, B, m)) return rc;
    if (!velocities || !times || !seg_rows || !row_offsets) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_dt(ctx, dt)) return rc;
    return uavac_launch_row_counts_v(ctx, wp, B, m, velocities, dt, times, seg_rows, row_offsets);
}

int uavac_minsnap_row_counts_ragged_v_dev(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B, int max_m,
                                          const double *velocities, double dt, double *times, int32_t *seg_rows,
                                          int64_t *row_offsets) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, wp, B, max_m)) return rc;
    if (!seg_offsets || !velocities || !times || !seg_rows || !row_offsets) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_dt(ctx, dt)) return rc;
    return uavac_launch_row_counts_v(ctx, wp, B, max_m, velocities, dt, times, seg_rows, row_offsets, seg_offsets);
}

int uavac_minsnap_plan_v_dev(uavac_ctx *ctx, const double *wp, int B, int m, const double *velocities, double dt, double *times,
                             int32_t *seg_rows, int64_t *row_offsets, double *coeffs, int32_t *status, double *traj,
                             int64_t traj_capacity_rows, double *yaw, double *first_yaw) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, wp, B, m)) return rc;
    if (!velocities || !times || !seg_rows || !row_offsets || !coeffs) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_dt(ctx, dt)) return rc;
    return plan_chain(ctx, wp, B, m, velocities, dt, times, seg_rows, row_offsets, coeffs, status, traj, traj_capacity_rows, yaw,
                      first_yaw);
}

// ---------------------------------------------------------------- missions that start and end in motion
int uavac_minsnap_solve_bc_dev(uavac_ctx *ctx, const double *wp, const double *times, const int64_t *seg_offsets, int B, int m,
                               const double *bc, double *coeffs, int32_t *status) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, wp, B, m)) return rc;
    if (!times || !bc || !coeffs) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    return uavac_launch_solve_bc(ctx, wp, times, B, m, bc, coeffs, status, seg_offsets, nullptr, 0);
}

int uavac_minsnap_plan_bc_dev(uavac_ctx *ctx, const double *wp, int B, int m, const double *velocities, double dt, const double *bc,
                              double *times, int32_t *seg_rows, int64_t *row_offsets, double *coeffs, int32_t *status, double *traj,
                              int64_t traj_capacity_rows, double *yaw, double *first_yaw) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, wp, B, m)) return rc;
    if (!velocities || !bc || !times || !seg_rows || !row_offsets || !coeffs) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_dt(ctx, dt)) return rc;
    return plan_chain(ctx, wp, B, m, velocities, dt, times, seg_rows, row_offsets, coeffs, status, traj, traj_capacity_rows, yaw,
                      first_yaw, bc);
}

// ---------------------------------------------------------------- retiming to the flight limits
static int check_retime_args(uavac_ctx *ctx, int B, const double *limits, double margin, RetimeLimits *L) {
    if (B < 1) return uavac_fail(ctx, UAVAC_EINVAL, "B must be >= 1");
    if (!limits) return uavac_fail(ctx, UAVAC_EINVAL, "null limits");
    for (int i = 0; i < 4; ++i)
        if (!(limits[i] > 0.0) || !std::isfinite(limits[i])) return uavac_fail(ctx, UAVAC_EINVAL, "every limit must be finite and > 0");
    if (!(margin >= 0.0 && margin < 1.0)) return uavac_fail(ctx, UAVAC_EINVAL, "margin must be in [0, 1)");
    *L = RetimeLimits{limits[0], limits[1], limits[2], limits[3]};
    return UAVAC_OK;
}

int uavac_minsnap_retime_factors_dev(uavac_ctx *ctx, const double *audit, int B, const double limits[4], double margin,
                                     double *velocities, double *factors, int32_t *counters) {
    UAVAC_ENTER(ctx);
    RetimeLimits L;
    if (int rc = check_retime_args(ctx, B, limits, margin, &L)) return rc;
    if (!audit || !velocities || !factors || !counters) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    return uavac_launch_retime_factors(ctx, audit, B, L, margin, 1, velocities, factors, counters, nullptr, nullptr);
}

// The loop of uavac_minsnap_retime_dev and uavac_minsnap_retime_demand_dev, arguments checked by the caller.  N == NULL: the four flight
// limits alone; otherwise one more launch per pass, the need kernel after the audit, and the factors kernel that reads both blocks.
static int retime_loop(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B, int m, double *velocities, double dt,
                       const RetimeLimits &L, const NeedLimits *N, double margin, int max_passes, double *times, int32_t *seg_rows,
                       int64_t *row_offsets, double *coeffs, int32_t *status, double *first_yaw, double *audit, double *need,
                       double *factors_total, int32_t *binding, int32_t *converged, int *passes) {
    *passes = 0;
    double *d_factors = nullptr;
    int32_t *d_counters = nullptr;
    Scratch s(ctx);
    s.want(&d_factors, (size_t)B); s.want(&d_counters, 2);
    if (int rc = s.commit()) return rc;
    if (int rc = uavac_launch_fill_f64(ctx, factors_total, (size_t)B, 1.0)) return rc;
    for (int retimed = 0;; ++retimed) {
        // the rows-free chain at the current speeds, its audit, and what the audit asks for -- no row is sampled anywhere
        if (int rc = uavac_launch_row_counts_v(ctx, wp, B, m, velocities, dt, times, seg_rows, row_offsets, seg_offsets)) return rc;
        if (int rc = uavac_launch_coeff_solve(ctx, wp, times, B, m, coeffs, status, seg_offsets)) return rc;
        if (first_yaw) if (int rc = uavac_launch_first_yaw(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, first_yaw)) return rc;
        if (int rc = uavac_launch_audit(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, nullptr, 0, audit, nullptr, nullptr)) return rc;
        if (N) if (int rc = uavac_launch_need(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, *N, need)) return rc;
        UAVAC_HIP(ctx, hipMemsetAsync(d_counters, 0, 2 * sizeof(int32_t), ctx->stream));
        const int apply = retimed < max_passes;            // out of passes: the verdict only, the speeds stay what the plan was made at
        if (int rc = N ? uavac_launch_retime_demand_factors(ctx, audit, need, B, L, margin, apply, velocities, d_factors, binding, d_counters,
                                                            factors_total, converged)
                       : uavac_launch_retime_factors(ctx, audit, B, L, margin, apply, velocities, d_factors, d_counters, factors_total,
                                                     converged)) return rc;
        int32_t cnt[2];
        if (int rc = uavac_d2h(ctx, cnt, d_counters, sizeof cnt)) return rc;           // the pass's one read-back (synchronises)
        if (cnt[0] == 0 || !apply) break;
        *passes = retimed + 1;
    }
    return UAVAC_OK;
}

int uavac_minsnap_retime_dev(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B, int m, double *velocities,
                             double dt, const double limits[4], double margin, int max_passes, double *times, int32_t *seg_rows,
                             int64_t *row_offsets, double *coeffs, int32_t *status, double *first_yaw, double *audit,
                             double *factors_total, int32_t *converged, int *passes) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, wp, B, m)) return rc;
    RetimeLimits L;
    if (int rc = check_retime_args(ctx, B, limits, margin, &L)) return rc;
    if (!velocities || !times || !seg_rows || !row_offsets || !coeffs || !audit || !factors_total || !converged || !passes)
        return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_dt(ctx, dt)) return rc;
    if (max_passes < 0) return uavac_fail(ctx, UAVAC_EINVAL, "negative max_passes");
    return retime_loop(ctx, wp, seg_offsets, B, m, velocities, dt, L, nullptr, margin, max_passes, times, seg_rows, row_offsets, coeffs, status,
                       first_yaw, audit, nullptr, factors_total, nullptr, converged, passes);
}

// ---------------------------------------------------------------- retiming to the tilt and thrust limits as well
// demand_limits [4] HOST: g, max_tilt, Fmax, Fmin -> the constants the need kernel reads, each ONE rounded operation (nothing contracted:
// the NumPy specification forms them the same way).  Refuses a vehicle that cannot hover, or whose least thrust holds it up.
static int need_limits(uavac_ctx *ctx, const double *demand_limits, NeedLimits *N) {
#pragma clang fp contract(off)
    if (!demand_limits) return uavac_fail(ctx, UAVAC_EINVAL, "null demand_limits");
    const double g = demand_limits[0], tau = demand_limits[1], fmax_ = demand_limits[2], fmin_ = demand_limits[3];
    if (!std::isfinite(g) || !(g > 0.0)) return uavac_fail(ctx, UAVAC_EINVAL, "g must be finite and > 0");
    if (!std::isfinite(tau) || !(tau > 0.0)) return uavac_fail(ctx, UAVAC_EINVAL, "max_tilt must be finite and > 0");
    if (!std::isfinite(fmax_) || !(fmax_ > g)) return uavac_fail(ctx, UAVAC_EINVAL, "the largest specific thrust must be finite and > g");
    if (!(fmin_ >= 0.0) || !(fmin_ < g)) return uavac_fail(ctx, UAVAC_EINVAL, "the least specific thrust must be in [0, g)");
    const double gg = g * g, hh = fmax_ * fmax_, ll = fmin_ * fmin_;
    N->g = g; N->tau = tau;
    N->t2 = tau * tau;
    N->tg = tau * g;
    N->D = hh - gg;
    N->E = gg - ll;
    if (!std::isfinite(N->D) || !(N->D > 0.0) || !(N->E > 0.0)) return uavac_fail(ctx, UAVAC_EINVAL, "thrust limits too close to g");
    return UAVAC_OK;
}

int uavac_minsnap_need_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                           double dt, const double demand_limits[4], double *need) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, coeffs, B, m)) return rc;
    if (!seg_rows || !need) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_dt_positive(ctx, dt)) return rc;
    NeedLimits N;
    if (int rc = need_limits(ctx, demand_limits, &N)) return rc;
    return uavac_launch_need(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, N, need);
}

int uavac_minsnap_retime_demand_factors_dev(uavac_ctx *ctx, const double *audit, const double *need, int B, const double limits[4],
                                            const double demand_limits[4], double margin, double *velocities, double *factors,
                                            int32_t *binding, int32_t *counters) {
    UAVAC_ENTER(ctx);
    RetimeLimits L;
    if (int rc = check_retime_args(ctx, B, limits, margin, &L)) return rc;
    NeedLimits N;                                          // (the need block was made with them: the same refusals, nothing else is read)
    if (int rc = need_limits(ctx, demand_limits, &N)) return rc;
    if (!audit || !need || !velocities || !factors || !binding || !counters) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    return uavac_launch_retime_demand_factors(ctx, audit, need, B, L, margin, 1, velocities, factors, binding, counters, nullptr, nullptr);
}

int uavac_minsnap_retime_demand_dev(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B, int m, double *velocities,
                                    double dt, const double limits[4], const double demand_limits[4], double margin, int max_passes,
                                    double *times, int32_t *seg_rows, int64_t *row_offsets, double *coeffs, int32_t *status,
                                    double *first_yaw, double *audit, double *need, double *factors_total, int32_t *binding,
                                    int32_t *converged, int *passes) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, wp, B, m)) return rc;
    RetimeLimits L;
    if (int rc = check_retime_args(ctx, B, limits, margin, &L)) return rc;
    NeedLimits N;
    if (int rc = need_limits(ctx, demand_limits, &N)) return rc;
    if (!velocities || !times || !seg_rows || !row_offsets || !coeffs || !audit || !need || !factors_total || !binding || !converged ||
        !passes)
        return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_dt(ctx, dt)) return rc;
    if (max_passes < 0) return uavac_fail(ctx, UAVAC_EINVAL, "negative max_passes");
    return retime_loop(ctx, wp, seg_offsets, B, m, velocities, dt, L, &N, margin, max_passes, times, seg_rows, row_offsets, coeffs, status,
                       first_yaw, audit, need, factors_total, binding, converged, passes);
}

// ---------------------------------------------------------------- given durations, the snap cost, optimised durations
int uavac_minsnap_row_counts_t_dev(uavac_ctx *ctx, const double *times, const int64_t *seg_offsets, int B, int m, double dt,
                                   int32_t *seg_rows, int64_t *row_offsets) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, times, B, m)) return rc;
    if (!seg_rows || !row_offsets) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_dt(ctx, dt)) return rc;
    return uavac_launch_row_counts_t(ctx, times, seg_offsets, B, m, dt, seg_rows, row_offsets);
}

int uavac_minsnap_plan_t_dev(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B, int m, const double *times, double dt,
                             int32_t *seg_rows, int64_t *row_offsets, double *coeffs, int32_t *status, double *traj,
                             int64_t traj_capacity_rows, double *yaw, double *first_yaw) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, wp, B, m)) return rc;
    if (!times || !seg_rows || !row_offsets || !coeffs) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_dt(ctx, dt)) return rc;
    if (yaw && (!traj || seg_offsets)) return uavac_fail(ctx, UAVAC_EINVAL, "a dense yaw column needs the rows of a uniform batch");
    if (!traj) {
        // rows-free, as in plan_chain: nothing to refuse, the counts go straight into the caller's arrays
        if (int rc = uavac_launch_row_counts_t(ctx, times, seg_offsets, B, m, dt, seg_rows, row_offsets)) return rc;
        if (int rc = uavac_launch_coeff_solve(ctx, wp, times, B, m, coeffs, status, seg_offsets)) return rc;
        return first_yaw ? uavac_launch_first_yaw(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, first_yaw) : UAVAC_OK;
    }
    if (traj_capacity_rows < 0) return uavac_fail(ctx, UAVAC_EINVAL, "negative capacity");
    // With a row capacity, as in plan_chain: counts and offsets to ctx scratch, every later stage reads row_offsets_s[B] on the device
    // and does nothing when the plan does not fit (the sampler raises flag 2).  A ragged batch has at most B * m segments.
    PlanScratch s;
    if (int rc = plan_scratch(ctx, B, m, false, s)) return rc;
    if (int rc = uavac_launch_row_counts_t(ctx, times, seg_offsets, B, m, dt, s.seg_rows, s.row_offsets)) return rc;
    if (int rc = uavac_launch_plan_t_commit(ctx, s.seg_rows, s.row_offsets, seg_offsets, B, m, traj_capacity_rows, seg_rows, row_offsets))
        return rc;
    if (int rc = uavac_launch_coeff_solve(ctx, wp, times, B, m, coeffs, status, seg_offsets, s.row_offsets + B, traj_capacity_rows)) return rc;
    SampleExtras x;
    x.yaw_dense = yaw;
    x.first_yaw = first_yaw;
    x.capacity_rows = traj_capacity_rows;
    x.seg_offsets = seg_offsets;
    if (seg_offsets) x.total_segments = (int64_t)B * m;       // (sizes the hit flags only, and there are none)
    return uavac_launch_sample(ctx, coeffs, s.seg_rows, s.row_offsets, B, m, dt, traj, x);
}

int uavac_minsnap_cost_dev(uavac_ctx *ctx, const double *coeffs, const double *times, const int64_t *seg_offsets, int B, int m,
                           double *cost) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, coeffs, B, m)) return rc;
    if (!times || !cost) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    return uavac_launch_cost(ctx, coeffs, times, seg_offsets, B, m, cost);
}

int uavac_minsnap_optimize_times_dev(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B, int m, double *times,
                                     int iterations, double *cost_before, double *cost_after, int32_t *accepted) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, wp, B, m)) return rc;
    if (!times || !cost_before || !cost_after || !accepted) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (iterations < 0) return uavac_fail(ctx, UAVAC_EINVAL, "negative iterations");
    return uavac_launch_optimize_times(ctx, wp, seg_offsets, B, m, times, iterations, cost_before, cost_after, accepted);
}

int uavac_minsnap_first_yaw_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B,
                                int m, double dt, double *first_yaw) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, coeffs, B, m)) return rc;
    if (!seg_rows || !first_yaw) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_dt_positive(ctx, dt)) return rc;
    return uavac_launch_first_yaw(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, first_yaw);
}

int uavac_minsnap_audit_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                            double dt, const double *cuboids, int n_cuboids, double *audit, int32_t *hit_rows, int32_t *first_hit) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, coeffs, B, m)) return rc;
    if (!seg_rows || !audit) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_dt_positive(ctx, dt)) return rc;
    if (int rc = check_n_cuboids(ctx, n_cuboids)) return rc;
    if (n_cuboids == 0 ? (cuboids || hit_rows || first_hit) : (!cuboids || !hit_rows || !first_hit))
        return uavac_fail(ctx, UAVAC_EINVAL, "cuboids, hit_rows and first_hit go with n_cuboids > 0: all three or none");
    return uavac_launch_audit(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, cuboids, n_cuboids, audit, hit_rows, first_hit);
}

int uavac_minsnap_demand_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                             double dt, double g, const double *cuboids, int n_cuboids, double *demand, int32_t *idemand,
                             double *clearance, int32_t *clearance_row) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, coeffs, B, m)) return rc;
    if (!seg_rows || !demand || !idemand) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_dt_positive(ctx, dt)) return rc;
    if (!std::isfinite(g) || !(g > 0.0)) return uavac_fail(ctx, UAVAC_EINVAL, "g must be finite and > 0");
    if (int rc = check_n_cuboids(ctx, n_cuboids)) return rc;
    if (n_cuboids == 0 ? (cuboids || clearance || clearance_row) : (!cuboids || !clearance || !clearance_row))
        return uavac_fail(ctx, UAVAC_EINVAL, "cuboids, clearance and clearance_row go with n_cuboids > 0: all three or none");
    return uavac_launch_demand(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, g, cuboids, n_cuboids, demand, idemand, clearance,
                               clearance_row);
}

int uavac_minsnap_envelope_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                               double dt, const double *reach, double *env) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, coeffs, B, m)) return rc;
    if (!seg_rows || !env) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_dt_positive(ctx, dt)) return rc;
    return uavac_launch_envelope(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, reach, env);
}

// what the fleet's pair calls (separation, stagger, layer) refuse alike, in this order; `outputs`: every output pointer of the call is there
static int check_pair_args(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, int B, int m, double dt, const int64_t *group_offsets,
                           int G, double radius, bool outputs) {
    if (int rc = check_plan_args(ctx, coeffs, B, m)) return rc;
    if (!seg_rows || !outputs) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_dt_positive(ctx, dt)) return rc;
    if (!std::isfinite(radius) || radius < 0.0) return uavac_fail(ctx, UAVAC_EINVAL, "radius must be finite and >= 0");
    if (group_offsets && G < 1) return uavac_fail(ctx, UAVAC_EINVAL, "G must be >= 1 when group_offsets are given");
    return UAVAC_OK;
}

int uavac_minsnap_separation_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                 double dt, const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, double *sep,
                                 int32_t *isep) {
    UAVAC_ENTER(ctx);
    if (int rc = check_pair_args(ctx, coeffs, seg_rows, B, m, dt, group_offsets, G, radius, sep && isep)) return rc;
    return uavac_launch_separation(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, start_rows, radius, sep, isep);
}

int uavac_minsnap_conflict_offsets_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B,
                                       int m, double dt, const int64_t *group_offsets, int G, const int32_t *start_rows, double radius,
                                       int64_t *pair_offsets) {
    UAVAC_ENTER(ctx);
    if (int rc = check_pair_args(ctx, coeffs, seg_rows, B, m, dt, group_offsets, G, radius, pair_offsets != nullptr)) return rc;
    return uavac_launch_conflict_offsets(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, start_rows, radius, pair_offsets);
}

int uavac_minsnap_conflicts_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                double dt, const int64_t *group_offsets, int G, const int32_t *start_rows, double radius,
                                const int64_t *pair_offsets, int64_t capacity, double *pair_d, int32_t *pair_i) {
    UAVAC_ENTER(ctx);
    if (int rc = check_pair_args(ctx, coeffs, seg_rows, B, m, dt, group_offsets, G, radius, pair_offsets != nullptr)) return rc;
    if (capacity < 0) return uavac_fail(ctx, UAVAC_EINVAL, "capacity must be >= 0");
    if (capacity > 0 && (!pair_d || !pair_i)) return uavac_fail(ctx, UAVAC_EINVAL, "pair_d and pair_i are required when capacity > 0");
    return uavac_launch_conflicts(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, start_rows, radius, pair_offsets, capacity,
                                  pair_d, pair_i);
}

// what uavac_minsnap_stagger_dev and uavac_minsnap_stagger_wide_dev refuse alike
static int check_stagger_args(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, int B, int m, double dt, const int64_t *group_offsets,
                              int G, double radius, int step, int max_steps, const int32_t *istag) {
    if (int rc = check_pair_args(ctx, coeffs, seg_rows, B, m, dt, group_offsets, G, radius, istag != nullptr)) return rc;
    if (step < 1) return uavac_fail(ctx, UAVAC_EINVAL, "step must be >= 1");
    if (max_steps < 0 || max_steps > UAVAC_STAGGER_MAX_STEPS) return uavac_fail(ctx, UAVAC_EINVAL, "max_steps must be in [0, UAVAC_STAGGER_MAX_STEPS]");
    if ((long long)step * max_steps > (1LL << 29)) return uavac_fail(ctx, UAVAC_EINVAL, "step * max_steps must not exceed 2^29 rows");
    return UAVAC_OK;
}

int uavac_minsnap_stagger_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                              double dt, const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, int step,
                              int max_steps, int32_t *istag) {
    UAVAC_ENTER(ctx);
    if (int rc = check_stagger_args(ctx, coeffs, seg_rows, B, m, dt, group_offsets, G, radius, step, max_steps, istag)) return rc;
    if (!group_offsets && B > UAVAC_STAGGER_MAX_GROUP)
        return uavac_fail(ctx, UAVAC_EINVAL, "one group of all B: B must not exceed UAVAC_STAGGER_MAX_GROUP");
    return uavac_launch_stagger(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, start_rows, radius, step, max_steps, istag);
}

// what the two block-wise searches refuse beside their narrow calls' lists
static int check_group_cap(uavac_ctx *ctx, int B, const int64_t *group_offsets, int group_cap) {
    if (group_cap < 1) return uavac_fail(ctx, UAVAC_EINVAL, "group_cap must be >= 1");
    if (!group_offsets && B > group_cap) return uavac_fail(ctx, UAVAC_EINVAL, "one group of all B: B must not exceed group_cap");
    return UAVAC_OK;
}

int uavac_minsnap_stagger_wide_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                   double dt, const int64_t *group_offsets, int G, int group_cap, const int32_t *start_rows, double radius,
                                   int step, int max_steps, int32_t *istag) {
    UAVAC_ENTER(ctx);
    if (int rc = check_stagger_args(ctx, coeffs, seg_rows, B, m, dt, group_offsets, G, radius, step, max_steps, istag)) return rc;
    if (int rc = check_group_cap(ctx, B, group_offsets, group_cap)) return rc;
    return uavac_launch_stagger_wide(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, group_cap, start_rows, radius, step,
                                     max_steps, istag);
}

int uavac_minsnap_delay_offsets_dev(uavac_ctx *ctx, const int64_t *seg_offsets, int B, int m, const int32_t *start_rows,
                                    int64_t *out_seg_offsets) {
    UAVAC_ENTER(ctx);
    if (!start_rows || !out_seg_offsets) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_take_shape(ctx, B, 1, m, true)) return rc;
    return uavac_launch_delay_offsets(ctx, seg_offsets, B, m, start_rows, out_seg_offsets);
}

int uavac_minsnap_delay_dev(uavac_ctx *ctx, const double *coeffs, const double *times, const int32_t *seg_rows, const int64_t *seg_offsets,
                            int B, int m, double dt, const int32_t *start_rows, const int64_t *out_seg_offsets, double *out_coeffs,
                            double *out_times, int32_t *out_seg_rows) {
    UAVAC_ENTER(ctx);
    if (!coeffs || !seg_rows || !start_rows || !out_seg_offsets || !out_coeffs || !out_seg_rows)
        return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_take_shape(ctx, B, 1, m, true)) return rc;
    if (int rc = check_dt_positive(ctx, dt)) return rc;
    if (!times != !out_times) return uavac_fail(ctx, UAVAC_EINVAL, "times and out_times go together: both or none");
    return uavac_launch_delay(ctx, coeffs, times, seg_rows, seg_offsets, B, m, dt, start_rows, out_seg_offsets, out_coeffs, out_times,
                              out_seg_rows);
}

// what uavac_minsnap_layer_dev and uavac_minsnap_layer_obs_dev refuse alike, and uavac_minsnap_layer_wide_dev (`wide`) but for the group limit
static int check_layer_args(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, int B, int m, double dt, const int64_t *group_offsets,
                            int G, double radius, double delta_x, double delta_y, double delta_z, int max_steps, const int32_t *ilayer,
                            const double *offsets, bool wide = false) {
    if (int rc = check_pair_args(ctx, coeffs, seg_rows, B, m, dt, group_offsets, G, radius, ilayer && offsets)) return rc;
    if (!std::isfinite(delta_x) || !std::isfinite(delta_y) || !std::isfinite(delta_z)) return uavac_fail(ctx, UAVAC_EINVAL, "delta must be finite");
    if (max_steps < 0 || max_steps > UAVAC_LAYER_MAX_STEPS) return uavac_fail(ctx, UAVAC_EINVAL, "max_steps must be in [0, UAVAC_LAYER_MAX_STEPS]");
    if (!wide && !group_offsets && B > UAVAC_LAYER_MAX_GROUP)
        return uavac_fail(ctx, UAVAC_EINVAL, "one group of all B: B must not exceed UAVAC_LAYER_MAX_GROUP");
    return UAVAC_OK;
}

int uavac_minsnap_layer_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                            double dt, const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, double delta_x,
                            double delta_y, double delta_z, int max_steps, int32_t *ilayer, double *offsets) {
    UAVAC_ENTER(ctx);
    if (int rc = check_layer_args(ctx, coeffs, seg_rows, B, m, dt, group_offsets, G, radius, delta_x, delta_y, delta_z, max_steps, ilayer, offsets))
        return rc;
    return uavac_launch_layer(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, start_rows, radius, delta_x, delta_y, delta_z,
                              max_steps, ilayer, offsets);
}

int uavac_minsnap_layer_obs_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                double dt, const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, double delta_x,
                                double delta_y, double delta_z, int max_steps, const double *cuboids, int n_cuboids, int32_t *ilayer,
                                double *offsets) {
    UAVAC_ENTER(ctx);
    if (int rc = check_layer_args(ctx, coeffs, seg_rows, B, m, dt, group_offsets, G, radius, delta_x, delta_y, delta_z, max_steps, ilayer, offsets))
        return rc;
    if (int rc = check_n_cuboids(ctx, n_cuboids)) return rc;
    if (n_cuboids > 0 && !cuboids) return uavac_fail(ctx, UAVAC_EINVAL, "cuboids must be given when n_cuboids > 0");
    return uavac_launch_layer_obs(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, start_rows, radius, delta_x, delta_y, delta_z,
                                  max_steps, cuboids, n_cuboids, ilayer, offsets);
}

int uavac_minsnap_layer_wide_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                 double dt, const int64_t *group_offsets, int G, int group_cap, const int32_t *start_rows, double radius,
                                 double delta_x, double delta_y, double delta_z, int max_steps, const double *cuboids, int n_cuboids,
                                 int32_t *ilayer, double *offsets) {
    UAVAC_ENTER(ctx);
    if (int rc = check_layer_args(ctx, coeffs, seg_rows, B, m, dt, group_offsets, G, radius, delta_x, delta_y, delta_z, max_steps, ilayer, offsets,
                                  true))
        return rc;
    if (int rc = check_n_cuboids(ctx, n_cuboids)) return rc;
    if (n_cuboids > 0 && !cuboids) return uavac_fail(ctx, UAVAC_EINVAL, "cuboids must be given when n_cuboids > 0");
    if (int rc = check_group_cap(ctx, B, group_offsets, group_cap)) return rc;
    return uavac_launch_layer_wide(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, group_cap, start_rows, radius, delta_x, delta_y,
                                   delta_z, max_steps, cuboids, n_cuboids, ilayer, offsets);
}

// what the three calls against traffic refuse about the traffic's side, behind their own calls' lists
static int check_traffic_args(uavac_ctx *ctx, const int64_t *group_offsets, const double *t_coeffs, const int32_t *t_seg_rows, int Bt, int mt,
                              const int64_t *t_group_offsets) {
    if (!t_coeffs || !t_seg_rows) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer (traffic)");
    if (Bt < 1) return uavac_fail(ctx, UAVAC_EINVAL, "Bt must be >= 1");
    if (mt < 1 || mt > UAVAC_MAX_SEGMENTS) return uavac_fail(ctx, UAVAC_EINVAL, "mt must be in [1, UAVAC_MAX_SEGMENTS]");
    if (!group_offsets != !t_group_offsets)
        return uavac_fail(ctx, UAVAC_EINVAL, "group_offsets and t_group_offsets go together: both or none");
    return UAVAC_OK;
}

int uavac_minsnap_separation_against_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B,
                                         int m, double dt, const int64_t *group_offsets, int G, const double *t_coeffs,
                                         const int32_t *t_seg_rows, const int64_t *t_seg_offsets, int Bt, int mt,
                                         const int64_t *t_group_offsets, const int32_t *t_start_rows, const int32_t *start_rows,
                                         double radius, double *sep, int32_t *isep) {
    UAVAC_ENTER(ctx);
    if (int rc = check_pair_args(ctx, coeffs, seg_rows, B, m, dt, group_offsets, G, radius, sep && isep)) return rc;
    if (int rc = check_traffic_args(ctx, group_offsets, t_coeffs, t_seg_rows, Bt, mt, t_group_offsets)) return rc;
    return uavac_launch_separation_against(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, start_rows, t_coeffs, t_seg_rows,
                                           t_seg_offsets, Bt, mt, t_group_offsets, t_start_rows, radius, sep, isep);
}

int uavac_minsnap_conflict_against_offsets_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B,
                                               int m, double dt, const int64_t *group_offsets, int G, const double *t_coeffs,
                                               const int32_t *t_seg_rows, const int64_t *t_seg_offsets, int Bt, int mt,
                                               const int64_t *t_group_offsets, const int32_t *t_start_rows, const int32_t *start_rows,
                                               double radius, int64_t *pair_offsets) {
    UAVAC_ENTER(ctx);
    if (int rc = check_pair_args(ctx, coeffs, seg_rows, B, m, dt, group_offsets, G, radius, pair_offsets != nullptr)) return rc;
    if (int rc = check_traffic_args(ctx, group_offsets, t_coeffs, t_seg_rows, Bt, mt, t_group_offsets)) return rc;
    return uavac_launch_conflict_against_offsets(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, start_rows, t_coeffs,
                                                 t_seg_rows, t_seg_offsets, Bt, mt, t_group_offsets, t_start_rows, radius, pair_offsets);
}

int uavac_minsnap_conflicts_against_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B,
                                        int m, double dt, const int64_t *group_offsets, int G, const double *t_coeffs,
                                        const int32_t *t_seg_rows, const int64_t *t_seg_offsets, int Bt, int mt,
                                        const int64_t *t_group_offsets, const int32_t *t_start_rows, const int32_t *start_rows, double radius,
                                        const int64_t *pair_offsets, int64_t capacity, double *pair_d, int32_t *pair_i) {
    UAVAC_ENTER(ctx);
    if (int rc = check_pair_args(ctx, coeffs, seg_rows, B, m, dt, group_offsets, G, radius, pair_offsets != nullptr)) return rc;
    if (int rc = check_traffic_args(ctx, group_offsets, t_coeffs, t_seg_rows, Bt, mt, t_group_offsets)) return rc;
    if (capacity < 0) return uavac_fail(ctx, UAVAC_EINVAL, "capacity must be >= 0");
    if (capacity > 0 && (!pair_d || !pair_i)) return uavac_fail(ctx, UAVAC_EINVAL, "pair_d and pair_i are required when capacity > 0");
    return uavac_launch_conflicts_against(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, start_rows, t_coeffs, t_seg_rows,
                                          t_seg_offsets, Bt, mt, t_group_offsets, t_start_rows, radius, pair_offsets, capacity, pair_d, pair_i);
}

int uavac_minsnap_stagger_against_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                      double dt, const int64_t *group_offsets, int G, const double *t_coeffs, const int32_t *t_seg_rows,
                                      const int64_t *t_seg_offsets, int Bt, int mt, const int64_t *t_group_offsets,
                                      const int32_t *t_start_rows, int group_cap, const int32_t *start_rows, double radius, int step,
                                      int max_steps, int32_t *istag) {
    UAVAC_ENTER(ctx);
    if (int rc = check_stagger_args(ctx, coeffs, seg_rows, B, m, dt, group_offsets, G, radius, step, max_steps, istag)) return rc;
    if (int rc = check_group_cap(ctx, B, group_offsets, group_cap)) return rc;
    if (int rc = check_traffic_args(ctx, group_offsets, t_coeffs, t_seg_rows, Bt, mt, t_group_offsets)) return rc;
    return uavac_launch_stagger_against(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, group_cap, start_rows, t_coeffs,
                                        t_seg_rows, t_seg_offsets, Bt, mt, t_group_offsets, t_start_rows, radius, step, max_steps, istag);
}

int uavac_minsnap_layer_against_dev(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                    double dt, const int64_t *group_offsets, int G, const double *t_coeffs, const int32_t *t_seg_rows,
                                    const int64_t *t_seg_offsets, int Bt, int mt, const int64_t *t_group_offsets,
                                    const int32_t *t_start_rows, int group_cap, const int32_t *start_rows, double radius, double delta_x,
                                    double delta_y, double delta_z, int max_steps, const double *cuboids, int n_cuboids, int32_t *ilayer,
                                    double *offsets) {
    UAVAC_ENTER(ctx);
    if (int rc = check_layer_args(ctx, coeffs, seg_rows, B, m, dt, group_offsets, G, radius, delta_x, delta_y, delta_z, max_steps, ilayer, offsets,
                                  true))
        return rc;
    if (int rc = check_n_cuboids(ctx, n_cuboids)) return rc;
    if (n_cuboids > 0 && !cuboids) return uavac_fail(ctx, UAVAC_EINVAL, "cuboids must be given when n_cuboids > 0");
    if (int rc = check_group_cap(ctx, B, group_offsets, group_cap)) return rc;
    if (int rc = check_traffic_args(ctx, group_offsets, t_coeffs, t_seg_rows, Bt, mt, t_group_offsets)) return rc;
    return uavac_launch_layer_against(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, group_cap, start_rows, t_coeffs, t_seg_rows,
                                      t_seg_offsets, Bt, mt, t_group_offsets, t_start_rows, radius, delta_x, delta_y, delta_z, max_steps, cuboids,
                                      n_cuboids, ilayer, offsets);
}

int uavac_minsnap_shift_dev(uavac_ctx *ctx, const double *coeffs, const int64_t *seg_offsets, int B, int m, int64_t total_segments,
                            const double *offsets, double *out_coeffs) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, coeffs, B, m)) return rc;
    if (!offsets || !out_coeffs) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (seg_offsets && (total_segments < 1 || total_segments > (int64_t)B * m))
        return uavac_fail(ctx, UAVAC_EINVAL, "total_segments must be in [1, B * m] for a ragged batch");
    return uavac_launch_shift(ctx, coeffs, seg_offsets, B, m, total_segments, offsets, out_coeffs);
}

int uavac_minsnap_take_offsets_dev(uavac_ctx *ctx, const int64_t *seg_offsets, int B, int m, const int32_t *index, int n,
                                   int64_t *out_seg_offsets) {
    UAVAC_ENTER(ctx);
    if (!index || !out_seg_offsets) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_take_shape(ctx, B, n, m)) return rc;
    return uavac_launch_take_offsets(ctx, seg_offsets, B, m, index, n, out_seg_offsets);
}

int uavac_minsnap_take_dev(uavac_ctx *ctx, const double *coeffs, const double *times, const int32_t *seg_rows, const int64_t *seg_offsets,
                           int B, int m, const double *first_yaw, const int32_t *index, int n, const int64_t *out_seg_offsets,
                           double *out_coeffs, double *out_times, int32_t *out_seg_rows, double *out_first_yaw) {
    UAVAC_ENTER(ctx);
    if (!coeffs || !seg_rows || !index || !out_seg_offsets || !out_coeffs || !out_seg_rows)
        return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_take_shape(ctx, B, n, m)) return rc;
    if (!times != !out_times) return uavac_fail(ctx, UAVAC_EINVAL, "times and out_times go together: both or none");
    if (!first_yaw != !out_first_yaw) return uavac_fail(ctx, UAVAC_EINVAL, "first_yaw and out_first_yaw go together: both or none");
    return uavac_launch_take(ctx, coeffs, times, seg_rows, seg_offsets, B, m, first_yaw, index, n, out_seg_offsets, out_coeffs, out_times,
                             out_seg_rows, out_first_yaw);
}

int uavac_fleet_order_dev(uavac_ctx *ctx, const double *priority, const int64_t *group_offsets, int G, int B, int32_t *order,
                          int32_t *rank) {
    UAVAC_ENTER(ctx);
    if (!priority || !order || !rank) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (B < 1) return uavac_fail(ctx, UAVAC_EINVAL, "B must be >= 1");
    if (group_offsets && G < 1) return uavac_fail(ctx, UAVAC_EINVAL, "G must be >= 1 when group_offsets are given");
    return uavac_launch_fleet_order(ctx, priority, group_offsets, G, B, order, rank);
}

int uavac_fleet_airspaces_dev(uavac_ctx *ctx, const double *env, const int64_t *group_offsets, int G, int B, double radius, int rounds,
                              int resume, int32_t *labels, int32_t *info) {
    UAVAC_ENTER(ctx);
    if (!env || !labels || !info) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (B < 1) return uavac_fail(ctx, UAVAC_EINVAL, "B must be >= 1");
    if (group_offsets && G < 1) return uavac_fail(ctx, UAVAC_EINVAL, "G must be >= 1 when group_offsets are given");
    if (!std::isfinite(radius) || radius < 0.0) return uavac_fail(ctx, UAVAC_EINVAL, "radius must be finite and >= 0");
    if (rounds < 1) return uavac_fail(ctx, UAVAC_EINVAL, "rounds must be >= 1");
    if (resume != 0 && resume != 1) return uavac_fail(ctx, UAVAC_EINVAL, "resume is 0 or 1");
    return uavac_launch_fleet_airspaces(ctx, env, group_offsets, G, B, radius, rounds, resume, labels, info);
}

// what the flown separation audit and the flown conflict list refuse alike; `outputs`: the call's required output pointers are there
static int check_flown_pair_args(uavac_ctx *ctx, const double *state_log, int K, int B, int64_t pitch, const int64_t *group_offsets, int G,
                                 double radius, bool outputs) {
    if (!state_log || !outputs) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (K < 1) return uavac_fail(ctx, UAVAC_EINVAL, "K must be >= 1");
    if (B < 1) return uavac_fail(ctx, UAVAC_EINVAL, "B must be >= 1");
    if (pitch < B) return uavac_fail(ctx, UAVAC_EINVAL, "pitch must be >= B");
    if (!std::isfinite(radius) || radius < 0.0) return uavac_fail(ctx, UAVAC_EINVAL, "radius must be finite and >= 0");
    if (group_offsets && G < 1) return uavac_fail(ctx, UAVAC_EINVAL, "G must be >= 1 when group_offsets are given");
    return UAVAC_OK;
}

int uavac_flown_separation_dev(uavac_ctx *ctx, const double *state_log, int K, int B, int64_t pitch, const int64_t *group_offsets, int G,
                               double radius, double *sep, int32_t *isep) {
    UAVAC_ENTER(ctx);
    if (int rc = check_flown_pair_args(ctx, state_log, K, B, pitch, group_offsets, G, radius, sep && isep)) return rc;
    return uavac_launch_flown_separation(ctx, state_log, K, B, pitch, group_offsets, G, radius, sep, isep);
}

int uavac_flown_conflict_offsets_dev(uavac_ctx *ctx, const double *state_log, int K, int B, int64_t pitch, const int64_t *group_offsets,
                                     int G, double radius, int64_t *pair_offsets) {
    UAVAC_ENTER(ctx);
    if (int rc = check_flown_pair_args(ctx, state_log, K, B, pitch, group_offsets, G, radius, pair_offsets != nullptr)) return rc;
    return uavac_launch_flown_conflict_offsets(ctx, state_log, K, B, pitch, group_offsets, G, radius, pair_offsets);
}

int uavac_flown_conflicts_dev(uavac_ctx *ctx, const double *state_log, int K, int B, int64_t pitch, const int64_t *group_offsets, int G,
                              double radius, const int64_t *pair_offsets, int64_t capacity, double *pair_d, int32_t *pair_i) {
    UAVAC_ENTER(ctx);
    if (int rc = check_flown_pair_args(ctx, state_log, K, B, pitch, group_offsets, G, radius, pair_offsets != nullptr)) return rc;
    if (capacity < 0) return uavac_fail(ctx, UAVAC_EINVAL, "capacity must be >= 0");
    if (capacity > 0 && (!pair_d || !pair_i)) return uavac_fail(ctx, UAVAC_EINVAL, "pair_d and pair_i are required when capacity > 0");
    return uavac_launch_flown_conflicts(ctx, state_log, K, B, pitch, group_offsets, G, radius, pair_offsets, capacity, pair_d, pair_i);
}

int uavac_flown_audit_dev(uavac_ctx *ctx, const double *state_log, int K, int B, int64_t pitch, const double *cuboids, int n_cuboids,
                          double *audit, int32_t *first_bad, int32_t *hit_ticks, int32_t *first_hit, double *clearance,
                          int32_t *clearance_tick) {
    UAVAC_ENTER(ctx);
    if (!state_log || !audit || !first_bad) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (K < 1) return uavac_fail(ctx, UAVAC_EINVAL, "K must be >= 1");
    if (B < 1) return uavac_fail(ctx, UAVAC_EINVAL, "B must be >= 1");
    if (pitch < B) return uavac_fail(ctx, UAVAC_EINVAL, "pitch must be >= B");
    if (int rc = check_n_cuboids(ctx, n_cuboids)) return rc;
    if (n_cuboids == 0 ? (cuboids || hit_ticks || first_hit || clearance || clearance_tick)
                       : (!cuboids || !hit_ticks || !first_hit || !clearance || !clearance_tick))
        return uavac_fail(ctx, UAVAC_EINVAL, "cuboids, hit_ticks, first_hit, clearance and clearance_tick go with n_cuboids > 0: all five or none");
    return uavac_launch_flown_audit(ctx, state_log, K, B, pitch, cuboids, n_cuboids, audit, first_bad, hit_ticks, first_hit, clearance,
                                    clearance_tick);
}

int uavac_minsnap_row_offsets_dev(uavac_ctx *ctx, const int32_t *seg_rows, int B, int m, int64_t *row_offsets) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, seg_rows, B, m)) return rc;
    if (!row_offsets) return uavac_fail(ctx, UAVAC_EINVAL, "null row_offsets");
    return uavac_launch_row_offsets(ctx, seg_rows, B, m, row_offsets);
}

int uavac_minsnap_row_offsets_ragged_dev(uavac_ctx *ctx, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int max_m,
                                         int64_t *row_offsets) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, seg_rows, B, max_m)) return rc;
    if (!seg_offsets || !row_offsets) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    return uavac_launch_row_offsets(ctx, seg_rows, B, max_m, row_offsets, seg_offsets);
}

int uavac_minsnap_obstacle_round_dev(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B, int max_m,
                                     double velocity, double dt, const double *aabb, int32_t *active, int32_t *overflow,
                                     int32_t *touched, double *wp_out, int64_t *seg_offsets_out, int32_t *counters,
                                     double *times, int32_t *seg_rows, int64_t *row_offsets, double *coeffs, int32_t *hit) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, wp, B, max_m)) return rc;
    if (!seg_offsets || !aabb || !active || !overflow || !touched || !wp_out || !seg_offsets_out || !counters || !times ||
        !seg_rows || !row_offsets || !coeffs || !hit)
        return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_velocity_dt(ctx, velocity, dt)) return rc;
    UAVAC_HIP(ctx, hipMemsetAsync(counters, 0, 4 * sizeof(int32_t), ctx->stream));
    if (int rc = uavac_launch_row_counts(ctx, wp, B, max_m, velocity, dt, times, seg_rows, row_offsets, seg_offsets)) return rc;
    if (int rc = uavac_launch_coeff_solve(ctx, wp, times, B, max_m, coeffs, nullptr, seg_offsets, nullptr, 0, active)) return rc;
    return uavac_launch_obstacle_scan_and_insert(ctx, wp, seg_offsets, coeffs, seg_rows, B, max_m, dt, aabb, active, overflow,
                                                 touched, hit, wp_out, seg_offsets_out, counters);
}

int uavac_yaw_scan_dev(uavac_ctx *ctx, const double *velocities, const int64_t *offsets, int B, double *yaws) {
    UAVAC_ENTER(ctx);
    if (!velocities || !offsets || !yaws || B < 1) return uavac_fail(ctx, UAVAC_EINVAL, "bad B or null pointer");
    return uavac_launch_yaw_scan(ctx, velocities, offsets, B, yaws);
}

// --------------------------------------------------------------------------------- planning, host
int uavac_minsnap_row_counts(uavac_ctx *ctx, const double *wp, int B, int m, double velocity, double dt,
                             double *times, int32_t *seg_rows, int64_t *row_offsets) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, wp, B, m)) return rc;
    if (!row_offsets) return uavac_fail(ctx, UAVAC_EINVAL, "null row_offsets");
    const size_t nwp = (size_t)B * (m + 1) * 3, nseg = (size_t)B * m;
    if (!finite_all(wp, nwp) || !std::isfinite(velocity) || !std::isfinite(dt))
        return uavac_fail(ctx, UAVAC_ENONFINITE, "non-finite waypoint, velocity or dt");
    double *dwp = nullptr, *dt_ = nullptr;
    int32_t *dsr = nullptr;
    int64_t *dro = nullptr;
    Scratch s(ctx);
    s.in(&dwp, wp, nwp); s.out(&dt_, times, nseg); s.out(&dsr, seg_rows, nseg); s.out(&dro, row_offsets, (size_t)B + 1);
    if (int rc = s.commit()) return rc;
    if (int rc = clear_flags(ctx)) return rc;
    if (int rc = s.upload()) return rc;
    if (int rc = uavac_minsnap_row_counts_dev(ctx, dwp, B, m, velocity, dt, dt_, dsr, dro)) return rc;
    if (int rc = s.download()) return rc;
    int32_t fl[4];
    if (int rc = read_flags(ctx, fl)) return rc;
    if (fl[0]) return uavac_fail(ctx, UAVAC_ENONFINITE, "non-finite segment duration");
    if (fl[3]) return uavac_fail(ctx, UAVAC_EINVAL, "a mission has more than 2^31-1 rows");
    return UAVAC_OK;
}

int uavac_minsnap_solve(uavac_ctx *ctx, const double *wp, int B, int m, double velocity, double *coeffs,
                        double *times) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, wp, B, m)) return rc;
    if (!coeffs) return uavac_fail(ctx, UAVAC_EINVAL, "null coeffs");
    const size_t nwp = (size_t)B * (m + 1) * 3, nseg = (size_t)B * m, nco = (size_t)B * 24 * m;
    if (!finite_all(wp, nwp) || !std::isfinite(velocity))
        return uavac_fail(ctx, UAVAC_ENONFINITE, "non-finite waypoint or velocity");
    if (!(velocity > 0.0)) return uavac_fail(ctx, UAVAC_EINVAL, "velocity must be > 0");
    double *dwp = nullptr, *dt_ = nullptr, *dco = nullptr;
    int32_t *dsr = nullptr;
    int64_t *dro = nullptr;
    Scratch s(ctx);
    s.in(&dwp, wp, nwp); s.out(&dt_, times, nseg); s.want(&dsr, nseg); s.want(&dro, (size_t)B + 1); s.out(&dco, coeffs, nco);
    if (int rc = s.commit()) return rc;
    if (int rc = clear_flags(ctx)) return rc;
    if (int rc = s.upload()) return rc;
    // dt only shapes the row counts, which this entry point does not return
    if (int rc = uavac_launch_row_counts(ctx, dwp, B, m, velocity, 1.0, dt_, dsr, dro)) return rc;
    if (int rc = uavac_launch_coeff_solve(ctx, dwp, dt_, B, m, dco, nullptr)) return rc;
    if (int rc = s.download()) return rc;
    int32_t fl[4];
    if (int rc = read_flags(ctx, fl)) return rc;
    if (fl[0]) return uavac_fail(ctx, UAVAC_ENONFINITE, "non-finite segment duration");
    if (fl[1]) return uavac_fail(ctx, UAVAC_ESINGULAR, "singular knot system (repeated waypoint?)");
    return UAVAC_OK;
}

int uavac_minsnap_sample(uavac_ctx *ctx, const double *coeffs, const double *times, int B, int m, double dt,
                         const int64_t *row_offsets, double *traj) {
    UAVAC_ENTER(ctx);
    if (int rc = check_plan_args(ctx, coeffs, B, m)) return rc;
    if (!times || !row_offsets || !traj) return uavac_fail(ctx, UAVAC_EINVAL, "null pointer");
    if (int rc = check_dt_positive(ctx, dt)) return rc;
    const size_t nseg = (size_t)B * m, nco = (size_t)B * 24 * m;
    // rows per segment, as uavac_minsnap_row_counts computes them; must agree with the caller's offsets
    std::vector<int32_t> sr(nseg);
    for (int b = 0; b < B; ++b) {
        int64_t tot = 0;
        for (int s = 0; s < m; ++s) {
            double q = std::ceil(times[(size_t)b * m + s] / dt);
            int32_t r = (std::isfinite(q) && q > 0.0 && q < 2.0e9) ? (int32_t)q : 0;
            sr[(size_t)b * m + s] = r;
            tot += r;
        }
        if (row_offsets[b + 1] - row_offsets[b] != tot)
            return uavac_fail(ctx, UAVAC_EINVAL, "row_offsets inconsistent with ceil(times/dt)");
    }
    const int64_t total = row_offsets[B] - row_offsets[0];
    if (row_offsets[0] != 0 || total < 0) return uavac_fail(ctx, UAVAC_EINVAL, "row_offsets must start at 0");
    const size_t ntr = (size_t)total * UAVAC_TRAJ_COLS;
    double *dco = nullptr, *dtr = nullptr;
    int32_t *dsr = nullptr;
    int64_t *dro = nullptr;
    Scratch s(ctx);
    s.in(&dco, coeffs, nco); s.in(&dsr, sr.data(), nseg); s.in(&dro, row_offsets, (size_t)B + 1); s.out(&dtr, traj, ntr);
    if (int rc = s.commit()) return rc;
    if (int rc = s.upload()) return rc;
    if (int rc = uavac_launch_sample(ctx, dco, dsr, dro, B, m, dt, dtr, SampleExtras{})) return rc;
    if (int rc = s.download()) return rc;
    UAVAC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return UAVAC_OK;
}

// One call for a ragged batch on host buffers: durations, row offsets, coefficients and rows.  `traj` may be NULL (or too small:
// traj_capacity_rows): then everything but the rows is produced, row_offsets[B] says how many rows a second call needs.
int uavac_minsnap_plan_ragged(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B, double velocity, double dt,
                              double *times, int64_t *row_offsets, double *coeffs, double *traj, int64_t traj_capacity_rows) {
    UAVAC_ENTER(ctx);
    if (B < 1 || !wp || !seg_offsets || !row_offsets) return uavac_fail(ctx, UAVAC_EINVAL, "bad B or null pointer");
    if (seg_offsets[0] != 0) return uavac_fail(ctx, UAVAC_EINVAL, "seg_offsets must start at 0");
    int max_m = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t mb = seg_offsets[b + 1] - seg_offsets[b];
        if (mb < 1 || mb > UAVAC_MAX_SEGMENTS)
            return uavac_fail(ctx, UAVAC_EINVAL, "every mission needs 1 .. UAVAC_MAX_SEGMENTS segments");
        if (mb > max_m) max_m = (int)mb;
    }
    const size_t S = (size_t)seg_offsets[B], nwp = (S + (size_t)B) * 3, nco = S * 24;
    if (!finite_all(wp, nwp) || !std::isfinite(velocity) || !std::isfinite(dt))
        return uavac_fail(ctx, UAVAC_ENONFINITE, "non-finite waypoint, velocity or dt");
    if (!(velocity > 0.0) || !(dt > 0.0)) return uavac_fail(ctx, UAVAC_EINVAL, "velocity and dt must be > 0");
    double *dwp = nullptr, *dtm = nullptr, *dco = nullptr, *dtr = nullptr;
    int64_t *dso = nullptr, *dro = nullptr;
    int32_t *dsr = nullptr;
    Scratch s(ctx);
    s.want(&dwp, nwp); s.want(&dso, (size_t)B + 1); s.want(&dtm, S); s.want(&dsr, S); s.want(&dro, (size_t)B + 1); s.want(&dco, nco);
    auto stage_inputs = [&]() -> int {          // (again once the rows are registered: a commit lays every piece out anew)
        if (int rc = s.commit()) return rc;
        if (int rc = uavac_h2d(ctx, dwp, wp, nwp * 8)) return rc;
        return uavac_h2d(ctx, dso, seg_offsets, ((size_t)B + 1) * 8);
    };
    if (int rc = clear_flags(ctx)) return rc;
    if (int rc = stage_inputs()) return rc;
    if (int rc = uavac_launch_row_counts(ctx, dwp, B, max_m, velocity, dt, dtm, dsr, dro, dso)) return rc;
    if (int rc = uavac_d2h(ctx, row_offsets, dro, ((size_t)B + 1) * 8)) return rc;
    UAVAC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    int32_t fl[4];
    if (int rc = read_flags(ctx, fl)) return rc;
    if (fl[0]) return uavac_fail(ctx, UAVAC_ENONFINITE, "non-finite segment duration");
    if (fl[3]) return uavac_fail(ctx, UAVAC_EINVAL, "a mission has more than 2^31-1 rows");
    const int64_t total = row_offsets[B];
    const bool rows = traj && traj_capacity_rows >= total && total > 0;
    if (rows) {             // the arena grows for the rows: stage again (cheap next to the rows) and redo the counts
        s.want(&dtr, (size_t)total * UAVAC_TRAJ_COLS);
        if (int rc = stage_inputs()) return rc;
        if (int rc = uavac_launch_row_counts(ctx, dwp, B, max_m, velocity, dt, dtm, dsr, dro, dso)) return rc;
    }
    if (int rc = uavac_launch_coeff_solve(ctx, dwp, dtm, B, max_m, dco, nullptr, dso)) return rc;
    if (rows) {
        SampleExtras x;
        x.seg_offsets = dso;
        x.total_segments = (int64_t)S;
        x.capacity_rows = total;
        if (int rc = uavac_launch_sample(ctx, dco, dsr, dro, B, max_m, dt, dtr, x)) return rc;
        if (int rc = uavac_d2h(ctx, traj, dtr, (size_t)total * UAVAC_TRAJ_COLS * 8)) return rc;
    }
    if (times) if (int rc = uavac_d2h(ctx, times, dtm, S * 8)) return rc;
    if (coeffs) if (int rc = uavac_d2h(ctx, coeffs, dco, nco * 8)) return rc;
    UAVAC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (int rc = read_flags(ctx, fl)) return rc;
    if (fl[1]) return uavac_fail(ctx, UAVAC_ESINGULAR, "singular knot system (repeated waypoint?)");
    if (traj && !rows && total > 0) return uavac_fail(ctx, UAVAC_EINVAL, "traj_capacity_rows < row_offsets[B]: nothing sampled");
    return UAVAC_OK;
}

// The obstacle loop of MinimumSnap._generate_collision_free_trajectory (minimum_snap.py:63-95) for B ragged missions on HOST
// buffers: every round is uavac_minsnap_obstacle_round_dev on device scratch of this ctx, the host keeps the bookkeeping the
// reference keeps (obstacles in order, earlier ones not re-checked; a bounded number of rounds per obstacle; optional re-check
// sweeps over the missions that received midpoints).  Returns the final waypoint lists; sample them with
// uavac_minsnap_plan_ragged.
int uavac_minsnap_obstacle_waypoints(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B, double velocity,
                                     double dt, const double *cuboids, int n_cuboids, int max_iterations, int recheck_passes,
                                     double *wp_out, int64_t wp_capacity, int64_t *seg_offsets_out, int32_t *converged) {
    UAVAC_ENTER(ctx);
    if (B < 1 || !wp || !seg_offsets || !wp_out || !seg_offsets_out || n_cuboids < 0 || (n_cuboids > 0 && !cuboids))
        return uavac_fail(ctx, UAVAC_EINVAL, "bad B or null pointer");
    if (seg_offsets[0] != 0) return uavac_fail(ctx, UAVAC_EINVAL, "seg_offsets must start at 0");
    if (max_iterations < 0 || recheck_passes < 0) return uavac_fail(ctx, UAVAC_EINVAL, "negative iteration count");
    int max_m = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t mb = seg_offsets[b + 1] - seg_offsets[b];
        if (mb < 1 || mb > UAVAC_MAX_SEGMENTS)
            return uavac_fail(ctx, UAVAC_EINVAL, "every mission needs 1 .. UAVAC_MAX_SEGMENTS segments");
        if (mb > max_m) max_m = (int)mb;
    }
    const size_t S0 = (size_t)seg_offsets[B], nB = (size_t)B;
    if (!finite_all(wp, (S0 + nB) * 3) || (n_cuboids && !finite_all(cuboids, (size_t)n_cuboids * 6)) || !std::isfinite(velocity) ||
        !std::isfinite(dt))
        return uavac_fail(ctx, UAVAC_ENONFINITE, "non-finite waypoint, cuboid, velocity or dt");
    if (!(velocity > 0.0) || !(dt > 0.0)) return uavac_fail(ctx, UAVAC_EINVAL, "velocity and dt must be > 0");
    const size_t S_cap = nB * UAVAC_MAX_SEGMENTS, W_cap = (S_cap + nB) * 3;         // no mission ever has more segments
    double *wp_a = nullptr, *wp_b = nullptr, *d_times = nullptr, *d_coeffs = nullptr, *d_cub = nullptr;
    int64_t *so_a = nullptr, *so_b = nullptr, *d_row_offsets = nullptr;
    int32_t *d_active = nullptr, *d_overflow = nullptr, *d_touched = nullptr, *d_counters = nullptr, *d_seg_rows = nullptr, *d_hit = nullptr;
    Scratch s(ctx);
    s.want(&wp_a, W_cap); s.want(&wp_b, W_cap); s.want(&so_a, nB + 1); s.want(&so_b, nB + 1);
    s.want(&d_active, nB); s.want(&d_overflow, nB); s.want(&d_touched, nB); s.want(&d_counters, 4);
    s.want(&d_times, S_cap); s.want(&d_seg_rows, S_cap); s.want(&d_hit, S_cap); s.want(&d_row_offsets, nB + 1);
    s.want(&d_coeffs, S_cap * 24); s.want(&d_cub, (size_t)n_cuboids * 6);
    if (int rc = s.commit()) return rc;
    if (int rc = clear_flags(ctx)) return rc;
    if (int rc = uavac_h2d(ctx, wp_a, wp, (S0 + nB) * 24)) return rc;
    if (int rc = uavac_h2d(ctx, so_a, seg_offsets, (nB + 1) * 8)) return rc;
    if (n_cuboids) if (int rc = uavac_h2d(ctx, d_cub, cuboids, (size_t)n_cuboids * 48)) return rc;
    UAVAC_HIP(ctx, hipMemsetAsync(d_overflow, 0, nB * 4, ctx->stream));
    std::vector<int32_t> todo(nB, 1), failed(nB, 0), active(nB), touched(nB), overflow(nB);
    for (int sweep = 0; sweep <= recheck_passes && n_cuboids > 0; ++sweep) {
        UAVAC_HIP(ctx, hipMemsetAsync(d_touched, 0, nB * 4, ctx->stream));
        for (int c = 0; c < n_cuboids; ++c) {
            int n_active = 0;
            for (size_t b = 0; b < nB; ++b) { active[b] = todo[b] && !failed[b]; n_active += active[b]; }
            if (int rc = uavac_h2d(ctx, d_active, active.data(), nB * 4)) return rc;
            int it = 0;
            for (; it <= max_iterations && n_active > 0; ++it) {
                if (int rc = uavac_minsnap_obstacle_round_dev(ctx, wp_a, so_a, B, max_m, velocity, dt, d_cub + 6 * c, d_active,
                                                              d_overflow, d_touched, wp_b, so_b, d_counters, d_times, d_seg_rows,
                                                              d_row_offsets, d_coeffs, d_hit)) return rc;
                std::swap(wp_a, wp_b);
                std::swap(so_a, so_b);
                int32_t cnt[4];
                if (int rc = uavac_d2h(ctx, cnt, d_counters, 16)) return rc;           // the round's one read-back (synchronises)
                n_active = cnt[0];
                if (cnt[2] > max_m) max_m = cnt[2];
                if (cnt[1]) {                                                           // outgrew UAVAC_MAX_SEGMENTS: stays as it is
                    if (int rc = uavac_d2h(ctx, overflow.data(), d_overflow, nB * 4)) return rc;
                    for (size_t b = 0; b < nB; ++b) failed[b] |= overflow[b];
                }
            }
            if (n_active > 0) {                                                         // the bounded loop ran out
                if (int rc = uavac_d2h(ctx, active.data(), d_active, nB * 4)) return rc;
                for (size_t b = 0; b < nB; ++b) failed[b] |= (active[b] != 0);
            }
        }
        if (int rc = uavac_d2h(ctx, touched.data(), d_touched, nB * 4)) return rc;
        int again = 0;
        for (size_t b = 0; b < nB; ++b) { todo[b] = touched[b] && !failed[b]; again += todo[b]; }
        if (!again) break;                                                              // only missions that changed can have new conflicts
    }
    if (int rc = uavac_d2h(ctx, seg_offsets_out, so_a, (nB + 1) * 8)) return rc;
    UAVAC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t n_wp = seg_offsets_out[B] + B;
    int32_t fl[4];
    if (int rc = read_flags(ctx, fl)) return rc;
    if (fl[0]) return uavac_fail(ctx, UAVAC_ENONFINITE, "non-finite segment duration");
    if (n_wp > wp_capacity) return uavac_fail(ctx, UAVAC_EINVAL, "wp_capacity too small: seg_offsets_out[B] + B waypoints are needed");
    if (int rc = uavac_d2h(ctx, wp_out, wp_a, (size_t)n_wp * 24)) return rc;
    UAVAC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (converged) for (size_t b = 0; b < nB; ++b) converged[b] = failed[b] ? 0 : 1;
    // a singular knot system (a repeated waypoint) gives NaN coefficients, and NaN positions are inside no cuboid: such a
    // mission would pass for collision-free.  The outputs are complete, the call says so (like uavac_minsnap_solve).
    if (fl[1]) return uavac_fail(ctx, UAVAC_ESINGULAR, "a mission's knot system is singular (repeated waypoint?): its collision scan is void");
    return UAVAC_OK;
}

int uavac_yaw_scan(uavac_ctx *ctx, const double *velocities, int64_t n, double *yaws) {
    UAVAC_ENTER(ctx);
    if (n < 0 || (n > 0 && (!velocities || !yaws))) return uavac_fail(ctx, UAVAC_EINVAL, "bad n or null pointer");
    if (n == 0) return UAVAC_OK;
    double *dv = nullptr, *dy = nullptr;
    int64_t *doff = nullptr;
    const int64_t off[2] = {0, n};
    Scratch s(ctx);
    s.in(&dv, velocities, (size_t)n * 3); s.out(&dy, yaws, (size_t)n); s.in(&doff, off, 2);
    if (int rc = s.commit()) return rc;
    if (int rc = s.upload()) return rc;
    if (int rc = uavac_launch_yaw_scan(ctx, dv, doff, 1, dy)) return rc;
    if (int rc = s.download()) return rc;
    UAVAC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return UAVAC_OK;
}

// -------------------------------------------------------------------------------- control, device
int uavac_state_init_dev(uavac_ctx *ctx, const uavac_vehicle *V, const double *positions, int B, int hover,
                         double *state, int32_t *istate) {
    UAVAC_ENTER(ctx);
    if (int rc = uavac_check_vehicle(ctx, V)) return rc;
    if (B < 1 || !state || !istate) return uavac_fail(ctx, UAVAC_EINVAL, "bad B or null state");
    return uavac_launch_state_init(ctx, uavac_make_vehk(*V), positions, B, hover, state, istate);
}

static int rollout_rows(uavac_ctx *ctx, const uavac_vehicle *V, const double *traj, const int64_t *row_offsets, double *state,
                        int32_t *istate, int B, int K, double *state_log, double *cmd_log, const double *aabbs, int n_obs,
                        double *score) {
    UAVAC_ENTER(ctx);
    if (int rc = uavac_check_vehicle(ctx, V)) return rc;
    if (B < 1 || K < 0 || !traj || !row_offsets || !state || !istate || n_obs < 0)
        return uavac_fail(ctx, UAVAC_EINVAL, "bad size or null pointer");
    if (K == 0) return UAVAC_OK;
    if ((state_log || cmd_log) && ctx->log_pitch > 0 && ctx->log_pitch < B)
        return uavac_fail(ctx, UAVAC_EINVAL, "option log_pitch is smaller than B");
    return uavac_launch_rollout(ctx, uavac_make_vehk(*V), traj, row_offsets, state, istate, B, K, state_log, cmd_log,
                                aabbs, n_obs, nullptr, score);
}

// The plan-fed rollout, uniform (`ragged` false: seg_offsets is NULL; the dense yaw column or the first headings) or ragged (seg_offsets
// and first_yaw are required, there is no dense yaw column: yaw is NULL)
static int rollout_plan(uavac_ctx *ctx, const uavac_vehicle *V, const double *coeffs, const int32_t *seg_rows, bool ragged,
                        const int64_t *seg_offsets, const int64_t *row_offsets, const double *yaw, const double *first_yaw, int m,
                        double dt, double *state, int32_t *istate, int B, int K, double *state_log, double *cmd_log,
                        const double *aabbs, int n_obs, double *score) {
    UAVAC_ENTER(ctx);
    if (int rc = uavac_check_vehicle(ctx, V)) return rc;
    if (int rc = check_plan_args(ctx, coeffs, B, m)) return rc;
    if (K < 0 || !seg_rows || !row_offsets || !state || !istate || n_obs < 0 || (ragged && (!seg_offsets || !first_yaw)))
        return uavac_fail(ctx, UAVAC_EINVAL, "bad size or null pointer");
    if (!yaw && !first_yaw) return uavac_fail(ctx, UAVAC_EINVAL, "need the dense yaw column or the missions' first headings");
    if (int rc = check_dt_positive(ctx, dt)) return rc;
    if (K == 0) return UAVAC_OK;
    if ((state_log || cmd_log) && ctx->log_pitch > 0 && ctx->log_pitch < B)
        return uavac_fail(ctx, UAVAC_EINVAL, "option log_pitch is smaller than B");
    PlanRef plan;
    plan.coeffs = coeffs; plan.seg_rows = seg_rows; plan.yaw = yaw; plan.first_yaw = first_yaw; plan.dt = dt; plan.m = m;
    plan.seg_offsets = seg_offsets;
    return uavac_launch_rollout(ctx, uavac_make_vehk(*V), nullptr, row_offsets, state, istate, B, K, state_log, cmd_log,
                                aabbs, n_obs, &plan, score);
}

// scores are accumulated without a command log only (include/uavac.h): the kernel instances stay few
static int check_score_args(uavac_ctx *ctx, const double *cmd_log, const double *score) {
    if (!score) return uavac_fail(ctx, UAVAC_EINVAL, "null score");
    if (cmd_log) return uavac_fail(ctx, UAVAC_EINVAL, "no scores together with a command log");
    return UAVAC_OK;
}

int uavac_control_rollout_dev(uavac_ctx *ctx, const uavac_vehicle *V, const double *traj, const int64_t *row_offsets,
                              double *state, int32_t *istate, int B, int K, double *state_log, double *cmd_log,
                              const double *aabbs, int n_obs) {
    return rollout_rows(ctx, V, traj, row_offsets, state, istate, B, K, state_log, cmd_log, aabbs, n_obs, nullptr);
}

int uavac_control_rollout_plan_dev(uavac_ctx *ctx, const uavac_vehicle *V, const double *coeffs, const int32_t *seg_rows,
                                   const int64_t *row_offsets, const double *yaw, const double *first_yaw, int m, double dt,
                                   double *state, int32_t *istate, int B, int K, double *state_log, double *cmd_log,
                                   const double *aabbs, int n_obs) {
    return rollout_plan(ctx, V, coeffs, seg_rows, false, nullptr, row_offsets, yaw, first_yaw, m, dt, state, istate, B, K, state_log,
                        cmd_log, aabbs, n_obs, nullptr);
}

int uavac_control_rollout_plan_ragged_dev(uavac_ctx *ctx, const uavac_vehicle *V, const double *coeffs, const int32_t *seg_rows,
                                          const int64_t *seg_offsets, const int64_t *row_offsets, const double *first_yaw,
                                          int max_m, double dt, double *state, int32_t *istate, int B, int K,
                                          double *state_log, double *cmd_log, const double *aabbs, int n_obs) {
    return rollout_plan(ctx, V, coeffs, seg_rows, true, seg_offsets, row_offsets, nullptr, first_yaw, max_m, dt, state, istate, B, K,
                        state_log, cmd_log, aabbs, n_obs, nullptr);
}

int uavac_control_rollout_scored_dev(uavac_ctx *ctx, const uavac_vehicle *V, const double *traj, const int64_t *row_offsets,
                                     double *state, int32_t *istate, int B, int K, double *state_log, double *cmd_log,
                                     const double *aabbs, int n_obs, double *score) {
    UAVAC_ENTER(ctx);
    if (int rc = check_score_args(ctx, cmd_log, score)) return rc;
    return rollout_rows(ctx, V, traj, row_offsets, state, istate, B, K, state_log, cmd_log, aabbs, n_obs, score);
}

int uavac_control_rollout_plan_scored_dev(uavac_ctx *ctx, const uavac_vehicle *V, const double *coeffs, const int32_t *seg_rows,
                                          const int64_t *row_offsets, const double *yaw, const double *first_yaw, int m, double dt,
                                          double *state, int32_t *istate, int B, int K, double *state_log, double *cmd_log,
                                          const double *aabbs, int n_obs, double *score) {
    UAVAC_ENTER(ctx);
    if (int rc = check_score_args(ctx, cmd_log, score)) return rc;
    return rollout_plan(ctx, V, coeffs, seg_rows, false, nullptr, row_offsets, yaw, first_yaw, m, dt, state, istate, B, K, state_log,
                        cmd_log, aabbs, n_obs, score);
}

int uavac_control_rollout_plan_ragged_scored_dev(uavac_ctx *ctx, const uavac_vehicle *V, const double *coeffs,
                                                 const int32_t *seg_rows, const int64_t *seg_offsets, const int64_t *row_offsets,
                                                 const double *first_yaw, int max_m, double dt, double *state, int32_t *istate,
                                                 int B, int K, double *state_log, double *cmd_log, const double *aabbs, int n_obs,
                                                 double *score) {
    UAVAC_ENTER(ctx);
    if (int rc = check_score_args(ctx, cmd_log, score)) return rc;
    return rollout_plan(ctx, V, coeffs, seg_rows, true, seg_offsets, row_offsets, nullptr, first_yaw, max_m, dt, state, istate, B, K,
                        state_log, cmd_log, aabbs, n_obs, score);
}

int uavac_control_step_dev(uavac_ctx *ctx, const uavac_vehicle *V, const double *traj, const int64_t *row_offsets,
                           double *state, int32_t *istate, int B) {
    return uavac_control_rollout_dev(ctx, V, traj, row_offsets, state, istate, B, 1, nullptr, nullptr, nullptr, 0);
}

// ---------------------------------------------------------------------------------- control, host
int uavac_state_init(uavac_ctx *ctx, const uavac_vehicle *V, const double *positions, int B, int hover,
                     double *state, int32_t *istate) {
    UAVAC_ENTER(ctx);
    if (B < 1 || !state || !istate) return uavac_fail(ctx, UAVAC_EINVAL, "bad B or null state");
    if (positions && !finite_all(positions, (size_t)B * 3)) return uavac_fail(ctx, UAVAC_ENONFINITE, "non-finite position");
    const size_t ns = (size_t)B * UAVAC_STATE_ROWS, ni = (size_t)B * UAVAC_ISTATE_ROWS;
    double *ds = nullptr, *dp = nullptr;
    int32_t *di = nullptr;
    Scratch s(ctx);
    s.out(&ds, state, ns); s.out(&di, istate, ni);
    if (positions) s.in(&dp, positions, (size_t)B * 3);
    if (int rc = s.commit()) return rc;
    if (int rc = s.upload()) return rc;
    if (int rc = uavac_state_init_dev(ctx, V, dp, B, hover, ds, di)) return rc;
    if (int rc = s.download()) return rc;
    UAVAC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return UAVAC_OK;
}

int uavac_control_rollout(uavac_ctx *ctx, const uavac_vehicle *V, const double *traj, const int64_t *row_offsets,
                          double *state, int32_t *istate, int B, int K, double *state_log, double *cmd_log,
                          const double *aabbs, int n_obs) {
    UAVAC_ENTER(ctx);
    if (B < 1 || K < 0 || !traj || !row_offsets || !state || !istate || n_obs < 0)
        return uavac_fail(ctx, UAVAC_EINVAL, "bad size or null pointer");
    if (row_offsets[0] != 0) return uavac_fail(ctx, UAVAC_EINVAL, "row_offsets must start at 0");
    for (int b = 0; b < B; ++b)
        if (row_offsets[b + 1] < row_offsets[b]) return uavac_fail(ctx, UAVAC_EINVAL, "row_offsets must be non-decreasing");
    const size_t total = (size_t)row_offsets[B];
    if (!finite_all(state, (size_t)B * UAVAC_STATE_ROWS)) return uavac_fail(ctx, UAVAC_ENONFINITE, "non-finite state");
    const size_t ntr = total * UAVAC_TRAJ_COLS, ns = (size_t)B * UAVAC_STATE_ROWS, ni = (size_t)B * UAVAC_ISTATE_ROWS;
    const size_t nsl = state_log ? (size_t)K * 13 * B : 0, ncl = cmd_log ? (size_t)K * UAVAC_CMD_COLS * B : 0;
    const bool obs = aabbs && n_obs > 0;
    double *dtr = nullptr, *ds = nullptr, *dsl = nullptr, *dcl = nullptr, *dab = nullptr;
    int64_t *dro = nullptr;
    int32_t *di = nullptr;
    Scratch s(ctx);
    s.in(&dtr, traj, ntr); s.in(&dro, row_offsets, (size_t)B + 1); s.inout(&ds, state, ns); s.inout(&di, istate, ni);
    if (state_log) s.out(&dsl, state_log, nsl);
    if (cmd_log) s.out(&dcl, cmd_log, ncl);
    if (obs) s.in(&dab, aabbs, (size_t)n_obs * 6);
    if (int rc = s.commit()) return rc;
    if (int rc = s.upload()) return rc;
    {
        const int pitch = ctx->log_pitch;              // the host logs are dense [K][13 | 12][B]
        ctx->log_pitch = 0;
        const int rc = uavac_control_rollout_dev(ctx, V, dtr, dro, ds, di, B, K, dsl, dcl, dab, obs ? n_obs : 0);
        ctx->log_pitch = pitch;
        if (rc) return rc;
    }
    if (int rc = s.download()) return rc;
    UAVAC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return UAVAC_OK;
}

}  // extern "C"
