// What a solved plan's sampled rows would show, per mission, WITHOUT writing one of them (gfx950): the row total, the peaks of the
// velocities and accelerations the control law clips (control_law.h: target climb rate, target horizontal velocity, horizontal
// acceleration command), and per cuboid how many samples lie inside it and which one does first.
//
// Between planning and flying nothing else can say whether a rows-free plan (uavac_minsnap_plan_dev with traj = NULL) is flyable,
// and the obstacle loop (minimum_snap.py:72-93) visits its cuboids in order without re-checking earlier ones: whether the final
// waypoints are clear of ALL of them is not reported by anything.  Getting the same answers from rows means writing 88 bytes per
// sample, one hit-sampler pass per cuboid and reductions over all of it.
//
// Shape: the row walk of row_walk.h -- a group of 16 or 64 lanes per mission (the option "audit_lanes") walks exactly the sampler's
// rows with the sampler's own arithmetic (minsnap_eval_row).  Every lane carries seven running maxima and, per cuboid, a count and a
// first index; after the walk the group reduces them with __shfl_xor: max, integer add and min, all exact and independent of order.
//
// ROUNDING (part of the contract, include/uavac.h): the squares are separately rounded products and sums (no fused multiply-add:
// contraction is off in the function, as in minsnap_yaw.h has_heading), the running maximum is taken of the SQUARES and one
// correctly rounded sqrt comes at the end.  Max and sqrt are monotone, so a peak equals np.sqrt(vx * vx + vy * vy).max() over the
// rows the sampler writes, bit for bit.
//
// fmax drops a NaN operand, so a non-finite sample -- a singular knot system's coefficients are NaN -- is carried as a flag: such a
// mission reports NaN peaks, no hits and first_hit -1.  A singular plan must never look feasible.

#include "uavac_internal.h"
#include "minsnap_eval.h"
#include "row_walk.h"

#include <cmath>
#include <limits>

namespace {

using namespace mission_walk;
constexpr int kWaves = 4;                                   // wavefronts per workgroup
constexpr int kNoHit = 0x7fffffff;                          // "no sample inside" while the minimum is being formed

// The seven squares / signed values a row contributes, rounded as NumPy rounds them.
struct RowPeaks {
    double vxy2, climb, descent, axy2, up, down, v2;
};
__device__ __forceinline__ RowPeaks row_peaks(double vx, double vy, double vz, double ax, double ay, double az) {
#pragma clang fp contract(off)
    RowPeaks p;
    const double xx = vx * vx, yy = vy * vy, zz = vz * vz;
    p.vxy2 = xx + yy;
    p.v2 = p.vxy2 + zz;                                      // (vx * vx + vy * vy) + vz * vz, left to right
    const double aa = ax * ax, bb = ay * ay;
    p.axy2 = aa + bb;
    p.climb = -vz; p.descent = vz;                           // NED: up is negative z
    p.up = -az; p.down = az;
    return p;
}

// kLanes (16 or 64) lanes per mission, 64 / kLanes missions per wavefront.  HITS: cuboids were given.
// Dynamic LDS (HITS only): the cuboids [n_cuboids][6] -- the same for every lane, so a read is one broadcast -- then every lane's
// own count and first index per cuboid, [n_cuboids][threads] i32 each.  They live there and not in registers because the loop over
// the cuboids has a run-time trip count (registers cannot be indexed by it, and unrolled sixteen times the compiler kept all 96
// bounds in registers: one wavefront per SIMD); a lane touches its slots only for a sample that IS inside, which is rare.
template <int kLanes, bool HITS>
__global__ void __launch_bounds__(64 * kWaves) minsnap_audit_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m,
    double dt, const double *__restrict__ cuboids, int n_cuboids, double *__restrict__ audit, int32_t *__restrict__ hit_rows,
    int32_t *__restrict__ first_hit) {
    constexpr int kThreads = 64 * kWaves;
    extern __shared__ double lds[];
    const double *box = lds;                                                      // [n_cuboids][6]
    int *count = reinterpret_cast<int *>(lds + 6 * n_cuboids) + threadIdx.x;      // [n_cuboids][kThreads], this lane's column
    int *first = count + n_cuboids * kThreads;                                    // [n_cuboids][kThreads]
    if (HITS) {
        stage_cuboids<kThreads>(lds, cuboids, n_cuboids);
        for (int q = 0; q < n_cuboids; ++q) { count[q * kThreads] = 0; first[q * kThreads] = kNoHit; }
        __syncthreads();
    }
    const RowWalk<kLanes, kWaves> W(coeffs, seg_rows, seg_offsets, B, m);
    const int b = W.b, l = W.l;
    const bool live = W.live;
    const long long total = W.total, n_rows = W.n_rows;

    const double ninf = -std::numeric_limits<double>::infinity();
    double m_vxy2 = ninf, m_climb = ninf, m_descent = ninf, m_axy2 = ninf, m_up = ninf, m_down = ninf, m_v2 = ninf;
    double bad = 0.0;                                        // becomes NaN with the first non-finite sample

    W.each_row(dt, [&](const double (&c)[24], double t, long long r) {
        double px, py, pz, vx, vy, vz, ax, ay, az;
        minsnap_eval_row<1>(c, t, px, py, pz, vx, vy, vz, ax, ay, az);
        const RowPeaks p = row_peaks(vx, vy, vz, ax, ay, az);
        m_vxy2 = fmax(m_vxy2, p.vxy2); m_climb = fmax(m_climb, p.climb); m_descent = fmax(m_descent, p.descent);
        m_axy2 = fmax(m_axy2, p.axy2); m_up = fmax(m_up, p.up); m_down = fmax(m_down, p.down);
        m_v2 = fmax(m_v2, p.v2);
        bad += nonfinite_probe(px, py, pz, vx, vy, vz, ax, ay, az);
        if (HITS) {
            // inclusive AABB test on the sampled position (minimum_snap.py:327-357), the sampler's own (minsnap_sample.hip)
#pragma nounroll
            for (int q = 0; q < n_cuboids; ++q) {            // (uniform trip count)
                const double *x = box + q * 6;
                const bool in = px >= x[0] && px <= x[1] && py >= x[2] && py <= x[3] && pz >= x[4] && pz <= x[5];
                if (in) {
                    count[q * kThreads] += 1;
                    first[q * kThreads] = min(first[q * kThreads], (int)r);
                }
            }
        }
    });

    // across the group: max, integer add, min -- exact whatever the order
    const auto peak = [](double a, double o) { return fmax(a, o); };
    m_vxy2 = group_reduce<kLanes>(m_vxy2, peak); m_climb = group_reduce<kLanes>(m_climb, peak);
    m_descent = group_reduce<kLanes>(m_descent, peak); m_axy2 = group_reduce<kLanes>(m_axy2, peak);
    m_up = group_reduce<kLanes>(m_up, peak); m_down = group_reduce<kLanes>(m_down, peak);
    m_v2 = group_reduce<kLanes>(m_v2, peak);
    bad = group_reduce<kLanes>(bad, Add());                  // (0 + 0 or NaN: order-free as well)
    const bool finite = bad == 0.0 && n_rows > 0;            // a mission without rows has no peaks either: NaN
    if (HITS) {
        for (int q = 0; q < n_cuboids; ++q) {
            const int n = group_reduce<kLanes>(count[q * kThreads], Add());
            const int f = group_reduce<kLanes>(first[q * kThreads], [](int a, int o) { return min(a, o); });
            if (live && l == 0) {
                hit_rows[(size_t)q * B + b] = finite ? n : 0;
                first_hit[(size_t)q * B + b] = (finite && f != kNoHit) ? f : -1;
            }
        }
    }
    if (live && l == 0) {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        const size_t P = (size_t)B;
        audit[b] = (double)total;
        audit[P + b] = finite ? sqrt(m_vxy2) : nan;
        audit[2 * P + b] = finite ? m_climb : nan;
        audit[3 * P + b] = finite ? m_descent : nan;
        audit[4 * P + b] = finite ? sqrt(m_axy2) : nan;
        audit[5 * P + b] = finite ? m_up : nan;
        audit[6 * P + b] = finite ? m_down : nan;
        audit[7 * P + b] = finite ? sqrt(m_v2) : nan;
    }
}

}  // namespace

int uavac_launch_audit(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                       double dt, const double *cuboids, int n_cuboids, double *audit, int32_t *hit_rows, int32_t *first_hit) {
    const size_t lds = (size_t)n_cuboids * (6 * sizeof(double) + 2 * sizeof(int) * 64 * kWaves);      // 16 cuboids: 33.5 KB
    return launch_by_lanes<kWaves>(ctx, B, [&](auto lanes, dim3 grid, dim3 block) {
        if (n_cuboids > 0)
            hipLaunchKernelGGL((minsnap_audit_kernel<lanes(), true>), grid, block, lds, ctx->stream, coeffs, seg_rows, seg_offsets, B, m, dt,
                               cuboids, n_cuboids, audit, hit_rows, first_hit);
        else
            hipLaunchKernelGGL((minsnap_audit_kernel<lanes(), false>), grid, block, 0, ctx->stream, coeffs, seg_rows, seg_offsets, B, m, dt,
                               cuboids, n_cuboids, audit, hit_rows, first_hit);
    });
}
