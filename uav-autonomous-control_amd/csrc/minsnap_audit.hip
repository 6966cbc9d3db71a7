// What a solved plan's sampled rows would show, per mission, WITHOUT writing one of them (gfx950): the row total, the peaks of the
// velocities and accelerations the control law clips (control_law.h: target climb rate, target horizontal velocity, horizontal
// acceleration command), and per cuboid how many samples lie inside it and which one does first.
//
// Between planning and flying nothing else can say whether a rows-free plan (uavac_minsnap_plan_dev with traj = NULL) is flyable,
// and the obstacle loop (minimum_snap.py:72-93) visits its cuboids in order without re-checking earlier ones: whether the final
// waypoints are clear of ALL of them is not reported by anything.  Getting the same answers from rows means writing 88 bytes per
// sample, one hit-sampler pass per cuboid and reductions over all of it.
//
// Shape of minsnap_first_yaw.hip: a group of lanes per mission walks the mission's rows a group-width at a time with the sampler's
// own arithmetic -- the segment of row r from the row counts (walked forward from where the lane stood: rows only grow), t = (r -
// first row of the segment) * dt, minsnap_eval_row -- no prefix sums, no row buffer.  A lane keeps its segment's 24 coefficients in
// registers and reloads them only when its row enters another segment.  Every lane carries seven running maxima and, per cuboid,
// a count and a first index; after the walk the group reduces them with __shfl_xor: max, integer add and min, all exact and
// independent of order, so the outputs depend neither on the lanes per mission nor on the launch shape or the batch split.
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
#include "mission_walk.h"

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

// 0 when all nine are finite, NaN otherwise (0 * inf and 0 * NaN are NaN; the sum of finite zeros is 0)
__device__ __forceinline__ double nonfinite_probe(double px, double py, double pz, double vx, double vy, double vz, double ax,
                                                  double ay, double az) {
    double z = 0.0 * px;
    z = fma(0.0, py, z); z = fma(0.0, pz, z);
    z = fma(0.0, vx, z); z = fma(0.0, vy, z); z = fma(0.0, vz, z);
    z = fma(0.0, ax, z); z = fma(0.0, ay, z); z = fma(0.0, az, z);
    return z;
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
        for (int i = threadIdx.x; i < n_cuboids * 6; i += kThreads) lds[i] = cuboids[i];
        for (int q = 0; q < n_cuboids; ++q) { count[q * kThreads] = 0; first[q * kThreads] = kNoHit; }
        __syncthreads();
    }
    const LaneGroup<kLanes, kWaves> G(B);                    // (dead groups shadow the last mission, walk nothing and write nothing)
    const int b = G.b, l = G.l;
    const bool live = G.live;
    const Mission M = mission_of(seg_offsets, G.shadow, m);
    const int mb = M.m;
    const int32_t *rows_of = seg_rows + M.s0;
    const double *cm = coeffs + (size_t)M.s0 * 24;

    long long total = 0;                                     // the mission's rows: what the sampler's row offsets give it
    for (int s = 0; s < mb; ++s) total += rows_of[s];
    const long long n_rows = live ? total : 0;

    const double ninf = -std::numeric_limits<double>::infinity();
    double m_vxy2 = ninf, m_climb = ninf, m_descent = ninf, m_axy2 = ninf, m_up = ninf, m_down = ninf, m_v2 = ninf;
    double bad = 0.0;                                        // becomes NaN with the first non-finite sample

    double c[24];                                            // coefficients of the segment this lane stands in
    int s = 0, loaded = -1, cnt = rows_of[0];                // this lane's segment, the one in `c`, its row count
    long long base = 0;                                      // ... and its first row
    for (long long r = l; r < n_rows; r += kLanes) {
        seek(rows_of, mb, r, s, base, cnt);
        if (s != loaded) {
#pragma unroll
            for (int k = 0; k < 24; ++k) c[k] = cm[s * 24 + k];
            loaded = s;
        }
        const double t = (double)(int)(r - base) * dt;
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
    }

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

template <int kLanes>
void launch(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
            const double *cuboids, int n_cuboids, double *audit, int32_t *hit_rows, int32_t *first_hit) {
    const int per_wg = kWaves * (64 / kLanes);
    const dim3 grid((B + per_wg - 1) / per_wg), block(64 * kWaves);
    const size_t lds = (size_t)n_cuboids * (6 * sizeof(double) + 2 * sizeof(int) * 64 * kWaves);      // 16 cuboids: 33.5 KB
    if (n_cuboids > 0)
        hipLaunchKernelGGL((minsnap_audit_kernel<kLanes, true>), grid, block, lds, ctx->stream, coeffs, seg_rows, seg_offsets, B, m, dt,
                           cuboids, n_cuboids, audit, hit_rows, first_hit);
    else
        hipLaunchKernelGGL((minsnap_audit_kernel<kLanes, false>), grid, block, 0, ctx->stream, coeffs, seg_rows, seg_offsets, B, m, dt,
                           cuboids, n_cuboids, audit, hit_rows, first_hit);
}

}  // namespace

int uavac_launch_audit(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                       double dt, const double *cuboids, int n_cuboids, double *audit, int32_t *hit_rows, int32_t *first_hit) {
    if (ctx->audit_lanes == 64) launch<64>(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, cuboids, n_cuboids, audit, hit_rows, first_hit);
    else launch<16>(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, cuboids, n_cuboids, audit, hit_rows, first_hit);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}
