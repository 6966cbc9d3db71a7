// Minimum-snap plans from GIVEN segment durations, the snap cost of a plan, and the optimisation of the durations at a fixed total
// time (gfx950) -- the second half of the minimum-snap method (Mellinger & Kumar 2011: minimise over the coefficients AND over the
// segment times).  Every other plan of the engine takes its durations from one rule, upstream's T_s = |leg_s| / velocity [* 1.5 on the
// first and last leg] (row_counts_kernel, minsnap_solve.hip); nothing here touches that rule or the kernels that implement it.
//
//   row_counts_t_kernel     seg_rows = ceil(T / dt) from durations that exist already: the tail of row_counts_kernel, the same single
//                           IEEE division and ceil, so seg_rows == len(np.arange(0, T, dt)); the offsets come from the existing scan
//   plan_t_commit_kernel    the all-or-nothing commit of the chain with a row capacity (durations are an input: nothing to commit)
//   minsnap_cost_kernel     J_b = sum over segments and axes of the integral of snap^2 over [0, T_s] -- upstream's c^T H c
//                           (_create_snap_cost_matrix, no 1/2) -- by four-point Gauss-Legendre quadrature, which is exact for the
//                           degree-6 integrand and sums non-negative terms only (c^T H c cancels T^(r+c-7) terms of both signs)
//   timeopt_*_kernel        the bookkeeping of the optimisation loop (include/uavac.h uavac_minsnap_optimize_times_dev): the probe and
//                           candidate durations, the projected gradient, the selection.  The solves in between are the existing
//                           dispatcher's (uavac_launch_coeff_solve) on EXPANDED batches: n copies of every mission of a chunk, copy k
//                           of mission j next to copy k - 1, with their own waypoint copies and (ragged) segment offsets in ctx scratch.
//
// Everything is per mission and in a fixed order: results depend neither on the launch shape nor on how a batch is split or chunked.
// Contraction is off in every kernel of this file: each step is one rounded IEEE operation.

#include "uavac_internal.h"
#include "uavac_scratch.h"
#include "mission_walk.h"

#include <cmath>
#include <limits>

namespace {

constexpr int kThreads = 256;

using namespace mission_walk;                               // Mission and the workgroup scan

// ------------------------------------------------------------------------------------------ rows from given durations
// One thread per mission, 256 missions per workgroup, which also leaves the tile's row total (as row_counts_kernel does).  A duration
// that is not positive and finite raises flag 0 and leaves its MISSION without rows: what a bad per-mission speed does.
template <bool RAGGED>
__global__ void __launch_bounds__(kThreads) row_counts_t_kernel(const double *__restrict__ times, int B, int m_uniform, double dt,
                                                                int32_t *__restrict__ seg_rows, int32_t *__restrict__ totals,
                                                                int64_t *__restrict__ tile_sum, int32_t *__restrict__ flags,
                                                                const int64_t *__restrict__ seg_offsets) {
#pragma clang fp contract(off)
    __shared__ int64_t wsum[4];
    const int b = blockIdx.x * kThreads + threadIdx.x;
    int64_t total = 0;
    if (b < B) {
        const Mission M = mission_of(RAGGED ? seg_offsets : nullptr, b, m_uniform);
        bool bad = false;
        if (RAGGED) {
            const int64_t mb = seg_offsets[b + 1] - seg_offsets[b];
            bad = mb < 1 || mb > m_uniform;
        }
        const double *tm = times + M.s0;
        int32_t *rows_of = seg_rows + M.s0;
        bool bad_time = false;
        for (int s = 0; s < M.m; ++s) {
            const double T = tm[s];
            bad_time = bad_time || !(T > 0.0 && isfinite(T));
        }
        for (int s = 0; s < M.m; ++s) {
            const double q = ceil(tm[s] / dt);
            int rows = (isfinite(q) && q > 0.0 && q < 2.0e9) ? (int)q : 0;
            if (bad_time) rows = 0;
            rows_of[s] = rows;
            total += rows;
        }
        if (total > 2147483647LL) { atomicOr(&flags[3], 1); total = 0; }     // a mission's rows are indexed with int
        totals[b] = (int32_t)total;
        if (bad || bad_time) atomicOr(&flags[0], 1);
    }
    const int64_t inc = block_inclusive_scan_256(total, wsum);
    if (threadIdx.x == kThreads - 1) tile_sum[blockIdx.x] = inc;
}

// seg_rows / row_offsets from scratch into the caller's arrays unless the plan outgrows the caller's row buffer (the sampler then
// raises flag 2, the solve does nothing): the all-or-nothing commit of uavac_minsnap_plan_dev for a chain whose durations are given.
__global__ void __launch_bounds__(kThreads) plan_t_commit_kernel(const int32_t *__restrict__ seg_rows_s,
                                                                 const int64_t *__restrict__ row_offsets_s, int B, int m,
                                                                 const int64_t *__restrict__ seg_offsets, int64_t capacity_rows,
                                                                 int32_t *__restrict__ seg_rows, int64_t *__restrict__ row_offsets) {
    if (row_offsets_s[B] > capacity_rows) return;
    size_t n_seg = (size_t)B * m;
    if (seg_offsets) {
        const int64_t S = seg_offsets[B];
        n_seg = S < 0 ? 0 : ((size_t)S < n_seg ? (size_t)S : n_seg);
    }
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n_seg; i += stride) seg_rows[i] = seg_rows_s[i];
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i <= (size_t)B; i += stride) row_offsets[i] = row_offsets_s[i];
}

// ------------------------------------------------------------------------------------------ the snap cost
// kCostLanes lanes of a wavefront per mission, four missions per wavefront (the audit's shape): lane l takes segments l, l + 16, ...
// in that order, the 16 partial sums meet in a fixed xor tree (8, 4, 2, 1: a + b == b + a, so every lane of the group holds the same
// bits).  A mission's 16 consecutive segments are 3 KB of consecutive coefficients, read as 16 runs of 192 B.
// Per segment: half = 0.5 T; for the four nodes x_i in ascending order t = half + half * x_i, snap per axis by Horner on
// (840 c7, 360 c6, 120 c5, 24 c4) -- polynom(8, 4, t) @ c -- q = (sx sx + sy sy) + sz sz, seg += (half * w_i) * q.
// A non-finite coefficient or duration anywhere in the mission gives NaN (0 * x summed beside the cost: inf^2 alone would give inf).
constexpr int kCostLanes = 16;
constexpr int kCostWaves = 4;
constexpr double kGlX0 = 0.8611363115940526, kGlX1 = 0.3399810435848563;
constexpr double kGlW0 = 0.3478548451374538, kGlW1 = 0.6521451548625461;

__device__ __forceinline__ double snap_sq(const double (&c)[24], double t) {
#pragma clang fp contract(off)
    double q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double s = 840.0 * c[21 + a];
        s = s * t + 360.0 * c[18 + a];
        s = s * t + 120.0 * c[15 + a];
        s = s * t + 24.0 * c[12 + a];
        q[a] = s * s;
    }
    return (q[0] + q[1]) + q[2];
}

__global__ void __launch_bounds__(64 * kCostWaves) minsnap_cost_kernel(const double *__restrict__ coeffs, const double *__restrict__ times,
                                                                       const int64_t *__restrict__ seg_offsets, int B, int m,
                                                                       double *__restrict__ cost) {
#pragma clang fp contract(off)
    constexpr int kPerWave = 64 / kCostLanes;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = lane / kCostLanes, l = lane % kCostLanes;
    const int b = (blockIdx.x * kCostWaves + w) * kPerWave + g;
    const bool live = b < B;
    const Mission M = mission_of(seg_offsets, live ? b : B - 1, m);
    const int mb = live ? M.m : 0;                           // (dead groups walk nothing and write nothing)
    const double *cm = coeffs + (size_t)M.s0 * 24;
    const double *tm = times + M.s0;
    double part = 0.0, bad = 0.0;
    for (int s = l; s < mb; s += kCostLanes) {
        double c[24];
#pragma unroll
        for (int k = 0; k < 24; ++k) c[k] = cm[(size_t)s * 24 + k];
        const double T = tm[s];
        double z = 0.0 * T;
#pragma unroll
        for (int k = 0; k < 24; ++k) z = z + 0.0 * c[k];
        bad = bad + z;
        const double half = 0.5 * T;
        double seg = (half * kGlW0) * snap_sq(c, half + half * -kGlX0);
        seg = seg + (half * kGlW1) * snap_sq(c, half + half * -kGlX1);
        seg = seg + (half * kGlW1) * snap_sq(c, half + half * kGlX1);
        seg = seg + (half * kGlW0) * snap_sq(c, half + half * kGlX0);
        part = part + seg;
    }
#pragma unroll
    for (int d = kCostLanes / 2; d >= 1; d >>= 1) {
        part = part + __shfl_xor(part, d);
        bad = bad + __shfl_xor(bad, d);
    }
    if (live && l == 0) cost[b] = part + bad;
}

// ------------------------------------------------------------------------------------------ the optimisation loop's bookkeeping
// A CHUNK is missions b0 .. b0 + Bc - 1 of the batch; j counts inside it.  An EXPANDED batch holds n copies of every mission of the
// chunk: virtual mission v = j * n + k is copy k of mission j, its first segment is segment n * (s0_j - s0_chunk) + k * m_j of the
// expanded arrays, its first waypoint is waypoint (that + v): for a uniform chunk the expanded batch is uniform again, for a ragged
// one its offsets are seg_offsets_x [Bc * n + 1].  Per-mission state of the loop lives in scratch: J, alpha, total, min(T0).
struct Chunk {
    const int64_t *so;     // the batch's seg_offsets, or NULL
    int b0, Bc, m;
};
__device__ __forceinline__ long long expanded_first(const Chunk &C, const Mission &M, int n, int k) {
    return (long long)n * (M.s0 - mission_of(C.so, C.b0, C.m).s0) + (long long)k * M.m;
}
__device__ __forceinline__ long long chunk_first(const Chunk &C, const Mission &M) { return M.s0 - mission_of(C.so, C.b0, C.m).s0; }
// The scratch of a chunk holds Bc * m segments per copy.  Offsets that do not ascend by 1 .. m per mission -- a malformed ragged batch,
// which only the device can see -- would point past it: such a mission is left out of every write below (and raises flag 0).
__device__ __forceinline__ bool fits(const Chunk &C, const Mission &M) {
    const long long first = chunk_first(C, M);
    return first >= 0 && first + M.m <= (long long)C.Bc * C.m;
}

// A mission the loop leaves alone, bit for bit: one segment, a first cost that is not finite, or a duration that is not positive.
__device__ __forceinline__ bool frozen(const Mission &M, double J, double min_t0) { return M.m < 2 || !isfinite(J) || !(min_t0 > 0.0); }

// waypoints (and, ragged, segment offsets) of the expanded batch: one thread per virtual mission
__global__ void __launch_bounds__(kThreads) timeopt_expand_kernel(Chunk C, const double *__restrict__ wp, int n, double *__restrict__ wp_x,
                                                                  int64_t *__restrict__ seg_offsets_x) {
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= C.Bc * n) return;
    const int j = v / n, k = v - j * n;
    const Mission M = mission_of(C.so, C.b0 + j, C.m);
    const bool ok = fits(C, M);
    const long long xs = ok ? expanded_first(C, M, n, k) : 0;
    const double *src = wp + (size_t)(M.s0 + C.b0 + j) * 3;
    double *dst = wp_x + (size_t)(xs + v) * 3;
    if (ok)
        for (int i = 0; i < (M.m + 1) * 3; ++i) dst[i] = src[i];
    if (seg_offsets_x) {
        seg_offsets_x[v] = xs;
        if (v == C.Bc * n - 1) seg_offsets_x[v + 1] = xs + M.m;
    }
}

// total = sum(T0) in index order, min(T0) (0 when a duration is not positive and finite), alpha, accepted = 0, and T0 as the chunk's own
// one-copy expanded batch (the first cost is the cost of its solve): one thread per mission
__global__ void __launch_bounds__(kThreads) timeopt_init_kernel(Chunk C, const double *__restrict__ times, double *__restrict__ times_x,
                                                                double *__restrict__ total, double *__restrict__ min_t0,
                                                                double *__restrict__ alpha, int32_t *__restrict__ accepted,
                                                                int32_t *__restrict__ flags) {
#pragma clang fp contract(off)
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= C.Bc) return;
    const Mission M = mission_of(C.so, C.b0 + j, C.m);
    accepted[C.b0 + j] = 0;
    if (!fits(C, M)) {
        total[j] = 0.0; min_t0[j] = 0.0; alpha[j] = 0.0;         // (frozen)
        atomicOr(&flags[0], 1);
        return;
    }
    const double *T = times + M.s0;
    double *out = times_x + chunk_first(C, M);
    double sum = 0.0, mn = std::numeric_limits<double>::infinity();
    bool ok = true;
    for (int i = 0; i < M.m; ++i) {
        const double t = T[i];
        sum = sum + t;
        mn = t < mn ? t : mn;
        ok = ok && t > 0.0 && isfinite(t);
        out[i] = t;
    }
    total[j] = sum;
    min_t0[j] = ok ? mn : 0.0;
    alpha[j] = UAVAC_TIMEOPT_ALPHA0;
}

// probe k of mission j: T + h g_k, g_k = +1 at k and -1 / (m - 1) elsewhere, h = 1e-6 total / m; a frozen mission's copies are T itself.
// One thread per virtual mission of the m-copy expanded batch (copies k >= m_j of a ragged mission are T as well and are never read).
__global__ void __launch_bounds__(kThreads) timeopt_probe_kernel(Chunk C, const double *__restrict__ times, const double *__restrict__ J,
                                                                 const double *__restrict__ total, const double *__restrict__ min_t0,
                                                                 double *__restrict__ times_x) {
#pragma clang fp contract(off)
    const int n = C.m;
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= C.Bc * n) return;
    const int j = v / n, k = v - j * n;
    const Mission M = mission_of(C.so, C.b0 + j, C.m);
    if (!fits(C, M)) return;
    const double *T = times + M.s0;
    double *out = times_x + expanded_first(C, M, n, k);
    const bool probe = !frozen(M, J[j], min_t0[j]) && k < M.m;
    const double h = UAVAC_TIMEOPT_PROBE_STEP * total[j] / (double)M.m;
    const double others = probe ? -1.0 / (double)(M.m - 1) : 0.0;
    for (int i = 0; i < M.m; ++i) {
        double t = T[i];
        if (probe) t = t + h * (i == k ? 1.0 : others);
        out[i] = t;
    }
}

// d_i = (J(T + h g_i) - J) / h; G_k = d_k - (sum_{i != k} d_i) / (m - 1) in index order; D = -G scaled so that max|D| = min(T).
// go [Bc] = 1 where the mission has a direction this iteration.  One thread per mission; d_i is re-read rather than kept (no arrays).
__global__ void __launch_bounds__(kThreads) timeopt_direction_kernel(Chunk C, const double *__restrict__ times, const double *__restrict__ J,
                                                                     const double *__restrict__ total, const double *__restrict__ min_t0,
                                                                     const double *__restrict__ cost_x, double *__restrict__ D,
                                                                     int32_t *__restrict__ go) {
#pragma clang fp contract(off)
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= C.Bc) return;
    const Mission M = mission_of(C.so, C.b0 + j, C.m);
    const double Jj = J[j];
    go[j] = 0;
    if (!fits(C, M) || frozen(M, Jj, min_t0[j])) return;
    const double *T = times + M.s0;
    const double *Jp = cost_x + (size_t)j * C.m;
    double *Dj = D + chunk_first(C, M);
    const double h = UAVAC_TIMEOPT_PROBE_STEP * total[j] / (double)M.m;
    const double m1 = (double)(M.m - 1);
    bool finite = true;
    double mx = 0.0, mn = std::numeric_limits<double>::infinity();
    for (int k = 0; k < M.m; ++k) {
        double others = 0.0;
        for (int i = 0; i < M.m; ++i)
            if (i != k) others = others + (Jp[i] - Jj) / h;
        const double dk = (Jp[k] - Jj) / h;
        finite = finite && isfinite(dk);
        const double Dk = -(dk - others / m1);
        Dj[k] = Dk;
        mx = fmax(mx, fabs(Dk));
        mn = T[k] < mn ? T[k] : mn;
    }
    if (!finite || !(mx > 0.0) || !isfinite(mx)) return;
    const double scale = mn / mx;
    for (int k = 0; k < M.m; ++k) Dj[k] = Dj[k] * scale;
    go[j] = 1;
}

// candidate c of mission j: Tc = T + (alpha 2^-c) D, dropped when min(Tc) < 0.2 min(T0), else scaled back to the total.  valid [Bc][6];
// a dropped candidate (and every candidate of a mission without a direction) is T itself and is never read.  One thread per virtual
// mission of the 6-copy expanded batch.
__global__ void __launch_bounds__(kThreads) timeopt_candidate_kernel(Chunk C, const double *__restrict__ times, const double *__restrict__ total,
                                                                     const double *__restrict__ min_t0, const double *__restrict__ alpha,
                                                                     const double *__restrict__ D, const int32_t *__restrict__ go,
                                                                     double *__restrict__ times_x, int32_t *__restrict__ valid) {
#pragma clang fp contract(off)
    constexpr int n = UAVAC_TIMEOPT_CANDIDATES;
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= C.Bc * n) return;
    const int j = v / n, c = v - j * n;
    const Mission M = mission_of(C.so, C.b0 + j, C.m);
    valid[v] = 0;
    if (!fits(C, M)) return;
    const double *T = times + M.s0;
    const double *Dj = D + chunk_first(C, M);
    double *out = times_x + expanded_first(C, M, n, c);
    const double a = alpha[j] * (1.0 / (double)(1 << c));
    bool ok = go[j] != 0;
    double scale = 1.0;
    if (ok) {
        double mn = std::numeric_limits<double>::infinity(), sum = 0.0;
        for (int i = 0; i < M.m; ++i) {
            const double t = T[i] + a * Dj[i];
            mn = t < mn ? t : mn;
            sum = sum + t;
        }
        ok = mn >= UAVAC_TIMEOPT_FLOOR * min_t0[j];
        scale = total[j] / sum;
    }
    for (int i = 0; i < M.m; ++i) out[i] = ok ? (T[i] + a * Dj[i]) * scale : T[i];
    valid[v] = ok ? 1 : 0;
}

// The candidate with the smallest cost strictly below J (the lowest c on a tie; a NaN never compares below) becomes T and J, accepted
// += 1, alpha = min(0.5, 2 alpha 2^-c); none: alpha *= 2^-6.  A mission without a direction keeps everything.  One thread per mission.
__global__ void __launch_bounds__(kThreads) timeopt_select_kernel(Chunk C, const double *__restrict__ times_x, const double *__restrict__ cost_x,
                                                                  const int32_t *__restrict__ valid, const int32_t *__restrict__ go,
                                                                  double *__restrict__ times, double *__restrict__ J,
                                                                  double *__restrict__ alpha, int32_t *__restrict__ accepted) {
#pragma clang fp contract(off)
    constexpr int n = UAVAC_TIMEOPT_CANDIDATES;
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= C.Bc || !go[j]) return;
    const Mission M = mission_of(C.so, C.b0 + j, C.m);
    double best = J[j];
    int pick = -1;
    for (int c = 0; c < n; ++c) {
        const double Jc = cost_x[(size_t)j * n + c];
        if (valid[(size_t)j * n + c] && Jc < best) { best = Jc; pick = c; }
    }
    if (pick < 0) {
        alpha[j] = alpha[j] * (1.0 / (double)(1 << UAVAC_TIMEOPT_CANDIDATES));
        return;
    }
    const double *src = times_x + expanded_first(C, M, n, pick);
    double *T = times + M.s0;
    for (int i = 0; i < M.m; ++i) T[i] = src[i];
    J[j] = best;
    accepted[C.b0 + j] += 1;
    alpha[j] = fmin(UAVAC_TIMEOPT_ALPHA_MAX, 2.0 * (alpha[j] * (1.0 / (double)(1 << pick))));
}

inline dim3 grid_for(size_t n) { return dim3((unsigned)((n + kThreads - 1) / kThreads)); }

}  // namespace

int uavac_launch_row_counts_t(uavac_ctx *ctx, const double *times, const int64_t *seg_offsets, int B, int m, double dt,
                              int32_t *seg_rows, int64_t *row_offsets) {
    int32_t *totals = nullptr;
    int64_t *tiles = nullptr;
    if (int rc = uavac_ensure_totals(ctx, B, &totals, &tiles)) return rc;
    if (seg_offsets)
        hipLaunchKernelGGL(row_counts_t_kernel<true>, grid_for((size_t)B), dim3(kThreads), 0, ctx->stream, times, B, m, dt, seg_rows, totals,
                           tiles, ctx->d_flags, seg_offsets);
    else
        hipLaunchKernelGGL(row_counts_t_kernel<false>, grid_for((size_t)B), dim3(kThreads), 0, ctx->stream, times, B, m, dt, seg_rows, totals,
                           tiles, ctx->d_flags, seg_offsets);
    UAVAC_HIP(ctx, hipGetLastError());
    return uavac_launch_totals_scan(ctx, B, row_offsets);
}

int uavac_launch_plan_t_commit(uavac_ctx *ctx, const int32_t *seg_rows_s, const int64_t *row_offsets_s, const int64_t *seg_offsets, int B,
                               int m, int64_t capacity_rows, int32_t *seg_rows, int64_t *row_offsets) {
    const size_t blocks = ((size_t)B * m + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(plan_t_commit_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(kThreads), 0, ctx->stream, seg_rows_s,
                       row_offsets_s, B, m, seg_offsets, capacity_rows, seg_rows, row_offsets);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}

int uavac_launch_cost(uavac_ctx *ctx, const double *coeffs, const double *times, const int64_t *seg_offsets, int B, int m, double *cost) {
    const int per_wg = kCostWaves * (64 / kCostLanes);
    hipLaunchKernelGGL(minsnap_cost_kernel, dim3((B + per_wg - 1) / per_wg), dim3(64 * kCostWaves), 0, ctx->stream, coeffs, times,
                       seg_offsets, B, m, cost);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}

// Scratch per mission of a chunk, in bytes, for missions of up to m segments: n = max(m, 6) copies of durations, coefficients and one
// cost; the waypoint copies and offsets of the three expanded batches (1, m and 6 copies); the direction; the loop's state -- and what
// the solve parks per virtual mission in its HBM workspace ([m - 1][28] doubles), which is the ctx's and grows with the batch it sees.
static size_t timeopt_bytes_per_mission(int m) {
    const size_t n = (size_t)(m > UAVAC_TIMEOPT_CANDIDATES ? m : UAVAC_TIMEOPT_CANDIDATES);
    const size_t copies = (size_t)1 + m + UAVAC_TIMEOPT_CANDIDATES;
    return n * ((size_t)m * (8 + 192) + 8 + (size_t)(m > 1 ? m - 1 : 1) * 28 * 8) + copies * ((size_t)(m + 1) * 24 + 8) + (size_t)m * 8 +
           4 * 8 + (size_t)UAVAC_TIMEOPT_CANDIDATES * 4 + 4;
}

int uavac_launch_optimize_times(uavac_ctx *ctx, const double *wp, const int64_t *seg_offsets, int B, int m, double *times, int iterations,
                                double *cost_before, double *cost_after, int32_t *accepted) {
    constexpr int NC = UAVAC_TIMEOPT_CANDIDATES;
    const int n_max = m > NC ? m : NC;
    // The chunk: as many missions as the scratch budget holds (the batch is walked in chunks; missions are independent and the solves
    // split-invariant, so the chunk size never shows in the results), or what option "timeopt_chunk" says.
    int64_t chunk = ctx->timeopt_chunk > 0 ? ctx->timeopt_chunk : (int64_t)(UAVAC_TIMEOPT_SCRATCH_BYTES / timeopt_bytes_per_mission(m));
    if (ctx->timeopt_chunk <= 0 && chunk > 256) chunk &= ~(int64_t)255;
    const int64_t most = ((int64_t)1 << 30) / n_max;                 // (virtual missions are counted with int)
    chunk = chunk < 1 ? 1 : (chunk > most ? most : chunk);
    if (chunk > B) chunk = B;
    const size_t Bc_max = (size_t)chunk, seg_max = Bc_max * m;
    const bool ragged = seg_offsets != nullptr;
    double *wp_1 = nullptr, *wp_p = nullptr, *wp_c = nullptr, *times_x = nullptr, *coeffs_x = nullptr, *cost_x = nullptr, *D = nullptr,
           *J = nullptr, *alpha = nullptr, *total = nullptr, *min_t0 = nullptr;
    int64_t *so_1 = nullptr, *so_p = nullptr, *so_c = nullptr;
    int32_t *valid = nullptr, *go = nullptr;
    Scratch s(ctx);
    s.want(&wp_1, (seg_max + Bc_max) * 3); s.want(&wp_p, (seg_max + Bc_max) * m * 3); s.want(&wp_c, (seg_max + Bc_max) * NC * 3);
    if (ragged) { s.want(&so_1, Bc_max + 1); s.want(&so_p, Bc_max * m + 1); s.want(&so_c, Bc_max * NC + 1); }
    s.want(&times_x, seg_max * n_max); s.want(&coeffs_x, seg_max * n_max * 24); s.want(&cost_x, Bc_max * n_max);
    s.want(&D, seg_max); s.want(&J, Bc_max); s.want(&alpha, Bc_max); s.want(&total, Bc_max); s.want(&min_t0, Bc_max);
    s.want(&valid, Bc_max * NC); s.want(&go, Bc_max);
    if (int rc = s.commit()) return rc;
    // cost of the expanded batch of n copies at times_x -> out [Bc * n]
    auto solve_and_cost = [&](const double *wp_x, const int64_t *so_x, int Bc, int n, double *out) -> int {
        if (int rc = uavac_launch_coeff_solve(ctx, wp_x, times_x, Bc * n, m, coeffs_x, nullptr, so_x)) return rc;
        return uavac_launch_cost(ctx, coeffs_x, times_x, so_x, Bc * n, m, out);
    };
    for (int b0 = 0; b0 < B; b0 += (int)chunk) {
        const int Bc = B - b0 < (int)chunk ? B - b0 : (int)chunk;
        const Chunk C{seg_offsets, b0, Bc, m};
        const dim3 per_mission = grid_for((size_t)Bc), block(kThreads);
        hipLaunchKernelGGL(timeopt_expand_kernel, per_mission, block, 0, ctx->stream, C, wp, 1, wp_1, so_1);
        hipLaunchKernelGGL(timeopt_expand_kernel, grid_for((size_t)Bc * m), block, 0, ctx->stream, C, wp, m, wp_p, so_p);
        hipLaunchKernelGGL(timeopt_expand_kernel, grid_for((size_t)Bc * NC), block, 0, ctx->stream, C, wp, NC, wp_c, so_c);
        hipLaunchKernelGGL(timeopt_init_kernel, per_mission, block, 0, ctx->stream, C, times, times_x, total, min_t0, alpha, accepted,
                           ctx->d_flags);
        UAVAC_HIP(ctx, hipGetLastError());
        if (int rc = solve_and_cost(wp_1, so_1, Bc, 1, J)) return rc;
        UAVAC_HIP(ctx, hipMemcpyAsync(cost_before + b0, J, (size_t)Bc * 8, hipMemcpyDeviceToDevice, ctx->stream));
        for (int it = 0; it < iterations; ++it) {
            hipLaunchKernelGGL(timeopt_probe_kernel, grid_for((size_t)Bc * m), block, 0, ctx->stream, C, times, J, total, min_t0, times_x);
            UAVAC_HIP(ctx, hipGetLastError());
            if (int rc = solve_and_cost(wp_p, so_p, Bc, m, cost_x)) return rc;
            hipLaunchKernelGGL(timeopt_direction_kernel, per_mission, block, 0, ctx->stream, C, times, J, total, min_t0, cost_x, D, go);
            hipLaunchKernelGGL(timeopt_candidate_kernel, grid_for((size_t)Bc * NC), block, 0, ctx->stream, C, times, total, min_t0, alpha, D,
                               go, times_x, valid);
            UAVAC_HIP(ctx, hipGetLastError());
            if (int rc = solve_and_cost(wp_c, so_c, Bc, NC, cost_x)) return rc;
            hipLaunchKernelGGL(timeopt_select_kernel, per_mission, block, 0, ctx->stream, C, times_x, cost_x, valid, go, times, J, alpha,
                               accepted);
            UAVAC_HIP(ctx, hipGetLastError());
        }
        UAVAC_HIP(ctx, hipMemcpyAsync(cost_after + b0, J, (size_t)Bc * 8, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return UAVAC_OK;
}
