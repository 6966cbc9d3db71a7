// Missions of a plan selected, reordered and merged on the device (gfx950): TAKE gathers missions, ORDER turns priorities into the
// within-group order that a take puts them in.  Together they are what a priority other than the batch index needs -- the plan is
// reordered within its groups, the searches (minsnap_stagger.hip, minsnap_layer.hip) run on it unchanged, the answers are gathered back
// -- and what takes unresolved missions out of a plan and puts re-planned ones back.  The contracts are in include/uavac.h
// (uavac_minsnap_take_offsets_dev, uavac_minsnap_take_dev, uavac_fleet_order_dev); uav_ac.scoring.take_parts and priority_order state
// them in NumPy.
//
//   take_counts_kernel    per OUTPUT mission (one thread each, 256 per workgroup): the segment count of the mission it takes and the
//                         workgroup's sum; the scan behind every row-offset table (uavac_launch_totals_scan) makes the offsets
//   minsnap_take_kernel   the copy, shaped like the delay transform's.  One thread per 16 bytes of the output's coefficients: twelve
//                         threads per segment, m segment slots per output mission (the slots past a mission's last segment idle), so
//                         that consecutive lanes read and write consecutive 16-byte pieces; the first thread of a segment also writes
//                         its row count and its duration, the first thread of a mission its first heading
//   fleet_order_kernel    a counting rank, one thread per mission: its slot is the number of missions of its group that come before
//                         it.  A workgroup's 256 missions walk the priorities of every group they belong to through LDS tiles of
//                         256 keys; a key is the priority as an integer that orders like the rule (-0.0 = +0.0, every NaN last), so
//                         each comparison is exact and the result does not depend on the launch shape
// An index outside 0 .. B - 1 cannot be refused by the host: it is clamped and raises sticky flag 0.  Every output of the take has one
// writer; no atomics but the flag (the order kernel also joins its workgroup's group ranges with two LDS atomics).

#include "uavac_internal.h"
#include "mission_walk.h"
#include "fleet_clock.h"

namespace {

using namespace mission_walk;                               // Mission, mission_of, the workgroup scan
constexpr int kTakeThreads = 256;
constexpr int kPairs = 12;                                  // 16-byte pieces of a segment's 24 coefficients

// The mission an output mission takes: index[i] clamped into 0 .. B - 1 (`bad`: it was outside).
__device__ __forceinline__ int taken(const int32_t *__restrict__ index, int i, int B, bool &bad) {
    const int raw = index[i];
    bad = raw < 0 || raw >= B;
    return raw < 0 ? 0 : (raw >= B ? B - 1 : raw);
}

__global__ void __launch_bounds__(kTakeThreads) take_counts_kernel(const int64_t *__restrict__ seg_offsets, int B, int m,
                                                                   const int32_t *__restrict__ index, int n, int32_t *__restrict__ totals,
                                                                   int64_t *__restrict__ tile_sum, int32_t *__restrict__ flags) {
    __shared__ int64_t wsum[4];
    const int i = blockIdx.x * kTakeThreads + threadIdx.x;
    int64_t total = 0;
    if (i < n) {
        bool bad;
        const int b = taken(index, i, B, bad);
        if (bad) atomicOr(&flags[0], 1);
        total = mission_of(seg_offsets, b, m).m;
        totals[i] = (int32_t)total;
    }
    const int64_t inc = block_inclusive_scan_256(total, wsum);
    if (threadIdx.x == kTakeThreads - 1) tile_sum[blockIdx.x] = inc;
}

struct alignas(8) Pair {                                    // 16 bytes that need the alignment of a double only
    double a, b;
};

__global__ void __launch_bounds__(kTakeThreads) minsnap_take_kernel(const double *__restrict__ coeffs, const double *__restrict__ times,
                                                                    const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets,
                                                                    int B, int m, const double *__restrict__ first_yaw,
                                                                    const int32_t *__restrict__ index, int n_out,
                                                                    const int64_t *__restrict__ out_seg_offsets, double *__restrict__ out_coeffs,
                                                                    double *__restrict__ out_times, int32_t *__restrict__ out_seg_rows,
                                                                    double *__restrict__ out_first_yaw, int32_t *__restrict__ flags) {
    const long long per_mission = (long long)m * kPairs, n = (long long)n_out * per_mission;
    for (long long e = (long long)blockIdx.x * kTakeThreads + threadIdx.x; e < n; e += (long long)gridDim.x * kTakeThreads) {
        const int i = (int)(e / per_mission), rest = (int)(e - i * per_mission);
        const int s = rest / kPairs, q = rest - s * kPairs; // the output mission's segment and the piece of it
        bool bad;
        const int b = taken(index, i, B, bad);
        const Mission M = mission_of(seg_offsets, b, m);
        if (s >= M.m) continue;
        const long long to = out_seg_offsets[i] + s, from = M.s0 + s;
        reinterpret_cast<Pair *>(out_coeffs + to * 24)[q] = reinterpret_cast<const Pair *>(coeffs + from * 24)[q];
        if (q == 0) {
            out_seg_rows[to] = seg_rows[from];
            if (out_times) out_times[to] = times[from];
            if (s == 0) {
                if (out_first_yaw) out_first_yaw[i] = first_yaw[b];
                if (bad) atomicOr(&flags[0], 1);
            }
        }
    }
}

constexpr int kOrderThreads = 256;

// The priority as an integer that orders like the rule: ascending numbers, -0.0 with +0.0, every NaN after +inf.
__device__ __forceinline__ unsigned long long order_key(double p) {
    if (p != p) return ~0ull;
    if (p == 0.0) p = 0.0;                                   // (-0.0 ties with +0.0)
    const unsigned long long u = (unsigned long long)__double_as_longlong(p);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}

// The group that holds mission b: the last group whose first mission is not past b, if b is below that group's end -- with offsets
// that ascend, the only group that can hold it.  Ranges are group_range's, clamped to the batch.
__device__ __forceinline__ bool group_of(const int64_t *__restrict__ group_offsets, int G, int B, int b, int &g0, int &g1) {
    int g = 0;
    if (group_offsets) {
        int lo = 0, hi = G - 1;                              // the last g in 0 .. G - 1 with group_offsets[g] <= b (0 when there is none)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (group_offsets[mid] <= b) lo = mid; else hi = mid - 1;
        }
        g = lo;
    }
    fleet::group_range(group_offsets, g, B, g0, g1);
    return b >= g0 && b < g1;
}

__global__ void __launch_bounds__(kOrderThreads) fleet_order_kernel(const double *__restrict__ priority,
                                                                    const int64_t *__restrict__ group_offsets, int G, int B,
                                                                    int32_t *__restrict__ order, int32_t *__restrict__ rank) {
    __shared__ unsigned long long keys[kOrderThreads];
    __shared__ int span[2];                                  // the missions that this workgroup's groups cover: [span[0], span[1])
    const int b = blockIdx.x * kOrderThreads + threadIdx.x;
    if (threadIdx.x == 0) { span[0] = B; span[1] = 0; }
    __syncthreads();
    int g0 = 0, g1 = 0;
    unsigned long long kb = 0;
    bool held = false;
    if (b < B) {
        held = group_of(group_offsets, G, B, b, g0, g1);
        if (held) {
            kb = order_key(priority[b]);
            atomicMin(&span[0], g0);
            atomicMax(&span[1], g1);
        } else {
            g0 = g1 = 0;
        }
    }
    __syncthreads();
    const int lo = span[0], hi = span[1];                    // (uniform)
    int slot = 0;
    for (int t0 = lo; t0 < hi; t0 += kOrderThreads) {
        const int j = t0 + threadIdx.x;
        keys[threadIdx.x] = j < hi ? order_key(priority[j]) : ~0ull;
        __syncthreads();
        const int j0 = max(g0, t0), j1 = min(g1, t0 + kOrderThreads);
        for (int jj = j0; jj < j1; ++jj) {
            const unsigned long long kj = keys[jj - t0];
            slot += (kj < kb || (kj == kb && jj < b)) ? 1 : 0;
        }
        __syncthreads();
    }
    if (b < B) {
        const int at = held ? g0 + slot : b;                 // (slot < g1 - g0: the mission does not come before itself)
        order[at] = b;
        rank[b] = at;
    }
}

}  // namespace

int uavac_launch_take_offsets(uavac_ctx *ctx, const int64_t *seg_offsets, int B, int m, const int32_t *index, int n, int64_t *out_seg_offsets) {
    int32_t *totals = nullptr;
    int64_t *tiles = nullptr;
    if (int rc = uavac_ensure_totals(ctx, n, &totals, &tiles)) return rc;
    hipLaunchKernelGGL(take_counts_kernel, dim3((n + kTakeThreads - 1) / kTakeThreads), dim3(kTakeThreads), 0, ctx->stream, seg_offsets, B, m,
                       index, n, totals, tiles, ctx->d_flags);
    return uavac_launch_totals_scan(ctx, n, out_seg_offsets);
}

int uavac_launch_take(uavac_ctx *ctx, const double *coeffs, const double *times, const int32_t *seg_rows, const int64_t *seg_offsets, int B,
                      int m, const double *first_yaw, const int32_t *index, int n, const int64_t *out_seg_offsets, double *out_coeffs,
                      double *out_times, int32_t *out_seg_rows, double *out_first_yaw) {
    const long long pieces = (long long)n * m * kPairs;
    const long long wanted = (pieces + kTakeThreads - 1) / kTakeThreads;
    const int grid = (int)(wanted < 1 << 16 ? wanted : 1 << 16);        // (grid-stride past that)
    hipLaunchKernelGGL(minsnap_take_kernel, dim3(grid), dim3(kTakeThreads), 0, ctx->stream, coeffs, times, seg_rows, seg_offsets, B, m,
                       first_yaw, index, n, out_seg_offsets, out_coeffs, out_times, out_seg_rows, out_first_yaw, ctx->d_flags);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}

int uavac_launch_fleet_order(uavac_ctx *ctx, const double *priority, const int64_t *group_offsets, int G, int B, int32_t *order,
                             int32_t *rank) {
    hipLaunchKernelGGL(fleet_order_kernel, dim3((B + kOrderThreads - 1) / kOrderThreads), dim3(kOrderThreads), 0, ctx->stream, priority,
                       group_offsets, G, B, order, rank);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}
