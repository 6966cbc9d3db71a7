// Delay as a plan transform (gfx950): the start delays that uavac_minsnap_stagger_dev grants become part of the plan.  A mission with
// start row S > 0 gets a leading HOLD segment -- c0 of its first segment bit for bit, c1 .. c7 = 0, S rows, duration (double)S * dt --
// and keeps its own segments unchanged behind it; a mission with S == 0 is copied as it is.  The result is a ragged plan like any
// other: the sampler writes S hold rows (the position c0, zero velocity and acceleration: every fma of the Horner chain is 0 * t + c)
// followed by the original rows bit for bit, and the ragged plan-fed rollout, the audits and the gathers fly and audit it unchanged.
// The contract is in include/uavac.h (uavac_minsnap_delay_offsets_dev, uavac_minsnap_delay_dev); uav_ac.scoring.delay_rows states it in
// NumPy on sampled rows.
//
//   delay_counts_kernel   per mission (one thread each, 256 per workgroup): its segment count after the transform, m_b + (S_b > 0), and
//                         the workgroup's sum; the scan behind every row-offset table (uavac_launch_totals_scan) makes the offsets
//   minsnap_delay_kernel  the copy.  One thread per 16 bytes of the output's coefficients: twelve threads per segment, (m + 1) segment
//                         slots per mission (the slots past a mission's last segment idle), so that consecutive lanes read and write
//                         consecutive 16-byte pieces; the first thread of a segment also writes its row count and its duration
// A start row outside 0 .. 2^29 cannot be refused by the host: it is clamped and raises sticky flag 0, as in the separation audit.
// Every output has one writer; no atomics but the flag.

#include "uavac_internal.h"
#include "mission_walk.h"

namespace {

using namespace mission_walk;                               // Mission, the clock's bound and the clamped start, the workgroup scan
constexpr int kThreads = 256;
constexpr int kPairs = 12;                                  // 16-byte pieces of a segment's 24 coefficients

__global__ void __launch_bounds__(kThreads) delay_counts_kernel(const int64_t *__restrict__ seg_offsets, int B, int m,
                                                                const int32_t *__restrict__ start_rows, int32_t *__restrict__ totals,
                                                                int64_t *__restrict__ tile_sum, int32_t *__restrict__ flags) {
    __shared__ int64_t wsum[4];
    const int b = blockIdx.x * kThreads + threadIdx.x;
    int64_t total = 0;
    if (b < B) {
        const int s = start_rows[b];
        if (s < 0 || s > kMaxClock) atomicOr(&flags[0], 1);
        total = mission_of(seg_offsets, b, m).m + (clamped_start(s) > 0 ? 1 : 0);
        totals[b] = (int32_t)total;
    }
    const int64_t inc = block_inclusive_scan_256(total, wsum);
    if (threadIdx.x == kThreads - 1) tile_sum[blockIdx.x] = inc;
}

struct alignas(8) Pair {                                    // 16 bytes that need the alignment of a double only
    double a, b;
};

__global__ void __launch_bounds__(kThreads) minsnap_delay_kernel(const double *__restrict__ coeffs, const double *__restrict__ times,
                                                                 const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets,
                                                                 int B, int m, double dt, const int32_t *__restrict__ start_rows,
                                                                 const int64_t *__restrict__ out_seg_offsets, double *__restrict__ out_coeffs,
                                                                 double *__restrict__ out_times, int32_t *__restrict__ out_seg_rows,
                                                                 int32_t *__restrict__ flags) {
    const long long per_mission = (long long)(m + 1) * kPairs, n = (long long)B * per_mission;
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < n; e += (long long)gridDim.x * kThreads) {
        const int b = (int)(e / per_mission), rest = (int)(e - b * per_mission);
        const int s = rest / kPairs, q = rest - s * kPairs; // the mission's output segment and the piece of it
        const Mission M = mission_of(seg_offsets, b, m);
        const int raw = start_rows[b], S = clamped_start(raw);
        const int hold = S > 0 ? 1 : 0;
        if (s >= M.m + hold) continue;
        const long long to = out_seg_offsets[b] + s;
        const bool is_hold = hold && s == 0;
        const long long from = M.s0 + (is_hold ? 0 : s - hold);          // (the hold takes c0 of the mission's first segment)
        Pair v = reinterpret_cast<const Pair *>(coeffs + from * 24)[q];
        if (is_hold) {                                       // c0 = (x, y, z) is the pieces 0 and half of 1; everything else is 0
            if (q == 1) v.b = 0.0;
            if (q > 1) v.a = v.b = 0.0;
        }
        reinterpret_cast<Pair *>(out_coeffs + to * 24)[q] = v;
        if (q == 0) {
            out_seg_rows[to] = is_hold ? S : seg_rows[from];
            if (out_times) out_times[to] = is_hold ? (double)S * dt : times[from];
            if (s == 0 && (raw < 0 || raw > kMaxClock)) atomicOr(&flags[0], 1);
        }
    }
}

}  // namespace

int uavac_launch_delay_offsets(uavac_ctx *ctx, const int64_t *seg_offsets, int B, int m, const int32_t *start_rows, int64_t *out_seg_offsets) {
    int32_t *totals = nullptr;
    int64_t *tiles = nullptr;
    if (int rc = uavac_ensure_totals(ctx, B, &totals, &tiles)) return rc;
    hipLaunchKernelGGL(delay_counts_kernel, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream, seg_offsets, B, m, start_rows,
                       totals, tiles, ctx->d_flags);
    return uavac_launch_totals_scan(ctx, B, out_seg_offsets);
}

int uavac_launch_delay(uavac_ctx *ctx, const double *coeffs, const double *times, const int32_t *seg_rows, const int64_t *seg_offsets, int B,
                       int m, double dt, const int32_t *start_rows, const int64_t *out_seg_offsets, double *out_coeffs, double *out_times,
                       int32_t *out_seg_rows) {
    const long long n = (long long)B * (m + 1) * kPairs;
    const long long wanted = (n + kThreads - 1) / kThreads;
    const int grid = (int)(wanted < 1 << 16 ? wanted : 1 << 16);        // (grid-stride past that)
    hipLaunchKernelGGL(minsnap_delay_kernel, dim3(grid), dim3(kThreads), 0, ctx->stream, coeffs, times, seg_rows, seg_offsets, B, m, dt,
                       start_rows, out_seg_offsets, out_coeffs, out_times, out_seg_rows, ctx->d_flags);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}
