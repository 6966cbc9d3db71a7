// What the kernels that walk ONE mission's SAMPLED ROWS without writing them share (gfx950) -- the plan audit (minsnap_audit.hip), the
// plan demand (minsnap_demand.hip) and the slowdown need (minsnap_need.hip).  Built on the indexing pieces of mission_walk.h; each
// piece is stated once, here:
//   RowWalk / each_row          a group of kLanes lanes per mission walks exactly the sampler's rows, a group-width at a time
//   nonfinite_probe             0 while every value of a row is finite, NaN from the first one that is not
//   stage_cuboids               cuboids[n][6] into the head of dynamic LDS
//   launch_by_lanes             the host side of the option "audit_lanes": the grid, <64> or <16>, the launch error
// The shape: the segment of row r comes from the row counts, walked forward from where the lane stood (rows only grow), t = (r -
// first row of the segment) * dt, no prefix sums, no row buffer.  A lane keeps its segment's 24 coefficients in registers and reloads
// them only when its row enters another segment.  What a kernel makes of a row is its own lambda with its own accumulators; after the
// walk it reduces them over the group (mission_walk.h group_reduce) with operations that are exact and independent of order, so the
// outputs depend neither on the lanes per mission nor on the launch shape or the batch split.
// One kernel measured slower through each_row than with the loop in its own text and keeps it, on RowWalk's members: the plan demand
// (profiles/NOTES.md R20).  It takes every other piece.
// mission_walk.h's rule holds: nothing here multiplies except the row time (and the probe's zeros) -- every kernel keeps its own
// arithmetic and its own contraction mode.
#pragma once

#include "mission_walk.h"

#include <type_traits>

namespace mission_walk {

// Who this lane is and which rows are its own: mission b, lane l of its group, the mission's row total (what the sampler's row offsets
// give it) and the rows this group walks -- none for a group past the batch's end, which shadows the last mission, walks nothing and
// must write nothing (`live`).
template <int kLanes, int kWaves>
struct RowWalk {
    int b, l;
    bool live;
    long long total, n_rows;
    int mb;                                                  // the mission's segments, their row counts and coefficients: what each_row
    const int32_t *rows_of;                                  // walks -- and the plan demand's kernel, which keeps the loop in its own
    const double *cm;                                        // text (profiles/NOTES.md R20)

    __device__ __forceinline__ RowWalk(const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows,
                                       const int64_t *__restrict__ seg_offsets, int B, int m) {
        const LaneGroup<kLanes, kWaves> G(B);
        b = G.b; l = G.l; live = G.live;
        const Mission M = mission_of(seg_offsets, G.shadow, m);
        mb = M.m;
        rows_of = seg_rows + M.s0;
        cm = coeffs + (size_t)M.s0 * 24;
        total = 0;
        for (int s = 0; s < mb; ++s) total += rows_of[s];
        n_rows = live ? total : 0;
    }

    // each(c, t, r) once per row of this lane, rows ascending: c the 24 coefficients of the row's segment, t its time within the
    // segment, r its index within the mission (long long: the row counts are the caller's and may sum past int).
    template <class Each>
    __device__ __forceinline__ void each_row(double dt, Each each) const {
        double c[24];                                        // coefficients of the segment this lane stands in
        int s = 0, loaded = -1, cnt = rows_of[0];            // this lane's segment, the one in `c`, its row count
        long long base = 0;                                  // ... and its first row
        for (long long r = l; r < n_rows; r += kLanes) {
            seek(rows_of, mb, r, s, base, cnt);
            if (s != loaded) {
#pragma unroll
                for (int k = 0; k < 24; ++k) c[k] = cm[s * 24 + k];
                loaded = s;
            }
            each(c, (double)(int)(r - base) * dt, r);
        }
    }
};

// 0 when all the values are finite, NaN otherwise (0 * inf and 0 * NaN are NaN; the sum of finite zeros is 0).  Added up per lane and
// over the group, only `== 0.0` is ever read from it: fmax drops a NaN operand, so a non-finite sample has to be carried as a flag.
template <class... Rest>
__device__ __forceinline__ double nonfinite_probe(double first, Rest... rest) {
    double z = 0.0 * first;
    ((z = fma(0.0, rest, z)), ...);
    return z;
}

// cuboids [n_cuboids][6] into the head of dynamic LDS -- the same for every lane, so a read is one broadcast.  The per-lane slots
// behind them and the __syncthreads() are the kernel's.
template <int kThreads>
__device__ __forceinline__ void stage_cuboids(double *lds, const double *__restrict__ cuboids, int n_cuboids) {
    for (int i = threadIdx.x; i < n_cuboids * 6; i += kThreads) lds[i] = cuboids[i];
}

// 16 or 64 lanes per mission (ctx->audit_lanes): launch(lanes, grid, block) with lanes an std::integral_constant, so that the caller
// names its kernel<lanes()>; 64 / lanes missions per wavefront, kWaves wavefronts per workgroup.
template <int kWaves, class Launch>
int launch_by_lanes(uavac_ctx *ctx, int B, Launch launch) {
    const auto grid = [B](int lanes) { const int per_wg = kWaves * (64 / lanes); return dim3((B + per_wg - 1) / per_wg); };
    if (ctx->audit_lanes == 64) launch(std::integral_constant<int, 64>(), grid(64), dim3(64 * kWaves));
    else launch(std::integral_constant<int, 16>(), grid(16), dim3(64 * kWaves));
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}

}  // namespace mission_walk
