// What the kernels that walk ONE mission of a batch share (gfx950) -- the plan audit, the snap cost, the delay transform, the obstacle
// scan and, through fleet_clock.h, the fleet's pair kernels.  Each piece is stated once, here:
//   Mission / mission_of        a mission's first segment and segment count, uniform or ragged
//   seek                        the segment of a mission's row, walked forward
//   LaneGroup                   kLanes lanes per mission, 64 / kLanes missions per wavefront: who this lane is
//   group_reduce                one __shfl_xor tree over such a group
//   block_inclusive_scan_256    the workgroup scan behind every per-mission total
//   kMaxClock / clamped_start   the bound of the group clock and the start row inside it
// and, in row_walk.h beside it (included only by the three kernels that walk a mission's sampled rows without writing them: the plan
// audit, the plan demand, the slowdown need):
//   RowWalk / each_row          the walk itself: seek, the 24 coefficients of the row's segment reloaded on a change, the row time
//   nonfinite_probe, stage_cuboids, launch_by_lanes
// Only indexing, the walk and the reductions: every kernel keeps its own arithmetic (and its own contraction mode -- nothing here
// multiplies; row_walk.h multiplies the row time only) and, but for the row walk's coefficients, its own loads.  Two kernels measured slower with these pieces than with their own text and keep it (profiles/NOTES.md
// R17-3): the cost kernel of minsnap_timeopt.hip takes mission_of only, minsnap_first_yaw.hip nothing.
#pragma once

#include "uavac_internal.h"

namespace mission_walk {

constexpr int kMaxClock = 1 << 29;                          // start rows and row totals above this cannot be clocked with int

// A start row outside 0 .. 2^29 cannot be refused by the host: it is clamped (and the caller raises flag 0).
__device__ __forceinline__ int clamped_start(int s) { return s < 0 ? 0 : (s > kMaxClock ? kMaxClock : s); }

// First segment and segment count of mission b: uniform (so == NULL) or ragged, clamped to 1 .. m like every ragged kernel clamps it.
struct Mission {
    long long s0;
    int m;
};
__device__ __forceinline__ Mission mission_of(const int64_t *__restrict__ so, int b, int m_uniform) {
    Mission M;
    if (so) {
        M.s0 = so[b];
        const long long n = so[b + 1] - M.s0;
        M.m = (int)(n < 1 ? 1 : (n > m_uniform ? m_uniform : n));
    } else {
        M.s0 = (long long)b * m_uniform;
        M.m = m_uniform;
    }
    return M;
}

// The segment of a mission's row r -- the first one whose rows reach past r, the last one beyond the mission's end -- walked forward from
// where the lane stood (rows only grow).  Row: int, or long long where the row counts are the caller's and may sum past int.
template <class Row>
__device__ __forceinline__ void seek(const int32_t *__restrict__ rows_of, int mb, Row r, int &s, Row &base, int &cnt) {
    while (s + 1 < mb && r >= base + cnt) { base += cnt; ++s; cnt = rows_of[s]; }
}

// kLanes lanes of a wavefront per mission, 64 / kLanes missions per wavefront, kWaves wavefronts per workgroup: mission b, lane l of its
// group, group g of the wavefront.  A group past the batch's end is not `live`; it shadows the last mission so that what it reads
// exists, and the kernel sees to it that it walks nothing and writes nothing.
template <int kLanes, int kWaves>
struct LaneGroup {
    int b, l, g, shadow;
    bool live;
    __device__ __forceinline__ explicit LaneGroup(int B) {
        const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        g = lane / kLanes;
        l = lane % kLanes;
        b = (blockIdx.x * kWaves + w) * (64 / kLanes) + g;
        live = b < B;
        shadow = live ? b : B - 1;
    }
};

// v combined over the kLanes lanes of a group: xor distances kLanes / 2 .. 1 stay inside the group, and with a commutative op every
// lane of the group ends with the same bits.
template <int kLanes, class T, class Op>
__device__ __forceinline__ T group_reduce(T v, Op op) {
#pragma unroll
    for (int d = kLanes / 2; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d));
    return v;
}
struct Add {
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};

// Inclusive scan of one value per thread over a workgroup of 256 (wsum: 4 shared slots); the scan kernel behind
// uavac_launch_totals_scan joins the workgroups' sums.
__device__ __forceinline__ int64_t block_inclusive_scan_256(int64_t v, int64_t *wsum /* [4] shared */) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    if (lane == 63) wsum[wv] = v;
    __syncthreads();
    int64_t base = 0;
    for (int w = 0; w < wv; ++w) base += wsum[w];
    return v + base;
}

}  // namespace mission_walk
