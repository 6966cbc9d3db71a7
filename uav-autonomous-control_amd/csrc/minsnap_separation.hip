// The fleet's audit against itself (gfx950): for every mission of a group that shares an airspace, the closest approach to any other
// mission of the group -- how near, to whom, at which row of the group's clock --, how many others come inside a protection radius and
// when the first one does.  From coefficients and row counts alone, like the plan audit (minsnap_audit.hip): no row is written, nothing
// is read back.  The contract -- the clock, the groups, the excluded missions, rounding and ties -- is in include/uavac.h
// (uavac_minsnap_separation_dev); uav_ac.scoring.separation_from_rows states it in NumPy on sampled rows, and the results are the same bits.
//
// Three launches on the ctx stream:
//   separation_prepass_kernel   per mission: fleet_clock.h's pre-pass and nothing else -- the row total N (0: EXCLUDED) and the clamped
//                               start row, in ctx scratch
//   minsnap_separation_kernel   the pairs: the sweep that pair_sweep.h describes, with positions walked from the coefficients and the
//                               full record kept -- WRITTEN OUT here, the one pair kernel that is not an instantiation of that
//                               template: as `sweep<Planned, Record>` the compiler scheduled its pair loop differently and the audit
//                               of 4 096 missions in one group took 1.003 x the time.  A change to the sweep's group loop,
//                               tile loop or barriers belongs in both places.  Per mission and share of its window one partial record
//                               in scratch: minimum (d^2, row, partner), conflicts, first row with anybody inside, and the partners
//                               compared: everybody else of the group who takes part
//   separation_merge_kernel     per mission: the P partial records merged the same way, one correctly rounded sqrt, the sentinels
// Every reduction is a lexicographic minimum, an integer sum over disjoint partners, an OR or an integer minimum: exact and independent
// of order, so the outputs depend neither on P, nor on the tile or chunk sizes, nor on what else is in the batch; each output has one
// writer and there are no atomics but the sticky flag.  The price is the factor 2 of not using d(i, j) = d(j, i).
// The reduction itself -- the pair loop of a row, the order, the meeting of the waves, the merge of the partial records, the shares per
// window -- is in separation_reduce.h; the clock -- a mission's segments, the pre-pass, the walk, the group clamp -- in fleet_clock.h,
// shared with the two searches that act on this audit's verdict (fleet_search.h).
//
// ROUNDING (part of the contract): positions by the sampler's fma chain (minsnap_eval_pos), the distance WITHOUT contraction: dx = xi -
// xj, ..., d^2 = (dx dx + dy dy) + dz dz, each product and sum rounded on its own.

#include "pair_sweep.h"
#include "uavac_scratch.h"

#include <cmath>
#include <limits>

namespace {

using namespace pair_sweep;                                 // the sweep and, through it, the clock, the pre-pass and sepred's tile and reduction

// ------------------------------------------------------------------------------------------------------------------ pre-pass
__global__ void __launch_bounds__(kThreads) separation_prepass_kernel(const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows,
                                                                      const int64_t *__restrict__ seg_offsets, int B, int m,
                                                                      const int32_t *__restrict__ start_rows, int32_t *__restrict__ n_rows,
                                                                      int32_t *__restrict__ start, int32_t *__restrict__ flags) {
    int b, s;                                                // (the audit keeps no record of its own for a mission)
    prepass_mission(coeffs, seg_rows, seg_offsets, B, m, start_rows, n_rows, start, flags, b, s);
}

// ------------------------------------------------------------------------------------------------------------------ the pairs
__global__ void __launch_bounds__(kThreads, 3) minsnap_separation_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
    const int64_t *__restrict__ group_offsets, int G, const int32_t *__restrict__ n_rows, const int32_t *__restrict__ start, double r2,
    double *__restrict__ part_d2, int32_t *__restrict__ part_i) {
    __shared__ double tile[kWaves * kRegion];
    const double inf = std::numeric_limits<double>::infinity();
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int P = gridDim.y, p = blockIdx.y;
    const int w0 = blockIdx.x * kTile, w1 = w0 + kTile;      // the window of missions this workgroup owns
    const int b = w0 + lane;
    const bool live = b < B;
    const int bb = live ? b : B - 1;
    const Mission Mi = mission_of(seg_offsets, bb, m);
    const int32_t *irows = seg_rows + Mi.s0;
    const double *icm = coeffs + (size_t)Mi.s0 * 24;
    const int ni = n_rows[bb], si = start[bb];
    double *mine = tile + w * kRegion;                       // this wavefront's quarter of the tile

    int g = 0;                                               // the group that holds mission w0: the last one that starts at or before it
    if (group_offsets) {
        int lo = 0, hi = G;
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (group_offsets[mid] <= w0) lo = mid; else hi = mid;
        }
        g = lo;
    }
    for (; g < G; ++g) {                                     // (uniform: every thread of the workgroup sees the same groups)
        int g0, g1;
        group_range(group_offsets, g, B, g0, g1);
        if (g0 >= w1 || g0 >= B) break;
        if (g1 <= w0 || g1 == g0) continue;
        const bool act = live && b >= g0 && b < g1;

        // the group's horizon and how many of its missions take part
        int h = 0, cnt = 0;
        for (int j = g0 + (int)threadIdx.x; j < g1; j += kThreads) {
            const int n = n_rows[j];
            if (n > 0) { h = max(h, start[j] + n); ++cnt; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { h = max(h, __shfl_xor(h, d)); cnt += __shfl_xor(cnt, d); }
        int *meet = reinterpret_cast<int *>(tile);
        if (lane == 0) { meet[2 * w] = h; meet[2 * w + 1] = cnt; }
        __syncthreads();
        int H = 0, n_in = 0;
#pragma unroll
        for (int v = 0; v < kWaves; ++v) { H = max(H, meet[2 * v]); n_in += meet[2 * v + 1]; }
        __syncthreads();

        double gb = inf;                                     // the group's results so far (held by wavefront 0)
        int gk = kNone, gj = kNone, gconf = 0, gfirst = kNone;
        const int n_tiles = (g1 - g0 + kTile - 1) / kTile;
        for (int t = n_in >= 2 ? p : n_tiles; t < n_tiles; t += P) {
            const int j0 = g0 + t * kTile;
            const bool jvalid = j0 + lane < g1;
            const int jb = jvalid ? j0 + lane : g1 - 1;
            const Mission Mj = mission_of(seg_offsets, jb, m);
            const int32_t *jrows = seg_rows + Mj.s0;
            const double *jcm = coeffs + (size_t)Mj.s0 * 24;
            const int nj = jvalid ? n_rows[jb] : 0, sj = start[jb];
            int js = 0, jbase = 0, jcnt = jrows[0];
            int is = 0, ibase = 0, icnt = irows[0];
            const int selfjj = b - j0;
            const bool self_tile = j0 < w1 && j0 + kTile > w0;
            double tb = inf;                                 // this wavefront's results of the tile
            int tk = kNone, tj = kNone, tfirst = kNone;
            unsigned long long mask = 0;
            for (int k0 = w * kRows; k0 < H; k0 += kChunk) {
                // the j-tile's positions at this wavefront's rows of the chunk, then the lane's own against them (a wavefront reads only
                // its own quarter)
                clock_walk_to_tile<false>(mine, lane, jrows, jcm, Mj.m, nj, sj, k0, H, dt, js, jbase, jcnt, AsPlanned{});
                lds_wave_fence();
                clock_walk<false>(irows, icm, Mi.m, ni, si, k0, H, dt, is, ibase, icnt, AsPlanned{}, [&](int r, int k, double xi, double yi, double zi) {
                    double rm = inf;
                    int rkey = 0;
                    if (self_tile) pair_row<true>(mine + r * kTile * 3, xi, yi, zi, r2, selfjj, rm, rkey, mask);
                    else pair_row<false>(mine + r * kTile * 3, xi, yi, zi, r2, selfjj, rm, rkey, mask);
                    if (rm < tb) { tb = rm; tk = k; tj = j0 + rkey; }
                    if (rm < r2) tfirst = min(tfirst, k);
                });
                lds_wave_fence();
            }
            // the four wavefronts meet: 1 .. 3 leave their results in their quarters, wavefront 0 merges
            if (w != 0) sep_waves_leave(mine, lane, tb, tk, tj, mask, tfirst);
            __syncthreads();
            if (w == 0) {
                sep_waves_meet(tile, lane, tb, tk, tj, mask, tfirst);
                gconf += __popcll(mask);
                if (lex_less(tb, tk, tj, gb, gk, gj)) { gb = tb; gk = tk; gj = tj; }
                gfirst = min(gfirst, tfirst);
            }
            __syncthreads();
        }
        // one partial record per mission and share p (an excluded mission's is ignored); its fifth row: the partners that took part
        if (w == 0 && act) sep_leave_partial(part_d2, part_i, p, b, B, gb, gj, gk, gconf, gfirst, n_in - 1);
    }
}

// ------------------------------------------------------------------------------------------------------------------ the merge
__global__ void __launch_bounds__(kThreads) separation_merge_kernel(const int32_t *__restrict__ n_rows, int B, int P,
                                                                    const double *__restrict__ part_d2, const int32_t *__restrict__ part_i,
                                                                    double *__restrict__ sep, int32_t *__restrict__ isep) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    const size_t Bs = (size_t)B;
    if (n_rows[b] == 0) {                                    // excluded: compared with nobody, and nobody with it
        sep[b] = std::numeric_limits<double>::quiet_NaN();
        isep[b] = -1; isep[Bs + b] = -1; isep[2 * Bs + b] = 0; isep[3 * Bs + b] = -1; isep[4 * Bs + b] = 0;
        return;
    }
    double d;
    int k, j, conf, first;
    sep_merge_partials(part_d2, part_i, P, b, B, d, k, j, conf, first);
    sep_write(sep, isep, b, B, d, k, j, conf, first, part_i[4 * Bs + b]);      // (compared: the same in every share)
}

}  // namespace

int uavac_launch_separation(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                            const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, double *sep, int32_t *isep) {
    int windows, P;
    sep_shares(ctx, B, group_offsets, G, windows, P);
    const size_t Bs = (size_t)B;
    int32_t *n_rows = nullptr, *start = nullptr, *part_i = nullptr;
    double *part_d2 = nullptr;
    Scratch s(ctx);
    s.want(&n_rows, Bs); s.want(&start, Bs);
    s.want(&part_d2, P * Bs); s.want(&part_i, P * 5 * Bs);
    if (int rc = s.commit()) return rc;
    hipLaunchKernelGGL(separation_prepass_kernel, dim3((B + kPreMissions - 1) / kPreMissions), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows,
                       seg_offsets, B, m, start_rows, n_rows, start, ctx->d_flags);
    hipLaunchKernelGGL(minsnap_separation_kernel, dim3(windows, P), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows, seg_offsets, B, m, dt,
                       group_offsets, group_offsets ? G : 1, n_rows, start, radius * radius, part_d2, part_i);
    hipLaunchKernelGGL(separation_merge_kernel, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream, n_rows, B, P, part_d2,
                       part_i, sep, isep);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}
