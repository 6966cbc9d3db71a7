// The CROSS audit (gfx950): every mission of a plan against the missions of ANOTHER plan -- committed traffic -- of its group, and against
// nobody else: how near the closest traffic mission comes, which one and at which row of the shared clock, how many come inside the
// protection radius and when the first one does.  From coefficients and row counts alone; no row is written, nothing is read back.
// The contract is in include/uavac.h (uavac_minsnap_separation_against_dev); uav_ac.scoring.separation_against_rows states it in NumPy
// on sampled rows, and the results are the same bits.
//
// Four launches on the ctx stream:
//   against_prepass_kernel      fleet_clock.h's pre-pass, once on the plan and once on the traffic: row totals (0: EXCLUDED) and clamped
//                               starts in ctx scratch
//   separation_against_kernel   the pairs, in the loop nest of pair_sweep.h: a workgroup owns a window of 64 plan missions, one per lane
//                               (i), visits every group that reaches into the window, walks the TRAFFIC of that group in j-tiles of 64
//                               staged in LDS and the group's clock in chunks of 32 rows, wave w taking rows 8 w .. 8 w + 7.  The group's
//                               horizon covers both sides.  No lane is its own partner here, so no entry is masked.  Per mission and share
//                               of its window one partial record; its fifth row is the included traffic of the group
//   against_merge_kernel        per mission: the P partial records merged, one correctly rounded sqrt, the sentinels
// The arithmetic, the order (d^2, row, partner), the meeting of the waves and the merge are separation_reduce.h's, the clock is
// fleet_clock.h's: every reduction is exact and independent of order, so the outputs depend neither on P nor on the tile or chunk sizes.

#include "fleet_clock.h"
#include "uavac_scratch.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace {

using namespace fleet;

__global__ void __launch_bounds__(kThreads) against_prepass_kernel(const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows,
                                                                   const int64_t *__restrict__ seg_offsets, int B, int m,
                                                                   const int32_t *__restrict__ start_rows, int32_t *__restrict__ n_rows,
                                                                   int32_t *__restrict__ start, int32_t *__restrict__ flags) {
    int b, s;
    prepass_mission(coeffs, seg_rows, seg_offsets, B, m, start_rows, n_rows, start, flags, b, s);
}

// the latest end and the number of the included missions [g0, g1) of one side (two barriers: `meet` is the meeting place)
__device__ __forceinline__ void side_of_group(int *meet, int lane, int w, int g0, int g1, const int32_t *__restrict__ n_rows,
                                              const int32_t *__restrict__ start, int &H, int &n_in) {
    int h = 0, cnt = 0;
    for (int j = g0 + (int)threadIdx.x; j < g1; j += kThreads) {
        const int n = n_rows[j];
        if (n > 0) { h = max(h, start[j] + n); ++cnt; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { h = max(h, __shfl_xor(h, d)); cnt += __shfl_xor(cnt, d); }
    if (lane == 0) { meet[2 * w] = h; meet[2 * w + 1] = cnt; }
    __syncthreads();
    H = 0; n_in = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) { H = max(H, meet[2 * v]); n_in += meet[2 * v + 1]; }
    __syncthreads();
}

__global__ void __launch_bounds__(kThreads, 3) separation_against_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
    const int64_t *__restrict__ group_offsets, int G, const int32_t *__restrict__ n_rows, const int32_t *__restrict__ start,
    const double *__restrict__ t_coeffs, const int32_t *__restrict__ t_seg_rows, const int64_t *__restrict__ t_seg_offsets, int Bt, int mt,
    const int64_t *__restrict__ t_group_offsets, const int32_t *__restrict__ t_n_rows, const int32_t *__restrict__ t_start, double r2,
    double *__restrict__ part_d2, int32_t *__restrict__ part_i) {
    __shared__ double tile[kWaves * kRegion];
    const double inf = std::numeric_limits<double>::infinity();
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int P = gridDim.y, p = blockIdx.y;
    const int w0 = blockIdx.x * kTile, w1 = w0 + kTile;      // the window of plan missions this workgroup owns
    const int b = w0 + lane;
    const bool live = b < B;
    const int bb = live ? b : B - 1;
    const Mission Mi = mission_of(seg_offsets, bb, m);
    const int32_t *irows = seg_rows + Mi.s0;
    const double *icm = coeffs + (size_t)Mi.s0 * 24;
    const int ni = n_rows[bb], si = start[bb];
    double *mine = tile + w * kRegion;                       // this wavefront's quarter of the tile
    int *meet = reinterpret_cast<int *>(tile);

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
        int g0, g1, t0, t1;
        group_range(group_offsets, g, B, g0, g1);
        if (g0 >= w1 || g0 >= B) break;
        if (g1 <= w0 || g1 == g0) continue;
        group_range(t_group_offsets, g, Bt, t0, t1);         // the partners: the traffic of the same group
        const bool act = live && b >= g0 && b < g1;

        int H, n_own, h_traffic, n_in;                       // the group's horizon over both sides; the included traffic
        side_of_group(meet, lane, w, g0, g1, n_rows, start, H, n_own);
        side_of_group(meet, lane, w, t0, t1, t_n_rows, t_start, h_traffic, n_in);
        H = max(H, h_traffic);

        double gb = inf;                                     // the group's results so far (held by wavefront 0)
        int gk = kNone, gj = kNone, gconf = 0, gfirst = kNone;
        const int n_tiles = (t1 - t0 + kTile - 1) / kTile;
        for (int t = n_in >= 1 ? p : n_tiles; t < n_tiles; t += P) {
            const int j0 = t0 + t * kTile;
            const bool jvalid = j0 + lane < t1;
            const int jb = jvalid ? j0 + lane : t1 - 1;
            const Mission Mj = mission_of(t_seg_offsets, jb, mt);
            const int32_t *jrows = t_seg_rows + Mj.s0;
            const double *jcm = t_coeffs + (size_t)Mj.s0 * 24;
            const int nj = jvalid ? t_n_rows[jb] : 0, sj = t_start[jb];
            int js = 0, jbase = 0, jcnt = jrows[0];
            int is = 0, ibase = 0, icnt = irows[0];
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
                    pair_row<false>(mine + r * kTile * 3, xi, yi, zi, r2, -1, rm, rkey, mask);
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
        // one partial record per mission and share p (an excluded mission's is ignored); its fifth row: the included traffic of the group
        if (w == 0 && act) sep_leave_partial(part_d2, part_i, p, b, B, gb, gj, gk, gconf, gfirst, n_in);
    }
}

__global__ void __launch_bounds__(kThreads) against_merge_kernel(const int32_t *__restrict__ n_rows, int B, int P,
                                                                 const double *__restrict__ part_d2, const int32_t *__restrict__ part_i,
                                                                 double *__restrict__ sep, int32_t *__restrict__ isep) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    const size_t Bs = (size_t)B;
    if (n_rows[b] == 0) {                                    // excluded: compared with nobody
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

int uavac_launch_separation_against(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                    double dt, const int64_t *group_offsets, int G, const int32_t *start_rows, const double *t_coeffs,
                                    const int32_t *t_seg_rows, const int64_t *t_seg_offsets, int Bt, int mt, const int64_t *t_group_offsets,
                                    const int32_t *t_start_rows, double radius, double *sep, int32_t *isep) {
    // the shares per window: as sep_shares has them, with the j-tiles of an average group's TRAFFIC
    const int groups = group_offsets ? G : 1;
    const int windows = (B + kTile - 1) / kTile;
    int P = ctx->separation_split;
    if (P <= 0) {
        const int tiles = (Bt / groups + kTile - 1) / kTile;
        P = std::min((ctx->n_simds * 4 + windows - 1) / windows, tiles);
    }
    P = std::max(1, std::min(P, UAVAC_SEP_MAX_SPLIT));
    const size_t Bs = (size_t)B;
    int32_t *n_rows = nullptr, *start = nullptr, *t_n_rows = nullptr, *t_start = nullptr, *part_i = nullptr;
    double *part_d2 = nullptr;
    Scratch s(ctx);
    s.want(&n_rows, Bs); s.want(&start, Bs); s.want(&t_n_rows, (size_t)Bt); s.want(&t_start, (size_t)Bt);
    s.want(&part_d2, P * Bs); s.want(&part_i, P * 5 * Bs);
    if (int rc = s.commit()) return rc;
    hipLaunchKernelGGL(against_prepass_kernel, dim3((B + kPreMissions - 1) / kPreMissions), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows,
                       seg_offsets, B, m, start_rows, n_rows, start, ctx->d_flags);
    hipLaunchKernelGGL(against_prepass_kernel, dim3((Bt + kPreMissions - 1) / kPreMissions), dim3(kThreads), 0, ctx->stream, t_coeffs, t_seg_rows,
                       t_seg_offsets, Bt, mt, t_start_rows, t_n_rows, t_start, ctx->d_flags);
    hipLaunchKernelGGL(separation_against_kernel, dim3(windows, P), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows, seg_offsets, B, m, dt,
                       group_offsets, groups, n_rows, start, t_coeffs, t_seg_rows, t_seg_offsets, Bt, mt, t_group_offsets, t_n_rows, t_start,
                       radius * radius, part_d2, part_i);
    hipLaunchKernelGGL(against_merge_kernel, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream, n_rows, B, P, part_d2, part_i,
                       sep, isep);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}
