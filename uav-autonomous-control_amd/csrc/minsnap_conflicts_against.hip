// The CROSS conflict list (gfx950): the conflict graph of the cross audit in CSR form.  Where the audit (minsnap_separation_against.hip)
// names a plan mission's one closest traffic mission and COUNTS the others that come inside the radius, this lists every one of them,
// with when and how near: first and last clock row inside, the number of rows inside, the pair's minimum distance and its row.  From
// coefficients and row counts alone: no row is written, nothing is read back, no array of either plan is written.  The contract -- the
// cross audit's clock, groups, excluded missions, rounding and bad inputs, the list's slices and bounds -- is in include/uavac.h
// (uavac_minsnap_conflict_against_offsets_dev, uavac_minsnap_conflicts_against_dev); uav_ac.scoring.conflicts_against_rows states it
// in NumPy on sampled rows, and the results are the same bits.
//
// Launches on the ctx stream:
//   conflict_against_prepass_kernel   fleet_clock.h's pre-pass, once on the plan and once on the traffic
//   conflict_against_discover_kernel  the pairs, in the cross audit's loop nest: a workgroup owns a window of 64 PLAN missions, one per
//                                     lane (i), visits every group that reaches into the window, walks the TRAFFIC of that group in
//                                     j-tiles of 64 staged in LDS and the group's clock in chunks of 32 rows, wave w taking rows 8 w ..
//                                     8 w + 7.  Nothing is kept but the bit per traffic mission that came inside the radius; the four
//                                     wavefronts' masks are ORed into one 64-bit word of (plan mission, traffic j-tile), which goes to
//                                     scratch, words [slot][B], slot = the j-tile's index within the round: ONE writer per word, shares
//                                     take whole tiles.  The first share of the first round also leaves, per plan mission, the TRAFFIC
//                                     group's first mission (so the list kernel produces traffic batch indices as they are), the horizon
//                                     over both sides and the traffic group's j-tiles (0: no included traffic) -- info [3][B].
//   conflict_count_kernel,            (conflict_csr.h, as they are) the popcounts of the round's words into the totals of the offsets'
//   conflict_list_kernel              scan; the words bit by bit into row 0 of the mission's slice, bounded, with flags 2 and 0
//   conflict_against_measure_kernel   per listed entry, sixteen lanes each: mission i walked from the PLAN's arrays and mission j from
//                                     the TRAFFIC's over the group's clock [0, H_g), H_g from info; the result of a lane's rows, the
//                                     merge of the sixteen lanes and the write are csr::Measure.  It reads nothing of the discovery.
// ROUNDS.  The most j-tiles a group can have is ceil(Bt / 64), the TRAFFIC's (csr::shape_of_sides).  The fill call repeats the discovery.
// Every reduction is an OR, a lexicographic minimum, a min, a max or an integer sum: the outputs depend neither on the shares P, nor on
// the slots, nor on the tile or chunk sizes.  ROUNDING: fleet_clock.h's.

#include "conflict_csr.h"
#include "fleet_clock.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace {

using namespace fleet;

constexpr int kPairLanes = 16;                              // lanes per entry of the measure
constexpr int kPairsPerWave = 64 / kPairLanes;
constexpr int kPairsPerGroup = kWaves * kPairsPerWave;      // entries per workgroup of the measure

// ------------------------------------------------------------------------------------------------------------------ pre-pass
__global__ void __launch_bounds__(kThreads) conflict_against_prepass_kernel(const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows,
                                                                            const int64_t *__restrict__ seg_offsets, int B, int m,
                                                                            const int32_t *__restrict__ start_rows,
                                                                            int32_t *__restrict__ n_rows, int32_t *__restrict__ start,
                                                                            int32_t *__restrict__ flags) {
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

// ------------------------------------------------------------------------------------------------------------------ discovery
// info [3][B]: the first mission of the TRAFFIC's group, the group's horizon over both sides, and the traffic's j-tiles (0: no included
// traffic).  Launched as dim3(windows, P) x kThreads; of the tiles [T0, T0 + slots) of a round, share p takes those with t = p (mod P).
__global__ void __launch_bounds__(kThreads, 3) conflict_against_discover_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
    const int64_t *__restrict__ group_offsets, int G, const int32_t *__restrict__ n_rows, const int32_t *__restrict__ start,
    const double *__restrict__ t_coeffs, const int32_t *__restrict__ t_seg_rows, const int64_t *__restrict__ t_seg_offsets, int Bt, int mt,
    const int64_t *__restrict__ t_group_offsets, const int32_t *__restrict__ t_n_rows, const int32_t *__restrict__ t_start, double r2, int T0,
    int slots, unsigned long long *__restrict__ words, int32_t *__restrict__ info) {
    __shared__ double tile[kWaves * kRegion];
    const double inf = std::numeric_limits<double>::infinity();
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int P = gridDim.y, p = blockIdx.y;
    const int w0 = blockIdx.x * kTile, w1 = w0 + kTile;      // the window of plan missions this workgroup owns
    const int b = w0 + lane;
    const bool live = b < B;
    const int bb = live ? b : B - 1;                         // (a lane past the batch shadows the last mission)
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
        const int n_tiles = (t1 - t0 + kTile - 1) / kTile;
        if (T0 >= n_tiles) continue;                         // a later round than the group's traffic has tiles (or no traffic at all)
        const bool act = live && b >= g0 && b < g1;

        int H, n_own, h_traffic, n_in;                       // the group's horizon over both sides; the included traffic
        side_of_group(meet, lane, w, g0, g1, n_rows, start, H, n_own);
        side_of_group(meet, lane, w, t0, t1, t_n_rows, t_start, h_traffic, n_in);
        H = max(H, h_traffic);
        const int live_tiles = n_in >= 1 ? n_tiles : 0;
        if (w == 0 && act && p == 0 && T0 == 0) {
            info[b] = t0;
            info[(size_t)B + b] = H;
            info[2 * (size_t)B + b] = live_tiles;
        }
        const int t_end = min(live_tiles, T0 + slots);
        for (int t = T0 + ((p - T0) % P + P) % P; t < t_end; t += P) {      // this share's tiles of the round: t = p (mod P)
            const int j0 = t0 + t * kTile;
            const bool jvalid = j0 + lane < t1;
            const int jb = jvalid ? j0 + lane : t1 - 1;
            const Mission Mj = mission_of(t_seg_offsets, jb, mt);
            const int32_t *jrows = t_seg_rows + Mj.s0;
            const double *jcm = t_coeffs + (size_t)Mj.s0 * 24;
            const int nj = jvalid ? t_n_rows[jb] : 0, sj = t_start[jb];
            int js = 0, jbase = 0, jcnt = jrows[0];
            int is = 0, ibase = 0, icnt = irows[0];
            unsigned long long mask = 0;                     // traffic missions of the tile that came inside the radius
            for (int k0 = w * kRows; k0 < H; k0 += kChunk) {
                // the j-tile's positions at this wavefront's rows of the chunk, then the lane's own against them (a wavefront reads only
                // its own quarter)
                clock_walk_to_tile<false>(mine, lane, jrows, jcm, Mj.m, nj, sj, k0, H, dt, js, jbase, jcnt, AsPlanned{});
                lds_wave_fence();
                clock_walk<false>(irows, icm, Mi.m, ni, si, k0, H, dt, is, ibase, icnt, AsPlanned{}, [&](int r, int, double xi, double yi, double zi) {
                    double rm = inf;                         // (of pair_row's results only the bits are kept)
                    int rkey = 0;
                    pair_row<false>(mine + r * kTile * 3, xi, yi, zi, r2, -1, rm, rkey, mask);
                });
                lds_wave_fence();
            }
            // the four wavefronts meet: 1 .. 3 leave their bits in their quarters, wavefront 0 ORs them and writes the word
            if (w != 0) sep_waves_leave_bits(mine, lane, mask);
            __syncthreads();
            if (w == 0) {
                sep_waves_meet_bits(tile, lane, mask);
                if (act) words[(size_t)(t - T0) * (size_t)B + b] = mask;
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ the measure
__global__ void __launch_bounds__(kThreads, 3) conflict_against_measure_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
    const int32_t *__restrict__ n_rows, const int32_t *__restrict__ start, const double *__restrict__ t_coeffs,
    const int32_t *__restrict__ t_seg_rows, const int64_t *__restrict__ t_seg_offsets, int Bt, int mt, const int32_t *__restrict__ t_n_rows,
    const int32_t *__restrict__ t_start, const int32_t *__restrict__ info, double r2, const int32_t *__restrict__ owner, long long capacity,
    double *__restrict__ pair_d, int32_t *__restrict__ pair_i) {
    __shared__ double tile[kWaves * kRegion];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int l = lane % kPairLanes;
    const long long e = ((long long)blockIdx.x * kWaves + w) * kPairsPerWave + lane / kPairLanes;
    // the entry's pair: the plan mission that owns it (-1: nobody listed it) and the traffic mission in row 0; an entry that is not
    // measured walks mission 0 of either side over an empty clock
    int i = e < capacity ? owner[e] : -1;
    int j = i >= 0 ? pair_i[e] : -1;
    bool live = i >= 0 && i < B && j >= 0 && j < Bt;
    i = live ? i : 0; j = live ? j : 0;
    const int ni = n_rows[i], nj = t_n_rows[j], si = start[i], sj = t_start[j];
    live = live && ni > 0 && nj > 0;
    const int H = live ? info[(size_t)B + i] : 0;
    const Mission Mi = mission_of(seg_offsets, i, m), Mj = mission_of(t_seg_offsets, j, mt);
    const int32_t *irows = seg_rows + Mi.s0, *jrows = t_seg_rows + Mj.s0;
    const double *icm = coeffs + (size_t)Mi.s0 * 24, *jcm = t_coeffs + (size_t)Mj.s0 * 24;
    double *mine = tile + w * kRegion;                       // the lane reads only the slots it wrote itself

    csr::Measure res;
    int js = 0, jbase = 0, jcnt = jrows[0];
    int is = 0, ibase = 0, icnt = irows[0];
    for (int k0 = l * kRows; k0 < H; k0 += kPairLanes * kRows) {
        clock_walk_to_tile<false>(mine, lane, jrows, jcm, Mj.m, nj, sj, k0, H, dt, js, jbase, jcnt, AsPlanned{});
        clock_walk<false>(irows, icm, Mi.m, ni, si, k0, H, dt, is, ibase, icnt, AsPlanned{}, [&](int r, int k, double xi, double yi, double zi) {
            const double *o = mine + (r * kTile + lane) * 3;
            res.row(csr::pair_d2(xi, yi, zi, o[0], o[1], o[2]), k, r2);
        });
    }
    // the sixteen lanes of the entry
#pragma unroll
    for (int d = kPairLanes / 2; d >= 1; d >>= 1)
        res.merge(__shfl_xor(res.bd, d), __shfl_xor(res.bk, d), __shfl_xor(res.first, d), __shfl_xor(res.last_in, d), __shfl_xor(res.inside, d));
    if (live && l == 0) res.write(pair_d, pair_i, e, capacity);
}

// ------------------------------------------------------------------------------------------------------------------ the host side
// What the two calls share: csr's shape (shares, slots, rounds; counts, words, owners) and the two pre-passes' and the discovery's records.
struct Shape : csr::Shape {
    int32_t *n_rows, *start, *t_n_rows, *t_start, *info;
};

// the plan's side of the cross list: what the two calls take alike
struct Sides {
    const double *coeffs;
    const int32_t *seg_rows;
    const int64_t *seg_offsets;
    int B, m;
    const int64_t *group_offsets;
    const int32_t *start_rows;
    const double *t_coeffs;
    const int32_t *t_seg_rows;
    const int64_t *t_seg_offsets;
    int Bt, mt;
    const int64_t *t_group_offsets;
    const int32_t *t_start_rows;
    int groups;                                              // 1 without offsets
};

int shape_of(uavac_ctx *ctx, Scratch &scratch, const Sides &a, long long capacity, Shape &s) {
    // the shares per window: the cross audit's rule (uavac_launch_separation_against), with the j-tiles of an average group's TRAFFIC
    const int windows = (a.B + kTile - 1) / kTile;
    int P = ctx->separation_split;
    if (P <= 0) {
        const int tiles = (a.Bt / a.groups + kTile - 1) / kTile;
        P = std::min((ctx->n_simds * 4 + windows - 1) / windows, tiles);
    }
    P = std::max(1, std::min(P, UAVAC_SEP_MAX_SPLIT));
    csr::shape_of_sides(ctx, windows, P, a.Bt, s);
    const size_t Bs = (size_t)a.B;
    scratch.want(&s.n_rows, Bs); scratch.want(&s.start, Bs); scratch.want(&s.t_n_rows, (size_t)a.Bt); scratch.want(&s.t_start, (size_t)a.Bt);
    scratch.want(&s.info, 3 * Bs);
    csr::shape_want(scratch, s, a.B, capacity);
    return scratch.commit();
}

int launch_prepass(uavac_ctx *ctx, const Shape &s, const Sides &a) {
    hipLaunchKernelGGL(conflict_against_prepass_kernel, dim3((a.B + kPreMissions - 1) / kPreMissions), dim3(kThreads), 0, ctx->stream, a.coeffs,
                       a.seg_rows, a.seg_offsets, a.B, a.m, a.start_rows, s.n_rows, s.start, ctx->d_flags);
    hipLaunchKernelGGL(conflict_against_prepass_kernel, dim3((a.Bt + kPreMissions - 1) / kPreMissions), dim3(kThreads), 0, ctx->stream, a.t_coeffs,
                       a.t_seg_rows, a.t_seg_offsets, a.Bt, a.mt, a.t_start_rows, s.t_n_rows, s.t_start, ctx->d_flags);
    // a mission that no group holds (offsets that do not cover the batch) or whose group has no traffic has no tiles
    UAVAC_HIP(ctx, hipMemsetAsync(s.info, 0, 3 * (size_t)a.B * 4, ctx->stream));
    return UAVAC_OK;
}

// one round of the discovery, from its first j-tile T0 (csr_offsets / csr_list call it once per round)
auto discovery(uavac_ctx *ctx, const Shape &s, const Sides &a, double dt, double radius) {
    return [=](int T0) {
        hipLaunchKernelGGL(conflict_against_discover_kernel, dim3(s.windows, s.P), dim3(kThreads), 0, ctx->stream, a.coeffs, a.seg_rows,
                           a.seg_offsets, a.B, a.m, dt, a.group_offsets, a.groups, s.n_rows, s.start, a.t_coeffs, a.t_seg_rows, a.t_seg_offsets,
                           a.Bt, a.mt, a.t_group_offsets, s.t_n_rows, s.t_start, radius * radius, T0, s.slots, s.words, s.info);
    };
}

}  // namespace

int uavac_launch_conflict_against_offsets(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B,
                                          int m, double dt, const int64_t *group_offsets, int G, const int32_t *start_rows,
                                          const double *t_coeffs, const int32_t *t_seg_rows, const int64_t *t_seg_offsets, int Bt, int mt,
                                          const int64_t *t_group_offsets, const int32_t *t_start_rows, double radius, int64_t *pair_offsets) {
    const Sides a{coeffs, seg_rows, seg_offsets, B, m, group_offsets, start_rows, t_coeffs, t_seg_rows, t_seg_offsets, Bt, mt, t_group_offsets,
                  t_start_rows, group_offsets ? G : 1};
    Scratch scratch(ctx);
    Shape s;
    if (int rc = shape_of(ctx, scratch, a, 0, s)) return rc;
    if (int rc = launch_prepass(ctx, s, a)) return rc;
    return csr::csr_offsets(ctx, s, B, s.n_rows, s.info + 2 * (size_t)B, discovery(ctx, s, a, dt, radius), pair_offsets);
}

int uavac_launch_conflicts_against(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                   double dt, const int64_t *group_offsets, int G, const int32_t *start_rows, const double *t_coeffs,
                                   const int32_t *t_seg_rows, const int64_t *t_seg_offsets, int Bt, int mt, const int64_t *t_group_offsets,
                                   const int32_t *t_start_rows, double radius, const int64_t *pair_offsets, int64_t capacity, double *pair_d,
                                   int32_t *pair_i) {
    const Sides a{coeffs, seg_rows, seg_offsets, B, m, group_offsets, start_rows, t_coeffs, t_seg_rows, t_seg_offsets, Bt, mt, t_group_offsets,
                  t_start_rows, group_offsets ? G : 1};
    Scratch scratch(ctx);
    Shape s;
    if (int rc = shape_of(ctx, scratch, a, capacity, s)) return rc;
    if (int rc = launch_prepass(ctx, s, a)) return rc;
    if (int rc = csr::csr_list(ctx, s, B, s.n_rows, s.info, s.info + 2 * (size_t)B, discovery(ctx, s, a, dt, radius), pair_offsets,
                               (long long)capacity, pair_i))
        return rc;
    if (capacity > 0) {
        const long long groups = (capacity + kPairsPerGroup - 1) / kPairsPerGroup;
        hipLaunchKernelGGL(conflict_against_measure_kernel, dim3((unsigned)groups), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows, seg_offsets,
                           B, m, dt, s.n_rows, s.start, t_coeffs, t_seg_rows, t_seg_offsets, Bt, mt, s.t_n_rows, s.t_start, s.info,
                           radius * radius, s.owner, (long long)capacity, pair_d, pair_i);
    }
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}
