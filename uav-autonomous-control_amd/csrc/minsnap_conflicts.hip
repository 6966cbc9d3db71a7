// The fleet's conflict list (gfx950): the conflict graph of the separation audit in CSR form.  Where the audit (minsnap_separation.hip)
// names a mission's one closest partner and COUNTS the others that come inside the radius, this lists every one of them, with when and
// how near: first and last clock row inside, the number of rows inside, the pair's minimum distance and its row.  From coefficients and
// row counts alone: no row is written, nothing is read back.  The contract -- the audit's clock, groups, excluded missions, rounding and
// bad inputs, the slices, the bounds -- is in include/uavac.h (uavac_minsnap_conflict_offsets_dev, uavac_minsnap_conflicts_dev);
// uav_ac.scoring.conflicts_from_rows states it in NumPy on sampled rows, and the results are the same bits.
//
// Launches on the ctx stream:
//   conflict_prepass_kernel    per mission: fleet_clock.h's pre-pass -- the row total N (0: EXCLUDED) and the clamped start row
//   conflict_discover_kernel   the pairs: the audit's pair loop (64-mission windows x j-tiles x P shares, four wavefronts that split each
//                              chunk of 32 clock rows and meet at the end of a j-tile through the dead LDS tile) with nothing kept but
//                              the bit per partner that came inside the radius.  The merged 64-bit word of (mission, j-tile) goes to
//                              scratch, words [slot][B], slot = the j-tile's index within the mission's group: ONE writer per word --
//                              the share that owns the tile --, no atomics decide a position.  The first share also leaves, per mission,
//                              its group's first mission, horizon and number of j-tiles.
//                              Discovery is repeated in ROUNDS over the slots [T0, T0 + slots) (conflict_csr.h); in a later round a
//                              workgroup whose groups have no tile that far finds that out from the group's size and leaves.
//   conflict_count_kernel,     (conflict_csr.h, one copy for this list and the flown one, flown_conflicts.hip) the popcounts of the
//   conflict_list_kernel       round's words into the totals of the offsets' scan; the words bit by bit into row 0 of the mission's
//                              slice, bounded, with flags 2 and 0
//   conflict_measure_kernel    per listed entry, sixteen lanes each: both missions walked over the group's clock [0, H_g) with
//                              clock_walk's arithmetic -- lane l takes the rows 8 (16 c + l) .. + 7 of every c --, the partner's eight
//                              positions parked in the lane's own slots of the LDS tile; first row inside (min), last row inside (max),
//                              rows inside (sum) and the lexicographic minimum of (d^2, row): exact reductions that do not depend on
//                              order, over the rows of a lane and then over the sixteen lanes.  One correctly rounded sqrt comes last.
//                              It reads a pair and nothing of the discovery, so that the same measure can follow for a state log.
// The fill call repeats the discovery: it does not rely on what the offsets call left in the arena, other calls may run in between.
// Work: discovery = the audit's pairs x horizon; the measure = entries x horizon, small beside it.
//
// ROUNDING (part of the contract): positions by the sampler's fma chain (minsnap_eval_pos), the distance WITHOUT contraction: dx = xi -
// xj, ..., d^2 = (dx dx + dy dy) + dz dz, each product and sum rounded on its own -- (xi - xj)^2 == (xj - xi)^2 bit for bit, so the two
// directions of a pair agree in everything but the partner.

#include "conflict_csr.h"
#include "fleet_clock.h"

#include <cmath>
#include <limits>

namespace {

using namespace fleet;                                      // the clock, the pre-pass and, through it, sepred's tile and reduction

constexpr int kPairLanes = 16;                              // lanes per entry of the measure
constexpr int kPairsPerWave = 64 / kPairLanes;
constexpr int kPairsPerGroup = kWaves * kPairsPerWave;      // entries per workgroup of the measure

// ------------------------------------------------------------------------------------------------------------------ pre-pass
__global__ void __launch_bounds__(kThreads) conflict_prepass_kernel(const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows,
                                                                    const int64_t *__restrict__ seg_offsets, int B, int m,
                                                                    const int32_t *__restrict__ start_rows, int32_t *__restrict__ n_rows,
                                                                    int32_t *__restrict__ start, int32_t *__restrict__ flags) {
    int b, s;
    prepass_mission(coeffs, seg_rows, seg_offsets, B, m, start_rows, n_rows, start, flags, b, s);
}

// ------------------------------------------------------------------------------------------------------------------ discovery
// info [3][B]: the first mission of the mission's group, the group's horizon, and its j-tiles (0: fewer than two missions take part).
__global__ void __launch_bounds__(kThreads, 3) conflict_discover_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
    const int64_t *__restrict__ group_offsets, int G, const int32_t *__restrict__ n_rows, const int32_t *__restrict__ start, double r2, int T0,
    int slots, unsigned long long *__restrict__ words, int32_t *__restrict__ info) {
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
    const size_t Bs = (size_t)B;

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
        const int n_tiles = (g1 - g0 + kTile - 1) / kTile;
        if (T0 >= n_tiles) continue;                         // a later round than this group has tiles (T0 == 0 never leaves here)
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

        const int live_tiles = n_in >= 2 ? n_tiles : 0;
        if (w == 0 && act && p == 0 && T0 == 0) { info[b] = g0; info[Bs + b] = H; info[2 * Bs + b] = live_tiles; }
        const int t_end = min(live_tiles, T0 + slots);
        for (int t = T0 + ((p - T0) % P + P) % P; t < t_end; t += P) {      // this share's tiles of the round: t = p (mod P)
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
            unsigned long long mask = 0;
            for (int k0 = w * kRows; k0 < H; k0 += kChunk) {
                // the j-tile's positions at this wavefront's rows of the chunk, then the lane's own against them (a wavefront reads only
                // its own quarter); of pair_row's results only the bits are kept
                clock_walk_to_tile<false>(mine, lane, jrows, jcm, Mj.m, nj, sj, k0, H, dt, js, jbase, jcnt, AsPlanned{});
                lds_wave_fence();
                clock_walk<false>(irows, icm, Mi.m, ni, si, k0, H, dt, is, ibase, icnt, AsPlanned{}, [&](int r, int, double xi, double yi, double zi) {
                    double rm = inf;
                    int rkey = 0;
                    if (self_tile) pair_row<true>(mine + r * kTile * 3, xi, yi, zi, r2, selfjj, rm, rkey, mask);
                    else pair_row<false>(mine + r * kTile * 3, xi, yi, zi, r2, selfjj, rm, rkey, mask);
                });
                lds_wave_fence();
            }
            // the four wavefronts meet: 1 .. 3 leave their bits in their quarters, wavefront 0 merges them and writes the word
            if (w != 0) sep_waves_leave_bits(mine, lane, mask);
            __syncthreads();
            if (w == 0) {
                sep_waves_meet_bits(tile, lane, mask);
                if (act) words[(size_t)(t - T0) * Bs + b] = mask;
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ the measure
__device__ __forceinline__ double pair_d2(double xi, double yi, double zi, const double *o) {
#pragma clang fp contract(off)
    const double dx = xi - o[0], dy = yi - o[1], dz = zi - o[2];
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return (xx + yy) + zz;
}

__global__ void __launch_bounds__(kThreads, 3) conflict_measure_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
    const int32_t *__restrict__ n_rows, const int32_t *__restrict__ start, const int32_t *__restrict__ info, double r2,
    const int32_t *__restrict__ owner, long long capacity, double *__restrict__ pair_d, int32_t *__restrict__ pair_i) {
    __shared__ double tile[kWaves * kRegion];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int l = lane % kPairLanes;
    const long long e = ((long long)blockIdx.x * kWaves + w) * kPairsPerWave + lane / kPairLanes;
    // the entry's pair: who owns it (-1: nobody listed it) and the partner in row 0; an entry that is not measured walks mission 0 over
    // an empty clock
    int i = e < capacity ? owner[e] : -1;
    int j = i >= 0 ? pair_i[e] : -1;
    bool live = i >= 0 && i < B && j >= 0 && j < B;
    i = live ? i : 0; j = live ? j : 0;
    const int ni = n_rows[i], nj = n_rows[j], si = start[i], sj = start[j];
    live = live && ni > 0 && nj > 0;
    const int H = live ? info[(size_t)B + i] : 0;
    const Mission Mi = mission_of(seg_offsets, i, m), Mj = mission_of(seg_offsets, j, m);
    const int32_t *irows = seg_rows + Mi.s0, *jrows = seg_rows + Mj.s0;
    const double *icm = coeffs + (size_t)Mi.s0 * 24, *jcm = coeffs + (size_t)Mj.s0 * 24;
    double *mine = tile + w * kRegion;                       // the lane reads only the slots it wrote itself

    double bd = std::numeric_limits<double>::infinity();
    int bk = kNone, first = kNone, last_in = -1, inside = 0;
    int js = 0, jbase = 0, jcnt = jrows[0];
    int is = 0, ibase = 0, icnt = irows[0];
    for (int k0 = l * kRows; k0 < H; k0 += kPairLanes * kRows) {
        clock_walk_to_tile<false>(mine, lane, jrows, jcm, Mj.m, nj, sj, k0, H, dt, js, jbase, jcnt, AsPlanned{});
        clock_walk<false>(irows, icm, Mi.m, ni, si, k0, H, dt, is, ibase, icnt, AsPlanned{}, [&](int r, int k, double xi, double yi, double zi) {
            const double d2 = pair_d2(xi, yi, zi, mine + (r * kTile + lane) * 3);
            if (d2 < bd) { bd = d2; bk = k; }                // (strict: the lane's rows ascend, the lowest row of a tie stays)
            if (d2 < r2) { first = min(first, k); last_in = max(last_in, k); ++inside; }
        });
    }
    // the sixteen lanes of the entry: the minimum by (d^2, row), the first row by min, the last by max, the rows inside by sum
#pragma unroll
    for (int d = kPairLanes / 2; d >= 1; d >>= 1) {
        const double od = __shfl_xor(bd, d);
        const int ok = __shfl_xor(bk, d);
        if (od < bd || (od == bd && ok < bk)) { bd = od; bk = ok; }
        first = min(first, __shfl_xor(first, d));
        last_in = max(last_in, __shfl_xor(last_in, d));
        inside += __shfl_xor(inside, d);
    }
    if (live && l == 0) {
        const size_t cap = (size_t)capacity;
        pair_d[e] = sqrt(bd);
        pair_i[cap + e] = first == kNone ? -1 : first;
        pair_i[2 * cap + e] = last_in;
        pair_i[3 * cap + e] = inside;
        pair_i[4 * cap + e] = bk == kNone ? -1 : bk;
    }
}

// ------------------------------------------------------------------------------------------------------------------ the host side
// What the two calls share: csr's shape (shares, slots, rounds; counts, words, owners) and the pre-pass's and the discovery's records.
struct Shape : csr::Shape {
    int32_t *n_rows, *start, *info;
};

int shape_of(uavac_ctx *ctx, int B, const int64_t *group_offsets, int G, long long capacity, Shape &s) {
    csr::shape_of(ctx, B, group_offsets, G, s);
    const size_t Bs = (size_t)B;
    if (int rc = uavac_arena_reserve(ctx, 2 * uavac_arena_size(Bs * 4) + uavac_arena_size(3 * Bs * 4) + csr::shape_bytes(s, B, capacity)))
        return rc;
    s.n_rows = static_cast<int32_t *>(uavac_arena_take(ctx, Bs * 4));
    s.start = static_cast<int32_t *>(uavac_arena_take(ctx, Bs * 4));
    s.info = static_cast<int32_t *>(uavac_arena_take(ctx, 3 * Bs * 4));
    if (!s.n_rows || !s.start || !s.info || !csr::shape_take(ctx, s, B, capacity))
        return uavac_fail(ctx, UAVAC_ENOMEM, "conflict list: scratch arena too small");
    return UAVAC_OK;
}

int launch_prepass(uavac_ctx *ctx, const Shape &s, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                   const int32_t *start_rows) {
    hipLaunchKernelGGL(conflict_prepass_kernel, dim3((B + kPreMissions - 1) / kPreMissions), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows,
                       seg_offsets, B, m, start_rows, s.n_rows, s.start, ctx->d_flags);
    // a mission that no group holds (offsets that do not cover the batch) has no tiles
    UAVAC_HIP(ctx, hipMemsetAsync(s.info, 0, 3 * (size_t)B * 4, ctx->stream));
    return UAVAC_OK;
}

// one round of the discovery, from its first j-tile T0 (csr_offsets / csr_list call it once per round)
auto discovery(uavac_ctx *ctx, const Shape &s, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
               double dt, const int64_t *group_offsets, int G, double radius) {
    return [=](int T0) {
        hipLaunchKernelGGL(conflict_discover_kernel, dim3(s.windows, s.P), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows, seg_offsets, B, m,
                           dt, group_offsets, group_offsets ? G : 1, s.n_rows, s.start, radius * radius, T0, s.slots, s.words, s.info);
    };
}

}  // namespace

int uavac_launch_conflict_offsets(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                  double dt, const int64_t *group_offsets, int G, const int32_t *start_rows, double radius,
                                  int64_t *pair_offsets) {
    Shape s;
    if (int rc = shape_of(ctx, B, group_offsets, G, 0, s)) return rc;
    if (int rc = launch_prepass(ctx, s, coeffs, seg_rows, seg_offsets, B, m, start_rows)) return rc;
    const auto discover = discovery(ctx, s, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, radius);
    return csr::csr_offsets(ctx, s, B, s.n_rows, s.info + 2 * (size_t)B, discover, pair_offsets);
}

int uavac_launch_conflicts(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                           const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, const int64_t *pair_offsets,
                           int64_t capacity, double *pair_d, int32_t *pair_i) {
    Shape s;
    if (int rc = shape_of(ctx, B, group_offsets, G, capacity, s)) return rc;
    if (int rc = launch_prepass(ctx, s, coeffs, seg_rows, seg_offsets, B, m, start_rows)) return rc;
    const auto discover = discovery(ctx, s, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, radius);
    if (int rc = csr::csr_list(ctx, s, B, s.n_rows, s.info, s.info + 2 * (size_t)B, discover, pair_offsets, (long long)capacity, pair_i))
        return rc;
    if (capacity > 0) {
        const long long groups = (capacity + kPairsPerGroup - 1) / kPairsPerGroup;
        hipLaunchKernelGGL(conflict_measure_kernel, dim3((unsigned)groups), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows, seg_offsets, B, m,
                           dt, s.n_rows, s.start, s.info, radius * radius, s.owner, (long long)capacity, pair_d, pair_i);
    }
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}
