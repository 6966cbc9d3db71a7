// The conflict list of a FLIGHT (gfx950): where the flown separation audit (flown_separation.hip) names a vehicle's one closest partner
// and COUNTS the others that came inside the radius, this lists every one of them, with when and how near -- first and last tick inside,
// the ticks inside, the pair's minimum distance and its tick -- from the positions in the rollout's state log ([K][13][pitch] f64, rows
// 0-2).  Nothing is read back and no log leaves the device.  The contract is in include/uavac.h (uavac_flown_conflict_offsets_dev,
// uavac_flown_conflicts_dev); uav_ac.scoring.conflicts_from_log states it in NumPy, and the results are the same bits.
//
// Launches on the ctx stream:
//   flown_discover_kernel     the pairs: flown_separation_kernel's loop (64-vehicle windows x j-tiles x P shares, four wavefronts that
//                             split each chunk of 32 ticks, a j-tile's x, y and z at one tick as three coalesced 512-byte loads into the
//                             wave's own quarter of the LDS tile, the partners as LDS broadcasts) with nothing kept but the bit per
//                             partner that came inside the radius.  A NaN d^2 is never below r^2: validity costs nothing here.  The
//                             merged 64-bit word of (vehicle, j-tile) goes to scratch, words [slot][B] (conflict_csr.h): ONE writer per
//                             word, the share that owns the tile.  The first share of the first round also leaves, per vehicle, its
//                             group's first vehicle and number of j-tiles (0 for a group of one).
//   conflict_count_kernel,    conflict_csr.h: the CSR machinery the plan's list (minsnap_conflicts.hip) uses, one copy -- the popcounts
//   conflict_list_kernel      into the offsets' scan; the words bit by bit into row 0 of the vehicle's slice, bounded, flags 2 and 0;
//                             the rounds over "conflict_slots"
//   flown_measure_kernel      per listed entry, both vehicles walked over the ticks 0 .. K - 1.  A workgroup takes 64 CONSECUTIVE
//                             entries, one per lane, and its four wavefronts split each chunk of 32 ticks as the discovery does (wave w:
//                             ticks 8 w .. 8 w + 7, 48 loads in flight per lane).  A pair needs 8 useful bytes of every log row, 13 *
//                             pitch doubles apart from tick to tick: nothing coalesces ALONG the clock, so the lanes are laid ACROSS
//                             the entries instead.  Consecutive entries have the same owner or the next one, and ascending partners of
//                             one group: at one tick the 64 lanes of a load read columns of one group's span of a log row -- 512 bytes
//                             in groups of 64, four cache lines per load instead of 64.  The reductions -- first tick inside (min), last
//                             (max), ticks inside (sum), the lexicographic minimum of (d^2, tick) -- are exact and independent of
//                             order: over the ticks of a wave in ascending order, then over the four waves through LDS; a NaN d^2 is
//                             neither below the minimum nor inside.  One correctly rounded sqrt comes last.  Every entry is measured by
//                             its own lane (both directions of a pair: twice the arithmetic, one writer per entry and no search for the
//                             reverse entry); workgroups that are neighbours in the list are placed on the same XCD (xcd_contiguous), so
//                             that a group's columns, which they re-read, are found in that XCD's L2.
// The fill call repeats the discovery: it does not rely on what the offsets call left in the arena, other calls may run in between.
// Every column index is below B (lanes past the batch or the group read column B - 1 or the group's last one and are masked; an entry
// nobody listed reads column 0 and writes nothing): columns B .. pitch - 1 are never read.
//
// ROUNDING (part of the contract): dx = xi - xj, ..., d^2 = (dx dx + dy dy) + dz dz WITHOUT contraction, each product and sum rounded on
// its own -- (xi - xj)^2 == (xj - xi)^2 bit for bit, so the two directions of a pair agree in everything but the partner.

#include "conflict_csr.h"
#include "fleet_clock.h"

#include <cmath>
#include <limits>

namespace {

using namespace sepred;                                     // the tile's shape and pair_row: shared with the audits
using fleet::group_range;

constexpr int kLogRows = 13;                                // rows of the state log per tick (positions: 0-2)
constexpr int kPairsPerGroup = 64;                          // entries per workgroup of the measure: one per lane

// ------------------------------------------------------------------------------------------------------------------ discovery
// first / tiles [B]: the first vehicle of the vehicle's group and the group's j-tiles (0: a group of one).
__global__ void __launch_bounds__(kThreads, 3) flown_discover_kernel(const double *__restrict__ slog, int K, int B, long long pitch,
                                                                     const int64_t *__restrict__ group_offsets, int G, double r2, int T0,
                                                                     int slots, unsigned long long *__restrict__ words,
                                                                     int32_t *__restrict__ first, int32_t *__restrict__ tiles) {
    __shared__ double tile[kWaves * kRegion];
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int P = gridDim.y, p = blockIdx.y;
    const int w0 = blockIdx.x * kTile, w1 = w0 + kTile;      // the window of vehicles this workgroup owns
    const int b = w0 + lane;
    const bool live = b < B;
    const double *own = slog + (live ? b : B - 1);           // the lane's own column (a lane past the batch shadows the last vehicle)
    const long long tick = kLogRows * pitch;                 // doubles from one tick of the log to the next
    double *mine = tile + w * kRegion;                       // this wavefront's quarter of the tile
    const size_t Bs = (size_t)B;

    int g = 0;                                               // the group that holds vehicle w0: the last one that starts at or before it
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
        const int n_tiles = (g1 - g0 + kTile - 1) / kTile;
        const int live_tiles = g1 - g0 >= 2 ? n_tiles : 0;
        if (w == 0 && act && p == 0 && T0 == 0) { first[b] = g0; tiles[b] = live_tiles; }
        const int t_end = min(live_tiles, T0 + slots);
        for (int t = T0 + ((p - T0) % P + P) % P; t < t_end; t += P) {      // this share's tiles of the round: t = p (mod P)
            const int j0 = g0 + t * kTile;
            const bool jvalid = j0 + lane < g1;
            const double *theirs = slog + (jvalid ? j0 + lane : g1 - 1);
            const int selfjj = b - j0;
            const bool self_tile = j0 < w1 && j0 + kTile > w0;
            unsigned long long mask = 0;                     // partners that came inside the radius
            for (int k0 = w * kRows; k0 < K; k0 += kChunk) {
                const int n = min(kRows, K - k0);            // this wavefront's ticks of the chunk
#pragma unroll
                for (int r = 0; r < kRows; ++r) {            // the j-tile's positions (the ticks past the log's end repeat its last one: unused)
                    const double *at = theirs + (long long)min(k0 + r, K - 1) * tick;
                    const double x = at[0], y = at[pitch], z = at[2 * pitch];
                    double *o = mine + (r * kTile + lane) * 3;
                    o[0] = jvalid ? x : nan; o[1] = jvalid ? y : nan; o[2] = jvalid ? z : nan;
                }
                lds_wave_fence();                            // (a wavefront reads only its own quarter)
                const double *at = own + (long long)k0 * tick;
                double nx = at[0], ny = at[pitch], nz = at[2 * pitch];      // the lane's own position, one tick ahead
#pragma nounroll
                for (int r = 0; r < n; ++r) {
                    const double xi = nx, yi = ny, zi = nz;
                    if (r + 1 < n) {
                        at = own + (long long)(k0 + r + 1) * tick;
                        nx = at[0]; ny = at[pitch]; nz = at[2 * pitch];
                    }
                    double rm = inf;                         // (of pair_row's results only the bits are kept)
                    int rkey = 0;
                    if (self_tile) pair_row<true>(mine + r * kTile * 3, xi, yi, zi, r2, selfjj, rm, rkey, mask);
                    else pair_row<false>(mine + r * kTile * 3, xi, yi, zi, r2, selfjj, rm, rkey, mask);
                }
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
__device__ __forceinline__ double pair_d2(double xi, double yi, double zi, double xj, double yj, double zj) {
#pragma clang fp contract(off)
    const double dx = xi - xj, dy = yi - yj, dz = zi - zj;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return (xx + yy) + zz;
}

__global__ void __launch_bounds__(kThreads, 4) flown_measure_kernel(const double *__restrict__ slog, int K, int B, long long pitch, double r2,
                                                                    const int32_t *__restrict__ owner, long long capacity,
                                                                    double *__restrict__ pair_d, int32_t *__restrict__ pair_i) {
    __shared__ double meet_d[kWaves - 1][kPairsPerGroup];
    __shared__ int meet_i[kWaves - 1][4][kPairsPerGroup];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // neighbours in the list share an XCD, and with it the L2 that holds their group's columns
    const long long e = (long long)xcd_contiguous((int)blockIdx.x, (int)gridDim.x) * kPairsPerGroup + lane;
    // the entry's pair: who owns it (-1: nobody listed it) and the partner in row 0; an entry that is not measured walks no tick
    int i = e < capacity ? owner[e] : -1;
    int j = i >= 0 ? pair_i[e] : -1;
    const bool live = i >= 0 && i < B && j >= 0 && j < B;
    i = live ? i : 0; j = live ? j : 0;
    const double *mine = slog + i, *theirs = slog + j;
    const long long tick = kLogRows * pitch;
    const int Kl = live ? K : 0;

    double bd = std::numeric_limits<double>::infinity();
    int bk = kNone, first = kNone, last_in = -1, inside = 0;
    for (int k0 = w * kRows; k0 < Kl; k0 += kChunk) {
        double pi[kRows][3], pj[kRows][3];
#pragma unroll
        for (int r = 0; r < kRows; ++r) {                    // (the ticks past the log's end repeat its last one: unused)
            const long long at = (long long)min(k0 + r, K - 1) * tick;
            pi[r][0] = mine[at]; pi[r][1] = mine[at + pitch]; pi[r][2] = mine[at + 2 * pitch];
            pj[r][0] = theirs[at]; pj[r][1] = theirs[at + pitch]; pj[r][2] = theirs[at + 2 * pitch];
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const int k = k0 + r;
            const double d2 = k < K ? pair_d2(pi[r][0], pi[r][1], pi[r][2], pj[r][0], pj[r][1], pj[r][2])
                                    : std::numeric_limits<double>::quiet_NaN();
            if (d2 < bd) { bd = d2; bk = k; }                // (strict: the wave's ticks ascend, the lowest tick of a tie stays)
            if (d2 < r2) { first = min(first, k); last_in = max(last_in, k); ++inside; }
        }
    }
    // the four wavefronts of the entry: the minimum by (d^2, tick), the first tick by min, the last by max, the ticks inside by sum
    if (w != 0) {
        meet_d[w - 1][lane] = bd;
        meet_i[w - 1][0][lane] = bk; meet_i[w - 1][1][lane] = first; meet_i[w - 1][2][lane] = last_in; meet_i[w - 1][3][lane] = inside;
    }
    __syncthreads();
    if (w == 0 && live) {
#pragma unroll
        for (int v = 0; v < kWaves - 1; ++v) {
            const double od = meet_d[v][lane];
            const int ok = meet_i[v][0][lane];
            if (od < bd || (od == bd && ok < bk)) { bd = od; bk = ok; }
            first = min(first, meet_i[v][1][lane]);
            last_in = max(last_in, meet_i[v][2][lane]);
            inside += meet_i[v][3][lane];
        }
        const size_t cap = (size_t)capacity;
        pair_d[e] = sqrt(bd);
        pair_i[cap + e] = first == kNone ? -1 : first;
        pair_i[2 * cap + e] = last_in;
        pair_i[3 * cap + e] = inside;
        pair_i[4 * cap + e] = bk == kNone ? -1 : bk;
    }
}

// ------------------------------------------------------------------------------------------------------------------ the host side
// What the two calls share: csr's shape (shares, slots, rounds; counts, words, owners) and the discovery's record of the groups.
struct Shape : csr::Shape {
    int32_t *first, *tiles;
};

int shape_of(uavac_ctx *ctx, int B, const int64_t *group_offsets, int G, long long capacity, Shape &s) {
    csr::shape_of(ctx, B, group_offsets, G, s);
    const size_t Bs = (size_t)B;
    if (int rc = uavac_arena_reserve(ctx, uavac_arena_size(2 * Bs * 4) + csr::shape_bytes(s, B, capacity))) return rc;
    s.first = static_cast<int32_t *>(uavac_arena_take(ctx, 2 * Bs * 4));
    if (!s.first || !csr::shape_take(ctx, s, B, capacity)) return uavac_fail(ctx, UAVAC_ENOMEM, "flown conflict list: scratch arena too small");
    s.tiles = s.first + Bs;
    // a vehicle that no group holds (offsets that do not cover the batch) has no tiles
    UAVAC_HIP(ctx, hipMemsetAsync(s.first, 0, 2 * Bs * 4, ctx->stream));
    return UAVAC_OK;
}

// one round of the discovery, from its first j-tile T0 (csr_offsets / csr_list call it once per round)
auto discovery(uavac_ctx *ctx, const Shape &s, const double *state_log, int K, int B, int64_t pitch, const int64_t *group_offsets, int G,
               double radius) {
    return [=](int T0) {
        hipLaunchKernelGGL(flown_discover_kernel, dim3(s.windows, s.P), dim3(kThreads), 0, ctx->stream, state_log, K, B, (long long)pitch,
                           group_offsets, group_offsets ? G : 1, radius * radius, T0, s.slots, s.words, s.first, s.tiles);
    };
}

}  // namespace

int uavac_launch_flown_conflict_offsets(uavac_ctx *ctx, const double *state_log, int K, int B, int64_t pitch, const int64_t *group_offsets,
                                        int G, double radius, int64_t *pair_offsets) {
    Shape s;
    if (int rc = shape_of(ctx, B, group_offsets, G, 0, s)) return rc;
    return csr::csr_offsets(ctx, s, B, nullptr, s.tiles, discovery(ctx, s, state_log, K, B, pitch, group_offsets, G, radius), pair_offsets);
}

int uavac_launch_flown_conflicts(uavac_ctx *ctx, const double *state_log, int K, int B, int64_t pitch, const int64_t *group_offsets, int G,
                                 double radius, const int64_t *pair_offsets, int64_t capacity, double *pair_d, int32_t *pair_i) {
    Shape s;
    if (int rc = shape_of(ctx, B, group_offsets, G, capacity, s)) return rc;
    if (int rc = csr::csr_list(ctx, s, B, nullptr, s.first, s.tiles, discovery(ctx, s, state_log, K, B, pitch, group_offsets, G, radius),
                               pair_offsets, (long long)capacity, pair_i))
        return rc;
    if (capacity > 0) {
        const long long groups = (capacity + kPairsPerGroup - 1) / kPairsPerGroup;
        hipLaunchKernelGGL(flown_measure_kernel, dim3((unsigned)groups), dim3(kThreads), 0, ctx->stream, state_log, K, B, (long long)pitch,
                           radius * radius, s.owner, (long long)capacity, pair_d, pair_i);
    }
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}
