// The conflict list of a FLIGHT (gfx950): where the flown separation audit (flown_separation.hip) names a vehicle's one closest partner
// and COUNTS the others that came inside the radius, this lists every one of them, with when and how near -- first and last tick inside,
// the ticks inside, the pair's minimum distance and its tick -- from the positions in the rollout's state log ([K][13][pitch] f64, rows
// 0-2).  Nothing is read back and no log leaves the device.  The contract is in include/uavac.h (uavac_flown_conflict_offsets_dev,
// uavac_flown_conflicts_dev); uav_ac.scoring.conflicts_from_log states it in NumPy, and the results are the same bits.
//
// Launches on the ctx stream:
//   flown_discover_kernel     the pairs: the sweep of pair_sweep.h, which describes it, with positions READ from the log (`Flown`) and
//                             nothing kept but the bit per partner that came inside the radius (`Bits`).  A NaN d^2 is never below
//                             r^2: validity costs nothing here.  The merged 64-bit word of (vehicle, j-tile) goes to scratch, words
//                             [slot][B] (conflict_csr.h): ONE writer per word.  The first share of the first round also leaves, per
//                             vehicle, its group's first vehicle and number of j-tiles (0 for a group of one).
//   conflict_count_kernel,    conflict_csr.h: the CSR machinery the plan's list (minsnap_conflicts.hip) uses, one copy -- the popcounts
//   conflict_list_kernel      into the offsets' scan; the words bit by bit into row 0 of the vehicle's slice, bounded, flags 2 and 0;
//                             the rounds over "conflict_slots"
//   flown_measure_kernel      per listed entry, both vehicles walked over the ticks 0 .. K - 1.  A workgroup takes 64 CONSECUTIVE
//                             entries, one per lane, and its four wavefronts split each chunk of 32 ticks as the discovery does (wave w:
//                             ticks 8 w .. 8 w + 7, 48 loads in flight per lane).  A pair needs 8 useful bytes of every log row, 13 *
//                             pitch doubles apart from tick to tick: nothing coalesces ALONG the clock, so the lanes are laid ACROSS
//                             the entries instead.  Consecutive entries have the same owner or the next one, and ascending partners of
//                             one group: at one tick the 64 lanes of a load read columns of one group's span of a log row -- 512 bytes
//                             in groups of 64, four cache lines per load instead of 64.  The result of a wave's ticks, the merge of the
//                             four waves (through LDS) and the write are csr::Measure (conflict_csr.h).  Every entry is measured by
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
#include "pair_sweep.h"

#include <cmath>
#include <limits>

namespace {

using namespace pair_sweep;                                 // the sweep and, through it, sepred's tile

constexpr int kPairsPerGroup = 64;                          // entries per workgroup of the measure: one per lane

// ------------------------------------------------------------------------------------------------------------------ discovery
// first / tiles [B]: the first vehicle of the vehicle's group and the group's j-tiles (0: a group of one).
__global__ void __launch_bounds__(kThreads, 3) flown_discover_kernel(const double *__restrict__ slog, int K, int B, long long pitch,
                                                                     const int64_t *__restrict__ group_offsets, int G, double r2, int T0,
                                                                     int slots, unsigned long long *__restrict__ words,
                                                                     int32_t *__restrict__ first, int32_t *__restrict__ tiles) {
    __shared__ double tile[kWaves * kRegion];
    Flown src{slog, K, pitch};
    Bits<false> keep{T0, slots, words, first, nullptr, tiles};
    sweep(tile, src, keep, B, group_offsets, G, r2);
}

// ------------------------------------------------------------------------------------------------------------------ the measure
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

    csr::Measure res;
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
            res.row(k < K ? csr::pair_d2(pi[r][0], pi[r][1], pi[r][2], pj[r][0], pj[r][1], pj[r][2]) : std::numeric_limits<double>::quiet_NaN(),
                    k, r2);
        }
    }
    // the four wavefronts of the entry
    if (w != 0) {
        meet_d[w - 1][lane] = res.bd;
        meet_i[w - 1][0][lane] = res.bk; meet_i[w - 1][1][lane] = res.first; meet_i[w - 1][2][lane] = res.last_in;
        meet_i[w - 1][3][lane] = res.inside;
    }
    __syncthreads();
    if (w == 0 && live) {
#pragma unroll
        for (int v = 0; v < kWaves - 1; ++v)
            res.merge(meet_d[v][lane], meet_i[v][0][lane], meet_i[v][1][lane], meet_i[v][2][lane], meet_i[v][3][lane]);
        res.write(pair_d, pair_i, e, capacity);
    }
}

// ------------------------------------------------------------------------------------------------------------------ the host side
// What the two calls share: csr's shape (shares, slots, rounds; counts, words, owners) and the discovery's record of the groups.
struct Shape : csr::Shape {
    int32_t *first, *tiles;
};

int shape_of(uavac_ctx *ctx, Scratch &scratch, int B, const int64_t *group_offsets, int G, long long capacity, Shape &s) {
    csr::shape_of(ctx, B, group_offsets, G, s);
    const size_t Bs = (size_t)B;
    scratch.want(&s.first, 2 * Bs);
    csr::shape_want(scratch, s, B, capacity);
    if (int rc = scratch.commit()) return rc;
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
    Scratch scratch(ctx);
    Shape s;
    if (int rc = shape_of(ctx, scratch, B, group_offsets, G, 0, s)) return rc;
    return csr::csr_offsets(ctx, s, B, nullptr, s.tiles, discovery(ctx, s, state_log, K, B, pitch, group_offsets, G, radius), pair_offsets);
}

int uavac_launch_flown_conflicts(uavac_ctx *ctx, const double *state_log, int K, int B, int64_t pitch, const int64_t *group_offsets, int G,
                                 double radius, const int64_t *pair_offsets, int64_t capacity, double *pair_d, int32_t *pair_i) {
    Scratch scratch(ctx);
    Shape s;
    if (int rc = shape_of(ctx, scratch, B, group_offsets, G, capacity, s)) return rc;
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
