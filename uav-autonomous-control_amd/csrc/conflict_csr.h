// The CSR machinery of the two conflict lists (gfx950): minsnap_conflicts.hip lists the pairs of a PLAN that come inside the radius,
// flown_conflicts.hip those of a FLIGHT, from a state log.  How a pair is DISCOVERED (positions evaluated from coefficients, or read
// from the log) and how it is MEASURED differ and stay with their object files; what happens to the discovered bits in between is the
// same in both and stated once, here.  One copy; every object file instantiates its own kernels.
//   the words              words [slot][B] u64: bit jj of the word of (vehicle b, slot s) says that partner g0 + (T0 + s) * 64 + jj of
//                          b's group came inside the radius, T0 the round's first j-tile.  ONE writer per word, the discovery's share
//                          that owns the tile: no atomics decide a position.  Per vehicle the discovery also leaves its group's first
//                          vehicle (`first`) and the group's number of j-tiles (`tiles`, 0: nobody to be compared with).
//   the rounds             the host knows the groups' sizes only on average (the offsets are on the device), so it cannot size the
//                          words for the largest group: it hands out `slots` (<= 64, option "conflict_slots") tile slots per vehicle
//                          and repeats the discovery in ROUNDS over the slots [T0, T0 + slots) until ceil(B / 64), the most a group can
//                          have, is covered.  A batch of up to 4 096 is one round whatever its groups.
//   conflict_count_kernel  (the offsets call) per vehicle: the popcounts of the round's words added up; the last round leaves the
//                          counts as the totals of the scan behind every offset table here (uavac_launch_totals_scan)
//   conflict_list_kernel   (the fill call) per vehicle: its words of the round in tile order, bit by bit -- ascending partners,
//                          ascending entry indices -- into row 0 of its slice, and who owns the entry into scratch.  Bounded: an
//                          entry is written iff it lies inside [pair_offsets[b], pair_offsets[b + 1]), at or above 0 and below
//                          `capacity`; what does not fit raises flag 2 (capacity) or, the last round, flag 0 (the slice holds another
//                          number of entries than the vehicle has partners: the input changed between the two calls).
//   csr_offsets / csr_list the round drivers of the two calls; `discover(T0)` enqueues the caller's discovery of one round.
//   pair_d2, Measure       the ends the two measure kernels share, whichever way they lay their lanes out: a pair-row's d^2, the
//                          result of a listed pair (update per row, merge of two partial results, the write with the sentinels)
// `takes_part` [B] (may be NULL: everybody does): 0 for a vehicle whose lanes walked garbage in the discovery -- a plan's EXCLUDED
// mission --, which lists nothing whatever its words hold.
#pragma once

#include "uavac_internal.h"
#include "uavac_scratch.h"
#include "mission_walk.h"
#include "separation_reduce.h"

namespace {

namespace csr {

using mission_walk::block_inclusive_scan_256;
using sepred::kTile;

constexpr int kMaxSlots = 64;                               // tile slots per vehicle and round: 512 bytes of words per vehicle at most

// a vehicle's words of the round: the slots [0, n) hold the tiles T0 .. T0 + n - 1 of its group
__device__ __forceinline__ int round_slots(const int32_t *__restrict__ takes_part, const int32_t *__restrict__ tiles, int b, int T0,
                                           int slots) {
    if (takes_part && takes_part[b] == 0) return 0;
    const int n = tiles[b] - T0;
    return n < 0 ? 0 : (n > slots ? slots : n);
}

// ------------------------------------------------------------------------------------------------------------------ the counts
__global__ void __launch_bounds__(256) conflict_count_kernel(const int32_t *__restrict__ takes_part, const int32_t *__restrict__ tiles,
                                                             const unsigned long long *__restrict__ words, int B, int T0, int slots, int last,
                                                             int32_t *__restrict__ count, int32_t *__restrict__ totals,
                                                             int64_t *__restrict__ tile_sum) {
    __shared__ int64_t wsum[4];
    const int b = blockIdx.x * 256 + threadIdx.x;
    int c = 0;
    if (b < B) {
        c = T0 == 0 ? 0 : count[b];
        const int n = round_slots(takes_part, tiles, b, T0, slots);
        for (int s = 0; s < n; ++s) c += __popcll(words[(size_t)s * B + b]);
        count[b] = c;
    }
    if (last) {                                              // (uniform) the totals and the workgroup sums of uavac_launch_totals_scan
        if (b < B) totals[b] = c;
        const int64_t inc = block_inclusive_scan_256(c, wsum);
        if (threadIdx.x == 255) tile_sum[blockIdx.x] = inc;
    }
}

// ------------------------------------------------------------------------------------------------------------------ the list
__global__ void __launch_bounds__(256) conflict_list_kernel(const int32_t *__restrict__ takes_part, const int32_t *__restrict__ first,
                                                            const int32_t *__restrict__ tiles, const unsigned long long *__restrict__ words,
                                                            int B, int T0, int slots, int last, const int64_t *__restrict__ pair_offsets,
                                                            long long capacity, int32_t *__restrict__ found, int32_t *__restrict__ owner,
                                                            int32_t *__restrict__ pair_i, int32_t *__restrict__ flags) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const long long lo = pair_offsets[b], hi = pair_offsets[b + 1];
    int f = T0 == 0 ? 0 : found[b];
    const int n = round_slots(takes_part, tiles, b, T0, slots), g0 = first[b];
    bool full = false;
    for (int s = 0; s < n; ++s) {
        unsigned long long word = words[(size_t)s * B + b];
        while (word) {
            const int j = g0 + (T0 + s) * kTile + __builtin_ctzll(word);
            word &= word - 1;
            const long long at = lo + f;
            ++f;
            if (at < 0 || at >= hi) continue;                // not in the vehicle's slice: flag 0 below
            if (at >= capacity) { full = true; continue; }   // the buffers end inside the slice
            pair_i[at] = j;
            owner[at] = b;
        }
    }
    found[b] = f;
    if (full) atomicOr(&flags[2], 1);
    if (last && (long long)f != hi - lo) atomicOr(&flags[0], 1);
}

// ------------------------------------------------------------------------------------------------------------------ the measure
// What the two measure kernels do with a listed pair's positions, whichever way their lanes are laid out.  The distance WITHOUT
// contraction, as everywhere (ROUNDING, separation_reduce.h).
__device__ __forceinline__ double pair_d2(double xi, double yi, double zi, double xj, double yj, double zj) {
#pragma clang fp contract(off)
    const double dx = xi - xj, dy = yi - yj, dz = zi - zj;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return (xx + yy) + zz;
}

// One entry's result, whole or partial: the minimum (d^2, row), the first and the last row inside the radius, the rows inside.  Exact
// reductions that do not depend on order: a lexicographic minimum, a min, a max, a sum; a NaN d^2 is neither below the minimum nor inside.
struct Measure {
    double bd = std::numeric_limits<double>::infinity();
    int bk = sepred::kNone, first = sepred::kNone, last_in = -1, inside = 0;

    __device__ __forceinline__ void row(double d2, int k, double r2) {
        if (d2 < bd) { bd = d2; bk = k; }                    // (strict: the caller's rows ascend, the lowest row of a tie stays)
        if (d2 < r2) { first = min(first, k); last_in = max(last_in, k); ++inside; }
    }
    __device__ __forceinline__ void merge(double od, int ok, int ofirst, int olast, int oinside) {
        if (od < bd || (od == bd && ok < bk)) { bd = od; bk = ok; }
        first = min(first, ofirst);
        last_in = max(last_in, olast);
        inside += oinside;
    }
    // rows 1 .. 4 of entry e (row 0 is the partner, the list's): one correctly rounded sqrt and the sentinels
    __device__ __forceinline__ void write(double *__restrict__ pair_d, int32_t *__restrict__ pair_i, long long e, long long capacity) const {
        const size_t cap = (size_t)capacity;
        pair_d[e] = sqrt(bd);
        pair_i[cap + e] = first == sepred::kNone ? -1 : first;
        pair_i[2 * cap + e] = last_in;
        pair_i[3 * cap + e] = inside;
        pair_i[4 * cap + e] = bk == sepred::kNone ? -1 : bk;
    }
};

// ------------------------------------------------------------------------------------------------------------------ the host side
// What the two calls of a list share: the shares per window (the audits' rule), the tile slots per round and the rounds, the scratch.
struct Shape {
    int windows, P, slots, rounds;
    int32_t *count, *owner;                                  // per vehicle: entries counted / found so far; per entry: who listed it
    unsigned long long *words;
};

inline void shape_of(const uavac_ctx *ctx, int B, const int64_t *group_offsets, int G, Shape &s) {
    sepred::sep_shares(ctx, B, group_offsets, G, s.windows, s.P);
    const int most = s.windows;                              // j-tiles of the largest group there can be
    s.slots = ctx->conflict_slots > 0 ? ctx->conflict_slots : kMaxSlots;
    s.slots = s.slots > most ? most : s.slots;
    s.rounds = (most + s.slots - 1) / s.slots;
}

// The same for a list whose partners are ANOTHER batch of Bt vehicles (minsnap_conflicts_against.hip): the windows and the shares are
// the caller's, and the most j-tiles a group can have is ceil(Bt / 64), the partners' side, not the owners'.
inline void shape_of_sides(const uavac_ctx *ctx, int windows, int P, int Bt, Shape &s) {
    s.windows = windows;
    s.P = P;
    const int most = (Bt + kTile - 1) / kTile;               // j-tiles of the largest partner group there can be
    s.slots = ctx->conflict_slots > 0 ? ctx->conflict_slots : kMaxSlots;
    s.slots = s.slots > most ? most : s.slots;
    s.rounds = (most + s.slots - 1) / s.slots;
}

// count, words and owner on the caller's Scratch, beside the caller's own pieces
inline void shape_want(Scratch &scratch, Shape &s, int B, long long capacity) {
    scratch.want(&s.count, (size_t)B);
    scratch.want(&s.words, s.slots * (size_t)B);
    scratch.want(&s.owner, (size_t)capacity);
}

// the offsets call: per round the discovery and the counts, then the scan -> pair_offsets [B + 1]
template <class Discover>
int csr_offsets(uavac_ctx *ctx, const Shape &s, int B, const int32_t *takes_part, const int32_t *tiles, Discover discover,
                int64_t *pair_offsets) {
    int32_t *totals = nullptr;
    int64_t *tile_sums = nullptr;
    if (int rc = uavac_ensure_totals(ctx, B, &totals, &tile_sums)) return rc;
    for (int r = 0; r < s.rounds; ++r) {
        discover(r * s.slots);
        hipLaunchKernelGGL(conflict_count_kernel, dim3((B + 255) / 256), dim3(256), 0, ctx->stream, takes_part, tiles, s.words, B, r * s.slots,
                           s.slots, r == s.rounds - 1 ? 1 : 0, s.count, totals, tile_sums);
    }
    return uavac_launch_totals_scan(ctx, B, pair_offsets);
}

// the fill call up to the measure: nobody owns an entry yet, then per round the discovery and the list
template <class Discover>
int csr_list(uavac_ctx *ctx, const Shape &s, int B, const int32_t *takes_part, const int32_t *first, const int32_t *tiles, Discover discover,
             const int64_t *pair_offsets, long long capacity, int32_t *pair_i) {
    if (capacity > 0) UAVAC_HIP(ctx, hipMemsetAsync(s.owner, 0xff, (size_t)capacity * 4, ctx->stream));      // -1: nobody listed the entry
    for (int r = 0; r < s.rounds; ++r) {
        discover(r * s.slots);
        hipLaunchKernelGGL(conflict_list_kernel, dim3((B + 255) / 256), dim3(256), 0, ctx->stream, takes_part, first, tiles, s.words, B,
                           r * s.slots, s.slots, r == s.rounds - 1 ? 1 : 0, pair_offsets, capacity, s.count, s.owner, pair_i, ctx->d_flags);
    }
    return UAVAC_OK;
}

}  // namespace csr

}  // namespace
