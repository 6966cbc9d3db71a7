// The sweep of the four pair kernels (gfx950): "which vehicles of a group come near each other, and when", asked of a PLAN or of a
// FLIGHT, answered as an audit record or as the bits of a conflict list.  One copy; a kernel is an instantiation in its own object:
//   conflict_discover_kernel   Planned + Bits        flown_separation_kernel   Flown + Record        flown_discover_kernel   Flown + Bits
// (Planned + Record is the plan audit, minsnap_separation_kernel: it compiles and gives the same bits, but was measured 0.3 % slower
// than its own body at one shape, and so minsnap_separation.hip keeps that body: the same loop nest, written out.)
// THE SWEEP.  A workgroup owns the 64 consecutive vehicles [64 x, 64 x + 64) of the batch, one per lane (i), and visits every group that
// reaches into this window, with the lanes of other groups idle; the group loop is uniform, every thread of the workgroup sees the same
// groups and meets the same barriers.  Per group it walks the group's vehicles in j-tiles of 64 and, per j-tile, the group's clock from
// 0 to its horizon in chunks of 32 rows.  The four wavefronts split each chunk: wave w takes rows 8 w .. 8 w + 7.  For its rows a wave
// first puts the j-tile's positions into its own quarter of the LDS tile as [row][64][3] (lane = j), then takes its OWN position once
// per row (lane = i) and reads the 64 partners' as LDS broadcasts (pair_row, separation_reduce.h).  A wave reads only what it wrote
// itself: no workgroup barrier inside the clock loop, two wave fences around a chunk.  A partner that does not take part and a lane past
// the group's end are NaN positions: a NaN distance is never below anything, so they cost no instruction; the lane's own entry is
// turned into +inf in the one tile that holds it.  At the end of a j-tile the four waves meet through the tile, which is dead by then:
// 1 .. 3 leave their results in their quarters, wavefront 0 merges them.  gridDim.y = P workgroups share a window: of the tiles [T0,
// T0 + slots) of a round, share p takes those with t = p (mod P).  Every reduction is a lexicographic minimum, an integer sum over
// disjoint partners, an OR or an integer minimum, and every word or record has one writer: the same bits whatever P, the tile, the
// chunk or the neighbours in the batch.
// THE SOURCE says where positions come from:
//   Planned   the coefficients, walked on the group's clock (fleet_clock.h: forward segment walk, position-only Horner, the segment's
//             coefficients fetched per chunk).  The horizon is the latest end of a mission that takes part, found by the workgroup.
//   Flown     the state log [K][13][pitch], rows 0-2.  A j-tile's x, y and z at one tick are three coalesced 512-byte loads (consecutive
//             columns of one log row), 24 loads in flight per wave and chunk; the lane's own position is three loads of the same kind,
//             fetched one tick ahead of the pair loop.  The horizon is K and every vehicle of the group takes part.  Every column index
//             is below B (lanes past the batch or the group read column B - 1 or the group's last one and are masked).
// WHAT IS KEPT, per (vehicle, j-tile):
//   Record    the minimum (d^2, row, partner), the bits, the first row with anybody inside; per group one partial record per vehicle
//             and share in scratch (sep_leave_partial), one round without a slot bound
//   Bits      the 64 bits only, the merged word to words[(t - T0) * B + b]; share 0 of round 0 also leaves the group's first vehicle,
//             its horizon (where the caller wants it) and its j-tiles (0: fewer than two take part)
// Source and keep meet in one place, the record's fifth row, `compared`: a plan is compared with everybody else who takes part, a
// flight with the partners that had a VALID pair-tick.  A pair-tick counts iff its d^2 is not NaN; inside the contract that is: none of
// the six coordinates is NaN -- so, if the lane's own position is a number, the ballot of "my three coordinates are numbers" over the
// tile (lane = j, read back from the tile), one OR per tick instead of a comparison per pair, with the lane's own bit taken out.  Only
// Flown + Record compiles it (Source::kValidity, Keep::kCompared).
#pragma once

#include "fleet_clock.h"

#include <limits>

namespace pair_sweep {

using namespace fleet;                                      // the clock and, through it, sepred's tile and reduction

// -------------------------------------------------------------------------------------------------------------------- sources
struct Planned {
    static constexpr bool kValidity = false;                // (a mission takes part or not as a whole: n_rows)
    const double *__restrict__ coeffs;
    const int32_t *__restrict__ seg_rows;
    const int64_t *__restrict__ seg_offsets;
    int m;
    double dt;
    const int32_t *__restrict__ n_rows, *__restrict__ start;
    Mission Mi, Mj;                                          // the lane's own mission and its partner of the tile, and where each stands
    const int32_t *irows, *jrows;
    const double *icm, *jcm;
    int ni, si, nj, sj, is, ibase, icnt, js, jbase, jcnt;

    __device__ __forceinline__ void own(int bb) {
        Mi = mission_of(seg_offsets, bb, m);
        irows = seg_rows + Mi.s0;
        icm = coeffs + (size_t)Mi.s0 * 24;
        ni = n_rows[bb]; si = start[bb];
    }
    // the group's horizon and how many of its missions take part (two barriers: the tile is the meeting place)
    __device__ __forceinline__ void group(double *tile, int lane, int w, int g0, int g1, int &H, int &n_in) const {
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
        H = 0; n_in = 0;
#pragma unroll
        for (int v = 0; v < kWaves; ++v) { H = max(H, meet[2 * v]); n_in += meet[2 * v + 1]; }
        __syncthreads();
    }
    __device__ __forceinline__ void partner(int jb, bool jvalid) {
        Mj = mission_of(seg_offsets, jb, m);
        jrows = seg_rows + Mj.s0;
        jcm = coeffs + (size_t)Mj.s0 * 24;
        nj = jvalid ? n_rows[jb] : 0; sj = start[jb];
        js = 0; jbase = 0; jcnt = jrows[0];
        is = 0; ibase = 0; icnt = irows[0];
    }
    __device__ __forceinline__ void stage(double *mine, int lane, bool, int k0, int H) {
        clock_walk_to_tile<false>(mine, lane, jrows, jcm, Mj.m, nj, sj, k0, H, dt, js, jbase, jcnt, AsPlanned{});
    }
    template <class Each>
    __device__ __forceinline__ void rows(const double *mine, int k0, int H, Each each) {
        clock_walk<false>(irows, icm, Mi.m, ni, si, k0, H, dt, is, ibase, icnt, AsPlanned{},
                          [&](int r, int k, double xi, double yi, double zi) { each(r, k, xi, yi, zi, mine + r * kTile * 3); });
    }
};

struct Flown {
    static constexpr bool kValidity = true;                 // (a position may be NaN tick by tick)
    const double *__restrict__ slog;
    int K;
    long long pitch;
    const double *mine_col, *theirs;                         // the lane's own column and its partner's of the tile

    __device__ __forceinline__ void own(int bb) { mine_col = slog + bb; }
    __device__ __forceinline__ void group(double *, int, int, int g0, int g1, int &H, int &n_in) const { H = K; n_in = g1 - g0; }
    __device__ __forceinline__ void partner(int jb, bool) { theirs = slog + jb; }
    __device__ __forceinline__ void stage(double *mine, int lane, bool jvalid, int k0, int) {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        const long long tick = kLogRows * pitch;             // doubles from one tick of the log to the next
#pragma unroll
        for (int r = 0; r < kRows; ++r) {                    // (the ticks past the log's end repeat its last one: unused)
            const double *at = theirs + (long long)min(k0 + r, K - 1) * tick;
            const double x = at[0], y = at[pitch], z = at[2 * pitch];
            double *o = mine + (r * kTile + lane) * 3;
            o[0] = jvalid ? x : nan; o[1] = jvalid ? y : nan; o[2] = jvalid ? z : nan;
        }
    }
    template <class Each>
    __device__ __forceinline__ void rows(const double *mine, int k0, int, Each each) {
        const long long tick = kLogRows * pitch;
        const int n = min(kRows, K - k0);                    // this wavefront's ticks of the chunk
        const double *at = mine_col + (long long)k0 * tick;
        double nx = at[0], ny = at[pitch], nz = at[2 * pitch];      // the lane's own position, one tick ahead
#pragma nounroll
        for (int r = 0; r < n; ++r) {
            const int k = k0 + r;
            const double xi = nx, yi = ny, zi = nz;
            if (r + 1 < n) {
                at = mine_col + (long long)(k + 1) * tick;
                nx = at[0]; ny = at[pitch]; nz = at[2 * pitch];
            }
            each(r, k, xi, yi, zi, mine + r * kTile * 3);
        }
    }
};

__device__ __forceinline__ bool is_number(double x, double y, double z) { return x == x && y == y && z == z; }

// ---------------------------------------------------------------------------------------------------------------------- keeps
struct Record {
    static constexpr bool kCompared = true;
    static constexpr int T0 = 0;                            // one round over all the tiles
    double *__restrict__ part_d2;
    int32_t *__restrict__ part_i;
    double gb, tb;                                           // the group's results so far (held by wavefront 0); this wavefront's of the tile
    int gk, gj, gconf, gfirst, tk, tj, tfirst;

    __device__ __forceinline__ bool past(int) const { return false; }
    __device__ __forceinline__ int end(int live_tiles) const { return live_tiles; }
    __device__ __forceinline__ void begin_group(bool, int, int, int, int, int) {
        gb = std::numeric_limits<double>::infinity();
        gk = kNone; gj = kNone; gconf = 0; gfirst = kNone;
    }
    __device__ __forceinline__ void begin_tile() {
        tb = std::numeric_limits<double>::infinity();
        tk = kNone; tj = kNone; tfirst = kNone;
    }
    __device__ __forceinline__ void row(double rm, int rkey, int k, int j0, double r2) {
        if (rm < tb) { tb = rm; tk = k; tj = j0 + rkey; }
        if (rm < r2) tfirst = min(tfirst, k);
    }
    __device__ __forceinline__ void leave(double *mine, int lane, unsigned long long mask) const {
        sep_waves_leave(mine, lane, tb, tk, tj, mask, tfirst);
    }
    __device__ __forceinline__ void meet(const double *tile, int lane, unsigned long long &mask, bool, int, int, int) {
        sep_waves_meet(tile, lane, tb, tk, tj, mask, tfirst);
        gconf += __popcll(mask);
        if (lex_less(tb, tk, tj, gb, gk, gj)) { gb = tb; gk = tk; gj = tj; }
        gfirst = min(gfirst, tfirst);
    }
    // one partial record per vehicle and share p (an excluded mission's is ignored); its fifth row: the partners compared
    __device__ __forceinline__ void end_group(int p, int b, int B, int compared) const {
        sep_leave_partial(part_d2, part_i, p, b, B, gb, gj, gk, gconf, gfirst, compared);
    }
};

template <bool HORIZON>                                     // whether the caller wants the group's horizon (a log's is K)
struct Bits {
    static constexpr bool kCompared = false;
    int T0, slots;                                           // the round's first j-tile and its tile slots (conflict_csr.h)
    unsigned long long *__restrict__ words;
    int32_t *__restrict__ first, *__restrict__ horizon, *__restrict__ tiles;      // [B] each

    __device__ __forceinline__ bool past(int n_tiles) const { return T0 >= n_tiles; }      // a later round than the group has tiles
    __device__ __forceinline__ int end(int live_tiles) const { return min(live_tiles, T0 + slots); }
    __device__ __forceinline__ void begin_group(bool writes, int p, int b, int g0, int H, int live_tiles) const {
        if (writes && p == 0 && T0 == 0) {
            first[b] = g0;
            if constexpr (HORIZON) horizon[b] = H;
            tiles[b] = live_tiles;
        }
    }
    __device__ __forceinline__ void begin_tile() const {}
    __device__ __forceinline__ void row(double, int, int, int, double) const {}      // (of pair_row's results only the bits are kept)
    __device__ __forceinline__ void leave(double *mine, int lane, unsigned long long mask) const { sep_waves_leave_bits(mine, lane, mask); }
    __device__ __forceinline__ void meet(const double *tile, int lane, unsigned long long &mask, bool act, int t, int b, int B) const {
        sep_waves_meet_bits(tile, lane, mask);
        if (act) words[(size_t)(t - T0) * (size_t)B + b] = mask;
    }
    __device__ __forceinline__ void end_group(int, int, int, int) const {}
};

// ------------------------------------------------------------------------------------------------------------------ the sweep
// tile: the workgroup's kWaves * kRegion doubles of LDS.  Launched as dim3(windows, P) x kThreads.
template <class Source, class Keep>
__device__ __forceinline__ void sweep(double *tile, Source src, Keep keep, int B, const int64_t *__restrict__ group_offsets, int G, double r2) {
    constexpr bool kSeen = Source::kValidity && Keep::kCompared;
    const double inf = std::numeric_limits<double>::infinity();
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int P = gridDim.y, p = blockIdx.y;
    __builtin_assume(p >= 0);                                // (what a launch guarantees: with T0 = 0 the start rule of the tile loop then
    __builtin_assume(P > 0);                                 // folds p % P to p, which saves the flown audit a scalar division per group)
    __builtin_assume((unsigned)p < (unsigned)P);
    const int w0 = blockIdx.x * kTile, w1 = w0 + kTile;      // the window of vehicles this workgroup owns
    const int b = w0 + lane;
    const bool live = b < B;
    src.own(live ? b : B - 1);                               // (a lane past the batch shadows the last vehicle)
    double *mine = tile + w * kRegion;                       // this wavefront's quarter of the tile

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
        const int n_tiles = (g1 - g0 + kTile - 1) / kTile;
        if (keep.past(n_tiles)) continue;
        const bool act = live && b >= g0 && b < g1;
        int H, n_in;                                         // the group's horizon and how many of its vehicles take part
        src.group(tile, lane, w, g0, g1, H, n_in);
        const int live_tiles = n_in >= 2 ? n_tiles : 0;
        keep.begin_group(w == 0 && act, p, b, g0, H, live_tiles);
        int gcomp = 0;
        const int t_end = keep.end(live_tiles);
        for (int t = keep.T0 + ((p - keep.T0) % P + P) % P; t < t_end; t += P) {      // this share's tiles of the round: t = p (mod P)
            const int j0 = g0 + t * kTile;
            const bool jvalid = j0 + lane < g1;
            src.partner(jvalid ? j0 + lane : g1 - 1, jvalid);
            const int selfjj = b - j0;
            const bool self_tile = j0 < w1 && j0 + kTile > w0;
            keep.begin_tile();
            unsigned long long mask = 0, seen = 0;           // partners that came inside the radius; partners with a valid pair-tick
            for (int k0 = w * kRows; k0 < H; k0 += kChunk) {
                // the j-tile's positions at this wavefront's rows of the chunk, then the lane's own against them (a wavefront reads only
                // its own quarter)
                src.stage(mine, lane, jvalid, k0, H);
                lds_wave_fence();
                src.rows(mine, k0, H, [&](int, int k, double xi, double yi, double zi, const double *row) {
                    if constexpr (kSeen) {
                        const unsigned long long numbers = __ballot(is_number(row[3 * lane], row[3 * lane + 1], row[3 * lane + 2]));
                        if (is_number(xi, yi, zi)) seen |= numbers;
                    }
                    double rm = inf;
                    int rkey = 0;
                    if (self_tile) pair_row<true>(row, xi, yi, zi, r2, selfjj, rm, rkey, mask);
                    else pair_row<false>(row, xi, yi, zi, r2, selfjj, rm, rkey, mask);
                    keep.row(rm, rkey, k, j0, r2);
                });
                lds_wave_fence();
            }
            if constexpr (kSeen) {
                if (selfjj >= 0 && selfjj < kTile) seen &= ~(1ull << selfjj);      // the lane's own vehicle is nobody's partner
            }
            // the four wavefronts meet: 1 .. 3 leave their results in their quarters, wavefront 0 merges
            if (w != 0) {
                keep.leave(mine, lane, mask);
                if constexpr (kSeen) sep_waves_leave_bits(mine, lane, seen);
            }
            __syncthreads();
            if (w == 0) {
                keep.meet(tile, lane, mask, act, t, b, B);
                if constexpr (kSeen) {
                    sep_waves_meet_bits(tile, lane, seen);
                    gcomp += __popcll(seen);
                }
            }
            __syncthreads();
        }
        if (w == 0 && act) keep.end_group(p, b, B, kSeen ? gcomp : n_in - 1);
    }
}

}  // namespace pair_sweep
