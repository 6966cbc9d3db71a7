// The reduction that the two separation audits share (gfx950): minsnap_separation.hip audits PLANS -- positions evaluated from the
// coefficients --, flown_separation.hip audits a FLIGHT -- positions read from the rollout's state log.  What happens to the positions
// once a wavefront holds them in its quarter of the LDS tile is the same in both, and stated once, here:
//   pair_row              one clock row of a lane's own position against the 64 partners of a j-tile (LDS broadcasts): the row's minimum
//                         and its partner, one bit per partner that came inside the radius
//   lex_less              the order of the contract: (d^2, clock row, partner)
//   sep_waves_leave/meet  the four wavefronts of a workgroup merge their results of a j-tile through the tile, which is dead by then
//   sep_merge_partials    the P partial records of a mission (one per workgroup that shared its window) merged the same way
//   sep_write             one correctly rounded sqrt and the sentinels
//   sep_shares            (host) the windows and the shares per window of a launch
// Every reduction is a lexicographic minimum, an integer sum over disjoint partners, an OR or an integer minimum: exact and independent
// of order.  ROUNDING (part of both contracts, include/uavac.h): the distance WITHOUT contraction, dx = xi - xj, ..., d^2 = (dx dx + dy
// dy) + dz dz, each product and sum rounded on its own.
#pragma once

#include "uavac_internal.h"

#include <cmath>
#include <limits>

namespace sepred {

constexpr int kTile = 64;                                   // missions per i-window and per j-tile: one per lane
constexpr int kWaves = 4;                                   // wavefronts per workgroup
constexpr int kRows = 8;                                    // clock rows of a chunk per wavefront
constexpr int kChunk = kWaves * kRows;                      // clock rows per chunk
constexpr int kThreads = 64 * kWaves;
constexpr int kRegion = kRows * kTile * 3;                  // doubles of the LDS tile per wavefront (12 KB; 48 KB per workgroup)
constexpr int kNone = 0x7fffffff;                           // "no row / no partner" while a minimum is being formed
constexpr int kUnroll = 8;                                  // partners per unrolled step of the pair loop

// (d, k, j) before (D, K, J) in the order of the contract: the smaller distance, then the lower row, then the lower partner
__device__ __forceinline__ bool lex_less(double d, int k, int j, double D, int K, int J) {
    return d < D || (d == D && (k < K || (k == K && j < J)));
}

// One row of the lane's own mission against the 64 positions of a j-tile at the same clock row (row [64][3] in LDS, the same for every
// lane).  rm / rkey: the row's minimum and the tile-local partner that gave it first; mask: bit jj is set once partner jj came inside.
template <bool SELF>
__device__ __forceinline__ void pair_row(const double *row, double xi, double yi, double zi, double r2, int selfjj, double &rm, int &rkey,
                                         unsigned long long &mask) {
#pragma clang fp contract(off)
    const double inf = std::numeric_limits<double>::infinity();
#pragma nounroll
    for (int q = 0; q < kTile / kUnroll; ++q) {
        unsigned in = 0;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int jj = q * kUnroll + u;
            const double dx = xi - row[3 * jj], dy = yi - row[3 * jj + 1], dz = zi - row[3 * jj + 2];
            const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
            double d2 = (xx + yy) + zz;
            if (SELF && jj == selfjj) d2 = inf;              // the lane's own mission is nobody's partner
            if (d2 < rm) { rm = d2; rkey = jj; }
            if (d2 < r2) in |= 1u << u;
        }
        mask |= (unsigned long long)in << (kUnroll * q);
    }
}

// The four wavefronts meet at the end of a j-tile.  Wavefronts 1 .. 3 leave their results -- minimum (d^2, row, partner), conflict
// bits, first row with anybody inside -- in their own quarters (`mine`); after a workgroup barrier wavefront 0 merges them into its
// own: the minima by the full lexicographic order, the bits by OR, the first rows by min.  (Another barrier before the tile is reused.)
__device__ __forceinline__ void sep_waves_leave(double *mine, int lane, double tb, int tk, int tj, unsigned long long mask, int tfirst) {
    int *q = reinterpret_cast<int *>(mine + 2 * kTile);
    mine[lane] = tb;
    reinterpret_cast<unsigned long long *>(mine)[kTile + lane] = mask;
    q[lane] = tk; q[kTile + lane] = tj; q[2 * kTile + lane] = tfirst;
}
__device__ __forceinline__ void sep_waves_meet(const double *tile, int lane, double &tb, int &tk, int &tj, unsigned long long &mask,
                                               int &tfirst) {
#pragma unroll
    for (int v = 1; v < kWaves; ++v) {
        const double *o = tile + v * kRegion;
        const int *q = reinterpret_cast<const int *>(o + 2 * kTile);
        const double od = o[lane];
        const int ok = q[lane], oj = q[kTile + lane];
        if (lex_less(od, ok, oj, tb, tk, tj)) { tb = od; tk = ok; tj = oj; }
        mask |= reinterpret_cast<const unsigned long long *>(o)[kTile + lane];
        tfirst = min(tfirst, q[2 * kTile + lane]);
    }
}
// a second set of bits takes the same way through the tile, past the record above (flown_separation.hip: the partners that were compared)
__device__ __forceinline__ void sep_waves_leave_bits(double *mine, int lane, unsigned long long bits) {
    reinterpret_cast<unsigned long long *>(mine)[4 * kTile + lane] = bits;
}
__device__ __forceinline__ void sep_waves_meet_bits(const double *tile, int lane, unsigned long long &bits) {
#pragma unroll
    for (int v = 1; v < kWaves; ++v) bits |= reinterpret_cast<const unsigned long long *>(tile + v * kRegion)[4 * kTile + lane];
}

// One partial record per mission b and share p: part_d2 [P][B] the minimum d^2, part_i [P][5][B] its partner, its row, the conflicts
// among the share's partners, the first row with one of them inside, and a fifth row that belongs to the caller.
__device__ __forceinline__ void sep_leave_partial(double *__restrict__ part_d2, int32_t *__restrict__ part_i, int p, int b, int B, double d,
                                                  int j, int k, int conf, int first, int fifth) {
    const size_t at = (size_t)p * 5 * B + b;
    part_d2[(size_t)p * B + b] = d;
    part_i[at] = j; part_i[at + B] = k; part_i[at + 2 * (size_t)B] = conf; part_i[at + 3 * (size_t)B] = first;
    part_i[at + 4 * (size_t)B] = fifth;
}
__device__ __forceinline__ void sep_merge_partials(const double *__restrict__ part_d2, const int32_t *__restrict__ part_i, int P, int b, int B,
                                                   double &d, int &k, int &j, int &conf, int &first) {
    const size_t Bs = (size_t)B;
    d = std::numeric_limits<double>::infinity();
    k = kNone; j = kNone; conf = 0; first = kNone;
    for (int p = 0; p < P; ++p) {
        const size_t at = (size_t)p * 5 * Bs + b;
        const double od = part_d2[(size_t)p * Bs + b];
        const int oj = part_i[at], ok = part_i[at + Bs];
        if (lex_less(od, ok, oj, d, k, j)) { d = od; k = ok; j = oj; }
        conf += part_i[at + 2 * Bs];
        first = min(first, part_i[at + 3 * Bs]);
    }
}
// the outputs of mission b from its merged record: one correctly rounded sqrt (+inf when no partner was compared), the sentinels
__device__ __forceinline__ void sep_write(double *__restrict__ sep, int32_t *__restrict__ isep, int b, int B, double d, int k, int j, int conf,
                                          int first, int compared) {
    const size_t Bs = (size_t)B;
    const bool any = k != kNone;
    sep[b] = sqrt(d);
    isep[b] = any ? j : -1;
    isep[Bs + b] = any ? k : -1;
    isep[2 * Bs + b] = conf;
    isep[3 * Bs + b] = first == kNone ? -1 : first;
    isep[4 * Bs + b] = compared;
}

// The launch shape of every kernel that sweeps the pairs (pair_sweep.h): the 64-vehicle windows of the batch, and the shares P per
// window -- a window's workgroups split the j-tiles of its group.  The host knows the groups' sizes only on average (B / G: the offsets
// are on the device), which is enough to see whether the windows alone give the chip enough workgroups to balance -- about four per
// SIMD -- or whether a few large groups have to be spread.  Measured at 4 096 missions in one group (64 windows): 1 / 8 / 12 / 24 / 64
// shares take 85.7 / 13.0 / 10.9 / 10.2 / 9.8 ms.  The results do not depend on it (option "separation_split").
inline void sep_shares(const uavac_ctx *ctx, int B, const int64_t *group_offsets, int G, int &windows, int &P) {
    windows = (B + kTile - 1) / kTile;
    P = ctx->separation_split;
    if (P <= 0) {
        const int groups = group_offsets ? G : 1;
        const int tiles = (B / groups + kTile - 1) / kTile;
        const int wanted = ctx->n_simds * 4;
        P = (wanted + windows - 1) / windows;
        P = P > tiles ? tiles : P;
    }
    P = P < 1 ? 1 : (P > UAVAC_SEP_MAX_SPLIT ? UAVAC_SEP_MAX_SPLIT : P);
}

}  // namespace sepred
