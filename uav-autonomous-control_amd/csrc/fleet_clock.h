// What the fleet's pair kernels share ahead of the reduction (gfx950): the separation audit (minsnap_separation.hip), the start delays
// (minsnap_stagger.hip) and the offset layers (fleet_search.h) all put missions on one group clock and evaluate "the audit's" rows with
// "the audit's" rounding.  That is stated once, here:
//   group_range            a group's missions from its offsets, clamped to the batch (flown_separation.hip uses it too)
//   prepass_mission        the pre-pass of a mission: its row total, its clamped start, whether it is EXCLUDED, flag 0
//   clock_walk             a wavefront's 8 rows of a chunk for one mission: seek, 24 coefficients, position-only Horner
//   inside_row             one position against a j-tile's positions at the same clock row: is anybody inside the radius?
//   inside_cuboids         one position against the cuboids
// The tile's shape is sepred's (separation_reduce.h), which also holds what happens to the positions in the audits; a mission's segments,
// the forward walk over its row counts, the lanes of a group and the clock's bound are mission_walk.h's, which every kernel that walks a
// mission shares.
// ROUNDING (part of every contract, include/uavac.h): positions by the sampler's fma chain (minsnap_eval_pos) on the coefficients as
// the caller's hook leaves them -- untouched without one --, the distance WITHOUT contraction: dx = xi - xj, ..., d^2 = (dx dx + dy dy)
// + dz dz, each product and sum rounded on its own.
#pragma once

#include "uavac_internal.h"
#include "minsnap_eval.h"
#include "mission_walk.h"
#include "separation_reduce.h"

namespace fleet {

using namespace sepred;                                     // the tile's shape
using mission_walk::Mission;
using mission_walk::mission_of;
using mission_walk::seek;
using mission_walk::kMaxClock;

constexpr int kPreLanes = 16;                               // lanes per mission of the pre-pass
constexpr int kPreMissions = kWaves * (64 / kPreLanes);     // missions per workgroup of the pre-pass

// The missions [g0, g1) of group g (group_offsets == NULL: all B in one), clamped: malformed offsets must not leave the batch.
__device__ __forceinline__ void group_range(const int64_t *__restrict__ group_offsets, int g, int B, int &g0, int &g1) {
    const long long a0 = group_offsets ? group_offsets[g] : 0, a1 = group_offsets ? group_offsets[g + 1] : B;
    g0 = (int)(a0 < 0 ? 0 : (a0 > B ? B : a0));
    g1 = (int)(a1 < g0 ? g0 : (a1 > B ? B : a1));
}

// The pre-pass of one mission, sixteen lanes each (kThreads per workgroup, kPreMissions missions): its row total N -- 0 for an EXCLUDED
// mission (no rows, too many, or a coefficient that is not finite) -- into n_rows, its start row clamped to 0 .. 2^29 into start, and
// flag 0 for what the host cannot refuse.  True in the one lane that wrote mission b, which adds the caller's own record at start s.
__device__ __forceinline__ bool prepass_mission(const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows,
                                                const int64_t *__restrict__ seg_offsets, int B, int m,
                                                const int32_t *__restrict__ start_rows, int32_t *__restrict__ n_rows,
                                                int32_t *__restrict__ start, int32_t *__restrict__ flags, int &b, int &s) {
    const mission_walk::LaneGroup<kPreLanes, kWaves> G(B);
    b = G.b;
    const Mission M = mission_of(seg_offsets, G.shadow, m);
    const int32_t *rows_of = seg_rows + M.s0;
    const double *cm = coeffs + (size_t)M.s0 * 24;
    long long total = 0;                                     // the mission's rows: what the sampler's row offsets give it
    for (int q = 0; q < M.m; ++q) total += rows_of[q];
    double z = 0.0;                                          // stays 0 while every coefficient is finite (0 * inf and 0 * NaN are NaN)
    for (int k = G.l; k < M.m * 24; k += kPreLanes) z = fma(0.0, cm[k], z);
    z = mission_walk::group_reduce<kPreLanes>(z, mission_walk::Add());
    s = 0;
    if (!(G.live && G.l == 0)) return false;
    s = start_rows ? start_rows[b] : 0;
    const bool bad = s < 0 || s > kMaxClock;                 // cannot be refused by the host: clamped, and flag 0
    s = mission_walk::clamped_start(s);
    const bool too_long = total > kMaxClock;
    const bool excluded = !(z == 0.0) || total < 1 || too_long;
    n_rows[b] = excluded ? 0 : (int)total;
    start[b] = s;
    if (bad || too_long) atomicOr(&flags[0], 1);
    return true;
}

// the after-load hook of a walk that leaves the coefficients as they are (never called)
struct AsPlanned {
    __device__ __forceinline__ void operator()(double (&)[24]) const {}
};

// This wavefront's rows k0 .. k0 + 7 (below the horizon H) of the group clock for one mission of n rows (rows_of, cm, mb: its row
// counts, coefficients and segment count) that starts at clock row `start`: before it the mission waits on its first row, after its end
// it holds its last.  (s, base, cnt) is where the lane stands in the mission and is carried from chunk to chunk.  The segment of the
// chunk's first row is fetched unconditionally -- the 24 coefficients then live inside this call only, not around the clock loop, and
// are indexed by constants only -- and again on a segment change; HOOK: hook(c) is applied to them after every load, otherwise the
// arithmetic is the sampler's on the untouched coefficients.  each(r, k, x, y, z) takes the position of row r of the chunk, clock row k.
template <bool HOOK, class Hook, class Each>
__device__ __forceinline__ void clock_walk(const int32_t *__restrict__ rows_of, const double *__restrict__ cm, int mb, int n, int start,
                                           int k0, int H, double dt, int &s, int &base, int &cnt, Hook hook, Each each) {
    double c[24];
    seek(rows_of, mb, min(max(k0 - start, 0), n - 1), s, base, cnt);
    int loaded = s;
#pragma unroll
    for (int q = 0; q < 24; ++q) c[q] = cm[s * 24 + q];
    if constexpr (HOOK) hook(c);
#pragma nounroll
    for (int r = 0; r < kRows && k0 + r < H; ++r) {
        const int row = min(max(k0 + r - start, 0), n - 1);
        seek(rows_of, mb, row, s, base, cnt);
        if (s != loaded) {
#pragma unroll
            for (int q = 0; q < 24; ++q) c[q] = cm[s * 24 + q];
            if constexpr (HOOK) hook(c);
            loaded = s;
        }
        double x, y, z;
        minsnap_eval_pos<1>(c, (double)(int)(row - base) * dt, x, y, z);
        each(r, k0 + r, x, y, z);
    }
}

// The j-tile's side of a chunk: lane = partner, its positions into this wavefront's quarter of the LDS tile (`mine`, [row][64][3]); a
// partner that does not take part (n = 0: excluded, or past the tile's end) is a NaN position, which is never inside anything.
template <bool HOOK, class Hook>
__device__ __forceinline__ void clock_walk_to_tile(double *mine, int lane, const int32_t *__restrict__ rows_of, const double *__restrict__ cm,
                                                   int mb, int n, int start, int k0, int H, double dt, int &s, int &base, int &cnt,
                                                   Hook hook) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    clock_walk<HOOK>(rows_of, cm, mb, n, start, k0, H, dt, s, base, cnt, hook, [&](int r, int, double x, double y, double z) {
        double *o = mine + (r * kTile + lane) * 3;
        o[0] = n > 0 ? x : nan; o[1] = n > 0 ? y : nan; o[2] = n > 0 ? z : nan;
    });
}

// One row of the lane's candidate against the first n positions of a j-tile at the same clock row (row [64][3] in LDS, the same for
// every lane; n a multiple of kUnroll, the entries past the tile's last partner are NaN): is anybody inside?
__device__ __forceinline__ bool inside_row(const double *row, int n, double xi, double yi, double zi, double r2) {
#pragma clang fp contract(off)
    bool in = false;
#pragma nounroll
    for (int q = 0; q < n; q += kUnroll) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int jj = q + u;
            const double dx = xi - row[3 * jj], dy = yi - row[3 * jj + 1], dz = zi - row[3 * jj + 2];
            const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
            const double d2 = (xx + yy) + zz;
            in |= d2 < r2;
        }
    }
    return in;
}

// One position against the cuboids (box [n][6] in LDS: xmin xmax ymin ymax zmin zmax, the same for every lane, so a read is one
// broadcast; uniform trip count): the audit's inclusive test, so a NaN bound or an inverted box contains nothing.
__device__ __forceinline__ bool inside_cuboids(const double *box, int n, double px, double py, double pz) {
    bool in = false;
#pragma nounroll
    for (int q = 0; q < n; ++q) {
        const double *x = box + q * 6;
        in |= px >= x[0] && px <= x[1] && py >= x[2] && py <= x[3] && pz >= x[4] && pz <= x[5];
    }
    return in;
}

}  // namespace fleet
