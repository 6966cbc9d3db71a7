// The layer search itself (gfx950): the pre-pass and the decision kernel of the deconfliction by offset layers, as templates over OBS --
// without cuboids (minsnap_layer.hip, uavac_minsnap_layer_dev) and with them (minsnap_layer_obs.hip, uavac_minsnap_layer_obs_dev).  One
// copy of the pair search; every object file instantiates exactly its own kernels.  The contract is in include/uavac.h, the structure of
// the decision kernel is described at the head of minsnap_layer.hip, what OBS adds to it at the head of minsnap_layer_obs.hip.
#pragma once

#include "uavac_internal.h"
#include "minsnap_eval.h"

#include <limits>

namespace {

constexpr int kTile = 64;                                   // earlier missions per j-tile, and candidate layers per round: one per lane
constexpr int kWaves = 4;                                   // wavefronts per workgroup
constexpr int kRows = 8;                                    // clock rows of a chunk per wavefront
constexpr int kChunk = kWaves * kRows;                      // clock rows per chunk
constexpr int kThreads = 64 * kWaves;
constexpr int kRegion = kRows * kTile * 3;                  // doubles of the LDS tile per wavefront (12 KB; 48 KB per workgroup)
constexpr int kMaxClock = 1 << 29;                          // start rows and row totals above this cannot be clocked with int
constexpr int kUnroll = 8;                                  // partners per unrolled step of the pair loop
constexpr int kPreLanes = 16;                               // lanes per mission of the pre-pass
constexpr int kMaxGroup = UAVAC_LAYER_MAX_GROUP;            // missions of a group: their granted layers live in LDS
constexpr int kMaxCuboids = UAVAC_AUDIT_MAX_CUBOIDS;        // cuboids of the obstacle-aware search: their bounds live in LDS

struct Delta {
    double x, y, z;
};

// First segment and segment count of mission b: uniform (so == NULL) or ragged, clamped to 1 .. m like every ragged kernel clamps it.
struct Mission {
    long long s0;
    int m;
};
__device__ __forceinline__ Mission mission_of(const int64_t *__restrict__ so, int b, int m_uniform) {
    Mission M;
    if (so) {
        M.s0 = so[b];
        const long long n = so[b + 1] - M.s0;
        M.m = (int)(n < 1 ? 1 : (n > m_uniform ? m_uniform : n));
    } else {
        M.s0 = (long long)b * m_uniform;
        M.m = m_uniform;
    }
    return M;
}

// the offset of layer q on one axis: one rounded product
__device__ __forceinline__ double layer_offset(int q, double delta) {
#pragma clang fp contract(off)
    const double o = (double)q * delta;
    return o;
}

// c0 of a mission on layer q: the product and the sum are rounded one after the other; layer 0 adds nothing
__device__ __forceinline__ double layer_c0(double c0, int q, double delta) {
#pragma clang fp contract(off)
    const double o = (double)q * delta;
    const double moved = c0 + o;
    return q == 0 ? c0 : moved;
}

// ------------------------------------------------------------------------------------------------------------------ pre-pass
// (the audit's pre-pass, restated as stagger restates it: every object file holds exactly its own kernels)
// OBS: ilayer has a fourth row, `blocked`: 0 for a mission that is never examined.
template <bool OBS>
__global__ void __launch_bounds__(kThreads) layer_prepass_kernel(const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows,
                                                                 const int64_t *__restrict__ seg_offsets, int B, int m,
                                                                 const int32_t *__restrict__ start_rows, Delta delta,
                                                                 int32_t *__restrict__ n_rows, int32_t *__restrict__ start,
                                                                 int32_t *__restrict__ ilayer, double *__restrict__ offsets,
                                                                 int32_t *__restrict__ flags) {
    constexpr int kPerWave = 64 / kPreLanes;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = lane / kPreLanes, l = lane % kPreLanes;
    const int b = (blockIdx.x * kWaves + w) * kPerWave + g;
    const bool live = b < B;
    const Mission M = mission_of(seg_offsets, live ? b : B - 1, m);
    const int32_t *rows_of = seg_rows + M.s0;
    const double *cm = coeffs + (size_t)M.s0 * 24;
    long long total = 0;                                     // the mission's rows: what the sampler's row offsets give it
    for (int s = 0; s < M.m; ++s) total += rows_of[s];
    double z = 0.0;                                          // stays 0 while every coefficient is finite (0 * inf and 0 * NaN are NaN)
    for (int k = l; k < M.m * 24; k += kPreLanes) z = fma(0.0, cm[k], z);
#pragma unroll
    for (int d = kPreLanes / 2; d >= 1; d >>= 1) z += __shfl_xor(z, d);
    if (live && l == 0) {
        int s = start_rows ? start_rows[b] : 0;
        bool bad = s < 0 || s > kMaxClock;                   // cannot be refused by the host: clamped, and flag 0
        s = s < 0 ? 0 : (s > kMaxClock ? kMaxClock : s);
        const bool too_long = total > kMaxClock;
        const bool excluded = !(z == 0.0) || total < 1 || too_long;
        n_rows[b] = excluded ? 0 : (int)total;
        start[b] = s;
        ilayer[b] = 0; ilayer[(size_t)B + b] = -2; ilayer[2 * (size_t)B + b] = 0;     // "not examined", until the decision kernel says otherwise
        if (OBS) ilayer[3 * (size_t)B + b] = 0;
        double *o = offsets + 3 * (size_t)b;
        o[0] = layer_offset(0, delta.x); o[1] = layer_offset(0, delta.y); o[2] = layer_offset(0, delta.z);
        if (bad || too_long) atomicOr(&flags[0], 1);
    }
}

// ------------------------------------------------------------------------------------------------------------------ the decisions
// the segment of a mission's row r, walked forward from where the lane stood (rows only grow): the audit's walk
__device__ __forceinline__ void seek(const int32_t *__restrict__ rows_of, int mb, int r, int &s, int &base, int &cnt) {
    while (s + 1 < mb && r >= base + cnt) { base += cnt; ++s; cnt = rows_of[s]; }
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

template <bool OBS>
__global__ void __launch_bounds__(kThreads, 3) minsnap_layer_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
    const int64_t *__restrict__ group_offsets, const int32_t *__restrict__ n_rows, const int32_t *__restrict__ start, double r2, Delta delta,
    int max_steps, const double *__restrict__ cuboids, int n_cuboids, int32_t *__restrict__ ilayer, double *__restrict__ offsets,
    int32_t *__restrict__ flags) {
    __shared__ double tile[kWaves * kRegion];
    __shared__ int granted[kMaxGroup];                       // the layers decided so far, by position in the group
    __shared__ unsigned long long round_hits[2];             // the candidate lanes of a round that met somebody, over all wavefronts; two
                                                             // words taken in turn: a slow reader of one round's is not overtaken by the next clearing
    __shared__ double box[OBS ? kMaxCuboids * 6 : 1];        // OBS: the cuboids
    __shared__ unsigned long long round_blocks[OBS ? 2 : 1]; // OBS: the candidate lanes of a round that a cuboid refuses, taken in turn likewise
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long a0 = group_offsets ? group_offsets[blockIdx.x] : 0, a1 = group_offsets ? group_offsets[blockIdx.x + 1] : B;
    const int g0 = (int)(a0 < 0 ? 0 : (a0 > B ? B : a0));   // clamped: malformed offsets must not leave the batch
    const int g1 = (int)(a1 < g0 ? g0 : (a1 > B ? B : a1));
    if (g1 == g0) return;
    if (g1 - g0 > kMaxGroup) {                               // cannot be refused by the host: its missions stay "not examined", and flag 0
        if (threadIdx.x == 0) atomicOr(&flags[0], 1);
        return;
    }
    const int nc = OBS ? min(max(n_cuboids, 0), kMaxCuboids) : 0;      // (the host refuses anything else: LDS is never left)
    if (OBS) {                                               // (visible to everybody behind the first barrier of the first round)
        for (int k = threadIdx.x; k < nc * 6; k += kThreads) box[k] = cuboids[k];
    }
    double *mine = tile + w * kRegion;                       // this wavefront's quarter of the tile
    const size_t Bs = (size_t)B;

    int turn = 0;
    int h_prev = 0, earlier = 0;                             // the row past which every decided mission holds its last row; how many there are
    for (int i = g0; i < g1; ++i) {                          // (uniform: every thread walks the same missions and takes the same decisions)
        const int ni = __builtin_amdgcn_readfirstlane(n_rows[i]), si = __builtin_amdgcn_readfirstlane(start[i]);
        if (ni == 0) {                                       // excluded: nobody is checked against it (its record is the pre-pass's)
            if (threadIdx.x == 0) granted[i - g0] = 0;
            continue;
        }
        const bool search = OBS || earlier > 0;              // without cuboids the first included mission of a group is never moved
        int layer = 0, steps = search ? -1 : 0, blocked = 0;
        if (search) {
            const Mission Mi = mission_of(seg_offsets, i, m);
            const int32_t *irows = seg_rows + Mi.s0;
            const double *icm = coeffs + (size_t)Mi.s0 * 24;
            const int n_tiles = (OBS && earlier == 0) ? 0 : (i - g0 + kTile - 1) / kTile;     // (nobody before it: the cuboids alone decide)
            const int H = max(h_prev, si + ni);              // past it everybody holds a last row, on whatever layer
            for (int q0 = 0; q0 <= max_steps && steps < 0; q0 += kTile) {
                const int n_live = min(kTile, max_steps - q0 + 1);                    // candidates of this round (the lanes past them shadow the last)
                const unsigned long long live = n_live == kTile ? ~0ull : (1ull << n_live) - 1ull;
                const int ql = q0 + min(lane, n_live - 1);                            // this lane's layer
                turn ^= 1;
                unsigned long long &round_hit = round_hits[turn];
                unsigned long long &round_block = round_blocks[OBS ? turn : 0];
                if (threadIdx.x == 0) {
                    round_hit = 0;
                    if (OBS) round_block = 0;
                }
                __syncthreads();                             // (also: `granted` of the previous mission is visible from here)
                unsigned long long refused = 0;              // OBS: the round's blocked mask, complete
                if (OBS) {
                    // The mission's own rows 0 .. ni - 1 -- they cover its whole clock: before its start it holds row 0, after its end
                    // row ni - 1 -- in chunks of 32, wave w taking rows 8 w .. 8 w + 7 of each; every lane its candidate's position by the
                    // sampler's arithmetic on layer_c0: the bit is what the sampler writes for the plan shifted by ql * delta.
                    if (nc > 0) {
                        bool in = false;
                        int is = 0, ibase = 0, icnt = irows[0];
                        for (int k0 = w * kRows; k0 < ni; k0 += kChunk) {
                            double c[24];
                            seek(irows, Mi.m, k0, is, ibase, icnt);
                            int iloaded = is;
#pragma unroll
                            for (int q = 0; q < 24; ++q) c[q] = icm[is * 24 + q];
                            c[0] = layer_c0(c[0], ql, delta.x); c[1] = layer_c0(c[1], ql, delta.y); c[2] = layer_c0(c[2], ql, delta.z);
#pragma nounroll
                            for (int r = 0; r < kRows && k0 + r < ni; ++r) {
                                const int row = k0 + r;
                                seek(irows, Mi.m, row, is, ibase, icnt);
                                if (is != iloaded) {
#pragma unroll
                                    for (int q = 0; q < 24; ++q) c[q] = icm[is * 24 + q];
                                    c[0] = layer_c0(c[0], ql, delta.x); c[1] = layer_c0(c[1], ql, delta.y); c[2] = layer_c0(c[2], ql, delta.z);
                                    iloaded = is;
                                }
                                double xi, yi, zi;
                                minsnap_eval_pos<1>(c, (double)(int)(row - ibase) * dt, xi, yi, zi);
                                in |= inside_cuboids(box, nc, xi, yi, zi);
                            }
                        }
                        const unsigned long long found = __ballot(in);
                        if (lane == 0 && found) {            // the mask on its own, and as the seed of round_hit: a refused lane is "hit" already
                            __hip_atomic_fetch_or(&round_block, found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            __hip_atomic_fetch_or(&round_hit, found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                    }
                    __syncthreads();                         // the mask is complete before anybody decides or counts: no answer depends on timing
                    refused = round_block & live;
                }
                bool hit = false;
                unsigned long long told = 0;                 // what this wavefront has put into round_hit
                for (int t = 0; t < n_tiles; ++t) {
                    const int j0 = g0 + t * kTile;
                    const int n_val = min(kTile, i - j0);    // partners of this tile: the missions before i
                    const int n_pad = (n_val + kUnroll - 1) / kUnroll * kUnroll;
                    const bool jvalid = lane < n_val;
                    const int jb = jvalid ? j0 + lane : j0;
                    const Mission Mj = mission_of(seg_offsets, jb, m);
                    const int32_t *jrows = seg_rows + Mj.s0;
                    const double *jcm = coeffs + (size_t)Mj.s0 * 24;
                    const int nj = jvalid ? n_rows[jb] : 0, sj = start[jb], lj = granted[jb - g0];
                    int js = 0, jbase = 0, jcnt = jrows[0];
                    int is = 0, ibase = 0, icnt = irows[0];
                    for (int k0 = w * kRows; k0 < H; k0 += kChunk) {
                        const bool over = (__hip_atomic_load(&round_hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & live) == live;
                        if (__builtin_amdgcn_readfirstlane((int)over)) break;       // no candidate of this round can be clear any more
                        {                                    // the j-tile's positions at this wavefront's rows of the chunk
                            double cj[24];
                            seek(jrows, Mj.m, min(max(k0 - sj, 0), nj - 1), js, jbase, jcnt);
                            int jloaded = js;
#pragma unroll
                            for (int q = 0; q < 24; ++q) cj[q] = jcm[js * 24 + q];
                            cj[0] = layer_c0(cj[0], lj, delta.x); cj[1] = layer_c0(cj[1], lj, delta.y); cj[2] = layer_c0(cj[2], lj, delta.z);
#pragma nounroll
                            for (int r = 0; r < kRows && k0 + r < H; ++r) {
                                const int row = min(max(k0 + r - sj, 0), nj - 1);
                                seek(jrows, Mj.m, row, js, jbase, jcnt);
                                if (js != jloaded) {
#pragma unroll
                                    for (int q = 0; q < 24; ++q) cj[q] = jcm[js * 24 + q];
                                    cj[0] = layer_c0(cj[0], lj, delta.x); cj[1] = layer_c0(cj[1], lj, delta.y);
                                    cj[2] = layer_c0(cj[2], lj, delta.z);
                                    jloaded = js;
                                }
                                double x, y, z;
                                minsnap_eval_pos<1>(cj, (double)(int)(row - jbase) * dt, x, y, z);
                                double *o = mine + (r * kTile + lane) * 3;
                                o[0] = nj > 0 ? x : nan; o[1] = nj > 0 ? y : nan; o[2] = nj > 0 ? z : nan;
                            }
                        }
                        lds_wave_fence();                    // (a wavefront reads only its own quarter)
                        double c[24];                        // the mission's own segment (the same for every lane), c0 on the lane's layer
                        seek(irows, Mi.m, min(max(k0 - si, 0), ni - 1), is, ibase, icnt);
                        int iloaded = is;
#pragma unroll
                        for (int q = 0; q < 24; ++q) c[q] = icm[is * 24 + q];
                        c[0] = layer_c0(c[0], ql, delta.x); c[1] = layer_c0(c[1], ql, delta.y); c[2] = layer_c0(c[2], ql, delta.z);
#pragma nounroll
                        for (int r = 0; r < kRows && k0 + r < H; ++r) {
                            const int row = min(max(k0 + r - si, 0), ni - 1);
                            seek(irows, Mi.m, row, is, ibase, icnt);
                            if (is != iloaded) {
#pragma unroll
                                for (int q = 0; q < 24; ++q) c[q] = icm[is * 24 + q];
                                c[0] = layer_c0(c[0], ql, delta.x); c[1] = layer_c0(c[1], ql, delta.y); c[2] = layer_c0(c[2], ql, delta.z);
                                iloaded = is;
                            }
                            double xi, yi, zi;
                            minsnap_eval_pos<1>(c, (double)(int)(row - ibase) * dt, xi, yi, zi);
                            hit |= inside_row(mine + r * kTile * 3, n_pad, xi, yi, zi, r2);
                        }
                        lds_wave_fence();
                        const unsigned long long now = __ballot(hit);
                        if (now != told) {
                            if (lane == 0) __hip_atomic_fetch_or(&round_hit, now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            told = now;
                        }
                    }
                }
                __syncthreads();                             // (every wavefront has put in what it found: after each chunk)
                const unsigned long long clear = ~round_hit & live;
                if (clear) {                                 // the lowest clear candidate
                    steps = q0 + __builtin_ctzll(clear);
                    layer = steps;
                }
                if (OBS)                                     // the refused candidates below the granted one, or all of a round without one
                    blocked += __builtin_popcountll(clear ? refused & ((1ull << __builtin_ctzll(clear)) - 1ull) : refused);
            }
        }
        if (threadIdx.x == 0) {
            granted[i - g0] = layer;
            ilayer[i] = layer; ilayer[Bs + i] = steps; ilayer[2 * Bs + i] = earlier;
            if (OBS) ilayer[3 * Bs + i] = blocked;
            double *o = offsets + 3 * (size_t)i;
            o[0] = layer_offset(layer, delta.x); o[1] = layer_offset(layer, delta.y); o[2] = layer_offset(layer, delta.z);
        }
        h_prev = max(h_prev, si + ni);
        ++earlier;
    }
}

// The two launches of a search, on the ctx stream: scratch (row totals and clamped starts) from the ctx arena.
template <bool OBS>
int launch_layer_search(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                        const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, Delta delta, int max_steps,
                        const double *cuboids, int n_cuboids, int32_t *ilayer, double *offsets) {
    const size_t Bs = (size_t)B;
    if (int rc = uavac_arena_reserve(ctx, 2 * uavac_arena_size(Bs * 4))) return rc;
    int32_t *n_rows = static_cast<int32_t *>(uavac_arena_take(ctx, Bs * 4)), *start = static_cast<int32_t *>(uavac_arena_take(ctx, Bs * 4));
    if (!n_rows || !start) return uavac_fail(ctx, UAVAC_ENOMEM, "layer: scratch arena too small");
    const int per_wg = kWaves * (64 / kPreLanes);
    hipLaunchKernelGGL(layer_prepass_kernel<OBS>, dim3((B + per_wg - 1) / per_wg), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows, seg_offsets,
                       B, m, start_rows, delta, n_rows, start, ilayer, offsets, ctx->d_flags);
    hipLaunchKernelGGL(minsnap_layer_kernel<OBS>, dim3(group_offsets ? G : 1), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows, seg_offsets, B,
                       m, dt, group_offsets, n_rows, start, radius * radius, delta, max_steps, cuboids, n_cuboids, ilayer, offsets,
                       ctx->d_flags);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}

}  // namespace
