// The fleet's prioritised search (gfx950): one decision kernel body for the deconfliction by start delay (minsnap_stagger.hip,
// uavac_minsnap_stagger_dev), by offset layers (minsnap_layer.hip, uavac_minsnap_layer_dev) and by offset layers that keep out of cuboids
// (minsnap_layer_obs.hip, uavac_minsnap_layer_obs_dev).  One copy of the search; every object file instantiates exactly its own kernels.
// The contracts are in include/uavac.h.
//
//   fleet_search<Policy>   the decisions.  One workgroup of four wavefronts per group walks the group's included missions in ascending
//                          order: the only sequential part.  For mission i THE 64 LANES ARE 64 CANDIDATES of that one mission, lane l
//                          is candidate q0 + l.  The rest is the audit's pair loop (fleet_clock.h): the earlier missions in j-tiles of 64,
//                          the clock from 0 to the horizon in chunks of 32 rows, wave w taking rows 8 w .. 8 w + 7; for its rows a wave
//                          evaluates the j-tile's positions AS THEY WERE GRANTED into its own quarter of the LDS tile (lane = j), then
//                          each lane evaluates its own candidate and reads the partners as LDS broadcasts.  A lane keeps one bit:
//                          somebody was inside.  Partners at or after i, excluded ones and the lanes past the tile's end are NaN
//                          positions: never inside.  After the last tile the four waves OR their bits through LDS and every thread
//                          takes the same decision: the lowest clear lane with q <= max_steps is granted; if there is none, the next
//                          64 candidates are examined; after the last candidate the mission is unresolved and stays where it was.  A
//                          mission that is clear at q = 0 costs one pass.  The OR lives in one LDS word (`round_hit`) that every wave
//                          feeds after each chunk in which a lane of its met somebody; once every live candidate is in it the round's
//                          answer is "none" whatever else would be found, and every wave leaves the round at its next chunk: reading
//                          the word early or late changes the time only.
//   the policy             what a candidate IS: Delay -- a start S_i + q * step, the mission as planned --, Layer -- the fixed start,
//                          the mission with fl(q * delta) added to c0 of every segment --, LayerObs -- Layer, and a candidate that puts
//                          a row of the mission's own into a cuboid is refused before the round (see minsnap_layer_obs.hip).
// What was granted in the group lives in LDS (256 int32: hence UAVAC_STAGGER_MAX_GROUP and UAVAC_LAYER_MAX_GROUP).  A workgroup never
// waits for another one, and nothing is spun on anywhere: round_hit is looked at once per chunk; the only atomic on global memory is
// the sticky flag.  Every decision is a comparison d^2 < r^2 on the audit's arithmetic, the horizon only has to reach the row past
// which both stand still (a longer one gives the same answer), so the outputs depend neither on the tile or chunk sizes nor on what
// else is in the batch.
//   fleet_search<Policy, true>   the BLOCK-WISE form (fleet_wide.h: groups of any size): a launch decides block k of every group --
//                          `blk` consecutive missions -- and nothing else.  `granted[]`, the j-tiles and the walk are the block's;
//                          `earlier` and the horizon come from the group's carry, which the launch of block k - 1 left in scratch;
//                          what the missions of the blocks before did to the candidates arrives as the start value of `round_hit`
//                          (the seed kernel of fleet_wide.h, one bit per candidate).  The narrow instantiations compile to what
//                          they compiled to before the form existed: every difference is an `if constexpr`.
#pragma once

#include "fleet_clock.h"
#include "uavac_scratch.h"

#include <limits>

namespace {

using namespace fleet;

constexpr int kMaxCuboids = UAVAC_AUDIT_MAX_CUBOIDS;        // cuboids of the obstacle-aware search: their bounds live in LDS

struct Delta {
    double x, y, z;
};

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

// the after-load hook of a mission on layer q (fleet_clock.h, clock_walk)
struct OnLayer {
    int q;
    Delta delta;
    __device__ __forceinline__ void operator()(double (&c)[24]) const {
        c[0] = layer_c0(c[0], q, delta.x); c[1] = layer_c0(c[1], q, delta.y); c[2] = layer_c0(c[2], q, delta.z);
    }
};

// ------------------------------------------------------------------------------------------------------------------ the policies
// What is granted to a mission is one int (`granted[]` in LDS): its start under Delay, its layer under Layer.
//   kMoves / hook      whether a grant changes the coefficients, and the hook of a mission with that grant
//   kObs               the cuboid pre-round, and the first included mission of a group is searched too
//   grant(si, q)       what candidate q of a mission with base start si is granted (q = 0: the mission as it is)
//   start_of           the clock row at which a mission with base start si and that grant starts
//   horizon            the row past which the mission on any candidate up to q_last, and everybody decided before (h_prev), holds a last row
//   record             the outputs of mission i
//   grants             row 0 of those outputs, where the grants of the missions decided by earlier LAUNCHES are read (fleet_wide.h)
struct Delay {
    static constexpr bool kMoves = false, kObs = false;
    static constexpr int kMaxGroup = UAVAC_STAGGER_MAX_GROUP;
    int step;
    int32_t *__restrict__ istag;
    __device__ __forceinline__ int grant(int si, int q) const { return si + q * step; }       // (<= 2^30: checked by the host)
    __device__ __forceinline__ int start_of(int, int granted) const { return granted; }
    __device__ __forceinline__ AsPlanned hook(int) const { return {}; }
    __device__ __forceinline__ int horizon(int h_prev, int si, int ni, int q_last) const { return max(h_prev, si + q_last * step + ni); }
    __device__ __forceinline__ void record(size_t B, int i, int granted, int steps, int earlier, int) const {
        istag[i] = granted; istag[B + i] = steps; istag[2 * B + i] = earlier;
    }
    __device__ __forceinline__ const int32_t *grants() const { return istag; }
};

template <bool OBS>
struct OnLayers {
    static constexpr bool kMoves = true, kObs = OBS;
    static constexpr int kMaxGroup = UAVAC_LAYER_MAX_GROUP;
    Delta delta;
    int32_t *__restrict__ ilayer;
    double *__restrict__ offsets;
    __device__ __forceinline__ int grant(int, int q) const { return q; }
    __device__ __forceinline__ int start_of(int si, int) const { return si; }
    __device__ __forceinline__ OnLayer hook(int granted) const { return {granted, delta}; }
    __device__ __forceinline__ int horizon(int h_prev, int si, int ni, int) const { return max(h_prev, si + ni); }
    __device__ __forceinline__ void record(size_t B, int i, int granted, int steps, int earlier, int blocked) const {
        ilayer[i] = granted; ilayer[B + i] = steps; ilayer[2 * B + i] = earlier;
        if (OBS) ilayer[3 * B + i] = blocked;
        double *o = offsets + 3 * (size_t)i;
        o[0] = layer_offset(granted, delta.x); o[1] = layer_offset(granted, delta.y); o[2] = layer_offset(granted, delta.z);
    }
    __device__ __forceinline__ const int32_t *grants() const { return ilayer; }
};
using Layer = OnLayers<false>;
using LayerObs = OnLayers<true>;

// What a launch of the block-wise form knows beside the search's arguments (fleet_wide.h lays the scratch out and fills it).
struct Block {
    int k, blk, group_cap;                                   // the block's number; missions per block (a multiple of kTile, at most
                                                             // kMaxGroup); the caller's bound on a group: a larger one is not examined
    unsigned long long *seed;                                // [B][words]: bit l of seed[i][r] = candidate 64 r + l of mission i meets a
    int words;                                               // mission of an earlier block of its group
    int32_t *carry;                                          // [groups][2]: the included missions decided so far, and their horizon
};

// ------------------------------------------------------------------------------------------------------------------ the decisions
// (the body of a __global__ kernel of kThreads threads and one workgroup per group: see the head of this file)
template <class Policy, bool WIDE = false>
__device__ __forceinline__ void fleet_search(const Policy pol, const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows,
                                             const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
                                             const int64_t *__restrict__ group_offsets, const int32_t *__restrict__ n_rows,
                                             const int32_t *__restrict__ start, double r2, int max_steps, const double *__restrict__ cuboids,
                                             int n_cuboids, int32_t *__restrict__ flags, const Block wide = {}) {
    constexpr bool OBS = Policy::kObs;
    __shared__ double tile[kWaves * kRegion];
    __shared__ int granted[Policy::kMaxGroup];               // what was decided so far, by position in the group
    __shared__ unsigned long long round_hits[2];             // the candidate lanes of a round that met somebody, over all wavefronts; two
                                                             // words taken in turn: a slow reader of one round's is not overtaken by the next clearing
    __shared__ double box[OBS ? kMaxCuboids * 6 : 1];        // OBS: the cuboids
    __shared__ unsigned long long round_blocks[OBS ? 2 : 1]; // OBS: the candidate lanes of a round that a cuboid refuses, taken in turn likewise
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int g0, g1;
    group_range(group_offsets, blockIdx.x, B, g0, g1);
    if (g1 == g0) return;
    if (g1 - g0 > (WIDE ? wide.group_cap : Policy::kMaxGroup)) {       // cannot be refused by the host: its missions stay "not examined", and flag 0
        if (threadIdx.x == 0) atomicOr(&flags[0], 1);
        return;
    }
    int b0 = g0, b1 = g1;                                    // the missions this launch decides; WIDE: block k of the group, if it has one
    if constexpr (WIDE) {
        b0 = g0 + wide.k * wide.blk; b1 = min(g1, b0 + wide.blk);
        if (b0 >= g1) return;
    }
    const int nc = OBS ? min(max(n_cuboids, 0), kMaxCuboids) : 0;      // (the host refuses anything else: LDS is never left)
    if (OBS) {                                               // (visible to everybody behind the first barrier of the first round)
        for (int k = threadIdx.x; k < nc * 6; k += kThreads) box[k] = cuboids[k];
    }
    double *mine = tile + w * kRegion;                       // this wavefront's quarter of the tile

    int turn = 0;
    int h_prev = 0, earlier = 0;                             // the row past which every decided mission holds its last row; how many there are
    if constexpr (WIDE) {                                    // (what the launch of the block before left; zeros ahead of block 0)
        earlier = __builtin_amdgcn_readfirstlane(wide.carry[2 * blockIdx.x]);
        h_prev = __builtin_amdgcn_readfirstlane(wide.carry[2 * blockIdx.x + 1]);
    }
    for (int i = b0; i < b1; ++i) {                          // (uniform: every thread walks the same missions and takes the same decisions)
        const int ni = __builtin_amdgcn_readfirstlane(n_rows[i]), si = __builtin_amdgcn_readfirstlane(start[i]);
        if (ni == 0) {                                       // excluded: nobody is checked against it (its record is the pre-pass's)
            if (threadIdx.x == 0) granted[i - b0] = pol.grant(si, 0);
            continue;
        }
        const bool search = OBS || earlier > 0;              // without cuboids the first included mission of a group stays as it is
        int steps = search ? -1 : 0, blocked = 0;
        if (search) {
            const Mission Mi = mission_of(seg_offsets, i, m);
            const int32_t *irows = seg_rows + Mi.s0;
            const double *icm = coeffs + (size_t)Mi.s0 * 24;
            const int n_tiles = (OBS && earlier == 0) ? 0 : (i - b0 + kTile - 1) / kTile;     // (nobody before it: the cuboids alone decide)
            for (int q0 = 0; q0 <= max_steps && steps < 0; q0 += kTile) {
                const int n_live = min(kTile, max_steps - q0 + 1);                    // candidates of this round (the lanes past them shadow the last)
                const unsigned long long live = n_live == kTile ? ~0ull : (1ull << n_live) - 1ull;
                const int gl = pol.grant(si, q0 + min(lane, n_live - 1));             // this lane's candidate
                const int sl = pol.start_of(si, gl);
                const int H = pol.horizon(h_prev, si, ni, q0 + n_live - 1);
                turn ^= 1;
                unsigned long long &round_hit = round_hits[turn];
                unsigned long long &round_block = round_blocks[OBS ? turn : 0];
                if (threadIdx.x == 0) {                      // (WIDE: the candidates that a mission of an earlier block is in the way of)
                    round_hit = WIDE ? wide.seed[(size_t)i * wide.words + q0 / kTile] & live : 0;
                    if (OBS) round_block = 0;
                }
                __syncthreads();                             // (also: `granted` of the previous mission is visible from here)
                unsigned long long refused = 0;              // OBS: the round's blocked mask, complete
                if constexpr (OBS) {
                    // The mission's own rows 0 .. ni - 1 -- they cover its whole clock: before its start it holds row 0, after its end
                    // row ni - 1 -- in chunks of 32, wave w taking rows 8 w .. 8 w + 7 of each; every lane its candidate's position by the
                    // sampler's arithmetic on the hooked coefficients: the bit is what the sampler writes for the plan on that candidate.
                    if (nc > 0) {
                        bool in = false;
                        int is = 0, ibase = 0, icnt = irows[0];
                        for (int k0 = w * kRows; k0 < ni; k0 += kChunk)
                            clock_walk<Policy::kMoves>(irows, icm, Mi.m, ni, 0, k0, ni, dt, is, ibase, icnt, pol.hook(gl),
                                                       [&](int, int, double xi, double yi, double zi) { in |= inside_cuboids(box, nc, xi, yi, zi); });
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
                    const int j0 = b0 + t * kTile;
                    const int n_val = min(kTile, i - j0);    // partners of this tile: the missions before i
                    const int n_pad = (n_val + kUnroll - 1) / kUnroll * kUnroll;
                    const bool jvalid = lane < n_val;
                    const int jb = jvalid ? j0 + lane : j0;
                    const Mission Mj = mission_of(seg_offsets, jb, m);
                    const int32_t *jrows = seg_rows + Mj.s0;
                    const double *jcm = coeffs + (size_t)Mj.s0 * 24;
                    const int nj = jvalid ? n_rows[jb] : 0, sb = start[jb], gj = granted[jb - b0];
                    const int sj = pol.start_of(sb, gj);
                    int js = 0, jbase = 0, jcnt = jrows[0];
                    int is = 0, ibase = 0, icnt = irows[0];
                    for (int k0 = w * kRows; k0 < H; k0 += kChunk) {
                        const bool over = (__hip_atomic_load(&round_hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & live) == live;
                        if (__builtin_amdgcn_readfirstlane((int)over)) break;       // no candidate of this round can be clear any more
                        // the j-tile's positions at this wavefront's rows of the chunk, then the lane's candidate against them (a
                        // wavefront reads only its own quarter)
                        clock_walk_to_tile<Policy::kMoves>(mine, lane, jrows, jcm, Mj.m, nj, sj, k0, H, dt, js, jbase, jcnt, pol.hook(gj));
                        lds_wave_fence();
                        clock_walk<Policy::kMoves>(irows, icm, Mi.m, ni, sl, k0, H, dt, is, ibase, icnt, pol.hook(gl),
                                                   [&](int r, int, double xi, double yi, double zi) {
                                                       hit |= inside_row(mine + r * kTile * 3, n_pad, xi, yi, zi, r2);
                                                   });
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
                if (clear) steps = q0 + __builtin_ctzll(clear);      // the lowest clear candidate
                if (OBS)                                     // the refused candidates below the granted one, or all of a round without one
                    blocked += __builtin_popcountll(clear ? refused & ((1ull << __builtin_ctzll(clear)) - 1ull) : refused);
            }
        }
        const int gi = pol.grant(si, max(steps, 0));         // (unresolved: the mission as it is)
        if (threadIdx.x == 0) {
            granted[i - b0] = gi;
            pol.record((size_t)B, i, gi, steps, earlier, blocked);
        }
        h_prev = max(h_prev, pol.start_of(si, gi) + ni);
        ++earlier;
    }
    if constexpr (WIDE) {                                    // for the launches of block k + 1
        if (threadIdx.x == 0) { wide.carry[2 * blockIdx.x] = earlier; wide.carry[2 * blockIdx.x + 1] = h_prev; }
    }
}

// ------------------------------------------------------------------------------------------------------------------ the layers' kernels
// (needed by two object files, minsnap_layer.o and minsnap_layer_obs.o, hence here; stagger's are in minsnap_stagger.hip and stagger_prepass.h)
// The pre-pass (fleet_clock.h) and the record of a mission that is never examined -- layer 0 / -2 / 0, OBS: blocked 0, and the offset
// of layer 0 -- which the decision kernel overwrites for everybody it decides.
template <bool OBS>
__global__ void __launch_bounds__(kThreads) layer_prepass_kernel(const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows,
                                                                 const int64_t *__restrict__ seg_offsets, int B, int m,
                                                                 const int32_t *__restrict__ start_rows, Delta delta,
                                                                 int32_t *__restrict__ n_rows, int32_t *__restrict__ start,
                                                                 int32_t *__restrict__ ilayer, double *__restrict__ offsets,
                                                                 int32_t *__restrict__ flags) {
    int b, s;
    if (!prepass_mission(coeffs, seg_rows, seg_offsets, B, m, start_rows, n_rows, start, flags, b, s)) return;
    ilayer[b] = 0; ilayer[(size_t)B + b] = -2; ilayer[2 * (size_t)B + b] = 0;
    if (OBS) ilayer[3 * (size_t)B + b] = 0;
    double *o = offsets + 3 * (size_t)b;
    o[0] = layer_offset(0, delta.x); o[1] = layer_offset(0, delta.y); o[2] = layer_offset(0, delta.z);
}

template <bool OBS>
__global__ void __launch_bounds__(kThreads, 3) minsnap_layer_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
    const int64_t *__restrict__ group_offsets, const int32_t *__restrict__ n_rows, const int32_t *__restrict__ start, double r2, Delta delta,
    int max_steps, const double *__restrict__ cuboids, int n_cuboids, int32_t *__restrict__ ilayer, double *__restrict__ offsets,
    int32_t *__restrict__ flags) {
    fleet_search(OnLayers<OBS>{delta, ilayer, offsets}, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, n_rows, start, r2, max_steps,
                 cuboids, n_cuboids, flags);
}

// The two launches of a search, on the ctx stream: scratch (row totals and clamped starts) from the ctx arena.
template <bool OBS>
int launch_layer_search(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                        const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, Delta delta, int max_steps,
                        const double *cuboids, int n_cuboids, int32_t *ilayer, double *offsets) {
    int32_t *n_rows = nullptr, *start = nullptr;
    Scratch s(ctx);
    s.want(&n_rows, B); s.want(&start, B);
    if (int rc = s.commit()) return rc;
    hipLaunchKernelGGL(layer_prepass_kernel<OBS>, dim3((B + kPreMissions - 1) / kPreMissions), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows,
                       seg_offsets, B, m, start_rows, delta, n_rows, start, ilayer, offsets, ctx->d_flags);
    hipLaunchKernelGGL(minsnap_layer_kernel<OBS>, dim3(group_offsets ? G : 1), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows, seg_offsets, B,
                       m, dt, group_offsets, n_rows, start, radius * radius, delta, max_steps, cuboids, n_cuboids, ilayer, offsets,
                       ctx->d_flags);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}

}  // namespace
