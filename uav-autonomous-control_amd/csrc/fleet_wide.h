// The prioritised search for groups of any size (gfx950): the block-wise form of fleet_search.h behind uavac_minsnap_stagger_wide_dev
// (minsnap_stagger_wide.hip) and uavac_minsnap_layer_wide_dev (minsnap_layer_wide.hip).  The contracts are in include/uavac.h; the
// rule is the narrow calls', and so is every answer.
//
// A group is cut into blocks of `blk` consecutive missions (64, 128 or 256: option "search_block").  Block k needs two launches:
//   fleet_seed<Policy>           k > 0 only, parallel over the whole chip.  For every included mission i of block k, every candidate q =
//                                0 .. max_steps and every mission j of the blocks 0 .. k - 1 of the group, AS IT WAS GRANTED (row 0 of
//                                the output block, which the launches before wrote; an unresolved one stands at candidate 0): is
//                                candidate q inside the radius of some j at some clock row?  One bit per (i, q), in seed[i][q / 64].
//                                The layout is the search's -- the 64 lanes are 64 candidates of one mission, rounds of 64 candidates,
//                                j-tiles of 64 partners in LDS, the clock in chunks of 32 rows, wave w rows 8 w .. 8 w + 7 -- and the
//                                arithmetic is the audit's (fleet_clock.h).  A workgroup takes one mission and every P-th j-tile; lane 0
//                                of a wave ORs the wave's ballot, the lanes past the last candidate masked out, into the word with an
//                                ordinary 64-bit atomicOr whenever it has changed.  All rounds are seeded: the kernel cannot know which
//                                candidate the search will take.  A workgroup leaves a round once every live candidate is hit in its
//                                LDS copy of the word, which starts from what the others have put there: early or late, the OR is the
//                                same.
//   fleet_search<Policy, true>   one workgroup per group decides the block's missions: fleet_search.h.
// and the launch order on the ctx stream, with no host read in between, is: the pre-pass; seed words and carries zeroed; for k = 0 ..
// ceil(group_cap / blk) - 1: seed(k) if k > 0, search(k).  No workgroup waits for another and nothing is spun on: order comes from the
// stream.  A workgroup whose group has no block k, or is larger than group_cap, exits at once.
// WHY THE ANSWERS ARE THE RULE'S.  A candidate is clear iff no partner decided before is inside the radius at any clock row: the blocks
// before contribute through the seed, the block's own missions through the search's loop, and an OR does not care how it is split.
// The horizon of a round only has to reach the row past which everybody concerned stands still -- max(the carry's horizon, the last
// candidate's end): a longer one gives the same answer (fleet_search.h).  So the outputs depend neither on blk nor on P.
#pragma once

#include "fleet_search.h"

#include <algorithm>

namespace {

constexpr int kWideBlock = 64;                              // missions per block when option "search_block" is 0: the fastest of the three for
                                                            // one group of 4 096 missions (tools/wide_rate.py)

// ------------------------------------------------------------------------------------------------------------------ the seed
// (the body of a __global__ kernel of kThreads threads; grid: x = group * blk + the mission's place in block k, y = the share of j-tiles)
template <class Policy>
__device__ __forceinline__ void fleet_seed(const Policy pol, const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows,
                                           const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
                                           const int64_t *__restrict__ group_offsets, const int32_t *__restrict__ n_rows,
                                           const int32_t *__restrict__ start, double r2, int max_steps, const Block wide) {
    __shared__ double tile[kWaves * kRegion];
    __shared__ unsigned long long round_hits[2];             // the workgroup's copy of the round's word, two taken in turn as in the search
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int g = (int)blockIdx.x / wide.blk;
    int g0, g1;
    group_range(group_offsets, g, B, g0, g1);
    if (g1 - g0 > wide.group_cap) return;                    // not examined (the search raises the flag)
    const int b0 = g0 + wide.k * wide.blk;                   // the partners are the missions g0 .. b0 - 1
    const int i = b0 + ((int)blockIdx.x - g * wide.blk);
    if (i >= g1) return;
    const int tiles = (b0 - g0 + kTile - 1) / kTile, P = gridDim.y;
    if ((int)blockIdx.y >= tiles) return;
    const int ni = __builtin_amdgcn_readfirstlane(n_rows[i]), si = __builtin_amdgcn_readfirstlane(start[i]);
    if (ni == 0 || wide.carry[2 * g] == 0) return;           // excluded, or nobody included before it: nobody to meet
    const int h_prev = __builtin_amdgcn_readfirstlane(wide.carry[2 * g + 1]);
    double *mine = tile + w * kRegion;
    const Mission Mi = mission_of(seg_offsets, i, m);
    const int32_t *irows = seg_rows + Mi.s0;
    const double *icm = coeffs + (size_t)Mi.s0 * 24;
    const int32_t *grants = pol.grants();

    int turn = 0;
    for (int q0 = 0; q0 <= max_steps; q0 += kTile) {
        const int n_live = min(kTile, max_steps - q0 + 1);
        const unsigned long long live = n_live == kTile ? ~0ull : (1ull << n_live) - 1ull;
        const int gl = pol.grant(si, q0 + min(lane, n_live - 1));
        const int sl = pol.start_of(si, gl);
        const int H = pol.horizon(h_prev, si, ni, q0 + n_live - 1);
        unsigned long long *word = wide.seed + (size_t)i * wide.words + q0 / kTile;
        turn ^= 1;
        unsigned long long &round_hit = round_hits[turn];
        if (threadIdx.x == 0) round_hit = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();                                     // (the only barrier of a round: the word of the round before is not touched again)
        bool hit = false;
        unsigned long long told = 0;                         // what this wavefront has put into the words
        for (int t = blockIdx.y; t < tiles; t += P) {
            const int j0 = g0 + t * kTile;
            const int n_val = min(kTile, b0 - j0);
            const int n_pad = (n_val + kUnroll - 1) / kUnroll * kUnroll;
            const bool jvalid = lane < n_val;
            const int jb = jvalid ? j0 + lane : j0;
            const Mission Mj = mission_of(seg_offsets, jb, m);
            const int32_t *jrows = seg_rows + Mj.s0;
            const double *jcm = coeffs + (size_t)Mj.s0 * 24;
            const int nj = jvalid ? n_rows[jb] : 0, sb = start[jb], gj = grants[jb];
            const int sj = pol.start_of(sb, gj);
            int js = 0, jbase = 0, jcnt = jrows[0];
            int is = 0, ibase = 0, icnt = irows[0];
            for (int k0 = w * kRows; k0 < H; k0 += kChunk) {
                const bool over = (__hip_atomic_load(&round_hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & live) == live;
                if (__builtin_amdgcn_readfirstlane((int)over)) break;
                clock_walk_to_tile<Policy::kMoves>(mine, lane, jrows, jcm, Mj.m, nj, sj, k0, H, dt, js, jbase, jcnt, pol.hook(gj));
                lds_wave_fence();
                clock_walk<Policy::kMoves>(irows, icm, Mi.m, ni, sl, k0, H, dt, is, ibase, icnt, pol.hook(gl),
                                           [&](int r, int, double xi, double yi, double zi) {
                                               hit |= inside_row(mine + r * kTile * 3, n_pad, xi, yi, zi, r2);
                                           });
                lds_wave_fence();
                const unsigned long long now = __ballot(hit) & live;
                if (now != told) {
                    if (lane == 0) {
                        __hip_atomic_fetch_or(&round_hit, now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        atomicOr(word, now);
                    }
                    told = now;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ the launches
// Scratch from the ctx arena: the pre-pass's row totals and clamped starts, B x words seed words, two ints of carry per group.
// `prepass(n_rows, start)` launches the policy's pre-pass, `seed(grid, n_rows, start, block)` and `search(grid, n_rows, start, block)` its
// two kernels; everything goes to the ctx stream.
// TRAFFIC (fleet_against.h: Bt > 0 missions of another plan that count as decided before block 0): their row totals and starts are
// two more pieces of the scratch; `traffic_prepass(t_n_rows, t_start)` is launched behind the pre-pass, `traffic_seed(t_n_rows,
// t_start, n_rows, start, block)` between the memsets and block 0 -- it fills the carries and ORs into the seed words.
template <class Prepass, class Seed, class Search, class TrafficPrepass, class TrafficSeed>
int launch_wide_search(uavac_ctx *ctx, int B, const int64_t *group_offsets, int G, int group_cap, int max_steps, Prepass prepass, Seed seed,
                       Search search, int Bt, TrafficPrepass traffic_prepass, TrafficSeed traffic_seed) {
    const int groups = group_offsets ? G : 1;
    const int blk = ctx->search_block ? ctx->search_block : kWideBlock;
    const int words = max_steps / kTile + 1;
    const int blocks = (std::min(group_cap, B) + blk - 1) / blk;  // (no group is larger than the batch)
    if ((long long)groups * blk > 0x7fffffffLL) return uavac_fail(ctx, UAVAC_EINVAL, "too many groups for the block-wise search: G * block above 2^31 - 1");
    int32_t *n_rows = nullptr, *start = nullptr, *carry = nullptr, *t_n_rows = nullptr, *t_start = nullptr;
    unsigned long long *words_of = nullptr;
    Scratch s(ctx);
    s.want(&n_rows, B); s.want(&start, B); s.want(&words_of, (size_t)B * words); s.want(&carry, 2 * (size_t)groups);
    if (Bt > 0) { s.want(&t_n_rows, Bt); s.want(&t_start, Bt); }
    if (s.commit()) {
        (void)hipGetLastError();
        return uavac_fail(ctx, UAVAC_ENOMEM, Bt > 0 ? "the search's scratch (8 + 8 (max_steps / 64 + 1) bytes per mission, 8 per group, 8 per traffic mission) does not fit on the device"
                                                    : "the block-wise search's scratch (8 + 8 (max_steps / 64 + 1) bytes per mission, 8 per group) does not fit on the device");
    }
    prepass(n_rows, start);
    if (Bt > 0) traffic_prepass(t_n_rows, t_start);
    UAVAC_HIP(ctx, hipMemsetAsync(words_of, 0, (size_t)B * words * sizeof(unsigned long long), ctx->stream));
    UAVAC_HIP(ctx, hipMemsetAsync(carry, 0, 2 * (size_t)groups * sizeof(int32_t), ctx->stream));
    if (Bt > 0) traffic_seed(t_n_rows, t_start, n_rows, start, Block{0, blk, group_cap, words_of, words, carry});
    for (int k = 0; k < blocks; ++k) {
        const Block block{k, blk, group_cap, words_of, words, carry};
        if (k > 0) {                                         // shares per mission: enough workgroups for the chip, at most one per j-tile
            const long long missions = (long long)groups * blk, wanted = (long long)ctx->n_simds * 4;
            const long long tiles = (long long)k * blk / kTile;
            const long long P = std::max(1LL, std::min(tiles, (wanted + missions - 1) / missions));
            seed(dim3((unsigned)missions, (unsigned)P), n_rows, start, block);
        }
        search(dim3(groups), n_rows, start, block);
    }
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}

// (without traffic: the two calls for groups of any size)
template <class Prepass, class Seed, class Search>
int launch_wide_search(uavac_ctx *ctx, int B, const int64_t *group_offsets, int G, int group_cap, int max_steps, Prepass prepass, Seed seed,
                       Search search) {
    return launch_wide_search(ctx, B, group_offsets, G, group_cap, max_steps, prepass, seed, search, 0, [](int32_t *, int32_t *) {},
                              [](int32_t *, int32_t *, const int32_t *, const int32_t *, Block) {});
}

}  // namespace
