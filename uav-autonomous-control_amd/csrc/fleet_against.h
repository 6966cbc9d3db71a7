// The prioritised search AGAINST COMMITTED TRAFFIC that never moves (gfx950): what uavac_minsnap_stagger_against_dev
// (minsnap_stagger_against.hip) and uavac_minsnap_layer_against_dev (minsnap_layer_against.hip) add to the block-wise search of
// fleet_wide.h.  The contracts are in include/uavac.h; uav_ac.scoring.stagger_against_rows and layer_against_rows state the rule.
//
// The traffic is a second plan with its own arrays.  To the search it is a VIRTUAL EARLIER BLOCK: the block-wise search decides a block
// from a seed word per (mission, 64 candidates), a carry of two ints per group -- `earlier` and the horizon -- and the block's own
// j-tiles, and the traffic arrives through the first two:
//   traffic_prepass_kernel       fleet_clock.h's pre-pass on the traffic's arrays: row totals (0: EXCLUDED) and clamped starts into
//                                scratch, flag 0 for what the host cannot refuse, and nothing else -- no output block is touched
//   traffic_carry_kernel         per group: the included traffic missions and max(start + rows) over them into carry[g], which the
//                                launch of block 0 reads as `earlier` and the horizon.  With earlier > 0 the first mission of a group is
//                                examined, and with no j-tile it is decided from the seed alone
//   fleet_seed_against<Policy>   fleet_seed's sibling, launched ONCE over all B missions before block 0, parallel over the chip: the 64
//                                lanes are 64 candidates of one plan mission, all rounds up to max_steps; the j-tiles are 64 traffic
//                                missions of the mission's group, walked AS PLANNED at their own starts into the wave's quarter of the LDS
//                                tile; the candidate is walked through the policy's own hook.  gridDim.y shares the j-tiles; a wave ORs
//                                its ballot, the lanes past the last candidate masked out, into the workgroup's LDS copy of the word and
//                                into seed[i][q0 / 64] with an ordinary 64-bit atomicOr.  A share without a tile, an excluded mission, a
//                                group without included traffic and a group above group_cap exit at once
// then fleet_search<Policy, true> per block as it is, and fleet_seed per block k > 0, which ORs into the same words.  Launch order on the
// ctx stream: the plan's pre-pass, the traffic's, the two memsets, the carry, the seed, then seed(k) / search(k).  Nothing spins and no
// workgroup waits for another.  The answers are the rule's for fleet_wide.h's reason: a candidate is clear iff no partner decided before
// it is inside the radius at any clock row, and an OR does not care how it is split; a round's horizon is pol.horizon(the traffic's
// horizon, ...), which reaches the row past which the candidate and every traffic mission stand still.
#pragma once

#include "fleet_wide.h"

namespace {

// the traffic's side of a call: a plan's arrays (ragged or uniform), its groups and its start rows
struct Traffic {
    const double *__restrict__ coeffs;
    const int32_t *__restrict__ seg_rows;
    const int64_t *__restrict__ seg_offsets;
    int B, m;
    const int64_t *__restrict__ group_offsets;
    const int32_t *__restrict__ start_rows;
};

__global__ void __launch_bounds__(kThreads) traffic_prepass_kernel(const Traffic tr, int32_t *__restrict__ n_rows, int32_t *__restrict__ start,
                                                                   int32_t *__restrict__ flags) {
    int b, s;                                                // (traffic has no record of its own)
    prepass_mission(tr.coeffs, tr.seg_rows, tr.seg_offsets, tr.B, tr.m, tr.start_rows, n_rows, start, flags, b, s);
}

// one workgroup per group
__global__ void __launch_bounds__(kThreads) traffic_carry_kernel(const int64_t *__restrict__ t_group_offsets, int Bt,
                                                                 const int32_t *__restrict__ t_n_rows, const int32_t *__restrict__ t_start,
                                                                 int32_t *__restrict__ carry) {
    __shared__ int meet[2 * kWaves];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int t0, t1;
    group_range(t_group_offsets, blockIdx.x, Bt, t0, t1);
    int h = 0, cnt = 0;
    for (int j = t0 + (int)threadIdx.x; j < t1; j += kThreads) {
        const int n = t_n_rows[j];
        if (n > 0) { h = max(h, t_start[j] + n); ++cnt; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { h = max(h, __shfl_xor(h, d)); cnt += __shfl_xor(cnt, d); }
    if (lane == 0) { meet[2 * w] = h; meet[2 * w + 1] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int H = 0, n_in = 0;
#pragma unroll
        for (int v = 0; v < kWaves; ++v) { H = max(H, meet[2 * v]); n_in += meet[2 * v + 1]; }
        carry[2 * blockIdx.x] = n_in; carry[2 * blockIdx.x + 1] = H;
    }
}

// ------------------------------------------------------------------------------------------------------------------ the seed
// (the body of a __global__ kernel of kThreads threads; grid: x = the plan mission, y = the share of the traffic's j-tiles)
template <class Policy>
__device__ __forceinline__ void fleet_seed_against(const Policy pol, const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows,
                                                   const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
                                                   const int64_t *__restrict__ group_offsets, int G, const int32_t *__restrict__ n_rows,
                                                   const int32_t *__restrict__ start, const Traffic tr, const int32_t *__restrict__ t_n_rows,
                                                   const int32_t *__restrict__ t_start, double r2, int max_steps, const Block wide) {
    __shared__ double tile[kWaves * kRegion];
    __shared__ unsigned long long round_hits[2];             // the workgroup's copy of the round's word, two taken in turn as in the search
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = blockIdx.x;
    if (i >= B) return;
    int g = 0;                                               // the group that holds mission i: the last one that starts at or before it
    if (group_offsets) {
        int lo = 0, hi = G;
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (group_offsets[mid] <= i) lo = mid; else hi = mid;
        }
        g = lo;
    }
    int g0, g1, t0, t1;
    group_range(group_offsets, g, B, g0, g1);
    if (i < g0 || i >= g1) return;                           // (malformed offsets: nobody's mission)
    if (g1 - g0 > wide.group_cap) return;                    // not examined (the search raises the flag)
    group_range(tr.group_offsets, g, tr.B, t0, t1);          // the partners are the traffic missions t0 .. t1 - 1
    const int tiles = (t1 - t0 + kTile - 1) / kTile, P = gridDim.y;
    if ((int)blockIdx.y >= tiles) return;
    const int ni = __builtin_amdgcn_readfirstlane(n_rows[i]), si = __builtin_amdgcn_readfirstlane(start[i]);
    if (ni == 0 || wide.carry[2 * g] == 0) return;           // excluded, or no included traffic in its group: nobody to meet
    const int h_traffic = __builtin_amdgcn_readfirstlane(wide.carry[2 * g + 1]);
    double *mine = tile + w * kRegion;
    const Mission Mi = mission_of(seg_offsets, i, m);
    const int32_t *irows = seg_rows + Mi.s0;
    const double *icm = coeffs + (size_t)Mi.s0 * 24;

    int turn = 0;
    for (int q0 = 0; q0 <= max_steps; q0 += kTile) {
        const int n_live = min(kTile, max_steps - q0 + 1);
        const unsigned long long live = n_live == kTile ? ~0ull : (1ull << n_live) - 1ull;
        const int gl = pol.grant(si, q0 + min(lane, n_live - 1));
        const int sl = pol.start_of(si, gl);
        const int H = pol.horizon(h_traffic, si, ni, q0 + n_live - 1);
        unsigned long long *word = wide.seed + (size_t)i * wide.words + q0 / kTile;
        turn ^= 1;
        unsigned long long &round_hit = round_hits[turn];
        if (threadIdx.x == 0) round_hit = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();                                     // (the only barrier of a round: the word of the round before is not touched again)
        bool hit = false;
        unsigned long long told = 0;                         // what this wavefront has put into the words
        for (int t = blockIdx.y; t < tiles; t += P) {
            const int j0 = t0 + t * kTile;
            const int n_val = min(kTile, t1 - j0);
            const int n_pad = (n_val + kUnroll - 1) / kUnroll * kUnroll;
            const bool jvalid = lane < n_val;
            const int jb = jvalid ? j0 + lane : j0;
            const Mission Mj = mission_of(tr.seg_offsets, jb, tr.m);
            const int32_t *jrows = tr.seg_rows + Mj.s0;
            const double *jcm = tr.coeffs + (size_t)Mj.s0 * 24;
            const int nj = jvalid ? t_n_rows[jb] : 0, sj = t_start[jb];
            int js = 0, jbase = 0, jcnt = jrows[0];
            int is = 0, ibase = 0, icnt = irows[0];
            for (int k0 = w * kRows; k0 < H; k0 += kChunk) {
                const bool over = (__hip_atomic_load(&round_hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & live) == live;
                if (__builtin_amdgcn_readfirstlane((int)over)) break;
                clock_walk_to_tile<false>(mine, lane, jrows, jcm, Mj.m, nj, sj, k0, H, dt, js, jbase, jcnt, AsPlanned{});
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
// The traffic's two hooks of launch_wide_search.  `seed(grid, t_n_rows, t_start, n_rows, start, block)` launches the policy's
// fleet_seed_against kernel: one workgroup per plan mission and share, enough shares for the chip, at most one per j-tile of an average
// group's traffic (the host knows the groups' sizes only on average: the offsets are on the device).
inline void launch_traffic_prepass(uavac_ctx *ctx, const Traffic &tr, int32_t *t_n_rows, int32_t *t_start) {
    hipLaunchKernelGGL(traffic_prepass_kernel, dim3((tr.B + kPreMissions - 1) / kPreMissions), dim3(kThreads), 0, ctx->stream, tr, t_n_rows,
                       t_start, ctx->d_flags);
}

template <class Seed>
void launch_traffic_seed(uavac_ctx *ctx, int B, int groups, const Traffic &tr, int32_t *t_n_rows, int32_t *t_start, const int32_t *n_rows,
                         const int32_t *start, Block block, Seed seed) {
    hipLaunchKernelGGL(traffic_carry_kernel, dim3(groups), dim3(kThreads), 0, ctx->stream, tr.group_offsets, tr.B, t_n_rows, t_start,
                       block.carry);
    const long long wanted = (long long)ctx->n_simds * 4, tiles = (tr.B / groups + kTile - 1) / kTile;
    const long long P = std::max(1LL, std::min(tiles, (wanted + B - 1) / B));
    seed(dim3((unsigned)B, (unsigned)P), t_n_rows, t_start, n_rows, start, block);
}

}  // namespace
