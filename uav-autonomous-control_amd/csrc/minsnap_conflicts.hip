// The fleet's conflict list (gfx950): the conflict graph of the separation audit in CSR form.  Where the audit (minsnap_separation.hip)
// names a mission's one closest partner and COUNTS the others that come inside the radius, this lists every one of them, with when and
// how near: first and last clock row inside, the number of rows inside, the pair's minimum distance and its row.  From coefficients and
// row counts alone: no row is written, nothing is read back.  The contract -- the audit's clock, groups, excluded missions, rounding and
// bad inputs, the slices, the bounds -- is in include/uavac.h (uavac_minsnap_conflict_offsets_dev, uavac_minsnap_conflicts_dev);
// uav_ac.scoring.conflicts_from_rows states it in NumPy on sampled rows, and the results are the same bits.
//
// Launches on the ctx stream:
//   conflict_prepass_kernel    per mission: fleet_clock.h's pre-pass -- the row total N (0: EXCLUDED) and the clamped start row
//   conflict_discover_kernel   the pairs: the sweep of pair_sweep.h, which describes it, with positions walked from the coefficients
//                              (`Planned`) and nothing kept but the bit per partner that came inside the radius (`Bits`).  The merged
//                              64-bit word of (mission, j-tile) goes to scratch, words [slot][B], slot = the j-tile's index within the
//                              round: ONE writer per word.  The first share of the first round also leaves, per mission, its group's
//                              first mission, horizon and number of j-tiles (info [3][B]).  Discovery is repeated in ROUNDS over the
//                              slots [T0, T0 + slots) (conflict_csr.h); in a later round a workgroup whose groups have no tile that far
//                              finds that out from the group's size and leaves.
//   conflict_count_kernel,     (conflict_csr.h, one copy for this list and the flown one, flown_conflicts.hip) the popcounts of the
//   conflict_list_kernel       round's words into the totals of the offsets' scan; the words bit by bit into row 0 of the mission's
//                              slice, bounded, with flags 2 and 0
//   conflict_measure_kernel    per listed entry, sixteen lanes each: both missions walked over the group's clock [0, H_g) with
//                              clock_walk's arithmetic -- lane l takes the rows 8 (16 c + l) .. + 7 of every c --, the partner's eight
//                              positions parked in the lane's own slots of the LDS tile; the result of a lane's rows, the merge of the
//                              sixteen lanes and the write are csr::Measure (conflict_csr.h), shared with the flown measure.
//                              It reads a pair and nothing of the discovery.
// The fill call repeats the discovery: it does not rely on what the offsets call left in the arena, other calls may run in between.
// Work: discovery = the audit's pairs x horizon; the measure = entries x horizon, small beside it.
//
// ROUNDING (part of the contract): positions by the sampler's fma chain (minsnap_eval_pos), the distance WITHOUT contraction: dx = xi -
// xj, ..., d^2 = (dx dx + dy dy) + dz dz, each product and sum rounded on its own -- (xi - xj)^2 == (xj - xi)^2 bit for bit, so the two
// directions of a pair agree in everything but the partner.

#include "conflict_csr.h"
#include "pair_sweep.h"

#include <cmath>
#include <limits>

namespace {

using namespace pair_sweep;                                 // the sweep and, through it, the clock, the pre-pass and sepred's tile and reduction

constexpr int kPairLanes = 16;                              // lanes per entry of the measure
constexpr int kPairsPerWave = 64 / kPairLanes;
constexpr int kPairsPerGroup = kWaves * kPairsPerWave;      // entries per workgroup of the measure

// ------------------------------------------------------------------------------------------------------------------ pre-pass
__global__ void __launch_bounds__(kThreads) conflict_prepass_kernel(const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows,
                                                                    const int64_t *__restrict__ seg_offsets, int B, int m,
                                                                    const int32_t *__restrict__ start_rows, int32_t *__restrict__ n_rows,
                                                                    int32_t *__restrict__ start, int32_t *__restrict__ flags) {
    int b, s;
    prepass_mission(coeffs, seg_rows, seg_offsets, B, m, start_rows, n_rows, start, flags, b, s);
}

// ------------------------------------------------------------------------------------------------------------------ discovery
// info [3][B]: the first mission of the mission's group, the group's horizon, and its j-tiles (0: fewer than two missions take part).
__global__ void __launch_bounds__(kThreads, 3) conflict_discover_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
    const int64_t *__restrict__ group_offsets, int G, const int32_t *__restrict__ n_rows, const int32_t *__restrict__ start, double r2, int T0,
    int slots, unsigned long long *__restrict__ words, int32_t *__restrict__ info) {
    __shared__ double tile[kWaves * kRegion];
    Planned src{coeffs, seg_rows, seg_offsets, m, dt, n_rows, start};
    Bits<true> keep{T0, slots, words, info, info + (size_t)B, info + 2 * (size_t)B};
    sweep(tile, src, keep, B, group_offsets, G, r2);
}

// ------------------------------------------------------------------------------------------------------------------ the measure
__global__ void __launch_bounds__(kThreads, 3) conflict_measure_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
    const int32_t *__restrict__ n_rows, const int32_t *__restrict__ start, const int32_t *__restrict__ info, double r2,
    const int32_t *__restrict__ owner, long long capacity, double *__restrict__ pair_d, int32_t *__restrict__ pair_i) {
    __shared__ double tile[kWaves * kRegion];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int l = lane % kPairLanes;
    const long long e = ((long long)blockIdx.x * kWaves + w) * kPairsPerWave + lane / kPairLanes;
    // the entry's pair: who owns it (-1: nobody listed it) and the partner in row 0; an entry that is not measured walks mission 0 over
    // an empty clock
    int i = e < capacity ? owner[e] : -1;
    int j = i >= 0 ? pair_i[e] : -1;
    bool live = i >= 0 && i < B && j >= 0 && j < B;
    i = live ? i : 0; j = live ? j : 0;
    const int ni = n_rows[i], nj = n_rows[j], si = start[i], sj = start[j];
    live = live && ni > 0 && nj > 0;
    const int H = live ? info[(size_t)B + i] : 0;
    const Mission Mi = mission_of(seg_offsets, i, m), Mj = mission_of(seg_offsets, j, m);
    const int32_t *irows = seg_rows + Mi.s0, *jrows = seg_rows + Mj.s0;
    const double *icm = coeffs + (size_t)Mi.s0 * 24, *jcm = coeffs + (size_t)Mj.s0 * 24;
    double *mine = tile + w * kRegion;                       // the lane reads only the slots it wrote itself

    csr::Measure res;
    int js = 0, jbase = 0, jcnt = jrows[0];
    int is = 0, ibase = 0, icnt = irows[0];
    for (int k0 = l * kRows; k0 < H; k0 += kPairLanes * kRows) {
        clock_walk_to_tile<false>(mine, lane, jrows, jcm, Mj.m, nj, sj, k0, H, dt, js, jbase, jcnt, AsPlanned{});
        clock_walk<false>(irows, icm, Mi.m, ni, si, k0, H, dt, is, ibase, icnt, AsPlanned{}, [&](int r, int k, double xi, double yi, double zi) {
            const double *o = mine + (r * kTile + lane) * 3;
            res.row(csr::pair_d2(xi, yi, zi, o[0], o[1], o[2]), k, r2);
        });
    }
    // the sixteen lanes of the entry
#pragma unroll
    for (int d = kPairLanes / 2; d >= 1; d >>= 1)
        res.merge(__shfl_xor(res.bd, d), __shfl_xor(res.bk, d), __shfl_xor(res.first, d), __shfl_xor(res.last_in, d), __shfl_xor(res.inside, d));
    if (live && l == 0) res.write(pair_d, pair_i, e, capacity);
}

// ------------------------------------------------------------------------------------------------------------------ the host side
// What the two calls share: csr's shape (shares, slots, rounds; counts, words, owners) and the pre-pass's and the discovery's records.
struct Shape : csr::Shape {
    int32_t *n_rows, *start, *info;
};

int shape_of(uavac_ctx *ctx, Scratch &scratch, int B, const int64_t *group_offsets, int G, long long capacity, Shape &s) {
    csr::shape_of(ctx, B, group_offsets, G, s);
    const size_t Bs = (size_t)B;
    scratch.want(&s.n_rows, Bs); scratch.want(&s.start, Bs); scratch.want(&s.info, 3 * Bs);
    csr::shape_want(scratch, s, B, capacity);
    return scratch.commit();
}

int launch_prepass(uavac_ctx *ctx, const Shape &s, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                   const int32_t *start_rows) {
    hipLaunchKernelGGL(conflict_prepass_kernel, dim3((B + kPreMissions - 1) / kPreMissions), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows,
                       seg_offsets, B, m, start_rows, s.n_rows, s.start, ctx->d_flags);
    // a mission that no group holds (offsets that do not cover the batch) has no tiles
    UAVAC_HIP(ctx, hipMemsetAsync(s.info, 0, 3 * (size_t)B * 4, ctx->stream));
    return UAVAC_OK;
}

// one round of the discovery, from its first j-tile T0 (csr_offsets / csr_list call it once per round)
auto discovery(uavac_ctx *ctx, const Shape &s, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
               double dt, const int64_t *group_offsets, int G, double radius) {
    return [=](int T0) {
        hipLaunchKernelGGL(conflict_discover_kernel, dim3(s.windows, s.P), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows, seg_offsets, B, m,
                           dt, group_offsets, group_offsets ? G : 1, s.n_rows, s.start, radius * radius, T0, s.slots, s.words, s.info);
    };
}

}  // namespace

int uavac_launch_conflict_offsets(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                                  double dt, const int64_t *group_offsets, int G, const int32_t *start_rows, double radius,
                                  int64_t *pair_offsets) {
    Scratch scratch(ctx);
    Shape s;
    if (int rc = shape_of(ctx, scratch, B, group_offsets, G, 0, s)) return rc;
    if (int rc = launch_prepass(ctx, s, coeffs, seg_rows, seg_offsets, B, m, start_rows)) return rc;
    const auto discover = discovery(ctx, s, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, radius);
    return csr::csr_offsets(ctx, s, B, s.n_rows, s.info + 2 * (size_t)B, discover, pair_offsets);
}

int uavac_launch_conflicts(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                           const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, const int64_t *pair_offsets,
                           int64_t capacity, double *pair_d, int32_t *pair_i) {
    Scratch scratch(ctx);
    Shape s;
    if (int rc = shape_of(ctx, scratch, B, group_offsets, G, capacity, s)) return rc;
    if (int rc = launch_prepass(ctx, s, coeffs, seg_rows, seg_offsets, B, m, start_rows)) return rc;
    const auto discover = discovery(ctx, s, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, radius);
    if (int rc = csr::csr_list(ctx, s, B, s.n_rows, s.info, s.info + 2 * (size_t)B, discover, pair_offsets, (long long)capacity, pair_i))
        return rc;
    if (capacity > 0) {
        const long long groups = (capacity + kPairsPerGroup - 1) / kPairsPerGroup;
        hipLaunchKernelGGL(conflict_measure_kernel, dim3((unsigned)groups), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows, seg_offsets, B, m,
                           dt, s.n_rows, s.start, s.info, radius * radius, s.owner, (long long)capacity, pair_d, pair_i);
    }
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}
