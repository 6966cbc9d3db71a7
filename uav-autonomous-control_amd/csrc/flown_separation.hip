// The separation the fleet FLEW (gfx950): the separation audit (minsnap_separation.hip) asks how close the PLANS of a group come; this
// one asks the same of the VEHICLES, which track their plans with an error, from the positions in the rollout's state log
// ([K][13][pitch] f64, rows 0-2) -- in the same terms: closest approach, partner, tick, conflicts inside a protection radius, the first
// tick with anybody inside, and how many partners were compared.  Nothing is read back and no log leaves the device.  The contract is
// in include/uavac.h (uavac_flown_separation_dev); uav_ac.scoring.separation_from_log states it in NumPy, and the results are the same bits.
//
// Two launches on the ctx stream:
//   flown_separation_kernel   the pairs, shaped like the plan audit's.  A workgroup owns the 64 consecutive vehicles [64 x, 64 x + 64)
//                             of the batch, one per lane (i), and visits every group that reaches into this window, with the lanes of
//                             other groups idle.  Per group it walks the group's vehicles in j-tiles of 64 and, per j-tile, the ticks
//                             0 .. K - 1 in chunks of 32.  Its four wavefronts split each chunk: wave w takes ticks 8 w .. 8 w + 7.
//                             Positions are not evaluated but READ: a j-tile's x, y and z at one tick are three coalesced 512-byte
//                             loads (lane = j, consecutive columns of one log row), 24 loads in flight per wave and chunk, staged into
//                             the wave's own quarter of the LDS tile as [tick][64][3]; the lane's own position at a tick is three
//                             loads of the same kind (lane = i), fetched one tick ahead of the pair loop.  The 64 partners' positions
//                             are LDS broadcasts (every lane reads the same address).  A wave reads only what it wrote itself: no
//                             workgroup barrier inside the tick loop.
//                             VALID pair-ticks.  A pair-tick counts iff its d^2 is not NaN.  Inside the contract (positions finite
//                             or NaN, differences that do not overflow) that is: none of the six coordinates is NaN -- so the
//                             partners a lane was compared with at a tick are, if its own position is a number, the ballot of "my
//                             three coordinates are numbers" over the tile (lane = j, read back from the tile), one OR per tick
//                             instead of a comparison per pair.  A NaN d^2 is never below anything: it costs the minimum and the
//                             conflict bits no instruction.  Lanes past the group's end are NaN positions; the lane's own entry is
//                             +inf in the one tile that holds it, and its bit is taken out of the compared set.
//                             The reduction is separation_reduce.h: per tick the minimum and its partner (strict <, partners
//                             ascending), per j-tile the minimum and its tick (strict <, ticks ascending), one bit per partner that
//                             came inside the radius, the first tick with anybody inside; the four waves meet through the tile at
//                             the end of a j-tile.  gridDim.y = P workgroups share a window: workgroup p takes j-tiles p, p + P, ...
//                             and leaves one partial record per vehicle in scratch (its fifth row: the partners compared)
//   flown_merge_kernel        per vehicle: the P partial records merged, the compared counts summed, one correctly rounded sqrt
// Exact and independent of order, so the outputs depend neither on P (option "separation_split", as for the plan audit), nor on the
// pitch, nor on what else is in the batch; each output has one writer and there are no atomics.  Every column index is below B (lanes
// past the batch or the group read column B - 1 or the group's last one and are masked): columns B .. pitch - 1 are never read.

#include "fleet_clock.h"

#include <limits>

namespace {

using namespace sepred;                                     // the tile's shape and the reduction: shared with minsnap_separation.hip
using fleet::group_range;                                   // (fleet_clock.h: the group clamp of every fleet kernel)

constexpr int kLogRows = 13;                                // rows of the state log per tick (positions: 0-2)

__device__ __forceinline__ bool is_number(double x, double y, double z) { return x == x && y == y && z == z; }

__global__ void __launch_bounds__(kThreads, 3) flown_separation_kernel(const double *__restrict__ slog, int K, int B, long long pitch,
                                                                       const int64_t *__restrict__ group_offsets, int G, double r2,
                                                                       double *__restrict__ part_d2, int32_t *__restrict__ part_i) {
    __shared__ double tile[kWaves * kRegion];
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int P = gridDim.y, p = blockIdx.y;
    const int w0 = blockIdx.x * kTile, w1 = w0 + kTile;      // the window of vehicles this workgroup owns
    const int b = w0 + lane;
    const bool live = b < B;
    const double *own = slog + (live ? b : B - 1);           // the lane's own column (a lane past the batch shadows the last vehicle)
    const long long tick = kLogRows * pitch;                 // doubles from one tick of the log to the next
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
        const bool act = live && b >= g0 && b < g1;

        double gb = inf;                                     // the group's results so far (held by wavefront 0)
        int gk = kNone, gj = kNone, gconf = 0, gfirst = kNone, gcomp = 0;
        const int n_tiles = (g1 - g0 + kTile - 1) / kTile;
        for (int t = g1 - g0 >= 2 ? p : n_tiles; t < n_tiles; t += P) {
            const int j0 = g0 + t * kTile;
            const bool jvalid = j0 + lane < g1;
            const double *theirs = slog + (jvalid ? j0 + lane : g1 - 1);
            const int selfjj = b - j0;
            const bool self_tile = j0 < w1 && j0 + kTile > w0;
            double tb = inf;                                 // this wavefront's results of the tile
            int tk = kNone, tj = kNone, tfirst = kNone;
            unsigned long long mask = 0, seen = 0;           // partners that came inside the radius; partners with a valid pair-tick
            for (int k0 = w * kRows; k0 < K; k0 += kChunk) {
                const int n = min(kRows, K - k0);            // this wavefront's ticks of the chunk
#pragma unroll
                for (int r = 0; r < kRows; ++r) {            // the j-tile's positions (the ticks past the log's end repeat its last one: unused)
                    const double *at = theirs + (long long)min(k0 + r, K - 1) * tick;
                    const double x = at[0], y = at[pitch], z = at[2 * pitch];
                    double *o = mine + (r * kTile + lane) * 3;
                    o[0] = jvalid ? x : nan; o[1] = jvalid ? y : nan; o[2] = jvalid ? z : nan;
                }
                lds_wave_fence();                            // (a wavefront reads only its own quarter)
                const double *at = own + (long long)k0 * tick;
                double nx = at[0], ny = at[pitch], nz = at[2 * pitch];      // the lane's own position, one tick ahead
#pragma nounroll
                for (int r = 0; r < n; ++r) {
                    const int k = k0 + r;
                    const double xi = nx, yi = ny, zi = nz;
                    if (r + 1 < n) {
                        at = own + (long long)(k + 1) * tick;
                        nx = at[0]; ny = at[pitch]; nz = at[2 * pitch];
                    }
                    const double *row = mine + r * kTile * 3;
                    const unsigned long long numbers = __ballot(is_number(row[3 * lane], row[3 * lane + 1], row[3 * lane + 2]));
                    if (is_number(xi, yi, zi)) seen |= numbers;
                    double rm = inf;
                    int rkey = 0;
                    if (self_tile) pair_row<true>(row, xi, yi, zi, r2, selfjj, rm, rkey, mask);
                    else pair_row<false>(row, xi, yi, zi, r2, selfjj, rm, rkey, mask);
                    if (rm < tb) { tb = rm; tk = k; tj = j0 + rkey; }
                    if (rm < r2) tfirst = min(tfirst, k);
                }
                lds_wave_fence();
            }
            if (selfjj >= 0 && selfjj < kTile) seen &= ~(1ull << selfjj);      // the lane's own vehicle is nobody's partner
            // the four wavefronts meet: 1 .. 3 leave their results in their quarters, wavefront 0 merges
            if (w != 0) {
                sep_waves_leave(mine, lane, tb, tk, tj, mask, tfirst);
                sep_waves_leave_bits(mine, lane, seen);
            }
            __syncthreads();
            if (w == 0) {
                sep_waves_meet(tile, lane, tb, tk, tj, mask, tfirst);
                sep_waves_meet_bits(tile, lane, seen);
                gconf += __popcll(mask);
                gcomp += __popcll(seen);
                if (lex_less(tb, tk, tj, gb, gk, gj)) { gb = tb; gk = tk; gj = tj; }
                gfirst = min(gfirst, tfirst);
            }
            __syncthreads();
        }
        // one partial record per vehicle and share p; its fifth row: the partners of the share that were compared
        if (w == 0 && act) sep_leave_partial(part_d2, part_i, p, b, B, gb, gj, gk, gconf, gfirst, gcomp);
    }
}

__global__ void __launch_bounds__(kThreads) flown_merge_kernel(int B, int P, const double *__restrict__ part_d2,
                                                               const int32_t *__restrict__ part_i, double *__restrict__ sep,
                                                               int32_t *__restrict__ isep) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    const size_t Bs = (size_t)B;
    double d;
    int k, j, conf, first, compared = 0;
    sep_merge_partials(part_d2, part_i, P, b, B, d, k, j, conf, first);
    for (int p = 0; p < P; ++p) compared += part_i[((size_t)p * 5 + 4) * Bs + b];      // disjoint partners: a sum
    sep_write(sep, isep, b, B, d, k, j, conf, first, compared);
}

}  // namespace

int uavac_launch_flown_separation(uavac_ctx *ctx, const double *state_log, int K, int B, int64_t pitch, const int64_t *group_offsets, int G,
                                  double radius, double *sep, int32_t *isep) {
    const int windows = (B + kTile - 1) / kTile;
    // Shares per window, sized as the plan audit sizes them (uavac_launch_separation): enough workgroups for about four per SIMD,
    // never more than the average group has j-tiles.  The results do not depend on it (option "separation_split").
    int P = ctx->separation_split;
    if (P <= 0) {
        const int groups = group_offsets ? G : 1;
        const int tiles = (B / groups + kTile - 1) / kTile;
        const int wanted = ctx->n_simds * 4;
        P = (wanted + windows - 1) / windows;
        P = P > tiles ? tiles : P;
    }
    P = P < 1 ? 1 : (P > UAVAC_SEP_MAX_SPLIT ? UAVAC_SEP_MAX_SPLIT : P);
    const size_t Bs = (size_t)B;
    if (int rc = uavac_arena_reserve(ctx, uavac_arena_size(P * Bs * 8) + uavac_arena_size(P * 5 * Bs * 4))) return rc;
    double *part_d2 = static_cast<double *>(uavac_arena_take(ctx, P * Bs * 8));
    int32_t *part_i = static_cast<int32_t *>(uavac_arena_take(ctx, P * 5 * Bs * 4));
    if (!part_d2 || !part_i) return uavac_fail(ctx, UAVAC_ENOMEM, "flown separation: scratch arena too small");
    hipLaunchKernelGGL(flown_separation_kernel, dim3(windows, P), dim3(kThreads), 0, ctx->stream, state_log, K, B, (long long)pitch,
                       group_offsets, group_offsets ? G : 1, radius * radius, part_d2, part_i);
    hipLaunchKernelGGL(flown_merge_kernel, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream, B, P, part_d2, part_i, sep,
                       isep);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}
