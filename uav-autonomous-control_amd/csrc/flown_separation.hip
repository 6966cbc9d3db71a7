// The separation the fleet FLEW (gfx950): the separation audit (minsnap_separation.hip) asks how close the PLANS of a group come; this
// one asks the same of the VEHICLES, which track their plans with an error, from the positions in the rollout's state log
// ([K][13][pitch] f64, rows 0-2) -- in the same terms: closest approach, partner, tick, conflicts inside a protection radius, the first
// tick with anybody inside, and how many partners were compared.  Nothing is read back and no log leaves the device.  The contract is
// in include/uavac.h (uavac_flown_separation_dev); uav_ac.scoring.separation_from_log states it in NumPy, and the results are the same bits.
//
// Two launches on the ctx stream:
//   flown_separation_kernel   the pairs: the sweep of pair_sweep.h, which describes it, with positions READ from the log (`Flown`) and
//                             the full record kept (`Record`): per vehicle and share of its window one partial record in scratch --
//                             minimum (d^2, tick, partner), conflicts, first tick with anybody inside, and the partners compared:
//                             those with a VALID pair-tick (a d^2 that is not NaN), the one place where this source and this record
//                             meet in the sweep
//   flown_merge_kernel        per vehicle: the P partial records merged, the compared counts summed, one correctly rounded sqrt
// Exact and independent of order, so the outputs depend neither on P (option "separation_split", as for the plan audit), nor on the
// pitch, nor on what else is in the batch; each output has one writer and there are no atomics.  Columns B .. pitch - 1 are never read.

#include "pair_sweep.h"
#include "uavac_scratch.h"

#include <limits>

namespace {

using namespace pair_sweep;                                 // the sweep and, through it, sepred's tile and reduction

__global__ void __launch_bounds__(kThreads, 3) flown_separation_kernel(const double *__restrict__ slog, int K, int B, long long pitch,
                                                                       const int64_t *__restrict__ group_offsets, int G, double r2,
                                                                       double *__restrict__ part_d2, int32_t *__restrict__ part_i) {
    __shared__ double tile[kWaves * kRegion];
    Flown src{slog, K, pitch};
    Record keep{part_d2, part_i};
    sweep(tile, src, keep, B, group_offsets, G, r2);
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
    int windows, P;
    sep_shares(ctx, B, group_offsets, G, windows, P);
    const size_t Bs = (size_t)B;
    double *part_d2 = nullptr;
    int32_t *part_i = nullptr;
    Scratch s(ctx);
    s.want(&part_d2, P * Bs); s.want(&part_i, P * 5 * Bs);
    if (int rc = s.commit()) return rc;
    hipLaunchKernelGGL(flown_separation_kernel, dim3(windows, P), dim3(kThreads), 0, ctx->stream, state_log, K, B, (long long)pitch,
                       group_offsets, group_offsets ? G : 1, radius * radius, part_d2, part_i);
    hipLaunchKernelGGL(flown_merge_kernel, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream, B, P, part_d2, part_i, sep,
                       isep);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}
