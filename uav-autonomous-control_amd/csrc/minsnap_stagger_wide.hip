// Fleet deconfliction by start delay for groups of any size (gfx950): uavac_minsnap_stagger_dev's rule (minsnap_stagger.hip) without
// its limit of UAVAC_STAGGER_MAX_GROUP missions per group.  The contract is in include/uavac.h (uavac_minsnap_stagger_wide_dev);
// uav_ac.scoring.stagger_from_rows(..., max_group=group_cap) states it in NumPy on sampled rows, and the results are the same integers.
//
// The kernels are the Delay instantiations of the block-wise search (fleet_wide.h, which describes the decomposition, the launch order
// and why the answers are the rule's):
//   stagger_prepass_kernel       stagger_prepass.h's, as in the narrow call
//   wide_stagger_seed_kernel     per block k > 0: which candidate delays of the block's missions meet a mission of an earlier block at
//                                its granted start (row 0 of istag)
//   wide_stagger_kernel          per block: the decisions, one workgroup per group
// A mission that is first in its block but not in its group has no j-tile: it is decided from the seed alone.

#include "fleet_wide.h"
#include "stagger_prepass.h"

namespace {

__global__ void __launch_bounds__(kThreads, 3) wide_stagger_seed_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
    const int64_t *__restrict__ group_offsets, const int32_t *__restrict__ n_rows, const int32_t *__restrict__ start, double r2, int step,
    int max_steps, int32_t *istag, Block block) {
    fleet_seed(Delay{step, istag}, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, n_rows, start, r2, max_steps, block);
}

__global__ void __launch_bounds__(kThreads, 3) wide_stagger_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
    const int64_t *__restrict__ group_offsets, const int32_t *__restrict__ n_rows, const int32_t *__restrict__ start, double r2, int step,
    int max_steps, int32_t *istag, int32_t *__restrict__ flags, Block block) {
    fleet_search<Delay, true>(Delay{step, istag}, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, n_rows, start, r2, max_steps, nullptr, 0,
                              flags, block);
}

}  // namespace

int uavac_launch_stagger_wide(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                              const int64_t *group_offsets, int G, int group_cap, const int32_t *start_rows, double radius, int step,
                              int max_steps, int32_t *istag) {
    const double r2 = radius * radius;
    return launch_wide_search(
        ctx, B, group_offsets, G, group_cap, max_steps,
        [&](int32_t *n_rows, int32_t *start) {
            hipLaunchKernelGGL(stagger_prepass_kernel, dim3((B + kPreMissions - 1) / kPreMissions), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows,
                               seg_offsets, B, m, start_rows, n_rows, start, istag, ctx->d_flags);
        },
        [&](dim3 grid, const int32_t *n_rows, const int32_t *start, Block block) {
            hipLaunchKernelGGL(wide_stagger_seed_kernel, grid, dim3(kThreads), 0, ctx->stream, coeffs, seg_rows, seg_offsets, B, m, dt,
                               group_offsets, n_rows, start, r2, step, max_steps, istag, block);
        },
        [&](dim3 grid, const int32_t *n_rows, const int32_t *start, Block block) {
            hipLaunchKernelGGL(wide_stagger_kernel, grid, dim3(kThreads), 0, ctx->stream, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets,
                               n_rows, start, r2, step, max_steps, istag, ctx->d_flags, block);
        });
}
