// Offset layers for groups of any size (gfx950): the rule of uavac_minsnap_layer_obs_dev (minsnap_layer_obs.hip) -- and, with no
// cuboids, of uavac_minsnap_layer_dev -- without the limit of UAVAC_LAYER_MAX_GROUP missions per group.  The contract is in
// include/uavac.h (uavac_minsnap_layer_wide_dev); uav_ac.scoring.layer_obstacles_from_rows(..., max_group=group_cap) states it in NumPy
// on sampled rows.
//
// The kernels are the LayerObs instantiations of the block-wise search (fleet_wide.h, which describes the decomposition, the launch
// order and why the answers are the rule's); the cuboid policy alone is instantiated, without cuboids it refuses nothing:
//   layer_prepass_kernel<true>   fleet_search.h's, as in the narrow call
//   wide_layer_seed_kernel       per block k > 0: which candidate layers of the block's missions meet a mission of an earlier block on
//                                its granted layer (row 0 of ilayer).  The cuboids are not its business: a refused candidate is refused
//                                by the search, whatever its seed bit says, and `blocked` is counted from the refusals alone
//   wide_layer_kernel            per block: the decisions, one workgroup per group

#include "fleet_wide.h"

namespace {

__global__ void __launch_bounds__(kThreads, 3) wide_layer_seed_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
    const int64_t *__restrict__ group_offsets, const int32_t *__restrict__ n_rows, const int32_t *__restrict__ start, double r2, Delta delta,
    int max_steps, int32_t *ilayer, Block block) {
    fleet_seed(LayerObs{delta, ilayer, nullptr}, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, n_rows, start, r2, max_steps, block);
}

__global__ void __launch_bounds__(kThreads, 3) wide_layer_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
    const int64_t *__restrict__ group_offsets, const int32_t *__restrict__ n_rows, const int32_t *__restrict__ start, double r2, Delta delta,
    int max_steps, const double *__restrict__ cuboids, int n_cuboids, int32_t *ilayer, double *__restrict__ offsets,
    int32_t *__restrict__ flags, Block block) {
    fleet_search<LayerObs, true>(LayerObs{delta, ilayer, offsets}, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, n_rows, start, r2,
                                 max_steps, cuboids, n_cuboids, flags, block);
}

}  // namespace

int uavac_launch_layer_wide(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                            const int64_t *group_offsets, int G, int group_cap, const int32_t *start_rows, double radius, double delta_x,
                            double delta_y, double delta_z, int max_steps, const double *cuboids, int n_cuboids, int32_t *ilayer,
                            double *offsets) {
    const double r2 = radius * radius;
    const Delta delta{delta_x, delta_y, delta_z};
    return launch_wide_search(
        ctx, B, group_offsets, G, group_cap, max_steps,
        [&](int32_t *n_rows, int32_t *start) {
            hipLaunchKernelGGL(layer_prepass_kernel<true>, dim3((B + kPreMissions - 1) / kPreMissions), dim3(kThreads), 0, ctx->stream, coeffs,
                               seg_rows, seg_offsets, B, m, start_rows, delta, n_rows, start, ilayer, offsets, ctx->d_flags);
        },
        [&](dim3 grid, const int32_t *n_rows, const int32_t *start, Block block) {
            hipLaunchKernelGGL(wide_layer_seed_kernel, grid, dim3(kThreads), 0, ctx->stream, coeffs, seg_rows, seg_offsets, B, m, dt,
                               group_offsets, n_rows, start, r2, delta, max_steps, ilayer, block);
        },
        [&](dim3 grid, const int32_t *n_rows, const int32_t *start, Block block) {
            hipLaunchKernelGGL(wide_layer_kernel, grid, dim3(kThreads), 0, ctx->stream, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets,
                               n_rows, start, r2, delta, max_steps, cuboids, n_cuboids, ilayer, offsets, ctx->d_flags, block);
        });
}
