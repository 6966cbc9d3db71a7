// Offset layers against committed traffic that never moves (gfx950): uavac_minsnap_layer_wide_dev's rule -- the cuboid policy -- with
// one more clause in "clear": the candidate layer is also outside the radius of every included traffic mission of its group, which is
// compared AS IT IS, on no layer.  The contract is in include/uavac.h (uavac_minsnap_layer_against_dev);
// uav_ac.scoring.layer_against_rows states it in NumPy on sampled rows.
//
// The kernels are the LayerObs instantiations of fleet_against.h -- which describes how the traffic reaches the block-wise search as a
// seed and a carry, the launch order and why the answers are the rule's -- and of fleet_wide.h:
//   layer_prepass_kernel<true>       fleet_search.h's, on the plan
//   traffic_prepass_kernel           the traffic's row totals and clamped starts
//   traffic_carry_kernel             per group: the included traffic and its horizon
//   against_layer_seed_kernel        once, before block 0: which candidate layers of every plan mission meet a traffic mission.  The
//                                    cuboids are the search's business alone, as in minsnap_layer_wide.hip
//   wide_layer_seed_kernel           per block k > 0
//   wide_layer_kernel                per block: the decisions, one workgroup per group

#include "fleet_against.h"

namespace {

__global__ void __launch_bounds__(kThreads, 3) against_layer_seed_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
    const int64_t *__restrict__ group_offsets, int G, const int32_t *__restrict__ n_rows, const int32_t *__restrict__ start, Traffic tr,
    const int32_t *__restrict__ t_n_rows, const int32_t *__restrict__ t_start, double r2, Delta delta, int max_steps, Block block) {
    fleet_seed_against(LayerObs{delta, nullptr, nullptr}, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, n_rows, start, tr, t_n_rows,
                       t_start, r2, max_steps, block);
}

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

int uavac_launch_layer_against(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                               const int64_t *group_offsets, int G, int group_cap, const int32_t *start_rows, const double *t_coeffs,
                               const int32_t *t_seg_rows, const int64_t *t_seg_offsets, int Bt, int mt, const int64_t *t_group_offsets,
                               const int32_t *t_start_rows, double radius, double delta_x, double delta_y, double delta_z, int max_steps,
                               const double *cuboids, int n_cuboids, int32_t *ilayer, double *offsets) {
    const double r2 = radius * radius;
    const Delta delta{delta_x, delta_y, delta_z};
    const int groups = group_offsets ? G : 1;
    const Traffic tr{t_coeffs, t_seg_rows, t_seg_offsets, Bt, mt, t_group_offsets, t_start_rows};
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
        },
        Bt, [&](int32_t *t_n_rows, int32_t *t_start) { launch_traffic_prepass(ctx, tr, t_n_rows, t_start); },
        [&](int32_t *t_n_rows, int32_t *t_start, const int32_t *n_rows, const int32_t *start, Block block) {
            launch_traffic_seed(ctx, B, groups, tr, t_n_rows, t_start, n_rows, start, block,
                                [&](dim3 grid, const int32_t *tn, const int32_t *ts, const int32_t *pn, const int32_t *ps, Block blk0) {
                                    hipLaunchKernelGGL(against_layer_seed_kernel, grid, dim3(kThreads), 0, ctx->stream, coeffs, seg_rows,
                                                       seg_offsets, B, m, dt, group_offsets, groups, pn, ps, tr, tn, ts, r2, delta, max_steps,
                                                       blk0);
                                });
        });
}
