// Host side that the launchers of the two block-Thomas kernels share (minsnap_solve_tw.hip, minsnap_solve_bt.hip): the HBM workspace
// and the launch of one kernel instantiation.  The shape rules (lanes, parking, keeping) are measured per kernel and stay in each file.

#pragma once

#include "uavac_internal.h"

namespace {

// The HBM workspace [m - 1][28][B] (rows = a knot's index in its mission) where blocks wait that have no place on chip.
int ensure_solve_workspace(uavac_ctx *ctx, int B, int m) {
    const size_t need = (size_t)(m > 1 ? m - 1 : 1) * 28 * (size_t)B;
    return uavac_grow(ctx, ctx->d_ws, ctx->ws_cap, need, sizeof(double) * need);
}

// Launches `kern`, the instantiation `family`<ragged, park_lds, n, nreg> of a block-Thomas kernel (one wave per workgroup), with
// `dyn_lds` bytes of dynamic LDS and leaves its name for uavac_last_solve_kernel().
template <typename Kernel>
int launch_solve_kernel(uavac_ctx *ctx, Kernel kern, const char *family, bool ragged, bool park_lds, int n, int nreg, dim3 grid,
                        size_t dyn_lds, const double *wp, const double *times, int B, int m, double *coeffs, int32_t *status,
                        const int64_t *seg_offsets, const int64_t *guard_rows, int64_t guard_capacity, const int32_t *active) {
    if (dyn_lds > 48 * 1024) UAVAC_HIP(ctx, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_lds));
    hipLaunchKernelGGL(kern, grid, dim3(64), dyn_lds, ctx->stream, wp, times, B, m, ctx->d_ws, coeffs, status, ctx->d_flags, seg_offsets,
                       guard_rows, guard_capacity, active);
    ctx->last_solve = std::string(family) + (ragged ? "<true, " : "<false, ") + (park_lds ? "true, " : "false, ") + std::to_string(n) + ", " +
                      std::to_string(nreg) + ">";
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}

}  // namespace
