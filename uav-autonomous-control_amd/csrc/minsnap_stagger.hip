// Fleet deconfliction by start delay (gfx950): the call that acts on the separation audit's verdict (minsnap_separation.hip).  Within a
// group the missions are taken in ascending batch index -- the priority --, and each gets the smallest start delay S_i + q * step,
// q = 0 .. max_steps, that keeps it outside the protection radius of every mission decided before it, over the whole shared clock.
// From coefficients and row counts alone: no row is written, nothing is read back.  The contract -- the clock, the groups, the
// excluded missions and the rounding are the audit's -- is in include/uavac.h (uavac_minsnap_stagger_dev);
// uav_ac.scoring.stagger_from_rows states it in NumPy on sampled rows, and the results are the same integers.
//
// Two launches on the ctx stream:
//   stagger_prepass_kernel   per mission: fleet_clock.h's pre-pass -- row total N (0: EXCLUDED), base start clamped to 0 .. 2^29, in ctx
//                            scratch -- and the record of a mission that is never examined -- base start / -2 / 0 -- in istag, which the
//                            decision kernel overwrites for everybody it decides
//   minsnap_stagger_kernel   the decisions: fleet_search.h's search with the Delay policy.  THE 64 LANES ARE 64 CANDIDATE DELAYS of one
//                            mission: lane l stands at start S_i + (q0 + l) * step, the partners at their GRANTED starts, nobody's
//                            coefficients are touched; the horizon of a round reaches past its last candidate's last row; a mission
//                            that is not resolved stays at its base start.
// The structure of the search, its rounding and why its outputs depend on nothing but the contract are described there.

#include "fleet_search.h"
#include "stagger_prepass.h"

namespace {

// (the pre-pass is stagger_prepass.h's: the block-wise form, minsnap_stagger_wide.hip, launches it too)
// ------------------------------------------------------------------------------------------------------------------ the decisions
__global__ void __launch_bounds__(kThreads, 3) minsnap_stagger_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
    const int64_t *__restrict__ group_offsets, const int32_t *__restrict__ n_rows, const int32_t *__restrict__ start, double r2, int step,
    int max_steps, int32_t *__restrict__ istag, int32_t *__restrict__ flags) {
    fleet_search(Delay{step, istag}, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, n_rows, start, r2, max_steps, nullptr, 0, flags);
}

}  // namespace

int uavac_launch_stagger(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                         const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, int step, int max_steps,
                         int32_t *istag) {
    int32_t *n_rows = nullptr, *start = nullptr;
    Scratch s(ctx);
    s.want(&n_rows, B); s.want(&start, B);
    if (int rc = s.commit()) return rc;
    hipLaunchKernelGGL(stagger_prepass_kernel, dim3((B + kPreMissions - 1) / kPreMissions), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows, seg_offsets, B,
                       m, start_rows, n_rows, start, istag, ctx->d_flags);
    hipLaunchKernelGGL(minsnap_stagger_kernel, dim3(group_offsets ? G : 1), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows, seg_offsets, B, m,
                       dt, group_offsets, n_rows, start, radius * radius, step, max_steps, istag, ctx->d_flags);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}
