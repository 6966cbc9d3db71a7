// Retiming factors (gfx950): by how much each mission of an audited plan has to be slowed down to stay inside the flight limits
// the control law clips its targets to (control_law.h: max_speed_xy, max_ascent, max_descent, max_horiz_accel).
//
// Scaling every segment duration of a mission by k > 1 -- planning it at velocity / k -- leaves the minimum-snap curve where it is,
// p'(t) = p(t / k): velocities scale by 1 / k, accelerations by 1 / k^2.  So from the four peaks of the plan audit
// (minsnap_audit.hip, rows 1-4 of the audit block) the factor a mission needs is
//     r = max(speed_xy / L0, ascent / L1, descent / L2, sqrt(accel_xy / L3))
// and, because the audit's peaks are maxima over SAMPLES and the samples of the slower plan fall elsewhere on the curve, a little
// more: k = r / (1 - margin).  A mission with r <= 1 is left alone, bit for bit.
//
// ROUNDING (part of the contract, include/uavac.h): every step is one rounded IEEE operation -- four divisions, one sqrt, three
// max, 1 - margin, r / (1 - margin), velocity / k, and factors_total * k in the loop -- contraction off; a NumPy restatement
// (uav_ac.scoring.retime_factors) reproduces factors and velocities bit for bit.
//
// retime_demand_factors_kernel is the same rule with the tilt, upright and thrust terms of the need block (minsnap_need.hip) beside the
// four above, and says which term binds; retime_factors_kernel is left as it was.
//
// One lane per mission.  The counters are summed per wavefront first (ballot + popcount), one atomicAdd per wavefront and counter.

#include "uavac_internal.h"

#include <cmath>
#include <limits>

namespace {

constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads) retime_factors_kernel(const double *__restrict__ audit, int B, RetimeLimits L,
                                                                  double margin, int apply, double *__restrict__ velocities,
                                                                  double *__restrict__ factors, int32_t *__restrict__ counters,
                                                                  double *__restrict__ factors_total,
                                                                  int32_t *__restrict__ converged) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * kThreads + threadIdx.x;
    bool slowed = false, broken = false;
    if (b < B) {
        const size_t P = (size_t)B;
        const double speed_xy = audit[P + b], ascent = audit[2 * P + b], descent = audit[3 * P + b], accel_xy = audit[4 * P + b];
        broken = isnan(speed_xy) || isnan(ascent) || isnan(descent) || isnan(accel_xy);
        double k = 1.0;
        if (broken) {
            k = std::numeric_limits<double>::quiet_NaN();
        } else {
            const double r = fmax(fmax(speed_xy / L.speed_xy, ascent / L.ascent), fmax(descent / L.descent, sqrt(accel_xy / L.horiz_accel)));
            slowed = r > 1.0;
            if (slowed) k = r / (1.0 - margin);
        }
        factors[b] = k;
        if (slowed && apply) velocities[b] = velocities[b] / k;
        if (factors_total) {
            if (broken) factors_total[b] = k;
            else if (slowed && apply) factors_total[b] = factors_total[b] * k;
        }
        if (converged) converged[b] = (!broken && !slowed) ? 1 : 0;
    }
    const int n_slowed = __popcll(__ballot(slowed)), n_broken = __popcll(__ballot(broken));
    if ((threadIdx.x & 63) == 0) {
        if (n_slowed) atomicAdd(&counters[0], n_slowed);
        if (n_broken) atomicAdd(&counters[1], n_broken);
    }
}

// The same rule with the four slowdown factors of the need block (minsnap_need.hip: tilt, upright, thrust_max, thrust_min) beside the
// audit's four terms: r = fmax(r_audit, fmax(fmax(need0, need1), fmax(need2, need3))), r_audit formed exactly as above; a NaN in either
// block breaks the mission.  binding [B]: the index 0 .. 7 of the FIRST term that attains r (speed_xy, ascent, descent, accel_xy, tilt,
// upright, thrust_max, thrust_min), -1 for a broken mission; written for every mission, also where r <= 1.
__global__ void __launch_bounds__(kThreads) retime_demand_factors_kernel(const double *__restrict__ audit, const double *__restrict__ need,
                                                                         int B, RetimeLimits L, double margin, int apply,
                                                                         double *__restrict__ velocities, double *__restrict__ factors,
                                                                         int32_t *__restrict__ binding, int32_t *__restrict__ counters,
                                                                         double *__restrict__ factors_total,
                                                                         int32_t *__restrict__ converged) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * kThreads + threadIdx.x;
    bool slowed = false, broken = false;
    if (b < B) {
        const size_t P = (size_t)B;
        const double speed_xy = audit[P + b], ascent = audit[2 * P + b], descent = audit[3 * P + b], accel_xy = audit[4 * P + b];
        double term[8];
        term[4] = need[b]; term[5] = need[P + b]; term[6] = need[2 * P + b]; term[7] = need[3 * P + b];
        broken = isnan(speed_xy) || isnan(ascent) || isnan(descent) || isnan(accel_xy) || isnan(term[4]) || isnan(term[5]) ||
                 isnan(term[6]) || isnan(term[7]);
        double k = 1.0;
        int first = -1;
        if (broken) {
            k = std::numeric_limits<double>::quiet_NaN();
        } else {
            term[0] = speed_xy / L.speed_xy; term[1] = ascent / L.ascent; term[2] = descent / L.descent;
            term[3] = sqrt(accel_xy / L.horiz_accel);
            const double r_audit = fmax(fmax(term[0], term[1]), fmax(term[2], term[3]));
            const double r = fmax(r_audit, fmax(fmax(term[4], term[5]), fmax(term[6], term[7])));
#pragma unroll
            for (int i = 7; i >= 0; --i) first = term[i] == r ? i : first;
            slowed = r > 1.0;
            if (slowed) k = r / (1.0 - margin);
        }
        factors[b] = k;
        binding[b] = first;
        if (slowed && apply) velocities[b] = velocities[b] / k;
        if (factors_total) {
            if (broken) factors_total[b] = k;
            else if (slowed && apply) factors_total[b] = factors_total[b] * k;
        }
        if (converged) converged[b] = (!broken && !slowed) ? 1 : 0;
    }
    const int n_slowed = __popcll(__ballot(slowed)), n_broken = __popcll(__ballot(broken));
    if ((threadIdx.x & 63) == 0) {
        if (n_slowed) atomicAdd(&counters[0], n_slowed);
        if (n_broken) atomicAdd(&counters[1], n_broken);
    }
}

__global__ void __launch_bounds__(kThreads) fill_f64_kernel(double *__restrict__ out, size_t n, double value) {
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) out[i] = value;
}

}  // namespace

int uavac_launch_retime_factors(uavac_ctx *ctx, const double *audit, int B, const RetimeLimits &limits, double margin, int apply,
                                double *velocities, double *factors, int32_t *counters, double *factors_total, int32_t *converged) {
    hipLaunchKernelGGL(retime_factors_kernel, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream, audit, B, limits,
                       margin, apply, velocities, factors, counters, factors_total, converged);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}

int uavac_launch_retime_demand_factors(uavac_ctx *ctx, const double *audit, const double *need, int B, const RetimeLimits &limits,
                                       double margin, int apply, double *velocities, double *factors, int32_t *binding, int32_t *counters,
                                       double *factors_total, int32_t *converged) {
    hipLaunchKernelGGL(retime_demand_factors_kernel, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream, audit, need, B,
                       limits, margin, apply, velocities, factors, binding, counters, factors_total, converged);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}

int uavac_launch_fill_f64(uavac_ctx *ctx, double *out, size_t n, double value) {
    const size_t blocks = (n + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(fill_f64_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(kThreads), 0, ctx->stream, out, n, value);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}
