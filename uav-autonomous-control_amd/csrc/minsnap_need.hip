// By how much a solved plan must be SLOWED DOWN for the vehicle to be able to give what it asks, per mission, without writing one of
// its rows (gfx950): the slowdown factor that the tilt bound, the upright condition, the largest and the least rotor thrust each ask
// for on their own.  The plan demand (minsnap_demand.hip) says WHAT a plan asks; this is what acting on it needs.
//
// Slowing a mission by k > 1 leaves its curve in place and divides the accelerations by u = k^2.  A row with acceleration a = (ax, ay,
// az) is admissible at u when (tau = max_tilt, Fmax / Fmin the specific thrust of four rotors at max_thrust / min_thrust, NED: hover
// has g - az = g):
//     tilt        ax^2 / n2 <= tau^2 and ay^2 / n2 <= tau^2   <=>  u >= (tau az + sqrt(q)) / (tau g),  q = max(ax^2 - tau^2 h, ay^2 -
//                                                                  tau^2 h, 0) > 0, h = ax^2 + ay^2 (an upright row)
//     upright     g u - az > 0                                <=   u >= az / g
//     thrust max  |a|^2 / u^2 - 2 g az / u + g^2 <= Fmax^2    <=>  u >= (sqrt((g az)^2 + |a|^2 D) - g az) / D,  D = Fmax^2 - g^2 > 0
//     thrust min  the same form >= Fmin^2                     <=   u >= (g az + sqrt(d)) / E,  E = g^2 - Fmin^2 > 0, az > 0 and
//                                                                  d = (g az)^2 - |a|^2 E >= 0
// The tilt condition is no power law in u, but per row each bound has this closed form, so the mission's answer is a maximum over rows:
// exact and order-free.  Division by a positive constant is monotone under rounding, so the NUMERATORS are reduced and lane 0 divides
// once per mission; no row is divided.
//
// Shape: the row walk of row_walk.h -- a group of 16 or 64 lanes per mission (the option "audit_lanes") walks exactly the sampler's
// rows --, four fmax accumulators start at -inf and the group reduces them with fmax.  No LDS, no scratch.
//
// ROUNDING (part of the contract, include/uavac.h): position, velocity and acceleration are the sampler's (the fma chains of
// minsnap_eval_row); every product, sum, difference, fmax and sqrt formed from them is ONE rounded operation -- contraction is off in
// row_need and in the final divides -- in the order the header states: bit for bit what NumPy computes from the sampled rows
// (uav_ac/scoring.py need_from_rows).
//
// fmax drops a NaN operand, so a non-finite sample is carried as a flag, as in the audit: such a mission (and one without rows) reports
// NaN in all four.  A singular plan never looks feasible.

#include "uavac_internal.h"
#include "minsnap_eval.h"
#include "row_walk.h"

#include <cmath>
#include <limits>

namespace {

using namespace mission_walk;
constexpr int kWaves = 4;                                   // wavefronts per workgroup

// The four numerators a row contributes; -inf where a bound does not count.
struct RowNeed {
    double tilt, upright, hi, lo;
};
__device__ __forceinline__ RowNeed row_need(double ax, double ay, double az, const NeedLimits &L) {
#pragma clang fp contract(off)
    const double ninf = -std::numeric_limits<double>::infinity();
    RowNeed n;
    const double xx = ax * ax, yy = ay * ay;
    const double h = xx + yy;
    const double A = h + az * az;
    const double gz = L.g * az;
    const double th = L.t2 * h;
    const double q = fmax(fmax(xx - th, yy - th), 0.0);
    n.tilt = q > 0.0 ? L.tau * az + sqrt(q) : ninf;
    n.upright = az;
    const double gg = gz * gz;
    n.hi = sqrt(gg + A * L.D) - gz;
    const double d = gg - A * L.E;
    n.lo = (az > 0.0 && d >= 0.0) ? gz + sqrt(d) : ninf;
    return n;
}

// the slowdown factor a reduced numerator asks for: one division, one fmax, one sqrt
__device__ __forceinline__ double factor_of(double numerator, double denominator) {
#pragma clang fp contract(off)
    return sqrt(fmax(numerator / denominator, 0.0));
}

// kLanes (16 or 64) lanes per mission, 64 / kLanes missions per wavefront.
template <int kLanes>
__global__ void __launch_bounds__(64 * kWaves) minsnap_need_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m,
    double dt, NeedLimits L, double *__restrict__ need) {
    const RowWalk<kLanes, kWaves> W(coeffs, seg_rows, seg_offsets, B, m);
    const int b = W.b, l = W.l;
    const bool live = W.live;
    const long long n_rows = W.n_rows;

    const double ninf = -std::numeric_limits<double>::infinity();
    double m_tilt = ninf, m_upright = ninf, m_hi = ninf, m_lo = ninf;
    double bad = 0.0;                                        // becomes NaN with the first non-finite sample

    W.each_row(dt, [&](const double (&c)[24], double t, long long) {
        double px, py, pz, vx, vy, vz, ax, ay, az;
        minsnap_eval_row<1>(c, t, px, py, pz, vx, vy, vz, ax, ay, az);
        const RowNeed n = row_need(ax, ay, az, L);
        m_tilt = fmax(m_tilt, n.tilt); m_upright = fmax(m_upright, n.upright);
        m_hi = fmax(m_hi, n.hi); m_lo = fmax(m_lo, n.lo);
        bad += nonfinite_probe(px, py, pz, vx, vy, vz, ax, ay, az);
    });

    // across the group: max -- exact whatever the order
    const auto peak = [](double x, double o) { return fmax(x, o); };
    m_tilt = group_reduce<kLanes>(m_tilt, peak); m_upright = group_reduce<kLanes>(m_upright, peak);
    m_hi = group_reduce<kLanes>(m_hi, peak); m_lo = group_reduce<kLanes>(m_lo, peak);
    bad = group_reduce<kLanes>(bad, Add());                  // (0 + 0 or NaN: order-free as well)
    const bool finite = bad == 0.0 && n_rows > 0;            // a mission without rows needs nothing that could be judged: NaN
    if (live && l == 0) {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        const size_t P = (size_t)B;
        need[b] = finite ? factor_of(m_tilt, L.tg) : nan;
        need[P + b] = finite ? factor_of(m_upright, L.g) : nan;
        need[2 * P + b] = finite ? factor_of(m_hi, L.D) : nan;
        need[3 * P + b] = finite ? factor_of(m_lo, L.E) : nan;
    }
}

}  // namespace

int uavac_launch_need(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                      const NeedLimits &limits, double *need) {
    return launch_by_lanes<kWaves>(ctx, B, [&](auto lanes, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((minsnap_need_kernel<lanes()>), grid, block, 0, ctx->stream, coeffs, seg_rows, seg_offsets, B, m, dt, limits, need);
    });
}
