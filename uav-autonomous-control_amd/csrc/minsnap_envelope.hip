// Every mission's SWEPT BOX, per mission, WITHOUT writing one of its rows (gfx950): the minimum and the maximum of the positions the
// sampler would write, per axis -- and, with a reach, of the positions of the same plan with the reach added to c0 of every segment as
// well.  What the split of a fleet into independent airspaces starts from (fleet_airspaces.hip): two missions whose boxes are a radius
// apart on some axis can never come inside that radius of each other, whatever their starts -- and, with reach = fl(max_steps * delta),
// whatever layers 0 .. max_steps the layer search grants them: rounded addition and the sampler's last fma are monotone in c0, so
// every row of every layer in between lies, per component, between the rows of layer 0 and of layer max_steps.  The contract is in
// include/uavac.h (uavac_minsnap_envelope_dev); uav_ac.scoring.envelope_from_rows states it in NumPy on sampled rows.
//
// Shape: the row walk of row_walk.h, the fourth kernel on it -- a group of 16 or 64 lanes per mission (the option "audit_lanes") walks
// exactly the sampler's rows.  Every lane carries three running minima and three maxima; after the walk the group reduces them with
// __shfl_xor.  Minimum and maximum are exact and independent of order, so the result depends neither on the lanes nor on the launch
// shape.  No LDS, no scratch, nothing is read back.
//
// ROUNDING (part of the contract).  Positions by the sampler's fma chain (minsnap_eval_pos: p = c7, then p = fma(p, t, c_i) for i = 6
// .. 0), hence the bits of the rows.  With a reach the coefficient of the second side is c0' = fl(c0 + reach[b][a]) -- a rounded sum of
// its own, never part of an fma: the rule of uavac_minsnap_shift_dev, which also leaves a mission alone whose three reach components
// are all zero -- and of the chain only the last fma sees it, as in minsnap_layer_kernel: one walk covers both sides.
//
// fmin / fmax drop a NaN operand, so a position that is not finite is carried as a flag (row_walk.h nonfinite_probe): such a mission,
// and one without rows, reports six NaN -- a box that is linked to nobody.

#include "uavac_internal.h"
#include "minsnap_eval.h"
#include "row_walk.h"

#include <cmath>
#include <limits>

namespace {

using namespace mission_walk;
constexpr int kWaves = 4;                                   // wavefronts per workgroup

// The chain of minsnap_eval_pos up to its last step: p = c7, p = fma(p, t, c_i) for i = 6 .. 1.  fma(p, t, c0) is the sampler's
// position, fma(p, t, c0') the position of the plan shifted by the reach.
__device__ __forceinline__ void eval_pos_head(const double (&c)[24], double t, double &hx, double &hy, double &hz) {
    hx = c[21]; hy = c[22]; hz = c[23];
#pragma unroll
    for (int i = 6; i >= 1; --i) {
        hx = fma(hx, t, c[3 * i]); hy = fma(hy, t, c[3 * i + 1]); hz = fma(hz, t, c[3 * i + 2]);
    }
}

// kLanes (16 or 64) lanes per mission, 64 / kLanes missions per wavefront.  REACH: a reach was given.
template <int kLanes, bool REACH>
__global__ void __launch_bounds__(64 * kWaves) minsnap_envelope_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m,
    double dt, const double *__restrict__ reach, double *__restrict__ env) {
#pragma clang fp contract(off)
    const RowWalk<kLanes, kWaves> W(coeffs, seg_rows, seg_offsets, B, m);
    const double inf = std::numeric_limits<double>::infinity();
    double lox = inf, loy = inf, loz = inf, hix = -inf, hiy = -inf, hiz = -inf;
    double bad = 0.0;                                        // becomes NaN with the first position that is not finite
    double rx = 0.0, ry = 0.0, rz = 0.0;
    bool moved = false;                                      // (uniform over the group)
    if (REACH) {
        const double *r = reach + 3 * (size_t)(W.live ? W.b : B - 1);
        rx = r[0]; ry = r[1]; rz = r[2];
        moved = !(rx == 0.0 && ry == 0.0 && rz == 0.0);      // an all-zero reach is not added (NaN != 0: a NaN reach is)
    }

    W.each_row(dt, [&](const double (&c)[24], double t, long long) {
        double hx, hy, hz;
        eval_pos_head(c, t, hx, hy, hz);
        const double px = fma(hx, t, c[0]), py = fma(hy, t, c[1]), pz = fma(hz, t, c[2]);
        lox = fmin(lox, px); loy = fmin(loy, py); loz = fmin(loz, pz);
        hix = fmax(hix, px); hiy = fmax(hiy, py); hiz = fmax(hiz, pz);
        bad += nonfinite_probe(px, py, pz);
        if (REACH && moved) {
            const double sx = c[0] + rx, sy = c[1] + ry, sz = c[2] + rz;      // c0' = fl(c0 + reach): rounded on its own
            const double qx = fma(hx, t, sx), qy = fma(hy, t, sy), qz = fma(hz, t, sz);
            lox = fmin(lox, qx); loy = fmin(loy, qy); loz = fmin(loz, qz);
            hix = fmax(hix, qx); hiy = fmax(hiy, qy); hiz = fmax(hiz, qz);
            bad += nonfinite_probe(qx, qy, qz);
        }
    });

    // across the group: min and max -- exact whatever the order
    const auto least = [](double a, double o) { return fmin(a, o); };
    const auto most = [](double a, double o) { return fmax(a, o); };
    lox = group_reduce<kLanes>(lox, least); loy = group_reduce<kLanes>(loy, least); loz = group_reduce<kLanes>(loz, least);
    hix = group_reduce<kLanes>(hix, most); hiy = group_reduce<kLanes>(hiy, most); hiz = group_reduce<kLanes>(hiz, most);
    bad = group_reduce<kLanes>(bad, Add());                  // (0 + 0 or NaN: order-free as well)
    if (W.live && W.l == 0) {
        const bool finite = bad == 0.0 && W.n_rows > 0;      // a mission without rows has no box either: NaN
        const double nan = std::numeric_limits<double>::quiet_NaN();
        double *e = env + 6 * (size_t)W.b;
        e[0] = finite ? lox : nan; e[1] = finite ? loy : nan; e[2] = finite ? loz : nan;
        e[3] = finite ? hix : nan; e[4] = finite ? hiy : nan; e[5] = finite ? hiz : nan;
    }
}

}  // namespace

int uavac_launch_envelope(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m,
                          double dt, const double *reach, double *env) {
    return launch_by_lanes<kWaves>(ctx, B, [&](auto lanes, dim3 grid, dim3 block) {
        if (reach)
            hipLaunchKernelGGL((minsnap_envelope_kernel<lanes(), true>), grid, block, 0, ctx->stream, coeffs, seg_rows, seg_offsets, B, m, dt,
                               reach, env);
        else
            hipLaunchKernelGGL((minsnap_envelope_kernel<lanes(), false>), grid, block, 0, ctx->stream, coeffs, seg_rows, seg_offsets, B, m, dt,
                               reach, env);
    });
}
