// Minimum-snap coefficient solve with BOUNDARY DERIVATIVES (gfx950): missions that start and end in motion.
//
// uavac_minsnap_solve_dev pins velocity, acceleration and jerk to zero at the first and last waypoint, like
// MinimumSnap._generate_start_and_goal_constraints upstream.  Here they are inputs: bc [B][6][3], rows 0-2 = (v, a, j) at the first
// waypoint, rows 3-5 = (v, a, j) at the last one, columns x y z.  In the knot-derivative coordinates of minsnap_kkt.h the boundary
// values are known "knot unknowns" x_0 and x_m, so they touch only the right-hand side of the first and last interior knot,
//     re_0[i]     -= sum_{j<3} B_0[j][i]     x_0[j]      (B_0^T x_0: what segment 0 couples from its start knot into knot 1)
//     rs_{m-1}[i] -= sum_{j<3} B_{m-1}[i][j] x_m[j]      (B_{m-1} x_m: what segment m-1 couples from its end knot into knot m-1)
// for i = 0..3 (the snap-continuity row included), and the coefficient reconstruction of the first and last segment, which takes
// x_0 / x_m where a knot's unknowns would be.  The 4x4 blocks, their elimination and the conditioning are those of the rest-to-rest
// system; m = 1 has no knot at all and its coefficients come straight from segment_coeffs.  By construction coefficients 1, 2, 3
// of a mission's first segment are v0, 0.5 a0 and j0 * (1/6) bit for bit.
//
// One lane per mission, one wave per workgroup, ONE-ENDED block-Thomas recurrence from the pieces of minsnap_kkt.h (same order of
// elimination as minsnap_solve_bt.hip).  [Ut | rt] of every knot but a lane's last waits in the HBM workspace [m-1][28][B] (coalesced
// over lanes); coefficients leave through the 64 x 24 LDS transpose of that file, last segment first.  Nothing is prefetched by
// hand: the kernel is new and unmeasured, and its inputs are (m + 1) x 24 + 144 bytes per mission.
// A singular knot system (repeated waypoint) reports status 1 and NaN coefficients; a non-finite value in a mission's bc gives that
// mission non-finite coefficients and status 0 (the pivots do not depend on bc), the other missions are unaffected.

#include "minsnap_kkt.h"
#include "minsnap_solve_launch.h"

#pragma clang fp contract(off)

namespace {

constexpr int TB = 64;          // lanes (missions) per workgroup = one wave

// RAGGED: mission b has m_b = seg_offsets[b + 1] - seg_offsets[b] segments (clamped to 1 .. m_uniform = the batch's maximum);
// waypoints, times and coefficients lie back to back.  The backward sweep counts segments from each mission's own end (lane l
// handles segment m_l - 1 - i in step i), so that the transpose moves one segment of every mission that has one left.
template <bool RAGGED>
__global__ void __launch_bounds__(TB) minsnap_solve_bc_kernel(const double *__restrict__ wp, const double *__restrict__ times,
                                                             const double *__restrict__ bc, int B, int m_uniform,
                                                             double *__restrict__ ws, double *__restrict__ coeffs,
                                                             int32_t *__restrict__ status, int32_t *__restrict__ flags,
                                                             const int64_t *__restrict__ seg_offsets,
                                                             const int64_t *__restrict__ guard_rows, int64_t guard_capacity) {
    // part of a planning chain whose rows would not fit the caller's buffer: the plan is refused as a whole (uniform over the launch)
    if (guard_rows && *guard_rows > guard_capacity) return;
    __shared__ double stage[TB * 25];                 // one segment's 24 coefficients per mission (+1 pad)
    __shared__ int64_t seg0_of[RAGGED ? TB : 1];      // ragged: first segment and segment count of every mission of the wave
    __shared__ int m_of[RAGGED ? TB : 1];
    const int lane = threadIdx.x;
    const int b0 = blockIdx.x * TB;
    const int b = b0 + lane;
    const bool live = b < B;
    const int bb = live ? b : B - 1;
    const size_t sB = (size_t)B;
    int m = m_uniform;
    const double *w = wp + (size_t)bb * (m_uniform + 1) * 3;
    const double *tm = times + (size_t)bb * m_uniform;
    int m_top = m_uniform;                            // steps of the backward sweep: the longest mission of the wave
    if (RAGGED) {
        const int64_t s0 = seg_offsets[bb], mb = seg_offsets[bb + 1] - s0;
        m = (int)(mb < 1 ? 1 : (mb > m_uniform ? m_uniform : mb));
        w = wp + ((size_t)s0 + (size_t)bb) * 3;
        tm = times + (size_t)s0;
        seg0_of[lane] = s0;
        m_of[lane] = m;
        m_top = live ? m : 1;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m_top = max(m_top, __shfl_xor(m_top, d));
        lds_wave_fence();
    }
    const int nk = m - 1;
    const double *bcb = bc + (size_t)bb * 18;
    double *park = ws + bb;                           // knot k's block: 28 values sB apart from park + k * 28 * sB
    bool ok = true;

    // ------------------------------------------------------------------ forward sweep over interior knots
    // ([Ut | rt] of a lane's LAST knot is what its backward sweep starts from: it stays in these registers, never parked)
    double Ut[4][4], rt[4][3];
    if (live && nk >= 1) {
        Seg prev, cur;
        double p0[3] = {w[0], w[1], w[2]}, p1[3] = {w[3], w[4], w[5]};
        build_segment(prev, tm[0], p0, p1);
        {
            double x0[3][3];
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int a = 0; a < 3; ++a) x0[j][a] = bcb[j * 3 + a];
            start_boundary_rhs(prev, x0);
        }
        for (int kk = 0; kk < nk; ++kk) {
            const int k = kk + 1;                      // knot k joins segments k-1 (prev) and k (cur)
#pragma unroll
            for (int a = 0; a < 3; ++a) { p0[a] = p1[a]; p1[a] = w[3 * (k + 1) + a]; }
            build_segment(cur, tm[k], p0, p1);
            if (k == m - 1) {
                double xg[3][3];
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int a = 0; a < 3; ++a) xg[j][a] = bcb[9 + j * 3 + a];
                goal_boundary_rhs(cur, xg);
            }
            double S[4][4], h[4][3], R[4][7];
            schur_behind(prev, kk > 0, Ut, rt, S, h);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    S[i][j] = S[i][j] + cur.A[i][j];
                    R[i][j] = cur.B[i][j];
                }
#pragma unroll
                for (int a = 0; a < 3; ++a) R[i][4 + a] = h[i][a] + cur.rs[i][a];
            }
            ok = solve4(S, R) && ok;
            if (kk < nk - 1) store_block(R, park + (size_t)kk * 28 * sB, sB);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) Ut[i][j] = R[i][j];
#pragma unroll
                for (int a = 0; a < 3; ++a) rt[i][a] = R[i][4 + a];
            }
            prev = cur;
        }
    }
    if (live) {
        if (!ok) atomicOr(&flags[1], 1);
        if (status) status[b] = ok ? 0 : 1;
    }

    // ------------------------------------------------ backward sweep + coefficients, last segment first
    // 64 missions x 24 doubles of one step leave the stage as 192-byte runs: mission q's segment sq = m_q - 1 - step, at
    // coeffs[(first segment of q + sq) * 24]
    auto flush = [&](int step) {
        for (int e = lane; e < TB * 24; e += TB) {
            const int q = e / 24, j = e - q * 24;
            const int sq = (RAGGED ? m_of[q] : m_uniform) - 1 - step;
            const size_t first = RAGGED ? (size_t)seg0_of[q] : (size_t)(b0 + q) * m_uniform;
            if (b0 + q < B && sq >= 0) coeffs[(first + (size_t)sq) * 24 + j] = stage[q * 25 + j];
        }
    };
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    double xn[4][3];                                    // unknowns of knot s+1: the goal's (v, a, j) to begin with (no multiplier there)
    double p1[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int j = 0; j < 3; ++j) xn[j][a] = bcb[9 + j * 3 + a];
        xn[3][a] = 0.0;
        p1[a] = w[3 * m + a];
    }
    for (int step = 0; step < m_top; ++step) {
        const int s = m - 1 - step;                     // this lane's segment; < 0: its mission is finished
        if (live && s >= 0) {
            const double T = tm[s];
            const double p0[3] = {w[3 * s], w[3 * s + 1], w[3 * s + 2]};
            double xs[4][3];                            // unknowns of knot s: the start's (v, a, j) for s = 0
            if (s >= 1) {
                double blk[28];
                if (s == nk) pack_block(Ut, rt, blk);
                else load_block(blk, park + (size_t)(s - 1) * 28 * sB, sB);
                substitute_knot(blk, s <= nk - 1, xn, xs);      // (s <= nk - 1: knot s has a successor among the unknowns)
            } else {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) xs[j][a] = bcb[j * 3 + a];
                    xs[3][a] = 0.0;
                }
            }
            double ip[8];
            const double r = 1.0 / T;
            ip[0] = 1.0;
#pragma unroll
            for (int e = 1; e < 8; ++e) ip[e] = ip[e - 1] * r;
            const double x0[3][3] = {{xs[0][0], xs[0][1], xs[0][2]}, {xs[1][0], xs[1][1], xs[1][2]}, {xs[2][0], xs[2][1], xs[2][2]}};
            const double x1[3][3] = {{xn[0][0], xn[0][1], xn[0][2]}, {xn[1][0], xn[1][1], xn[1][2]}, {xn[2][0], xn[2][1], xn[2][2]}};
            double c[8][3];
            segment_coeffs(ip, T, p0, p1, x0, x1, c);
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int a = 0; a < 3; ++a) stage[lane * 25 + i * 3 + a] = ok ? c[i][a] : qnan;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int a = 0; a < 3; ++a) xn[i][a] = xs[i][a];
#pragma unroll
            for (int a = 0; a < 3; ++a) p1[a] = p0[a];
        }
        lds_wave_fence();
        flush(step);
        lds_wave_fence();                               // (one wave: its LDS operations execute in order; this one is for the compiler)
    }
}

}  // namespace

int uavac_launch_solve_bc(uavac_ctx *ctx, const double *wp, const double *times, int B, int m, const double *bc, double *coeffs,
                          int32_t *status, const int64_t *seg_offsets, const int64_t *guard_rows, int64_t guard_capacity) {
    if (int rc = ensure_solve_workspace(ctx, B, m)) return rc;
    const dim3 grid((B + TB - 1) / TB);
    if (seg_offsets)
        hipLaunchKernelGGL(minsnap_solve_bc_kernel<true>, grid, dim3(TB), 0, ctx->stream, wp, times, bc, B, m, ctx->d_ws, coeffs, status,
                           ctx->d_flags, seg_offsets, guard_rows, guard_capacity);
    else
        hipLaunchKernelGGL(minsnap_solve_bc_kernel<false>, grid, dim3(TB), 0, ctx->stream, wp, times, bc, B, m, ctx->d_ws, coeffs, status,
                           ctx->d_flags, seg_offsets, guard_rows, guard_capacity);
    ctx->last_solve = seg_offsets ? "minsnap_solve_bc_kernel<true>" : "minsnap_solve_bc_kernel<false>";
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}
