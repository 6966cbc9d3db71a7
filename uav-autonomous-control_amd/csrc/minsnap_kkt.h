// The minimum-snap KKT system in knot-derivative coordinates: the pieces every form of the coefficient solve shares (gfx950).
// Included by minsnap_solve_tw.hip (two-ended block-Thomas, the default), minsnap_solve_bt.hip (one-ended, its cross-check),
// minsnap_solve_bc.hip (one-ended with boundary derivatives) and minsnap_solve.hip (pivoted banded LU: the tables only).  The C oracle of the tests keeps a copy of its own on purpose: it shares no code with the product.
//
// Replaces uav_ac/planning/minimum_snap.py:138-255 (_create_polynom_matrices / _create_snap_cost_matrix /
// _compute_spline_parameters).  The reference solves one dense (14m+2)^2 KKT system per mission in the monomial
// basis (cond ~1e10).  Here the same QP is restated in knot-derivative coordinates:
// unknowns are (v, a, j) at the m-1 interior knots, C1..C3 continuity and the
// position / rest constraints hold by construction, and the only equality left is
// continuity of the 4th derivative at each interior knot.  Per segment everything
// is a fixed 8x8 map scaled by powers of T (tau = t/T):
//     cost_s   = T^-7 * e^T Q1 e ,  e = diag(1,T,T^2,T^3,1,T,T^2,T^3) d
//     snap(0)  = T^-4 * S0 . e ,    snap(T) = T^-4 * S1 . e
//     c_tau    = W e ,              c_t[i]  = c_tau[i] T^-i
// with d = [p,v,a,j]@start (+) [p,v,a,j]@end and Q1, S0, S1, W exact small rationals
// (W = inverse of the README's 8x8 boundary matrix at T=1, Q1 = W^T H1 W).
// Unique optimum => identical coefficients to the reference's KKT solve.
//
// Ordered by knot, the KKT matrix of order 4(m-1) (cond ~4e4) is block tridiagonal with 4x4 blocks, unknowns
// (v, a, j, lambda) per interior knot:
//     D_k = C_{k-1} + A_k ,  U_k = B_k ,  L_k = B_{k-1}^T
// where segment s contributes the symmetric 8x8 local block [[A_s, B_s], [B_s^T, C_s]] (start knot /
// end knot), every entry a fixed small integer times a power of T_s.  The block-Thomas recurrence on it,
//     S_k = D_k - B_{k-1}^T Ut_{k-1} ;  [Ut_k | rt_k] = S_k^{-1} [B_k | r_k - B_{k-1}^T rt_{k-1}]
//     x_k = rt_k - Ut_k x_{k+1}
// runs in a lane's registers.  Each S_k is a saddle block [[G, c], [c^T, -e]] with G positive definite (the Hessian
// of the cost-to-go in the knot's derivatives) and e >= 0, so natural-order elimination needs no pivoting.
// [Ut_k | rt_k] waits for the substitution as a BLOCK of 28 doubles: Ut[i][j] at i * 4 + j, rt[i][a] at 16 + i * 3 + a.

#pragma once

#include "uavac_internal.h"

// File scope, as in control_law.h and minsnap_yaw.h: the pragma stays in force in the including file after the #include (clang does
// not restore it at the end of a header).  The two block-Thomas files want exactly that and say so again themselves; an includer that
// wants contraction has to turn it back on, as minsnap_solve.hip does.
#pragma clang fp contract(off)

namespace {

// Q1 = W^T H1 W: snap cost of a unit-duration septic in endpoint-derivative coordinates.
constexpr double Q1c[8][8] = {
    {100800, 50400, 10080, 840, -100800, 50400, -10080, 840},
    {50400, 25920, 5400, 480, -50400, 24480, -4680, 360},
    {10080, 5400, 1200, 120, -10080, 4680, -840, 60},
    {840, 480, 120, 16, -840, 360, -60, 4},
    {-100800, -50400, -10080, -840, 100800, -50400, 10080, -840},
    {50400, 24480, 4680, 360, -50400, 25920, -5400, 480},
    {-10080, -4680, -840, -60, 10080, -5400, 1200, -120},
    {840, 360, 60, 4, -840, 480, -120, 16}};
// 4th derivative at tau=0 / tau=1 as a function of the endpoint derivatives.
constexpr double S0c[8] = {-840, -480, -120, -16, 840, -360, 60, -4};
constexpr double S1c[8] = {840, 360, 60, 4, -840, 480, -120, 16};
// W = M1^-1: endpoint derivatives -> ascending monomial coefficients (rows 4..7; rows 0..3 are 1,1,1/2,1/6 diag).
constexpr double Wc[4][8] = {
    {-35, -20, -5, -2.0 / 3.0, 35, -15, 2.5, -1.0 / 6.0},
    {84, 45, 10, 1, -84, 39, -7, 0.5},
    {-70, -36, -7.5, -2.0 / 3.0, 70, -34, 6.5, -0.5},
    {20, 10, 2, 1.0 / 6.0, -20, 10, -2, 1.0 / 6.0}};

// Local 8x8 KKT entry (la, lb) of a segment as coefficient * T^-e.  Local index: 0..3 = (v, a, j, lambda)
// at the start knot, 4..7 at the end knot.  Both functions fold to literals once la, lb are unrolled.
__device__ __forceinline__ constexpr double loc_coef(int la, int lb) {
    const int ca = la & 3, cb = lb & 3;
    if (ca == 3 && cb == 3) return 0.0;
    if (ca == 3 || cb == 3) {
        const int ll = (ca == 3) ? la : lb, ld = (ca == 3) ? lb : la;
        const int d = (ld & 4) + (ld & 3) + 1;
        return (ll & 4) ? S1c[d] : -S0c[d];        // knot constraint: snap_end(prev) - snap_start(next) = 0
    }
    return Q1c[(la & 4) + ca + 1][(lb & 4) + cb + 1];
}
__device__ __forceinline__ constexpr int loc_exp(int la, int lb) {
    const int ca = la & 3, cb = lb & 3;
    if (ca == 3 && cb == 3) return 0;
    if (ca == 3) return 4 - (cb + 1);
    if (cb == 3) return 4 - (ca + 1);
    return 7 - (ca + 1) - (cb + 1);
}
// right-hand side of local row la: coefficient of p_start / p_end, times T^-e
__device__ __forceinline__ constexpr double rhs_c0(int la) {
    const int ca = la & 3;
    if (ca == 3) return (la & 4) ? -S1c[0] : S0c[0];
    return -Q1c[(la & 4) + ca + 1][0];
}
__device__ __forceinline__ constexpr double rhs_c1(int la) {
    const int ca = la & 3;
    if (ca == 3) return (la & 4) ? -S1c[4] : S0c[4];
    return -Q1c[(la & 4) + ca + 1][4];
}
__device__ __forceinline__ constexpr int rhs_exp(int la) { return ((la & 3) == 3) ? 4 : 7 - ((la & 3) + 1); }

struct Seg {
    double A[4][4], B[4][4], C[4][4];     // start-start, start-end, end-end blocks
    double rs[4][3], re[4][3];            // right-hand side rows of the start / end knot, per axis
    double ip[8];                         // T^-e
};

__device__ __forceinline__ void build_segment(Seg &g, double T, const double p0[3], const double p1[3]) {
    const double r = 1.0 / T;
    g.ip[0] = 1.0;
#pragma unroll
    for (int e = 1; e < 8; ++e) g.ip[e] = g.ip[e - 1] * r;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            g.A[i][j] = loc_coef(i, j) * g.ip[loc_exp(i, j)];
            g.B[i][j] = loc_coef(i, 4 + j) * g.ip[loc_exp(i, 4 + j)];
            g.C[i][j] = loc_coef(4 + i, 4 + j) * g.ip[loc_exp(4 + i, 4 + j)];
        }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            g.rs[i][a] = (rhs_c0(i) * p0[a] + rhs_c1(i) * p1[a]) * g.ip[rhs_exp(i)];
            g.re[i][a] = (rhs_c0(4 + i) * p0[a] + rhs_c1(4 + i) * p1[a]) * g.ip[rhs_exp(4 + i)];
        }
}

// Solve S X = R (4x4, 7 right-hand sides) in natural order; returns false on a zero / non-finite pivot.
__device__ __forceinline__ bool solve4(double S[4][4], double R[4][7]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double piv = S[j][j];
        ok = ok && (fabs(piv) > 0.0) && isfinite(piv);
        const double inv = 1.0 / piv;
#pragma unroll
        for (int i = j + 1; i < 4; ++i) {
            const double l = S[i][j] * inv;
#pragma unroll
            for (int c = j + 1; c < 4; ++c) S[i][c] = fma(-l, S[j][c], S[i][c]);
#pragma unroll
            for (int c = 0; c < 7; ++c) R[i][c] = fma(-l, R[j][c], R[i][c]);
        }
    }
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        const double inv = 1.0 / S[i][i];
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            double s = R[i][c];
#pragma unroll
            for (int q = i + 1; q < 4; ++q) s = fma(-S[i][q], R[q][c], s);
            R[i][c] = s * inv;
        }
    }
    return ok;
}

// H = C_prev - B_prev^T Ut, h = re_prev - B_prev^T rt: what the segments BEHIND a knot contribute to its 4x4 system (the Schur
// complement of everything eliminated so far).  With `any` false nothing has been eliminated yet: H = C_prev, h = re_prev.
__device__ __forceinline__ void schur_behind(const Seg &prev, bool any, const double Ut[4][4], const double rt[4][3], double H[4][4],
                                             double h[4][3]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double s = prev.C[i][j];
            if (any) {
#pragma unroll
                for (int l = 0; l < 4; ++l) s = fma(-prev.B[l][i], Ut[l][j], s);
            }
            H[i][j] = s;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double s = prev.re[i][a];
            if (any) {
#pragma unroll
                for (int l = 0; l < 4; ++l) s = fma(-prev.B[l][i], rt[l][a], s);
            }
            h[i][a] = s;
        }
    }
}

// ---- the 28-double block of a knot: solve4's R = [Ut | rt] out to where the block waits (`o`, values `stride` apart: registers,
// an LDS slab or the HBM workspace) and back.
// What the two kernels still spell out themselves, because every form of it as a function of this header moved their instruction
// streams (same operations, other schedule): the assembly of S and R ahead of solve4, the predicated store of R to park_at(), and
// the powers T^-e of the substitution step.
__device__ __forceinline__ void store_block(const double R[4][7], double *o, size_t stride) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[(size_t)(i * 4 + j) * stride] = R[i][j];
#pragma unroll
        for (int a = 0; a < 3; ++a) o[(size_t)(16 + i * 3 + a) * stride] = R[i][4 + a];
    }
}
__device__ __forceinline__ void pack_block(const double Ut[4][4], const double rt[4][3], double blk[28]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) blk[i * 4 + j] = Ut[i][j];
#pragma unroll
        for (int a = 0; a < 3; ++a) blk[16 + i * 3 + a] = rt[i][a];
    }
}
__device__ __forceinline__ void load_block(double blk[28], const double *o, size_t stride) {
#pragma unroll
    for (int i = 0; i < 28; ++i) blk[i] = o[(size_t)i * stride];
}

// Substitution at one knot: xs = rt - Ut xn from the knot's block and the unknowns xn of the knot solved before it
// (`coupled` false: there is none, xs = rt)
__device__ __forceinline__ void substitute_knot(const double blk[28], bool coupled, const double xn[4][3], double xs[4][3]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double v = blk[16 + i * 3 + a];
            if (coupled) {
#pragma unroll
                for (int l = 0; l < 4; ++l) v = fma(-blk[i * 4 + l], xn[l][a], v);
            }
            xs[i][a] = v;
        }
}

// 24 monomial coefficients (ascending powers, [8][3]) of one segment from its knot data
__device__ __forceinline__ void segment_coeffs(const double ip[8], double T, const double p0[3], const double p1[3],
                                               const double x0[3][3], const double x1[3][3], double out[8][3]) {
    const double T2 = T * T, T3 = T2 * T;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        // e = diag(1, T, T^2, T^3, 1, T, T^2, T^3) [p v a j]_start (+) [p v a j]_end
        const double e[8] = {p0[a], T * x0[0][a], T2 * x0[1][a], T3 * x0[2][a],
                             p1[a], T * x1[0][a], T2 * x1[1][a], T3 * x1[2][a]};
        out[0][a] = p0[a];
        out[1][a] = x0[0][a];
        out[2][a] = 0.5 * x0[1][a];
        out[3][a] = x0[2][a] * (1.0 / 6.0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) s = fma(Wc[i][q], e[q], s);
            out[4 + i][a] = s * ip[4 + i];
        }
    }
}

// ---- boundary derivatives (minsnap_solve_bc.hip): a mission that starts / ends in motion.  The known (v, a, j) of the first / last
// waypoint act like a knot's unknowns without a multiplier; what the first / last segment couples from them into its other knot
// moves to that knot's right-hand side, the snap-continuity row (i = 3) included.
// first segment: re -= B^T x0
__device__ __forceinline__ void start_boundary_rhs(Seg &g, const double x0[3][3]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double s = g.re[i][a];
#pragma unroll
            for (int j = 0; j < 3; ++j) s = fma(-g.B[j][i], x0[j][a], s);
            g.re[i][a] = s;
        }
}
// last segment: rs -= B xg
__device__ __forceinline__ void goal_boundary_rhs(Seg &g, const double xg[3][3]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double s = g.rs[i][a];
#pragma unroll
            for (int j = 0; j < 3; ++j) s = fma(-g.B[i][j], xg[j][a], s);
            g.rs[i][a] = s;
        }
}

}  // namespace
