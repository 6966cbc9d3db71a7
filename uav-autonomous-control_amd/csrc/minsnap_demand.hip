// What a solved plan ASKS OF THE VEHICLE, per mission, without writing one of its rows (gfx950): the specific thrust a perfectly
// tracked plan needs (largest and smallest), the bank it needs about each axis, the roll / pitch rate the curve demands, the rows that
// ask for thrust downward, and per cuboid how near the sampled positions pass it and at which row first.
//
// The plan audit (minsnap_audit.hip) reports the four peaks the control law clips its TARGETS to.  The law clips a fifth thing, the bank
// command (control_law.h: bxc = clamp(acx / acc_z, +-max_tilt)), which on a perfectly tracked plan is |ax| / |a - g e3|: it depends on
// the vertical acceleration of the same row, binds long before max_horiz_accel does, and divides by g - az, which a fast plan can drive
// through zero.  The flight side has these columns (flown_audit.hip: bank_x, bank_y, body_rate, clearance); this is their plan side.
//
// Shape: the row walk of row_walk.h -- a group of 16 or 64 lanes per mission (the option "audit_lanes") walks exactly the sampler's
// rows -- and the group reduces at the end: max, min, integer add and a lexicographic minimum of (d2, row), all exact and independent
// of order.  Of that header's pieces this kernel takes all but each_row: the loop stands here in the kernel's own text, because the
// sixteen-cuboid launches measured slower through the lambda (profiles/NOTES.md R20).
//
// ROUNDING (part of the contract, include/uavac.h): position, velocity and acceleration are the sampler's (the fma chains of
// minsnap_eval_row), the jerk is that of minsnap_eval_jerk_snap; everything formed from them is separately rounded -- contraction is off
// in row_demand and gap2 -- in the order the header states, every maximum or minimum is taken of the SQUARES and one correctly rounded
// sqrt comes at the end: bit for bit what NumPy computes from the sampled rows and jerk (uav_ac/scoring.py demand_from_rows).
//
// fmax drops a NaN operand, so a non-finite sample is carried as a flag, as in the audit: such a mission (and one without rows) reports
// NaN demands, NaN clearances, every index -1 and no inverted row.  A singular plan never looks feasible.

#include "uavac_internal.h"
#include "row_walk.h"

#include <cmath>
#include <limits>

namespace {

using namespace mission_walk;
constexpr int kWaves = 4;                                   // wavefronts per workgroup
constexpr int kNoRow = 0x7fffffff;                          // "no such row" while a minimum is being formed

// Position, velocity, acceleration and jerk of one sample: the Horner of minsnap_eval.h with the third running derivative carried
// alongside.  Each level's fma chain reads only the levels below it, and the levels are updated top down, so p, d1 and d2 are the
// chains of minsnap_eval_row and d3 is the chain of minsnap_eval_jerk_snap: the same operations in the same order, the same bits.
__device__ __forceinline__ void eval_row_jerk(const double *c, double t, double p[3], double v[3], double a[3], double j[3]) {
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        double d0 = c[21 + x], d1 = 0, d2 = 0, d3 = 0;
#pragma unroll
        for (int i = 6; i >= 0; --i) {
            d3 = fma(d3, t, d2);
            d2 = fma(d2, t, d1);
            d1 = fma(d1, t, d0);
            d0 = fma(d0, t, c[3 * i + x]);
        }
        p[x] = d0; v[x] = d1; a[x] = 2.0 * d2; j[x] = 6.0 * d3;
    }
}

// What a row asks for, squared: specific thrust n2, the banks bx2 and by2, the roll / pitch rate w2; and whether it asks for thrust
// downward.  Every product, sum, quotient and fmax is one rounded operation, in the header's order.
struct RowDemand {
    double n2, bx2, by2, w2;
    bool inverted;
};
__device__ __forceinline__ RowDemand row_demand(const double a[3], const double j[3], double g) {
#pragma clang fp contract(off)
    RowDemand d;
    const double fz = g - a[2];                              // NED: hover has fz = g
    const double xx = a[0] * a[0], yy = a[1] * a[1];
    d.n2 = (xx + yy) + fz * fz;
    const bool some = d.n2 > 0.0;
    d.bx2 = some ? xx / d.n2 : 0.0;
    d.by2 = some ? yy / d.n2 : 0.0;
    const double jj = (j[0] * j[0] + j[1] * j[1]) + j[2] * j[2];
    const double jf = (j[0] * a[0] + j[1] * a[1]) - j[2] * fz;          // jerk along the thrust direction, times the thrust
    d.w2 = some ? fmax(jj - (jf * jf) / d.n2, 0.0) / d.n2 : 0.0;        // what is left across it, over the thrust: a rate squared
    d.inverted = fz <= 0.0;
    return d;
}

// Squared distance from a position to a cuboid x[6] = xmin xmax ymin ymax zmin zmax (0 inside or on a face), as scoring.audit_from_log
// forms it: a NaN bound compares false both ways and contributes 0.
__device__ __forceinline__ double gap2(const double *x, double px, double py, double pz) {
#pragma clang fp contract(off)
    const double ex = px < x[0] ? x[0] - px : (px > x[1] ? px - x[1] : 0.0);
    const double ey = py < x[2] ? x[2] - py : (py > x[3] ? py - x[3] : 0.0);
    const double ez = pz < x[4] ? x[4] - pz : (pz > x[5] ? pz - x[5] : 0.0);
    return (ex * ex + ey * ey) + ez * ez;
}

// kLanes (16 or 64) lanes per mission, 64 / kLanes missions per wavefront.  BOXES: cuboids were given.
// Dynamic LDS (BOXES only): the cuboids [n_cuboids][6] -- the same for every lane, so a read is one broadcast -- then every lane's own
// smallest d2 per cuboid, [n_cuboids][threads] f64, and the row that attained it, [n_cuboids][threads] i32.  They live there for the
// audit's reason: the loop over the cuboids has a run-time trip count.  Sixteen cuboids: 768 + 256 * 16 * 12 = 49 920 bytes, three
// workgroups per CU.  A lane's rows ascend, so replacing on a strictly smaller d2 keeps the first row that attains the minimum.
template <int kLanes, bool BOXES>
__global__ void __launch_bounds__(64 * kWaves) minsnap_demand_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m,
    double dt, double g, const double *__restrict__ cuboids, int n_cuboids, double *__restrict__ demand, int32_t *__restrict__ idemand,
    double *__restrict__ clearance, int32_t *__restrict__ clearance_row) {
    constexpr int kThreads = 64 * kWaves;
    extern __shared__ double lds[];
    const double *box = lds;                                                              // [n_cuboids][6]
    double *near2 = lds + 6 * n_cuboids + threadIdx.x;                                    // [n_cuboids][kThreads], this lane's column
    int *near_row = reinterpret_cast<int *>(lds + (6 + kThreads) * n_cuboids) + threadIdx.x;      // [n_cuboids][kThreads]

    const RowWalk<kLanes, kWaves> W(coeffs, seg_rows, seg_offsets, B, m);
    const int b = W.b, l = W.l;
    const bool live = W.live;
    const long long total = W.total, n_rows = W.n_rows;

    const double inf = std::numeric_limits<double>::infinity();
    if (BOXES) {
        stage_cuboids<kThreads>(lds, cuboids, n_cuboids);
        // before any row: (+inf, the lane's first row) -- the lowest row wins a tie, also among rows that are all infinitely far
        for (int q = 0; q < n_cuboids; ++q) { near2[q * kThreads] = inf; near_row[q * kThreads] = l < n_rows ? l : kNoRow; }
        __syncthreads();
    }

    double m_nmax = -inf, m_nmin = inf, m_bx2 = -inf, m_by2 = -inf, m_w2 = -inf;
    double bad = 0.0;                                        // becomes NaN with the first non-finite sample
    int inv_count = 0, inv_first = kNoRow;

    // RowWalk::each_row's loop, kept as text: through the lambda the launches with sixteen cuboids measured 1.3 % (16 lanes) and 2.2 %
    // (64 lanes) slower at equal registers and instruction count -- the cuboid loop lands four bytes later (profiles/NOTES.md R20).  A
    // change to the walk is made there AND here.
    const int mb = W.mb;
    const int32_t *rows_of = W.rows_of;
    const double *cm = W.cm;
    double c[24];                                            // coefficients of the segment this lane stands in
    int s = 0, loaded = -1, cnt = rows_of[0];                // this lane's segment, the one in `c`, its row count
    long long base = 0;                                      // ... and its first row
    for (long long r = l; r < n_rows; r += kLanes) {
        seek(rows_of, mb, r, s, base, cnt);
        if (s != loaded) {
#pragma unroll
            for (int k = 0; k < 24; ++k) c[k] = cm[s * 24 + k];
            loaded = s;
        }
        const double t = (double)(int)(r - base) * dt;
        double p[3], v[3], a[3], j[3];
        eval_row_jerk(c, t, p, v, a, j);
        const RowDemand d = row_demand(a, j, g);
        m_nmax = fmax(m_nmax, d.n2); m_nmin = fmin(m_nmin, d.n2);
        m_bx2 = fmax(m_bx2, d.bx2); m_by2 = fmax(m_by2, d.by2); m_w2 = fmax(m_w2, d.w2);
        if (d.inverted) { inv_count += 1; inv_first = min(inv_first, (int)r); }
        bad += nonfinite_probe(p[0], p[1], p[2], v[0], v[1], v[2], a[0], a[1], a[2], j[0], j[1], j[2]);
        if (BOXES) {
#pragma nounroll
            for (int q = 0; q < n_cuboids; ++q) {            // (uniform trip count)
                const double d2 = gap2(box + q * 6, p[0], p[1], p[2]);
                if (d2 < near2[q * kThreads]) { near2[q * kThreads] = d2; near_row[q * kThreads] = (int)r; }
            }
        }
    }

    // across the group: max, min, integer add -- exact whatever the order
    const auto peak = [](double x, double o) { return fmax(x, o); };
    const auto least = [](int x, int o) { return min(x, o); };
    m_nmax = group_reduce<kLanes>(m_nmax, peak);
    m_nmin = group_reduce<kLanes>(m_nmin, [](double x, double o) { return fmin(x, o); });
    m_bx2 = group_reduce<kLanes>(m_bx2, peak); m_by2 = group_reduce<kLanes>(m_by2, peak); m_w2 = group_reduce<kLanes>(m_w2, peak);
    inv_count = group_reduce<kLanes>(inv_count, Add());
    inv_first = group_reduce<kLanes>(inv_first, least);
    bad = group_reduce<kLanes>(bad, Add());                  // (0 + 0 or NaN: order-free as well)
    const bool finite = bad == 0.0 && n_rows > 0;            // a mission without rows demands nothing that could be judged: NaN
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (BOXES) {
        for (int q = 0; q < n_cuboids; ++q) {
            // the lexicographic minimum of (d2, row): a total order, so the tree's shape does not matter
            double d2 = near2[q * kThreads];
            int row = near_row[q * kThreads];
#pragma unroll
            for (int w = kLanes / 2; w >= 1; w >>= 1) {
                const double od2 = __shfl_xor(d2, w);
                const int orow = __shfl_xor(row, w);
                if (od2 < d2 || (od2 == d2 && orow < row)) { d2 = od2; row = orow; }
            }
            if (live && l == 0) {
                clearance[(size_t)q * B + b] = finite ? sqrt(d2) : nan;
                clearance_row[(size_t)q * B + b] = finite ? row : -1;
            }
        }
    }
    if (live && l == 0) {
        const size_t P = (size_t)B;
        demand[b] = (double)total;
        demand[P + b] = finite ? sqrt(m_nmax) : nan;
        demand[2 * P + b] = finite ? sqrt(m_nmin) : nan;
        demand[3 * P + b] = finite ? sqrt(m_bx2) : nan;
        demand[4 * P + b] = finite ? sqrt(m_by2) : nan;
        demand[5 * P + b] = finite ? sqrt(m_w2) : nan;
        idemand[b] = finite ? inv_count : 0;
        idemand[P + b] = (finite && inv_first != kNoRow) ? inv_first : -1;
    }
}

}  // namespace

int uavac_launch_demand(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                        double g, const double *cuboids, int n_cuboids, double *demand, int32_t *idemand, double *clearance,
                        int32_t *clearance_row) {
    const size_t lds = (size_t)n_cuboids * (6 * sizeof(double) + (sizeof(double) + sizeof(int)) * 64 * kWaves);      // 16 cuboids: 48.75 KB
    return launch_by_lanes<kWaves>(ctx, B, [&](auto lanes, dim3 grid, dim3 block) {
        if (n_cuboids > 0)
            hipLaunchKernelGGL((minsnap_demand_kernel<lanes(), true>), grid, block, lds, ctx->stream, coeffs, seg_rows, seg_offsets, B, m, dt,
                               g, cuboids, n_cuboids, demand, idemand, clearance, clearance_row);
        else
            hipLaunchKernelGGL((minsnap_demand_kernel<lanes(), false>), grid, block, 0, ctx->stream, coeffs, seg_rows, seg_offsets, B, m, dt,
                               g, cuboids, n_cuboids, demand, idemand, clearance, clearance_row);
    });
}
