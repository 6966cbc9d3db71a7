// The plan audit of a FLIGHT (gfx950): the plan audit (minsnap_audit.hip) says what a plan's rows would show against the flight limits
// and the cuboids; this one says what the VEHICLES did, which track their plans with an error, from the rollout's state log ([K][13][pitch]
// f64: x y z | q0 q1 q2 q3 | vx vy vz | p q r, quaternion scalar first) -- per vehicle the valid ticks, the peaks of horizontal speed,
// climb, descent, speed, the two rotation-matrix elements the control law clips with max_tilt, and the body rate; and per cuboid the
// ticks inside it, the first one, and the closest approach with its tick.  One pass over the log, nothing is read back and no log leaves
// the device.  The contract is in include/uavac.h (uavac_flown_audit_dev); uav_ac.scoring.audit_from_log states it in NumPy, and the
// results are the same bits.
//
// Two launches on the ctx stream:
//   flown_audit_kernel         a stream over the log.  A workgroup owns the 64 consecutive vehicles [64 x, 64 x + 64), one per lane, so a
//                              log row of a tick is one coalesced 512-byte load per wavefront and a tick is thirteen of them.  gridDim.y =
//                              P workgroups share a window and the four wavefronts of each split its share: wavefront w of share p is
//                              slot s = 4 p + w of S = 4 P and takes the ticks s, s + S, s + 2 S, ... two at a time, so 26 loads are in
//                              flight per wavefront before the first is waited for.  A tick is VALID iff its thirteen values are
//                              finite; only valid ticks count.  The peaks are running maxima of squares (or signed values) in
//                              registers.  The cuboids' bounds are uniform: scalar loads.  The per-cuboid state of a lane -- the
//                              smallest d^2 and its tick, the ticks inside, the first of them -- lives in LDS as [cuboid][thread]
//                              (20 bytes per cuboid and lane; a run-time cuboid count cannot index registers), read and written once
//                              per cuboid and pair of ticks.  At the end the four wavefronts meet through LDS and wavefront 0 leaves ONE
//                              partial record per vehicle and share in scratch.
//   flown_audit_merge_kernel   per vehicle: the P partial records merged, one correctly rounded sqrt per peak and clearance
// Every reduction is a maximum, an integer sum, an integer minimum or a lexicographic minimum of (d^2, tick): exact and independent of
// order, so the outputs depend neither on P (option "flown_audit_split"), nor on the pitch, nor on what else is in the batch; each output
// has one writer and there are no atomics.  Every column index is below B (lanes past the batch read column B - 1 and are masked):
// columns B .. pitch - 1 are never read.
//
// ROUNDING (part of the contract): contraction is off wherever a product meets a sum; the maxima are taken of the squares and the sqrt
// comes last (max and sqrt are monotone), so a peak equals np.sqrt(vx * vx + vy * vy).max() over the valid ticks bit for bit.

#include "uavac_internal.h"
#include "uavac_scratch.h"

#include <limits>

namespace {

constexpr int kTile = 64;                                   // vehicles per workgroup: one per lane
constexpr int kWaves = 4;                                   // wavefronts per workgroup: they split the workgroup's ticks
constexpr int kThreads = kTile * kWaves;
constexpr int kNone = 0x7fffffff;                           // "no such tick" while a minimum is being formed
constexpr int kPeaks = 7;                                   // audit rows 1 .. 7
constexpr int kExchange = (kWaves - 1) * kTile * (kPeaks + 1) * 8;      // LDS through which wavefronts 1 .. 3 hand their peaks over

// scratch: part_d [P][kPeaks + n][B] f64 (the peaks as squares / signed values, then the cuboids' smallest d^2),
//          part_i [P][2 + 3 n][B] i32 (valid ticks, first invalid tick, then per cuboid: tick of the smallest d^2, ticks inside, first inside)
__host__ __device__ constexpr int rows_d(int n) { return kPeaks + n; }
__host__ __device__ constexpr int rows_i(int n) { return 2 + 3 * n; }

__host__ __device__ constexpr size_t lds_bytes(int n) {
    return (size_t)n * kThreads * 20 > (size_t)kExchange ? (size_t)n * kThreads * 20 : (size_t)kExchange;
}

__device__ __forceinline__ bool lex_less(double d, int k, double od, int ok) { return d < od || (d == od && k < ok); }

struct Tick {
    double v[kLogRows];
};

__device__ __forceinline__ Tick load_tick(const double *__restrict__ col, long long k, long long tick, long long pitch) {
    Tick t;
    const double *at = col + k * tick;
#pragma unroll
    for (int r = 0; r < kLogRows; ++r) t.v[r] = at[r * pitch];
    return t;
}

__device__ __forceinline__ bool all_finite(const Tick &t) {
    bool ok = true;
#pragma unroll
    for (int r = 0; r < kLogRows; ++r) ok = ok & (bool)__builtin_isfinite(t.v[r]);
    return ok;
}

struct Peaks {
    double m[kPeaks];                                        // vxy^2, climb, descent, v^2, |R13|, |R23|, w^2
    int valid, first_bad;
};

__device__ __forceinline__ void take(Peaks &a, const Tick &t, bool ok, int k) {
#pragma clang fp contract(off)
    if (ok) {
        const double vx = t.v[7], vy = t.v[8], vz = t.v[9];
        const double xx = vx * vx, yy = vy * vy, zz = vz * vz;
        const double vxy2 = xx + yy;
        const double v2 = vxy2 + zz;                         // (vx * vx + vy * vy) + vz * vz, left to right
        const double q0 = t.v[3], q1 = t.v[4], q2 = t.v[5], q3 = t.v[6];
        const double a13 = q1 * q3, b13 = q0 * q2, a23 = q2 * q3, b23 = q0 * q1;
        const double r13 = 2.0 * (a13 + b13), r23 = 2.0 * (a23 - b23);
        const double p = t.v[10], q = t.v[11], r = t.v[12];
        const double pp = p * p, qq = q * q, rr = r * r;
        const double w2 = (pp + qq) + rr;
        a.m[0] = fmax(a.m[0], vxy2);
        a.m[1] = fmax(a.m[1], -vz);                          // NED: up is negative z
        a.m[2] = fmax(a.m[2], vz);
        a.m[3] = fmax(a.m[3], v2);
        a.m[4] = fmax(a.m[4], fabs(r13));
        a.m[5] = fmax(a.m[5], fabs(r23));
        a.m[6] = fmax(a.m[6], w2);
        a.valid += 1;
    } else {
        a.first_bad = min(a.first_bad, k);
    }
}

// one axis of the distance to a cuboid: selects, so that a NaN or inverted bound has the result np.where gives
__device__ __forceinline__ double outside(double p, double lo, double hi) { return p < lo ? lo - p : (p > hi ? p - hi : 0.0); }

struct Box {
    double x0, x1, y0, y1, z0, z1;
};

__device__ __forceinline__ double box_d2(double px, double py, double pz, const Box &c) {
#pragma clang fp contract(off)
    const double ex = outside(px, c.x0, c.x1), ey = outside(py, c.y0, c.y1), ez = outside(pz, c.z0, c.z1);
    const double xx = ex * ex, yy = ey * ey, zz = ez * ez;
    return (xx + yy) + zz;
}

// the inclusive test of the rollout's `collided` and of the plan audit; combined without short-circuit, as the rollout combines it
__device__ __forceinline__ bool box_in(double px, double py, double pz, const Box &c) {
    return (px >= c.x0) & (px <= c.x1) & (py >= c.y0) & (py <= c.y1) & (pz >= c.z0) & (pz <= c.z1);
}

// the cuboids against (up to) two ticks of this lane, ka < kb: the lane's state of cuboid q is read and written once
struct CuboidState {
    double *d2;                                              // [n][kThreads], this thread's column
    int *tick, *count, *first;
};

__device__ __forceinline__ void take_cuboids(const CuboidState &s, const double *__restrict__ cuboids, int n, const Tick &a, bool oka, int ka,
                                             const Tick &b, bool okb, int kb) {
#pragma nounroll
    for (int q = 0; q < n; ++q) {                            // (uniform trip count, uniform addresses of the bounds)
        const double *c = cuboids + q * 6;                   // all six bounds first: one scalar-cache round trip per cuboid
        const Box x = {c[0], c[1], c[2], c[3], c[4], c[5]};
        double best = s.d2[q * kThreads];
        int at = s.tick[q * kThreads], hits = 0, first = kNone;
        if (oka) {
            const double d = box_d2(a.v[0], a.v[1], a.v[2], x);
            if (lex_less(d, ka, best, at)) { best = d; at = ka; }
            if (box_in(a.v[0], a.v[1], a.v[2], x)) { hits += 1; first = ka; }
        }
        if (okb) {
            const double d = box_d2(b.v[0], b.v[1], b.v[2], x);
            if (lex_less(d, kb, best, at)) { best = d; at = kb; }
            if (box_in(b.v[0], b.v[1], b.v[2], x)) { hits += 1; first = min(first, kb); }
        }
        s.d2[q * kThreads] = best;
        s.tick[q * kThreads] = at;
        if (hits) {                                          // (rare)
            s.count[q * kThreads] += hits;
            s.first[q * kThreads] = min(s.first[q * kThreads], first);
        }
    }
}

__global__ void __launch_bounds__(kThreads, 4) flown_audit_kernel(const double *__restrict__ slog, int K, int B, long long pitch,
                                                                  const double *__restrict__ cuboids, int n, double *__restrict__ part_d,
                                                                  int32_t *__restrict__ part_i) {
    extern __shared__ double lds[];
    const double inf = std::numeric_limits<double>::infinity();
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int P = gridDim.y, p = blockIdx.y;
    const int b = blockIdx.x * kTile + lane;
    const bool live = b < B;
    const double *col = slog + (live ? b : B - 1);           // the lane's own column (a lane past the batch shadows the last vehicle)
    const long long tick = kLogRows * pitch;                 // doubles from one tick of the log to the next

    CuboidState st;
    st.d2 = lds + threadIdx.x;
    st.tick = reinterpret_cast<int *>(lds + (size_t)n * kThreads) + threadIdx.x;
    st.count = st.tick + n * kThreads;
    st.first = st.count + n * kThreads;
    for (int q = 0; q < n; ++q) {                            // (a thread touches its own column only: no barrier)
        st.d2[q * kThreads] = inf; st.tick[q * kThreads] = kNone; st.count[q * kThreads] = 0; st.first[q * kThreads] = kNone;
    }

    Peaks pk;
#pragma unroll
    for (int i = 0; i < kPeaks; ++i) pk.m[i] = -inf;
    pk.valid = 0; pk.first_bad = kNone;

    const int S = kWaves * P;
    int k = kWaves * p + w;                                  // this wavefront's ticks: k, k + S, ...
    for (; k < K - S; k += 2 * S) {                          // two ticks at a time: 26 loads in flight
        const Tick ta = load_tick(col, k, tick, pitch), tb = load_tick(col, k + S, tick, pitch);
        const bool oka = all_finite(ta), okb = all_finite(tb);
        take(pk, ta, oka, k);
        take(pk, tb, okb, k + S);
        if (n > 0) take_cuboids(st, cuboids, n, ta, oka, k, tb, okb, k + S);
    }
    if (k < K) {
        const Tick ta = load_tick(col, k, tick, pitch);
        const bool oka = all_finite(ta);
        take(pk, ta, oka, k);
        if (n > 0) take_cuboids(st, cuboids, n, ta, oka, k, ta, false, k);
    }

    // the four wavefronts meet.  The cuboids first: their state is in LDS already, wavefront 0 merges its lane's four columns
    const size_t Bs = (size_t)B;
    double *out_d = part_d + (size_t)p * rows_d(n) * Bs + b;
    int32_t *out_i = part_i + (size_t)p * rows_i(n) * Bs + b;
    if (n > 0) {
        __syncthreads();
        if (w == 0 && live) {
            const int *tk = reinterpret_cast<const int *>(lds + (size_t)n * kThreads), *cn = tk + n * kThreads, *fs = cn + n * kThreads;
            for (int q = 0; q < n; ++q) {
                double best = inf;
                int at = kNone, hits = 0, first = kNone;
#pragma unroll
                for (int v = 0; v < kWaves; ++v) {
                    const int i = q * kThreads + v * kTile + lane;
                    if (lex_less(lds[i], tk[i], best, at)) { best = lds[i]; at = tk[i]; }
                    hits += cn[i];
                    first = min(first, fs[i]);
                }
                out_d[(size_t)(kPeaks + q) * Bs] = best;
                out_i[(size_t)(2 + 3 * q) * Bs] = at;
                out_i[(size_t)(3 + 3 * q) * Bs] = hits;
                out_i[(size_t)(4 + 3 * q) * Bs] = first;
            }
        }
        __syncthreads();                                     // the cuboids' state has been read: its LDS carries the peaks now
    }
    // the peaks: wavefronts 1 .. 3 leave theirs as [wavefront - 1][8][64] (the eighth row: the two counters), wavefront 0 merges
    if (w != 0) {
        double *mine = lds + (size_t)(w - 1) * (kPeaks + 1) * kTile + lane;
#pragma unroll
        for (int i = 0; i < kPeaks; ++i) mine[i * kTile] = pk.m[i];
        int *c = reinterpret_cast<int *>(mine + kPeaks * kTile);      // (the lane's eight bytes of the eighth row)
        c[0] = pk.valid; c[1] = pk.first_bad;
    }
    __syncthreads();
    if (w == 0 && live) {
#pragma unroll
        for (int v = 0; v < kWaves - 1; ++v) {
            const double *theirs = lds + (size_t)v * (kPeaks + 1) * kTile + lane;
#pragma unroll
            for (int i = 0; i < kPeaks; ++i) pk.m[i] = fmax(pk.m[i], theirs[i * kTile]);
            const int *c = reinterpret_cast<const int *>(theirs + kPeaks * kTile);
            pk.valid += c[0];
            pk.first_bad = min(pk.first_bad, c[1]);
        }
#pragma unroll
        for (int i = 0; i < kPeaks; ++i) out_d[(size_t)i * Bs] = pk.m[i];
        out_i[0] = pk.valid;
        out_i[Bs] = pk.first_bad;
    }
}

__global__ void __launch_bounds__(kThreads) flown_audit_merge_kernel(int B, int P, int n, const double *__restrict__ part_d,
                                                                     const int32_t *__restrict__ part_i, double *__restrict__ audit,
                                                                     int32_t *__restrict__ first_bad, int32_t *__restrict__ hit_ticks,
                                                                     int32_t *__restrict__ first_hit, double *__restrict__ clearance,
                                                                     int32_t *__restrict__ clearance_tick) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    const size_t Bs = (size_t)B;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    double m[kPeaks];
#pragma unroll
    for (int i = 0; i < kPeaks; ++i) m[i] = -inf;
    int valid = 0, bad = kNone;
    for (int p = 0; p < P; ++p) {
        const double *d = part_d + (size_t)p * rows_d(n) * Bs + b;
        const int32_t *i32 = part_i + (size_t)p * rows_i(n) * Bs + b;
#pragma unroll
        for (int i = 0; i < kPeaks; ++i) m[i] = fmax(m[i], d[(size_t)i * Bs]);
        valid += i32[0];                                     // disjoint ticks: a sum
        bad = min(bad, i32[Bs]);
    }
    const bool any = valid > 0;
    audit[b] = (double)valid;
    audit[Bs + b] = any ? sqrt(m[0]) : nan;
    audit[2 * Bs + b] = any ? m[1] : nan;
    audit[3 * Bs + b] = any ? m[2] : nan;
    audit[4 * Bs + b] = any ? sqrt(m[3]) : nan;
    audit[5 * Bs + b] = any ? m[4] : nan;
    audit[6 * Bs + b] = any ? m[5] : nan;
    audit[7 * Bs + b] = any ? sqrt(m[6]) : nan;
    first_bad[b] = bad == kNone ? -1 : bad;
    for (int q = 0; q < n; ++q) {
        double best = inf;
        int at = kNone, hits = 0, first = kNone;
        for (int p = 0; p < P; ++p) {
            const double d = part_d[((size_t)p * rows_d(n) + kPeaks + q) * Bs + b];
            const int32_t *i32 = part_i + ((size_t)p * rows_i(n) + 2 + 3 * q) * Bs + b;
            const int k = i32[0];
            if (lex_less(d, k, best, at)) { best = d; at = k; }
            hits += i32[Bs];
            first = min(first, i32[2 * Bs]);
        }
        const size_t o = (size_t)q * Bs + b;
        hit_ticks[o] = hits;
        first_hit[o] = first == kNone ? -1 : first;
        clearance[o] = at == kNone ? nan : sqrt(best);
        clearance_tick[o] = at == kNone ? -1 : at;
    }
}

}  // namespace

int uavac_launch_flown_audit(uavac_ctx *ctx, const double *state_log, int K, int B, int64_t pitch, const double *cuboids, int n_cuboids,
                             double *audit, int32_t *first_bad, int32_t *hit_ticks, int32_t *first_hit, double *clearance,
                             int32_t *clearance_tick) {
    const int windows = (B + kTile - 1) / kTile;
    // Shares per window: enough workgroups for four wavefronts per SIMD (one workgroup per SIMD), never so many that a wavefront is left
    // with fewer than two pairs of ticks.  The results do not depend on it (option "flown_audit_split").
    int P = ctx->flown_audit_split;
    if (P <= 0) {
        P = (ctx->n_simds + windows - 1) / windows;
        const int most = K / (4 * kWaves);
        P = P > most ? most : P;
    }
    P = P < 1 ? 1 : (P > UAVAC_FLOWN_AUDIT_MAX_SPLIT ? UAVAC_FLOWN_AUDIT_MAX_SPLIT : P);
    double *part_d = nullptr;
    int32_t *part_i = nullptr;
    Scratch s(ctx);
    s.want(&part_d, (size_t)P * rows_d(n_cuboids) * B);
    s.want(&part_i, (size_t)P * rows_i(n_cuboids) * B);
    if (int rc = s.commit()) return rc;
    const size_t lds = lds_bytes(n_cuboids);                 // 16 cuboids: 80 KB, two workgroups per CU
    if (lds > 64 * 1024)
        UAVAC_HIP(ctx, hipFuncSetAttribute((const void *)flown_audit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(flown_audit_kernel, dim3(windows, P), dim3(kThreads), lds, ctx->stream, state_log, K, B, (long long)pitch, cuboids,
                       n_cuboids, part_d, part_i);
    hipLaunchKernelGGL(flown_audit_merge_kernel, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream, B, P, n_cuboids, part_d,
                       part_i, audit, first_bad, hit_ticks, first_hit, clearance, clearance_tick);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}
