// Fleet deconfliction by offset layers (gfx950), and the offset as a plan transform.  Where uavac_minsnap_stagger_dev makes a mission
// WAIT, this call MOVES it: within a group the missions are taken in ascending batch index -- the priority --, the starts are FIXED,
// and each mission gets the lowest layer q = 0 .. max_steps -- the mission with the offset fl(q * delta) added to c0 of every one of
// its segments -- that keeps it outside the protection radius of every mission decided before it, over the whole shared clock.  From
// coefficients and row counts alone: no row is written, nothing is read back.  The contract -- the clock, the groups, the excluded
// missions and the rounding are the audit's and stagger's -- is in include/uavac.h (uavac_minsnap_layer_dev, uavac_minsnap_shift_dev);
// uav_ac.scoring.layer_from_rows states the search in NumPy on sampled rows, uav_ac.scoring.shift_coeffs the transform.
//
// Three kernels, all on the ctx stream:
//   layer_prepass_kernel   per mission (sixteen lanes each), the audit's and stagger's: its row total N, its start clamped to 0 ..
//                          2^29, whether it is EXCLUDED (kept as N = 0 in ctx scratch); and the record of a mission that is never
//                          examined -- layer 0 / -2 / 0 and the offset of layer 0 -- which the decision kernel overwrites for everybody
//                          it decides
//   minsnap_layer_kernel   the decisions.  Stagger's structure with another candidate axis: one workgroup of four wavefronts per group
//                          walks the group's included missions in ascending order; for mission i THE 64 LANES ARE 64 CANDIDATE LAYERS
//                          of that one mission, lane l stands on layer q0 + l.  The earlier missions come in j-tiles of 64, the clock
//                          from 0 to the horizon in chunks of 32 rows, wave w taking rows 8 w .. 8 w + 7; for its rows a wave evaluates
//                          the j-tile's positions ON THEIR GRANTED LAYERS into its own quarter of the LDS tile (lane = j), then each
//                          lane evaluates its own candidate and reads the partners as LDS broadcasts.  All 64 candidates share the
//                          start, hence the clock row, the segment and t: only c0 differs between the lanes, and of the Horner chain
//                          only the last fma per axis sees it.  A lane keeps one bit: somebody was inside.  After the last tile the
//                          four waves OR their bits through LDS and every thread takes the same decision: the lowest clear lane with
//                          q <= max_steps is granted; if there is none the next 64 layers are examined; after the last one the mission
//                          is unresolved and stays on layer 0.  The OR lives in one LDS word (`round_hit`) that every wave feeds after
//                          each chunk in which a lane of its met somebody; once every live candidate is in it the round's answer is
//                          "none" whatever else would be found, and every wave leaves the round at its next chunk: reading the word
//                          early or late changes the time only.
//   minsnap_shift_kernel   the transform: out = coeffs with offsets[b] added to c0 of every segment of mission b.  One thread per 16
//                          bytes of the coefficients, twelve per segment; c0 = (x, y, z) is piece 0 and the first half of piece 1.
// The granted layers of the group live in LDS (256 int32: hence UAVAC_LAYER_MAX_GROUP).  A workgroup never waits for another one, and
// nothing is spun on anywhere: round_hit is looked at once per chunk; the only atomic on global memory is the sticky flag.
//
// ROUNDING (part of the contract).  The offset of layer q on axis a is o = fl((double)q * delta_a), the candidate's coefficient
// c0' = fl(c0 + o): two roundings, never one fma; layer 0 is the mission as it is (nothing is added).  Positions by the sampler's fma
// chain on those coefficients (minsnap_eval_pos), the distance WITHOUT contraction: d^2 = (dx dx + dy dy) + dz dz.

#include "uavac_internal.h"
#include "minsnap_eval.h"

#include <limits>

namespace {

constexpr int kTile = 64;                                   // earlier missions per j-tile, and candidate layers per round: one per lane
constexpr int kWaves = 4;                                   // wavefronts per workgroup
constexpr int kRows = 8;                                    // clock rows of a chunk per wavefront
constexpr int kChunk = kWaves * kRows;                      // clock rows per chunk
constexpr int kThreads = 64 * kWaves;
constexpr int kRegion = kRows * kTile * 3;                  // doubles of the LDS tile per wavefront (12 KB; 48 KB per workgroup)
constexpr int kMaxClock = 1 << 29;                          // start rows and row totals above this cannot be clocked with int
constexpr int kUnroll = 8;                                  // partners per unrolled step of the pair loop
constexpr int kPreLanes = 16;                               // lanes per mission of the pre-pass
constexpr int kMaxGroup = UAVAC_LAYER_MAX_GROUP;            // missions of a group: their granted layers live in LDS
constexpr int kPairs = 12;                                  // 16-byte pieces of a segment's 24 coefficients

struct Delta {
    double x, y, z;
};

// First segment and segment count of mission b: uniform (so == NULL) or ragged, clamped to 1 .. m like every ragged kernel clamps it.
struct Mission {
    long long s0;
    int m;
};
__device__ __forceinline__ Mission mission_of(const int64_t *__restrict__ so, int b, int m_uniform) {
    Mission M;
    if (so) {
        M.s0 = so[b];
        const long long n = so[b + 1] - M.s0;
        M.m = (int)(n < 1 ? 1 : (n > m_uniform ? m_uniform : n));
    } else {
        M.s0 = (long long)b * m_uniform;
        M.m = m_uniform;
    }
    return M;
}

// the offset of layer q on one axis: one rounded product
__device__ __forceinline__ double layer_offset(int q, double delta) {
#pragma clang fp contract(off)
    const double o = (double)q * delta;
    return o;
}

// c0 of a mission on layer q: the product and the sum are rounded one after the other; layer 0 adds nothing
__device__ __forceinline__ double layer_c0(double c0, int q, double delta) {
#pragma clang fp contract(off)
    const double o = (double)q * delta;
    const double moved = c0 + o;
    return q == 0 ? c0 : moved;
}

// ------------------------------------------------------------------------------------------------------------------ pre-pass
// (the audit's pre-pass, restated as stagger restates it: every object file holds exactly its own kernels)
__global__ void __launch_bounds__(kThreads) layer_prepass_kernel(const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows,
                                                                 const int64_t *__restrict__ seg_offsets, int B, int m,
                                                                 const int32_t *__restrict__ start_rows, Delta delta,
                                                                 int32_t *__restrict__ n_rows, int32_t *__restrict__ start,
                                                                 int32_t *__restrict__ ilayer, double *__restrict__ offsets,
                                                                 int32_t *__restrict__ flags) {
    constexpr int kPerWave = 64 / kPreLanes;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = lane / kPreLanes, l = lane % kPreLanes;
    const int b = (blockIdx.x * kWaves + w) * kPerWave + g;
    const bool live = b < B;
    const Mission M = mission_of(seg_offsets, live ? b : B - 1, m);
    const int32_t *rows_of = seg_rows + M.s0;
    const double *cm = coeffs + (size_t)M.s0 * 24;
    long long total = 0;                                     // the mission's rows: what the sampler's row offsets give it
    for (int s = 0; s < M.m; ++s) total += rows_of[s];
    double z = 0.0;                                          // stays 0 while every coefficient is finite (0 * inf and 0 * NaN are NaN)
    for (int k = l; k < M.m * 24; k += kPreLanes) z = fma(0.0, cm[k], z);
#pragma unroll
    for (int d = kPreLanes / 2; d >= 1; d >>= 1) z += __shfl_xor(z, d);
    if (live && l == 0) {
        int s = start_rows ? start_rows[b] : 0;
        bool bad = s < 0 || s > kMaxClock;                   // cannot be refused by the host: clamped, and flag 0
        s = s < 0 ? 0 : (s > kMaxClock ? kMaxClock : s);
        const bool too_long = total > kMaxClock;
        const bool excluded = !(z == 0.0) || total < 1 || too_long;
        n_rows[b] = excluded ? 0 : (int)total;
        start[b] = s;
        ilayer[b] = 0; ilayer[(size_t)B + b] = -2; ilayer[2 * (size_t)B + b] = 0;     // "not examined", until the decision kernel says otherwise
        double *o = offsets + 3 * (size_t)b;
        o[0] = layer_offset(0, delta.x); o[1] = layer_offset(0, delta.y); o[2] = layer_offset(0, delta.z);
        if (bad || too_long) atomicOr(&flags[0], 1);
    }
}

// ------------------------------------------------------------------------------------------------------------------ the decisions
// the segment of a mission's row r, walked forward from where the lane stood (rows only grow): the audit's walk
__device__ __forceinline__ void seek(const int32_t *__restrict__ rows_of, int mb, int r, int &s, int &base, int &cnt) {
    while (s + 1 < mb && r >= base + cnt) { base += cnt; ++s; cnt = rows_of[s]; }
}

// One row of the lane's candidate against the first n positions of a j-tile at the same clock row (row [64][3] in LDS, the same for
// every lane; n a multiple of kUnroll, the entries past the tile's last partner are NaN): is anybody inside?
__device__ __forceinline__ bool inside_row(const double *row, int n, double xi, double yi, double zi, double r2) {
#pragma clang fp contract(off)
    bool in = false;
#pragma nounroll
    for (int q = 0; q < n; q += kUnroll) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int jj = q + u;
            const double dx = xi - row[3 * jj], dy = yi - row[3 * jj + 1], dz = zi - row[3 * jj + 2];
            const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
            const double d2 = (xx + yy) + zz;
            in |= d2 < r2;
        }
    }
    return in;
}

__global__ void __launch_bounds__(kThreads, 3) minsnap_layer_kernel(
    const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows, const int64_t *__restrict__ seg_offsets, int B, int m, double dt,
    const int64_t *__restrict__ group_offsets, const int32_t *__restrict__ n_rows, const int32_t *__restrict__ start, double r2, Delta delta,
    int max_steps, int32_t *__restrict__ ilayer, double *__restrict__ offsets, int32_t *__restrict__ flags) {
    __shared__ double tile[kWaves * kRegion];
    __shared__ int granted[kMaxGroup];                       // the layers decided so far, by position in the group
    __shared__ unsigned long long round_hits[2];             // the candidate lanes of a round that met somebody, over all wavefronts; two
                                                             // words taken in turn: a slow reader of one round's is not overtaken by the next clearing
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long a0 = group_offsets ? group_offsets[blockIdx.x] : 0, a1 = group_offsets ? group_offsets[blockIdx.x + 1] : B;
    const int g0 = (int)(a0 < 0 ? 0 : (a0 > B ? B : a0));   // clamped: malformed offsets must not leave the batch
    const int g1 = (int)(a1 < g0 ? g0 : (a1 > B ? B : a1));
    if (g1 == g0) return;
    if (g1 - g0 > kMaxGroup) {                               // cannot be refused by the host: its missions stay "not examined", and flag 0
        if (threadIdx.x == 0) atomicOr(&flags[0], 1);
        return;
    }
    double *mine = tile + w * kRegion;                       // this wavefront's quarter of the tile
    const size_t Bs = (size_t)B;

    int turn = 0;
    int h_prev = 0, earlier = 0;                             // the row past which every decided mission holds its last row; how many there are
    for (int i = g0; i < g1; ++i) {                          // (uniform: every thread walks the same missions and takes the same decisions)
        const int ni = __builtin_amdgcn_readfirstlane(n_rows[i]), si = __builtin_amdgcn_readfirstlane(start[i]);
        if (ni == 0) {                                       // excluded: nobody is checked against it (its record is the pre-pass's)
            if (threadIdx.x == 0) granted[i - g0] = 0;
            continue;
        }
        int layer = 0, steps = earlier > 0 ? -1 : 0;         // the first included mission of a group is never moved
        if (earlier > 0) {
            const Mission Mi = mission_of(seg_offsets, i, m);
            const int32_t *irows = seg_rows + Mi.s0;
            const double *icm = coeffs + (size_t)Mi.s0 * 24;
            const int n_tiles = (i - g0 + kTile - 1) / kTile;
            const int H = max(h_prev, si + ni);              // past it everybody holds a last row, on whatever layer
            for (int q0 = 0; q0 <= max_steps && steps < 0; q0 += kTile) {
                const int n_live = min(kTile, max_steps - q0 + 1);                    // candidates of this round (the lanes past them shadow the last)
                const unsigned long long live = n_live == kTile ? ~0ull : (1ull << n_live) - 1ull;
                const int ql = q0 + min(lane, n_live - 1);                            // this lane's layer
                unsigned long long &round_hit = round_hits[turn ^= 1];
                if (threadIdx.x == 0) round_hit = 0;
                __syncthreads();                             // (also: `granted` of the previous mission is visible from here)
                bool hit = false;
                unsigned long long told = 0;                 // what this wavefront has put into round_hit
                for (int t = 0; t < n_tiles; ++t) {
                    const int j0 = g0 + t * kTile;
                    const int n_val = min(kTile, i - j0);    // partners of this tile: the missions before i
                    const int n_pad = (n_val + kUnroll - 1) / kUnroll * kUnroll;
                    const bool jvalid = lane < n_val;
                    const int jb = jvalid ? j0 + lane : j0;
                    const Mission Mj = mission_of(seg_offsets, jb, m);
                    const int32_t *jrows = seg_rows + Mj.s0;
                    const double *jcm = coeffs + (size_t)Mj.s0 * 24;
                    const int nj = jvalid ? n_rows[jb] : 0, sj = start[jb], lj = granted[jb - g0];
                    int js = 0, jbase = 0, jcnt = jrows[0];
                    int is = 0, ibase = 0, icnt = irows[0];
                    for (int k0 = w * kRows; k0 < H; k0 += kChunk) {
                        const bool over = (__hip_atomic_load(&round_hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & live) == live;
                        if (__builtin_amdgcn_readfirstlane((int)over)) break;       // no candidate of this round can be clear any more
                        {                                    // the j-tile's positions at this wavefront's rows of the chunk
                            double cj[24];
                            seek(jrows, Mj.m, min(max(k0 - sj, 0), nj - 1), js, jbase, jcnt);
                            int jloaded = js;
#pragma unroll
                            for (int q = 0; q < 24; ++q) cj[q] = jcm[js * 24 + q];
                            cj[0] = layer_c0(cj[0], lj, delta.x); cj[1] = layer_c0(cj[1], lj, delta.y); cj[2] = layer_c0(cj[2], lj, delta.z);
#pragma nounroll
                            for (int r = 0; r < kRows && k0 + r < H; ++r) {
                                const int row = min(max(k0 + r - sj, 0), nj - 1);
                                seek(jrows, Mj.m, row, js, jbase, jcnt);
                                if (js != jloaded) {
#pragma unroll
                                    for (int q = 0; q < 24; ++q) cj[q] = jcm[js * 24 + q];
                                    cj[0] = layer_c0(cj[0], lj, delta.x); cj[1] = layer_c0(cj[1], lj, delta.y);
                                    cj[2] = layer_c0(cj[2], lj, delta.z);
                                    jloaded = js;
                                }
                                double x, y, z;
                                minsnap_eval_pos<1>(cj, (double)(int)(row - jbase) * dt, x, y, z);
                                double *o = mine + (r * kTile + lane) * 3;
                                o[0] = nj > 0 ? x : nan; o[1] = nj > 0 ? y : nan; o[2] = nj > 0 ? z : nan;
                            }
                        }
                        lds_wave_fence();                    // (a wavefront reads only its own quarter)
                        double c[24];                        // the mission's own segment (the same for every lane), c0 on the lane's layer
                        seek(irows, Mi.m, min(max(k0 - si, 0), ni - 1), is, ibase, icnt);
                        int iloaded = is;
#pragma unroll
                        for (int q = 0; q < 24; ++q) c[q] = icm[is * 24 + q];
                        c[0] = layer_c0(c[0], ql, delta.x); c[1] = layer_c0(c[1], ql, delta.y); c[2] = layer_c0(c[2], ql, delta.z);
#pragma nounroll
                        for (int r = 0; r < kRows && k0 + r < H; ++r) {
                            const int row = min(max(k0 + r - si, 0), ni - 1);
                            seek(irows, Mi.m, row, is, ibase, icnt);
                            if (is != iloaded) {
#pragma unroll
                                for (int q = 0; q < 24; ++q) c[q] = icm[is * 24 + q];
                                c[0] = layer_c0(c[0], ql, delta.x); c[1] = layer_c0(c[1], ql, delta.y); c[2] = layer_c0(c[2], ql, delta.z);
                                iloaded = is;
                            }
                            double xi, yi, zi;
                            minsnap_eval_pos<1>(c, (double)(int)(row - ibase) * dt, xi, yi, zi);
                            hit |= inside_row(mine + r * kTile * 3, n_pad, xi, yi, zi, r2);
                        }
                        lds_wave_fence();
                        const unsigned long long now = __ballot(hit);
                        if (now != told) {
                            if (lane == 0) __hip_atomic_fetch_or(&round_hit, now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            told = now;
                        }
                    }
                }
                __syncthreads();                             // (every wavefront has put in what it found: after each chunk)
                const unsigned long long clear = ~round_hit & live;
                if (clear) {                                 // the lowest clear candidate
                    steps = q0 + __builtin_ctzll(clear);
                    layer = steps;
                }
            }
        }
        if (threadIdx.x == 0) {
            granted[i - g0] = layer;
            ilayer[i] = layer; ilayer[Bs + i] = steps; ilayer[2 * Bs + i] = earlier;
            double *o = offsets + 3 * (size_t)i;
            o[0] = layer_offset(layer, delta.x); o[1] = layer_offset(layer, delta.y); o[2] = layer_offset(layer, delta.z);
        }
        h_prev = max(h_prev, si + ni);
        ++earlier;
    }
}

// ------------------------------------------------------------------------------------------------------------------ the transform
struct alignas(8) Pair {                                    // 16 bytes that need the alignment of a double only
    double a, b;
};

// the mission of segment s of a ragged batch: the last b with seg_offsets[b] <= s, kept inside 0 .. B - 1 whatever the offsets hold
__device__ __forceinline__ int mission_of_segment(const int64_t *__restrict__ so, int B, long long s) {
    int lo = 0, hi = B;                                      // so[lo] <= s < so[hi] for well-formed offsets
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (so[mid] <= s) lo = mid; else hi = mid;
    }
    return lo;
}

// (coeffs and out may be the same buffer: every thread reads and writes its own 16 bytes)
__global__ void __launch_bounds__(256) minsnap_shift_kernel(const double *coeffs, const int64_t *__restrict__ seg_offsets, int B, int m,
                                                            long long n_segments, const double *__restrict__ offsets, double *out) {
#pragma clang fp contract(off)
    const long long n = n_segments * kPairs;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const long long s = e / kPairs;
        const int q = (int)(e - s * kPairs);
        Pair v = reinterpret_cast<const Pair *>(coeffs + s * 24)[q];
        if (q < 2) {                                         // c0 = (x, y, z): piece 0 and the first half of piece 1
            const int b = seg_offsets ? mission_of_segment(seg_offsets, B, s) : (int)(s / m);
            const double *o = offsets + 3 * (size_t)b;
            const double ox = o[0], oy = o[1], oz = o[2];
            if (!(ox == 0.0 && oy == 0.0 && oz == 0.0)) {    // a mission that is not moved is copied bit for bit (-0.0 stays -0.0)
                if (q == 0) { v.a = v.a + ox; v.b = v.b + oy; }
                else v.a = v.a + oz;
            }
        }
        reinterpret_cast<Pair *>(out + s * 24)[q] = v;
    }
}

}  // namespace

int uavac_launch_layer(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                       const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, double delta_x, double delta_y,
                       double delta_z, int max_steps, int32_t *ilayer, double *offsets) {
    const size_t Bs = (size_t)B;
    if (int rc = uavac_arena_reserve(ctx, 2 * uavac_arena_size(Bs * 4))) return rc;
    int32_t *n_rows = static_cast<int32_t *>(uavac_arena_take(ctx, Bs * 4)), *start = static_cast<int32_t *>(uavac_arena_take(ctx, Bs * 4));
    if (!n_rows || !start) return uavac_fail(ctx, UAVAC_ENOMEM, "layer: scratch arena too small");
    const Delta delta{delta_x, delta_y, delta_z};
    const int per_wg = kWaves * (64 / kPreLanes);
    hipLaunchKernelGGL(layer_prepass_kernel, dim3((B + per_wg - 1) / per_wg), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows, seg_offsets, B, m,
                       start_rows, delta, n_rows, start, ilayer, offsets, ctx->d_flags);
    hipLaunchKernelGGL(minsnap_layer_kernel, dim3(group_offsets ? G : 1), dim3(kThreads), 0, ctx->stream, coeffs, seg_rows, seg_offsets, B, m, dt,
                       group_offsets, n_rows, start, radius * radius, delta, max_steps, ilayer, offsets, ctx->d_flags);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}

int uavac_launch_shift(uavac_ctx *ctx, const double *coeffs, const int64_t *seg_offsets, int B, int m, int64_t total_segments,
                       const double *offsets, double *out_coeffs) {
    const long long n_segments = seg_offsets ? (long long)total_segments : (long long)B * m;
    const long long wanted = (n_segments * kPairs + 255) / 256;
    const int grid = (int)(wanted < 1 << 16 ? wanted : 1 << 16);        // (grid-stride past that)
    hipLaunchKernelGGL(minsnap_shift_kernel, dim3(grid), dim3(256), 0, ctx->stream, coeffs, seg_offsets, B, m, n_segments, offsets, out_coeffs);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}
