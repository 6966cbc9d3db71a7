// Fleet deconfliction by offset layers (gfx950), and the offset as a plan transform.  Where uavac_minsnap_stagger_dev makes a mission
// WAIT, this call MOVES it: within a group the missions are taken in ascending batch index -- the priority --, the starts are FIXED,
// and each mission gets the lowest layer q = 0 .. max_steps -- the mission with the offset fl(q * delta) added to c0 of every one of
// its segments -- that keeps it outside the protection radius of every mission decided before it, over the whole shared clock.  From
// coefficients and row counts alone: no row is written, nothing is read back.  The contract -- the clock, the groups, the excluded
// missions and the rounding are the audit's and stagger's -- is in include/uavac.h (uavac_minsnap_layer_dev, uavac_minsnap_shift_dev);
// uav_ac.scoring.layer_from_rows states the search in NumPy on sampled rows, uav_ac.scoring.shift_coeffs the transform.
//
// Three kernels, all on the ctx stream:
//   layer_prepass_kernel   per mission: fleet_clock.h's pre-pass -- row total N (0: EXCLUDED), start clamped to 0 .. 2^29, in ctx scratch
//                          -- and the record of a mission that is never examined -- layer 0 / -2 / 0 and the offset of layer 0 --
//                          which the decision kernel overwrites for everybody it decides (fleet_search.h: two object files need it)
//   minsnap_layer_kernel   the decisions: fleet_search.h's search with the Layer policy.  THE 64 LANES ARE 64 CANDIDATE LAYERS of one
//                          mission, lane l stands on layer q0 + l, the partners ON THEIR GRANTED LAYERS.  All 64 candidates share the
//                          start, hence the clock row, the segment and t: only c0 differs between the lanes (the walk's after-load
//                          hook, layer_c0), and of the Horner chain only the last fma per axis sees it.  A mission that is not
//                          resolved stays on layer 0.
//   minsnap_shift_kernel   the transform: out = coeffs with offsets[b] added to c0 of every segment of mission b.  One thread per 16
//                          bytes of the coefficients, twelve per segment; c0 = (x, y, z) is piece 0 and the first half of piece 1.
//
// ROUNDING (part of the contract).  The offset of layer q on axis a is o = fl((double)q * delta_a), the candidate's coefficient
// c0' = fl(c0 + o): two roundings, never one fma; layer 0 is the mission as it is (nothing is added).  Positions by the sampler's fma
// chain on those coefficients (minsnap_eval_pos), the distance WITHOUT contraction: d^2 = (dx dx + dy dy) + dz dz.
// This file instantiates the search without cuboids and holds the transform.

#include "fleet_search.h"

namespace {

constexpr int kPairs = 12;                                  // 16-byte pieces of a segment's 24 coefficients

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
    return launch_layer_search<false>(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, start_rows, radius,
                                      Delta{delta_x, delta_y, delta_z}, max_steps, nullptr, 0, ilayer, offsets);
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
