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
// The pre-pass and the decision kernel are templates (minsnap_layer_search.h) that the obstacle-aware search shares: this file
// instantiates them without cuboids and holds the transform.

#include "minsnap_layer_search.h"

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
