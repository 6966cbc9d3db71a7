// A fleet split into INDEPENDENT AIRSPACES (gfx950): the connected components of the graph "the swept boxes of two missions of a group
// are nearer than the radius on every axis", labelled by their lowest batch index.  Two missions in different components can never be
// inside the radius of each other (minsnap_envelope.hip says why), a mission's greedy decision in the prioritised searches
// (minsnap_stagger.hip, minsnap_layer.hip) depends only on earlier missions that can meet it, and those are all in its component: the
// searches run per component give every mission the answer of the search over the whole group.  The contract is in include/uavac.h
// (uavac_fleet_airspaces_dev); uav_ac.scoring.airspaces_from_envelopes states it in NumPy, round for round.
//
// One ROUND is two kernels, double-buffered through ctx scratch so that it is reproducible:
//   airspace_link_kernel   m[i] = min(lab[i], min of lab[j] over the linked j).  One lane per mission, 64 missions per workgroup; they walk
//                          the boxes and labels of every group they belong to through LDS tiles of 256 missions (six doubles and a
//                          label each, 13 KB), as fleet_order_kernel streams its keys: every read of the inner loop is a broadcast.
//                          The workgroup's four wavefronts hold the same 64 missions and take every fourth partner of a tile each
//                          -- a group of 4 096 is then 64 workgroups instead of 16 --; their minima meet in LDS, and a minimum
//                          does not care how it was split.  The cost of a round is the sum of g^2 box tests over the groups.
//   airspace_jump_kernel   lab'[i] = m[m[i]] -- the pointer jump, without which a chain of n boxes whose labels descend along it takes
//                          n rounds --, written over lab[i] (every thread reads m, which this round's link kernel finished, and
//                          writes its own label), and the round's word `changed` when lab'[i] != lab[i].
// A round whose predecessor changed nothing exits at once (both kernels read the predecessor's word first): no workgroup waits for
// another, there is no grid-wide barrier and no spin.  airspace_begin_kernel clears the words (and sets lab[i] = i unless the call
// resumes), airspace_info_kernel counts them.  All on the ctx stream; nothing is read back.
//
// THE LINK: on all three axes fl(lo_i - hi_j) < radius and fl(lo_j - hi_i) < radius -- plain rounded subtractions, nothing to
// contract --, strictly: a gap of exactly the radius is no link, and a NaN fails every comparison, so a NaN box links to nobody.
// Labels only ever go down, towards the lowest index of the component, and the labels at the fixed point are unique: the result
// does not depend on the launch shape.

#include "uavac_internal.h"
#include "uavac_scratch.h"
#include "fleet_clock.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMissions = 64;                               // missions per workgroup of the link kernel: one per lane, and its
constexpr int kSlices = kThreads / kMissions;               // four wavefronts take every fourth partner of a tile each

// (the group that holds mission b, as fleet_order_kernel finds it: the last group whose first mission is not past b, if b is below
// that group's end; ranges are group_range's, clamped to the batch)
__device__ __forceinline__ bool group_of(const int64_t *__restrict__ group_offsets, int G, int B, int b, int &g0, int &g1) {
    int g = 0;
    if (group_offsets) {
        int lo = 0, hi = G - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (group_offsets[mid] <= b) lo = mid; else hi = mid - 1;
        }
        g = lo;
    }
    fleet::group_range(group_offsets, g, B, g0, g1);
    return b >= g0 && b < g1;
}

// a label as an index into [B]: a resumed call's labels are the caller's and may hold anything
__device__ __forceinline__ int as_index(int v, int B) { return v < 0 ? 0 : (v >= B ? B - 1 : v); }

struct alignas(16) Box {                                    // lo x y z, hi x y z: 48 bytes, three 16-byte LDS reads
    double v[6];
};

__global__ void __launch_bounds__(kThreads) airspace_begin_kernel(int B, int rounds, int resume, int32_t *__restrict__ labels,
                                                                  int32_t *__restrict__ changed) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < B && !resume) labels[i] = i;
    if (i < rounds) changed[i] = 0;
}

__global__ void __launch_bounds__(kThreads) airspace_link_kernel(const double *__restrict__ env, const int64_t *__restrict__ group_offsets,
                                                                 int G, int B, double radius, const int32_t *__restrict__ labels,
                                                                 const int32_t *__restrict__ before, int32_t *__restrict__ least) {
    __shared__ Box box[kThreads];
    __shared__ int lab[kThreads];
    __shared__ int part[kSlices][kMissions];                 // every wavefront's minimum per mission
    __shared__ int span[2];                                  // the missions that this workgroup's groups cover: [span[0], span[1])
    if (before && *before == 0) return;                      // the round before changed nothing: the labels are final (uniform)
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x * kMissions + lane;             // (the same mission in lane `lane` of all four wavefronts)
    if (threadIdx.x == 0) { span[0] = B; span[1] = 0; }
    __syncthreads();
    int g0 = 0, g1 = 0, mine = 0;
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    if (b < B) {
        mine = as_index(labels[b], B);
        if (group_of(group_offsets, G, B, b, g0, g1)) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = env[6 * (size_t)b + a]; hi[a] = env[6 * (size_t)b + 3 + a]; }
            if (w == 0) {
                atomicMin(&span[0], g0);
                atomicMax(&span[1], g1);
            }
        } else {
            g0 = g1 = 0;                                     // no group holds it: linked to nobody
        }
    }
    __syncthreads();
    const int first = span[0], last = span[1];               // (uniform)
    for (int t0 = first; t0 < last; t0 += kThreads) {
        const int j = t0 + threadIdx.x;
        if (j < last) {
#pragma unroll
            for (int k = 0; k < 6; ++k) box[threadIdx.x].v[k] = env[6 * (size_t)j + k];
            lab[threadIdx.x] = as_index(labels[j], B);
        }
        __syncthreads();
        const int n = min(kThreads, last - t0);              // (uniform: the trip count is the wavefront's, the group a predicate)
#pragma unroll 4
        for (int k = w; k < n; k += kSlices) {               // this wavefront's partners of the tile
            const int jj = t0 + k;
            const Box x = box[k];                            // (the same address in every lane: broadcasts)
            const bool linked = lo[0] - x.v[3] < radius && x.v[0] - hi[0] < radius && lo[1] - x.v[4] < radius &&
                                x.v[1] - hi[1] < radius && lo[2] - x.v[5] < radius && x.v[2] - hi[2] < radius;
            if (linked && jj >= g0 && jj < g1 && jj != b) mine = min(mine, lab[k]);
        }
        __syncthreads();
    }
    part[w][lane] = mine;
    __syncthreads();
    if (w == 0 && b < B) {
#pragma unroll
        for (int v = 1; v < kSlices; ++v) mine = min(mine, part[v][lane]);             // (a minimum: exact whatever the split)
        least[b] = mine;
    }
}

__global__ void __launch_bounds__(kThreads) airspace_jump_kernel(int B, const int32_t *__restrict__ least, const int32_t *__restrict__ before,
                                                                 int32_t *__restrict__ labels, int32_t *__restrict__ changed) {
    if (before && *before == 0) return;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= B) return;
    const int next = least[least[i]];                        // (least holds indices: as_index went over every label it was made from)
    if (next != labels[i]) {
        labels[i] = next;
        *changed = 1;                                        // (every writer writes the same word with the same value)
    }
}

// info[0] = the rounds that changed a label; info[1] = 1 iff the last round that ran changed nothing.  The rounds run up to and with
// the first one that changed nothing, so both follow from the first clear word.
__global__ void airspace_info_kernel(int rounds, const int32_t *__restrict__ changed, int32_t *__restrict__ info) {
    int r = 0;
    while (r < rounds && changed[r] != 0) ++r;
    info[0] = r;
    info[1] = r < rounds ? 1 : 0;
}

}  // namespace

int uavac_launch_fleet_airspaces(uavac_ctx *ctx, const double *env, const int64_t *group_offsets, int G, int B, double radius, int rounds,
                                 int resume, int32_t *labels, int32_t *info) {
    // after B rounds that changed a label nothing is left to change (a label is an index and only goes down towards the lowest of
    // its component, a hop per round at least): more rounds than that would all exit at once
    if (rounds > B + 1) rounds = B + 1;
    int32_t *least = nullptr, *changed = nullptr;
    Scratch s(ctx);
    s.want(&least, (size_t)B);
    s.want(&changed, (size_t)rounds);
    if (int rc = s.commit()) return rc;
    const dim3 grid((B + kThreads - 1) / kThreads), block(kThreads);
    const int first = (B > rounds ? B : rounds);
    hipLaunchKernelGGL(airspace_begin_kernel, dim3((first + kThreads - 1) / kThreads), block, 0, ctx->stream, B, rounds, resume, labels, changed);
    for (int r = 0; r < rounds; ++r) {
        const int32_t *before = r ? changed + r - 1 : nullptr;
        hipLaunchKernelGGL(airspace_link_kernel, dim3((B + kMissions - 1) / kMissions), block, 0, ctx->stream, env, group_offsets, G, B, radius, labels, before, least);
        hipLaunchKernelGGL(airspace_jump_kernel, grid, block, 0, ctx->stream, B, least, before, labels, changed + r);
    }
    hipLaunchKernelGGL(airspace_info_kernel, dim3(1), dim3(1), 0, ctx->stream, rounds, changed, info);
    UAVAC_HIP(ctx, hipGetLastError());
    return UAVAC_OK;
}
