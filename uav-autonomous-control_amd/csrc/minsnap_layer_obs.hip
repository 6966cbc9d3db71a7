// Offset layers that also keep out of cuboids (gfx950): uavac_minsnap_layer_dev's search (minsnap_layer.hip) with one more reason to
// refuse a candidate -- a row of the mission's OWN on that layer lies inside a cuboid.  The contract is in include/uavac.h
// (uavac_minsnap_layer_obs_dev); uav_ac.scoring.layer_obstacles_from_rows states the search in NumPy on sampled rows.
//
// The kernels are the OBS = true instantiations of fleet_search.h (the LayerObs policy); the search is the one copy there.  What it adds to
// the decision kernel, per mission i and round of 64 candidates (the 64 lanes are the layers q0 .. q0 + 63 of mission i):
//   the cuboids    [n][6] in LDS, loaded once per workgroup: a read is one broadcast, the trip count is uniform
//   the blocked    before the round's pair search the four wavefronts split the mission's own rows 0 .. N_i - 1 (they cover its whole
//   mask           clock: before its start it holds row 0, after its end row N_i - 1); every lane evaluates its candidate's position --
//                  the clock walk (fleet_clock.h) with layer_c0(c0, q, delta) as its hook: all lanes share the row, the segment and t, only the last fma per axis
//                  sees c0 -- and tests it against the cuboids with the audit's inclusive comparison.  The bit is therefore what the
//                  sampler writes, and the audit counts, for the plan shifted by q * delta, bit for bit
//   the seed       the waves OR their ballots into a word of their own (`round_blocks`) and into the round's `round_hit`; behind a
//                  barrier the mask is complete.  A refused lane is "hit" before the pair search begins: the early exit (every live
//                  candidate is hit) and the decision (the lowest clear lane) are the search's own, and a refused candidate is never
//                  reported as anything but refused -- `blocked` is counted from the complete mask, never from what the pair search adds
//   blocked        the refused live candidates of the full rounds before the granted one plus the refused lanes below the granted
//                  lane (all of them for an unresolved mission)
//   the first      included mission of a group has nobody to clear: it runs the blocked pass only and gets the lowest layer that no
//   mission        cuboid refuses ("the lowest index is never moved" becomes "is moved only by a cuboid")
// LDS: the search's 50 192 B, 768 B of cuboids and two more words -- three workgroups per CU as before.  Plain C++ and vector stores;
// the only atomic on global memory is the sticky flag.

#include "fleet_search.h"

int uavac_launch_layer_obs(uavac_ctx *ctx, const double *coeffs, const int32_t *seg_rows, const int64_t *seg_offsets, int B, int m, double dt,
                           const int64_t *group_offsets, int G, const int32_t *start_rows, double radius, double delta_x, double delta_y,
                           double delta_z, int max_steps, const double *cuboids, int n_cuboids, int32_t *ilayer, double *offsets) {
    return launch_layer_search<true>(ctx, coeffs, seg_rows, seg_offsets, B, m, dt, group_offsets, G, start_rows, radius,
                                     Delta{delta_x, delta_y, delta_z}, max_steps, cuboids, n_cuboids, ilayer, offsets);
}
