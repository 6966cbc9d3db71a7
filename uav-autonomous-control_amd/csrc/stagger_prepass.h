// The pre-pass of the deconfliction by start delay (gfx950), for the two object files that launch it: minsnap_stagger.o and
// minsnap_stagger_wide.o (a header of its own: fleet_search.h is also the layers', whose objects must not get this kernel).
#pragma once

#include "fleet_clock.h"

namespace {

// (fleet_clock.h) and the record of a mission that is never examined -- base start / -2 / 0 -- in istag, which the decision kernel
// overwrites for everybody it decides
__global__ void __launch_bounds__(fleet::kThreads) stagger_prepass_kernel(const double *__restrict__ coeffs, const int32_t *__restrict__ seg_rows,
                                                                          const int64_t *__restrict__ seg_offsets, int B, int m,
                                                                          const int32_t *__restrict__ start_rows, int32_t *__restrict__ n_rows,
                                                                          int32_t *__restrict__ start, int32_t *__restrict__ istag,
                                                                          int32_t *__restrict__ flags) {
    int b, s;
    if (!fleet::prepass_mission(coeffs, seg_rows, seg_offsets, B, m, start_rows, n_rows, start, flags, b, s)) return;
    istag[b] = s; istag[(size_t)B + b] = -2; istag[2 * (size_t)B + b] = 0;
}

}  // namespace
