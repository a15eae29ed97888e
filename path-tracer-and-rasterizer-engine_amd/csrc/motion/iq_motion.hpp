// iq_motion.hpp — what the motion runtime (iq_motion.cpp) and its kernels (iq_motion_kernels.hip) share. The view's
// parameters and planes are temporal reprojection's (temporal/iq_temporal.hpp); what these implement is DESIGN.md §15.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "motion/iqpt_motion.h"
#include "temporal/iq_temporal.hpp"

namespace iqm {

// launchers (iq_motion_kernels.hip); each enqueues on `s` and returns the launch status.
// Steps 1 and 2 of §15.1: cur.pos and hist of cur.normal_z / cur.id, gathered from prev and out through `table`
// (device, n entries; n == 0: §11's step 2 for every pixel and the table is not read).
hipError_t launch_view(hipStream_t s, const iqt::view_params& p, const iqt::view_planes& cur, const iqt::view_planes& prev,
                       const void* out, void* hist, const iqpt_motion_entry* table, uint32_t n);
// counts[0] += pixels with id != NO_PRIM, [1] += those with hist.w > 0, [2] += pixels with id < n whose entry has
// moved == 1, [3] += those of [2] with hist.w > 0 (counts zeroed by the caller).
hipError_t launch_stats(hipStream_t s, uint32_t npix, const uint32_t* id, const void* hist, const iqpt_motion_entry* table,
                        uint32_t n, unsigned long long* counts);

}  // namespace iqm
