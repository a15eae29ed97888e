// iq_temporal.hpp — types shared by the temporal runtime (iq_temporal.cpp) and its kernels
// (iq_temporal_kernels.hip). What these implement is DESIGN.md §11.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

struct iqpt_temporal_params;

namespace iqt {

// IQPT_OK, or the status of the first field out of range with its message as the last error (iq_temporal.cpp);
// the variance-guided filter checks the same three fields of its own parameters with it.
int check_params(const iqpt_temporal_params& p);

// Kernel arguments of one begin_view: wave-uniform, so the 64 matrix words are read through the scalar cache.
struct view_params {
    uint32_t width, height;
    uint32_t have_prev;          // 0: no previous view or no result, the history is +0 everywhere
    float normal_min, plane_tolerance, max_history;
    float inv_proj[16], inv_view[16];      // of the new view
    float view_prev[16], proj_prev[16];    // of the previous one
};

// The planes of one view, each width*height entries; two sets swap at every begin_view.
struct view_planes {
    void* normal_z;     // float4 (n, z)
    uint32_t* id;
    void* pos;          // float4 world position
};

// launchers (iq_temporal_kernels.hip); each enqueues on `s` and returns the launch status.
// Steps 1 and 2 of §11: cur.pos and hist of cur.normal_z / cur.id, gathered from prev and out.
hipError_t launch_view(hipStream_t s, const view_params& p, const view_planes& cur, const view_planes& prev,
                       const void* out, void* hist);
// The blend of hist and colour (nf samples, 0 <= nf <= 2^24) into out and its BGRA8 encoding.
hipError_t launch_resolve(hipStream_t s, uint32_t width, uint32_t height, float nf, const void* hist, const void* colour,
                          void* out, uint32_t* bgra);
// counts[0] += pixels with id != NO_PRIM, counts[1] += those with hist.w > 0 (counts zeroed by the caller).
hipError_t launch_stats(hipStream_t s, uint32_t npix, const uint32_t* id, const void* hist, unsigned long long* counts);

}  // namespace iqt
