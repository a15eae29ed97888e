// iq_upscale.hpp — types shared by the upscaler's runtime (iq_upscale.cpp) and its kernel
// (iq_upscale_kernels.hip). The definition these implement is DESIGN.md §14.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace iqu {

struct run_params {
    uint32_t width, height;         // the hi frame, W x H
    uint32_t lo_width, lo_height;   // the lo frame, w x h: W = factor w, H = factor h
    uint32_t factor;                // f: 2, 3 or 4
    uint32_t squarings;             // q
    float depth_sharpness;          // s_z
};

// The planes one run reads, all device pointers: the lo colour and both pairs of guides.
struct run_planes {
    const void* colour_lo;          // w h float4
    const void* normal_z_lo;        // w h float4
    const uint32_t* id_lo;          // w h
    const void* normal_z_hi;        // W H float4
    const uint32_t* id_hi;          // W H
};

// launchers (iq_upscale_kernels.hip); each enqueues on `s` and returns the launch status.
// One run: out = W H float4 (w = the class), bgra = W H.
hipError_t launch_upscale(hipStream_t s, const run_params& p, const run_planes& g, void* out, uint32_t* bgra);
// The pixels of each class in a result, added to the three counters, which the caller has cleared on `s` before.
hipError_t launch_stats(hipStream_t s, uint32_t width, uint32_t height, const void* out, unsigned long long* counts);

}  // namespace iqu
