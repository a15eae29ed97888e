// iq_denoise.hpp — types shared by the denoiser's runtime (iq_denoise.cpp) and its kernels
// (iq_denoise_kernels.hip). The filter these implement is DESIGN.md §10.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace iqd {

constexpr int kBlockX = 32;   // lanes run along x: every tap of a wave is two coalesced 512-byte row reads
constexpr int kBlockY = 8;

struct level_params {
    uint32_t width, height;
    int32_t step;             // 2^i
    uint32_t squarings;       // q
    float depth_sharpness;    // s_z
    float colour_scale;       // k_i = RN(s_c s_c) 4^i
};

// launchers (iq_denoise_kernels.hip); each enqueues on `s` and returns the launch status.
// One à-trous level: out = c_{i+1} of in = c_i under the guides; bgra (may be NULL) also gets the encoded frame.
hipError_t launch_level(hipStream_t s, const level_params& p, const void* in, const void* normal_z, const uint32_t* id,
                        void* out, uint32_t* bgra);
// The BGRA8 encoding alone (levels = 0).
hipError_t launch_encode(hipStream_t s, uint32_t width, uint32_t height, const void* in, uint32_t* bgra);

}  // namespace iqd
