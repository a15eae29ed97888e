// iq_denoise.hpp — types shared by the denoiser's runtime (iq_denoise.cpp) and its kernels
// (iq_denoise_kernels.hip). The filter these implement is DESIGN.md §10.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace iqd {

struct level_params {
    uint32_t width, height;
    int32_t step;             // 2^i
    uint32_t squarings;       // q
    float depth_sharpness;    // s_z
    float colour_scale;       // k_i = RN(s_c s_c) 4^i
};

// launcher (iq_denoise_kernels.hip); enqueues on `s` and returns the launch status. levels = 0 is
// iqp::launch_encode alone.
// One à-trous level: out = c_{i+1} of in = c_i under the guides; bgra (may be NULL) also gets the encoded frame.
hipError_t launch_level(hipStream_t s, const level_params& p, const void* in, const void* normal_z, const uint32_t* id,
                        void* out, uint32_t* bgra);

}  // namespace iqd
