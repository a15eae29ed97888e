// iq_svgf.hpp — types shared by the variance-guided filter's runtime (iq_svgf.cpp) and its kernels
// (iq_svgf_kernels.hip). What these implement is DESIGN.md §12.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "post/iq_post_device.hpp"

namespace iqs {

using iqp::kBlockX;
using iqp::kBlockY;
constexpr int kHalo = 3;      // the spatial estimate's window is 7 x 7
constexpr int kTileW = kBlockX + 2 * kHalo, kTileH = kBlockY + 2 * kHalo;   // 38 x 14 entries staged in LDS

struct variance_params {
    uint32_t width, height;
    float ne;                 // fmax(F(min(n, 2^24)), 1)
    float min_weight;         // F(min_history) * ne: the history length the temporal estimate needs
};

struct level_params {
    uint32_t width, height;
    int step;                 // 2^i
    uint32_t squarings;
    float depth_sharpness;
    float sigma2;             // RN(sigma * sigma)
    float variance_floor;
};

// launchers (iq_svgf_kernels.hip); each enqueues on `s` and returns the launch status.
// M = (L, L L, +0, +0) of npix colours.
hipError_t launch_moments(hipStream_t s, uint32_t npix, const void* colour, void* moments);
// c0 = (o.xyz, v) of the two histories' results; block_spatial[block] = the block's pixels that took the spatial
// estimate, one entry per 32x8 block of the grid, row-major (iqp::num_blocks entries).
hipError_t launch_variance(hipStream_t s, const variance_params& p, const void* o, const void* mu, const uint32_t* id,
                           void* c0, uint32_t* block_spatial);
// One level; bgra != NULL: the last one, which also encodes. levels = 0 is iqp::launch_encode of c0.
hipError_t launch_level(hipStream_t s, const level_params& p, const void* in, const void* normal_z, const uint32_t* id,
                        void* out, uint32_t* bgra);

}  // namespace iqs
