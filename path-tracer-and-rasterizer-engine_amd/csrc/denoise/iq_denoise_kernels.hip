// iq_denoise_kernels.hip — the denoiser's kernels for gfx950 (wave64): one edge-avoiding à-trous level per
// launch, lane = pixel; the last one also encodes the result as BGRA8. The tap and the encoding are
// post/iq_post_device.hpp's. DESIGN.md §10 is the filter these restate; every float operation below is written
// in that section's order and compiled with -ffp-contract=off and correctly rounded division and square root.
#include <hip/hip_runtime.h>

#include "denoise/iq_denoise.hpp"
#include "post/iq_post_device.hpp"

namespace iqd {

using namespace iqp;

namespace {

// One level, direct global loads: 25 taps of 36 bytes (colour, normal and depth, id), each tap of a wave two
// contiguous row segments. Pixels without a guide or with a non-finite colour are copied; a wave whose lanes
// are all such pixels skips the tap loop (the branch is then wave-uniform), which is what a frame's sky costs.
template <bool kEncode>
__global__ void __launch_bounds__(kBlockX* kBlockY) iqd_level_kernel(level_params p, const float4* __restrict__ in,
                                                                     const float4* __restrict__ normal_z,
                                                                     const uint32_t* __restrict__ id,
                                                                     float4* __restrict__ out,
                                                                     uint32_t* __restrict__ bgra) {
    const int px = (int)(blockIdx.x * kBlockX + threadIdx.x), py = (int)(blockIdx.y * kBlockY + threadIdx.y);
    if (px >= (int)p.width || py >= (int)p.height) return;
    const size_t pix = (size_t)py * p.width + (size_t)px;
    const float4 cp = in[pix];
    const uint32_t idp = id[pix];
    float4 res = cp;
    if (idp != kNoPrim && finite3(cp)) {
        const float4 np = normal_z[pix];
        const atrous_planes g = {p.width, p.height, in, normal_z, id};
        const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
        float nx = 0.0f, ny = 0.0f, nz = 0.0f, den = 0.0f;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const float hw = h[dy + 2] * h[dx + 2];
                if (dy == 0 && dx == 0) {
                    nx = nx + hw * cp.x;
                    ny = ny + hw * cp.y;
                    nz = nz + hw * cp.z;
                    den = den + hw;
                    continue;
                }
                size_t q;
                float4 cq;
                float w;
                if (!tap_colour(g, px + dx * p.step, py + dy * p.step, idp, q, cq)) continue;
                if (!tap_weight(g, q, cq, cp, np, hw, p.squarings, p.depth_sharpness, p.colour_scale, w)) continue;
                nx = nx + w * cq.x;
                ny = ny + w * cq.y;
                nz = nz + w * cq.z;
                den = den + w;
            }
        }
        res = make_float4(nx / den, ny / den, nz / den, 0.0f);
    }
    out[pix] = res;
    if (kEncode) bgra[pix] = encode(res);
}

}  // namespace

hipError_t launch_level(hipStream_t s, const level_params& p, const void* in, const void* normal_z, const uint32_t* id,
                        void* out, uint32_t* bgra) {
    const dim3 g = grid(p.width, p.height), b(kBlockX, kBlockY);
    if (bgra)
        iqd_level_kernel<true><<<g, b, 0, s>>>(p, static_cast<const float4*>(in), static_cast<const float4*>(normal_z), id,
                                               static_cast<float4*>(out), bgra);
    else
        iqd_level_kernel<false><<<g, b, 0, s>>>(p, static_cast<const float4*>(in), static_cast<const float4*>(normal_z), id,
                                                static_cast<float4*>(out), nullptr);
    return hipGetLastError();
}

}  // namespace iqd
