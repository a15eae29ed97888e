// iq_denoise_kernels.hip — the denoiser's kernels for gfx950 (wave64): one edge-avoiding à-trous level per
// launch, lane = pixel, and the BGRA8 encoding of the result. DESIGN.md §10 is the filter these restate; every
// float operation below is written in that section's order and compiled with -ffp-contract=off and correctly
// rounded division and square root.
#include <hip/hip_runtime.h>

#include "denoise/iq_denoise.hpp"

namespace iqd {

namespace {

constexpr uint32_t kNoPrim = 0xffffffffu;

__device__ inline bool finite3(const float4& c) {
    return (__float_as_uint(c.x) & 0x7f800000u) != 0x7f800000u && (__float_as_uint(c.y) & 0x7f800000u) != 0x7f800000u &&
           (__float_as_uint(c.z) & 0x7f800000u) != 0x7f800000u;
}

// uint8_t conversion of the path tracer's frame: NaN -> 0, saturate to [0, 255], truncate toward zero
__device__ inline uint32_t to_u8(float f) {
    if (!(f > 0.0f)) return 0u;
    if (f >= 255.0f) return 255u;
    return (uint32_t)f;
}

__device__ inline uint32_t encode(const float4& c) {
    return to_u8(255.0f * sqrtf(c.z)) | to_u8(255.0f * sqrtf(c.y)) << 8 | to_u8(255.0f * sqrtf(c.x)) << 16 | 0xff000000u;
}

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
                const int qx = px + dx * p.step, qy = py + dy * p.step;
                if (qx < 0 || qy < 0 || qx >= (int)p.width || qy >= (int)p.height) continue;
                const size_t q = (size_t)qy * p.width + (size_t)qx;
                if (id[q] != idp) continue;
                const float4 cq = in[q];
                if (!finite3(cq)) continue;
                const float4 nq = normal_z[q];
                float d = fmaxf(np.x * nq.x + np.y * nq.y + np.z * nq.z, 0.0f);
                for (uint32_t k = 0; k < p.squarings; ++k) d = d * d;
                const float t = (np.w - nq.w) * p.depth_sharpness;
                const float ex = cp.x - cq.x, ey = cp.y - cq.y, ez = cp.z - cq.z;
                const float d2 = ex * ex + ey * ey + ez * ez;
                const float w = (hw * d) / ((1.0f + t * t) * (1.0f + d2 * p.colour_scale));
                if (!(w > 0.0f)) continue;      // a NaN weight fails too
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

__global__ void __launch_bounds__(kBlockX* kBlockY) iqd_encode_kernel(uint32_t width, uint32_t height,
                                                                      const float4* __restrict__ in,
                                                                      uint32_t* __restrict__ bgra) {
    const uint32_t px = blockIdx.x * kBlockX + threadIdx.x, py = blockIdx.y * kBlockY + threadIdx.y;
    if (px >= width || py >= height) return;
    const size_t pix = (size_t)py * width + px;
    bgra[pix] = encode(in[pix]);
}

inline dim3 grid(uint32_t width, uint32_t height) {
    return dim3((width + kBlockX - 1) / kBlockX, (height + kBlockY - 1) / kBlockY);
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

hipError_t launch_encode(hipStream_t s, uint32_t width, uint32_t height, const void* in, uint32_t* bgra) {
    iqd_encode_kernel<<<grid(width, height), dim3(kBlockX, kBlockY), 0, s>>>(width, height, static_cast<const float4*>(in), bgra);
    return hipGetLastError();
}

}  // namespace iqd
