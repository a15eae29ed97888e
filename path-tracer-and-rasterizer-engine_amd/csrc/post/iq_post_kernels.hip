// iq_post_kernels.hip — the one kernel the post-process stages share, for gfx950 (wave64), lane = pixel: the BGRA8
// encoding of a float4 plane, which the denoiser and the variance-guided filter run at levels = 0.
#include <hip/hip_runtime.h>

#include "post/iq_post.hpp"
#include "post/iq_post_device.hpp"

namespace iqp {

namespace {

// 16 bytes in, 4 out per lane.
__global__ void __launch_bounds__(kBlockX* kBlockY) iqp_encode_kernel(uint32_t width, uint32_t height,
                                                                      const float4* __restrict__ in,
                                                                      uint32_t* __restrict__ bgra) {
    const uint32_t px = blockIdx.x * kBlockX + threadIdx.x, py = blockIdx.y * kBlockY + threadIdx.y;
    if (px >= width || py >= height) return;
    const size_t pix = (size_t)py * width + px;
    bgra[pix] = encode(in[pix]);
}

}  // namespace

hipError_t launch_encode(hipStream_t s, uint32_t width, uint32_t height, const void* in, uint32_t* bgra) {
    iqp_encode_kernel<<<grid(width, height), dim3(kBlockX, kBlockY), 0, s>>>(width, height, static_cast<const float4*>(in), bgra);
    return hipGetLastError();
}

}  // namespace iqp
