// iq_post_device.hpp — what the kernels of the post-process stages (denoise/, temporal/, svgf/) share: the block
// they all launch with, the finite tests, the BGRA8 encoding (normative) and the edge-avoiding
// à-trous tap (§10.1 and §12.1, normative). Every float operation is written in those sections' order and compiled
// with -ffp-contract=off and correctly rounded division and square root.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "raster/iq_raster.hpp"

namespace iqp {

using iqr::kNoPrim;           // the id plane's "no guide here" is the rasterizer's

constexpr int kBlockX = 32;   // lanes run along x: every plane access of a wave is two coalesced row segments
constexpr int kBlockY = 8;

inline dim3 grid(uint32_t width, uint32_t height) {
    return dim3((width + kBlockX - 1) / kBlockX, (height + kBlockY - 1) / kBlockY);
}

// the blocks of grid(width, height)
inline size_t num_blocks(uint32_t width, uint32_t height) {
    return (size_t)((width + kBlockX - 1) / kBlockX) * ((height + kBlockY - 1) / kBlockY);
}

__device__ inline bool finite1(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }

// written out, not as three finite1 calls: the compiler then merges the tests with the one before them at every
// use, and a colour fetched for them is fetched whole
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

// The colour plane and the guides one à-trous level reads.
struct atrous_planes {
    uint32_t width, height;
    const float4* in;
    const float4* normal_z;
    const uint32_t* id;
};

// The pixel (qx, qy) as a tap of a pixel whose id is idp: false where it is off the frame, has another id or a
// colour that is not finite; else q is its index and cq its colour. The id is read first and the colour only
// under it, so a tap across an edge costs 4 bytes.
__device__ __forceinline__ bool tap_colour(const atrous_planes& g, int qx, int qy, uint32_t idp, size_t& q, float4& cq) {
    if (qx < 0 || qy < 0 || qx >= (int)g.width || qy >= (int)g.height) return false;
    q = (size_t)qy * g.width + (size_t)qx;
    if (g.id[q] != idp) return false;
    cq = g.in[q];
    const float4 c = cq;      // the test on a copy: the compiler then keeps the 16 bytes one load
    return finite3(c);
}

// The weight of tap q (colour cq, kernel weight hw) for the pixel with colour cp and guide np:
// (hw d) / ((1 + t t)(1 + d2 colour_scale)), d the clamped normal dot product squared `squarings` times, t the
// depth difference times depth_sharpness, d2 the squared colour distance. false where !(w > 0): a NaN weight
// fails too.
__device__ __forceinline__ bool tap_weight(const atrous_planes& g, size_t q, const float4& cq, const float4& cp,
                                           const float4& np, float hw, uint32_t squarings, float depth_sharpness,
                                           float colour_scale, float& w) {
    const float4 nq = g.normal_z[q];
    float d = fmaxf(np.x * nq.x + np.y * nq.y + np.z * nq.z, 0.0f);
    for (uint32_t k = 0; k < squarings; ++k) d = d * d;
    const float t = (np.w - nq.w) * depth_sharpness;
    const float ex = cp.x - cq.x, ey = cp.y - cq.y, ez = cp.z - cq.z;
    const float d2 = ex * ex + ey * ey + ez * ez;
    w = (hw * d) / ((1.0f + t * t) * (1.0f + d2 * colour_scale));
    return w > 0.0f;
}

}  // namespace iqp
