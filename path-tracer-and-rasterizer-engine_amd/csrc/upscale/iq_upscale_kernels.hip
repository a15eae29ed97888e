// iq_upscale_kernels.hip — the upscaler's kernel for gfx950 (wave64): joint bilateral upsampling of the lo
// frame's colour to the hi frame, lane = hi pixel; it also encodes the result as BGRA8. A second kernel counts the
// pixels of each class, on request. The tap's tests and the encoding are post/iq_post_device.hpp's. DESIGN.md §14
// is the definition this restates; every float operation below is written in that section's order and compiled
// with -ffp-contract=off and correctly rounded division and square root.
#include <hip/hip_runtime.h>

#include "post/iq_post_device.hpp"
#include "upscale/iq_upscale.hpp"

namespace iqu {

using namespace iqp;

namespace {

// The running sums of one stage: num (three channels) and den, from +0, in tap order.
struct sums {
    float x = 0.0f, y = 0.0f, z = 0.0f, den = 0.0f;
};

// The lo pixel (qx, qy) as a tap of the hi pixel with id idp and guide np, with kernel weight g: it is added
// where it lies in the lo frame, has the same id and a finite colour (tap_colour: the id is read first, the colour
// under it, the normal and depth under both) and its weight is > 0 (a NaN weight fails).
__device__ __forceinline__ void add_tap(const atrous_planes& lo, int qx, int qy, uint32_t idp, const float4& np, float g,
                                        uint32_t squarings, float depth_sharpness, sums& s) {
    size_t q;
    float4 cq;
    if (!tap_colour(lo, qx, qy, idp, q, cq)) return;
    float w = g;
    if (idp != kNoPrim) {
        const float4 nq = lo.normal_z[q];
        float d = fmaxf(np.x * nq.x + np.y * nq.y + np.z * nq.z, 0.0f);
        for (uint32_t k = 0; k < squarings; ++k) d = d * d;
        const float t = (np.w - nq.w) * depth_sharpness;
        w = (g * d) / (1.0f + t * t);
    }
    if (!(w > 0.0f)) return;
    s.x = s.x + w * cq.x;
    s.y = s.y + w * cq.y;
    s.z = s.z + w * cq.z;
    s.den = s.den + w;
}

// u = 2 X + 1 - f over 2 f: the lo pixel at or left of the hi pixel's centre (floor; u is negative at the
// border) and the centre's offset from it in lo pixels, a multiple of 1 / 2f in [0, 1).
__device__ __forceinline__ void position(int X, int f, int& x0, float& fx) {
    const int u = 2 * X + 1 - f;
    x0 = u < 0 ? -1 : u / (2 * f);
    fx = (float)(u - 2 * f * x0) / (float)(2 * f);
}

// Direct global loads: stage A is four taps of 36 bytes (colour, normal and depth, id) from a footprint every
// f x f hi pixels share, so the lines come from L1/L2 after their first use. Stage B (sixteen taps) sits behind
// a per-lane branch: a wave with no lane in it skips it. The class goes out in the result's fourth component and
// is counted from there by iqu_stats_kernel: counted here, one atomic add per wave on the three counters, the
// kernel took 0.40 ms at 1920x1080 whatever the factor, the atomics of 32400 waves on one address.
__global__ void __launch_bounds__(kBlockX* kBlockY) iqu_upscale_kernel(run_params p, const float4* __restrict__ colour_lo,
                                                                       const float4* __restrict__ normal_z_lo,
                                                                       const uint32_t* __restrict__ id_lo,
                                                                       const float4* __restrict__ normal_z_hi,
                                                                       const uint32_t* __restrict__ id_hi,
                                                                       float4* __restrict__ out, uint32_t* __restrict__ bgra) {
    const int px = (int)(blockIdx.x * kBlockX + threadIdx.x), py = (int)(blockIdx.y * kBlockY + threadIdx.y);
    if (px >= (int)p.width || py >= (int)p.height) return;
    const size_t pix = (size_t)py * p.width + (size_t)px;
    const uint32_t idp = id_hi[pix];
    const float4 np = normal_z_hi[pix];
    const atrous_planes lo = {p.lo_width, p.lo_height, colour_lo, normal_z_lo, id_lo};
    const int f = (int)p.factor;
    int x0, y0;
    float fx, fy;
    position(px, f, x0, fx);
    position(py, f, y0, fy);
    sums s;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const float gy = b ? fy : 1.0f - fy;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const float gx = a ? fx : 1.0f - fx;
            add_tap(lo, x0 + a, y0 + b, idp, np, gy * gx, p.squarings, p.depth_sharpness, s);
        }
    }
    int cls = 0;
    if (!(s.den > 0.0f)) {
        s = sums();
        for (int b = -1; b <= 2; ++b)
            for (int a = -1; a <= 2; ++a) add_tap(lo, x0 + a, y0 + b, idp, np, 1.0f, p.squarings, p.depth_sharpness, s);
        cls = 1;
    }
    float4 res;
    if (s.den > 0.0f) {
        res = make_float4(s.x / s.den, s.y / s.den, s.z / s.den, (float)cls);
    } else {
        const float4 c = colour_lo[(size_t)(py / f) * p.lo_width + (size_t)(px / f)];
        res = make_float4(c.x, c.y, c.z, 2.0f);
    }
    out[pix] = res;
    bgra[pix] = encode(res);
}

constexpr unsigned kStatsBlock = 256;
constexpr unsigned kStatsMaxBlocks = 1024;

// The three counts of iqpt_upscale_stats, from the classes in the result's fourth component: every thread counts
// its pixels of a grid-stride loop, then one wave reduction per class and one 64-bit atomic add per wave and class
// that occurs, of at most 4096 waves. Integer sums are order-free, so the counts are exact. Run on request only.
__global__ void __launch_bounds__(kStatsBlock) iqu_stats_kernel(size_t npix, const float4* __restrict__ out,
                                                                unsigned long long* __restrict__ counts) {
    unsigned n[3] = {0u, 0u, 0u};
    for (size_t i = (size_t)blockIdx.x * kStatsBlock + threadIdx.x; i < npix; i += (size_t)gridDim.x * kStatsBlock) {
        const float c = out[i].w;
        n[0] += c == 0.0f;
        n[1] += c == 1.0f;
        n[2] += c == 2.0f;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        unsigned v = n[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63u) == 0u && v != 0u) atomicAdd(&counts[k], (unsigned long long)v);
    }
}

}  // namespace

hipError_t launch_upscale(hipStream_t s, const run_params& p, const run_planes& g, void* out, uint32_t* bgra) {
    iqu_upscale_kernel<<<grid(p.width, p.height), dim3(kBlockX, kBlockY), 0, s>>>(
        p, static_cast<const float4*>(g.colour_lo), static_cast<const float4*>(g.normal_z_lo), g.id_lo,
        static_cast<const float4*>(g.normal_z_hi), g.id_hi, static_cast<float4*>(out), bgra);
    return hipGetLastError();
}

hipError_t launch_stats(hipStream_t s, uint32_t width, uint32_t height, const void* out, unsigned long long* counts) {
    const size_t npix = (size_t)width * height;
    const size_t blocks = (npix + kStatsBlock - 1) / kStatsBlock;
    iqu_stats_kernel<<<dim3((unsigned)(blocks < kStatsMaxBlocks ? blocks : kStatsMaxBlocks)), dim3(kStatsBlock), 0, s>>>(
        npix, static_cast<const float4*>(out), counts);
    return hipGetLastError();
}

}  // namespace iqu
