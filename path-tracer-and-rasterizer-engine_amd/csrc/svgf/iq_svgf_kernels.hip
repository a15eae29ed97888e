// iq_svgf_kernels.hip — the variance-guided filter's kernels for gfx950 (wave64), lane = pixel: the luminance
// moments of a colour plane, the per-pixel variance estimate (temporal from the moments history, spatial from a
// 7x7 window staged in LDS) and one variance-guided à-trous level per launch, over the tap and the BGRA8 encoding
// of post/iq_post_device.hpp. DESIGN.md §12 is the definition these restate; every float operation below is
// written in that section's order and compiled with -ffp-contract=off and correctly rounded division and square
// root.
#include <hip/hip_runtime.h>

#include "svgf/iq_svgf.hpp"

namespace iqs {

using namespace iqp;

namespace {

__device__ inline float luminance(const float4& c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

// a where a > 0, else +0: a NaN, a negative value and -0 all give +0
__device__ inline float pos(float a) { return a > 0.0f ? a : 0.0f; }
// and +inf gives +0 as well: what keeps every variance finite and >= 0
__device__ inline float pos_finite(float a) { return a > 0.0f && a < __builtin_huge_valf() ? a : 0.0f; }

// 16 bytes in, 16 out per lane.
__global__ void __launch_bounds__(256) iqs_moments_kernel(uint32_t npix, const float4* __restrict__ colour,
                                                          float4* __restrict__ moments) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= npix) return;
    const float l = luminance(colour[i]);
    moments[i] = make_float4(l, l * l, 0.0f, 0.0f);
}

// The tile's 32x8 pixels and a 3-pixel halo go to LDS once: L(o) and the id, the id replaced by NO_PRIM where
// the entry is off the frame or o.xyz is not finite, which is how the finite flag is staged (a tap needs
// id(q) == id(p), and a pixel that estimates anything has id(p) != NO_PRIM). Every lane stages its own pixel,
// whose o it needs in full anyway, then the 276 halo entries are shared out; each is read once from global
// memory. No lane leaves before either barrier. The window loop runs under a per-lane test that is wave-uniform in
// practice (every pixel on a first view, few after a move).
__global__ void __launch_bounds__(kBlockX* kBlockY) iqs_variance_kernel(variance_params p, const float4* __restrict__ o,
                                                                        const float4* __restrict__ mu,
                                                                        const uint32_t* __restrict__ id,
                                                                        float4* __restrict__ c0,
                                                                        uint32_t* __restrict__ block_spatial) {
    __shared__ float s_lum[kTileH][kTileW];
    __shared__ uint32_t s_id[kTileH][kTileW];
    const int tx = (int)threadIdx.x, ty = (int)threadIdx.y;
    const int px = (int)(blockIdx.x * kBlockX) + tx, py = (int)(blockIdx.y * kBlockY) + ty;
    const bool inside = px < (int)p.width && py < (int)p.height;
    const size_t pix = (size_t)py * p.width + (size_t)px;
    float4 op = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint32_t idp = kNoPrim;
    bool live = false;
    if (inside) {
        op = o[pix];
        idp = id[pix];
        live = idp != kNoPrim && finite3(op);
    }
    const bool fin = inside && finite3(op);
    s_lum[ty + kHalo][tx + kHalo] = fin ? luminance(op) : 0.0f;
    s_id[ty + kHalo][tx + kHalo] = fin ? idp : kNoPrim;
    const int x0 = (int)(blockIdx.x * kBlockX) - kHalo, y0 = (int)(blockIdx.y * kBlockY) - kHalo;
    for (int e = ty * kBlockX + tx; e < kTileW * kTileH; e += kBlockX * kBlockY) {
        const int ey = e / kTileW, ex = e - ey * kTileW;
        if (ex >= kHalo && ex < kHalo + kBlockX && ey >= kHalo && ey < kHalo + kBlockY) continue;   // a lane's own
        const int qx = x0 + ex, qy = y0 + ey;
        float l = 0.0f;
        uint32_t iq = kNoPrim;
        if (qx >= 0 && qy >= 0 && qx < (int)p.width && qy < (int)p.height) {
            const size_t q = (size_t)qy * p.width + (size_t)qx;
            const float4 oq = o[q];
            if (finite3(oq)) {
                l = luminance(oq);
                iq = id[q];
            }
        }
        s_lum[ey][ex] = l;
        s_id[ey][ex] = iq;
    }
    __syncthreads();

    float v = 0.0f;
    bool spatial = false;
    if (live) {
        const float4 m = mu[pix];
        if (m.w >= p.min_weight && finite1(m.x) && finite1(m.y)) {
            v = pos_finite(pos(m.y - m.x * m.x) * (p.ne / op.w));
        } else {
            spatial = true;
            float s1 = 0.0f, s2 = 0.0f;
            uint32_t k = 0;
            for (int dy = 0; dy <= 2 * kHalo; ++dy) {
#pragma unroll
                for (int dx = 0; dx <= 2 * kHalo; ++dx) {
                    // selects, not branches: the sums of a tap that does not count are discarded, so the lanes of
                    // a wave stay together through the window (the centre's own entry holds idp)
                    const bool use = s_id[ty + dy][tx + dx] == idp;
                    const float l = s_lum[ty + dy][tx + dx];
                    const float t1 = s1 + l, t2 = s2 + l * l;
                    s1 = use ? t1 : s1;
                    s2 = use ? t2 : s2;
                    k += use ? 1u : 0u;
                }
            }
            const float kf = (float)k, m1 = s1 / kf;
            v = pos_finite(s2 / kf - m1 * m1);
        }
    }
    if (inside) c0[pix] = make_float4(op.x, op.y, op.z, v);
    // the block's count into its own slot, summed by iqpt_svgf_stats on request: on a first view every wave has
    // spatial lanes, and one atomic per wave on a single counter then costs more than the kernel itself
    const int count = __syncthreads_count(spatial ? 1 : 0);
    if (ty == 0 && tx == 0) block_spatial[blockIdx.y * gridDim.x + blockIdx.x] = (uint32_t)count;
}

// One level, direct global loads as iqd_level_kernel: 9 taps of the variance normaliser at step 1, then 25 taps
// of 36 bytes at the level's step. Pixels without a guide or with a non-finite colour are copied, all four
// components.
template <bool kEncode>
__global__ void __launch_bounds__(kBlockX* kBlockY) iqs_level_kernel(level_params p, const float4* __restrict__ in,
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
        const atrous_planes a = {p.width, p.height, in, normal_z, id};
        const float g[3] = {1.0f / 4.0f, 1.0f / 2.0f, 1.0f / 4.0f};
        float vsum = 0.0f, gsum = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const float gw = g[dy + 1] * g[dx + 1];
                if (dy == 0 && dx == 0) {
                    vsum = vsum + gw * cp.w;
                    gsum = gsum + gw;
                    continue;
                }
                size_t q;
                float4 cq;
                if (!tap_colour(a, px + dx, py + dy, idp, q, cq)) continue;
                vsum = vsum + gw * cq.w;
                gsum = gsum + gw;
            }
        }
        const float vb = vsum / gsum;
        const float r = 1.0f / (p.sigma2 * vb + p.variance_floor);

        const float4 np = normal_z[pix];
        const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
        float nx = 0.0f, ny = 0.0f, nz = 0.0f, den = 0.0f, vnum = 0.0f;
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
                    vnum = vnum + (hw * hw) * cp.w;
                    continue;
                }
                size_t q;
                float4 cq;
                float w;
                if (!tap_colour(a, px + dx * p.step, py + dy * p.step, idp, q, cq)) continue;
                if (!tap_weight(a, q, cq, cp, np, hw, p.squarings, p.depth_sharpness, r, w)) continue;
                nx = nx + w * cq.x;
                ny = ny + w * cq.y;
                nz = nz + w * cq.z;
                den = den + w;
                vnum = vnum + (w * w) * cq.w;
            }
        }
        res = make_float4(nx / den, ny / den, nz / den, pos_finite(vnum / (den * den)));
    }
    out[pix] = res;
    if (kEncode) bgra[pix] = encode(res);
}

}  // namespace

hipError_t launch_moments(hipStream_t s, uint32_t npix, const void* colour, void* moments) {
    iqs_moments_kernel<<<dim3((npix + 255u) / 256u), dim3(256), 0, s>>>(npix, static_cast<const float4*>(colour),
                                                                        static_cast<float4*>(moments));
    return hipGetLastError();
}

hipError_t launch_variance(hipStream_t s, const variance_params& p, const void* o, const void* mu, const uint32_t* id,
                           void* c0, uint32_t* block_spatial) {
    iqs_variance_kernel<<<grid(p.width, p.height), dim3(kBlockX, kBlockY), 0, s>>>(
        p, static_cast<const float4*>(o), static_cast<const float4*>(mu), id, static_cast<float4*>(c0), block_spatial);
    return hipGetLastError();
}

hipError_t launch_level(hipStream_t s, const level_params& p, const void* in, const void* normal_z, const uint32_t* id,
                        void* out, uint32_t* bgra) {
    const dim3 g = grid(p.width, p.height), b(kBlockX, kBlockY);
    if (bgra)
        iqs_level_kernel<true><<<g, b, 0, s>>>(p, static_cast<const float4*>(in), static_cast<const float4*>(normal_z), id,
                                               static_cast<float4*>(out), bgra);
    else
        iqs_level_kernel<false><<<g, b, 0, s>>>(p, static_cast<const float4*>(in), static_cast<const float4*>(normal_z), id,
                                                static_cast<float4*>(out), nullptr);
    return hipGetLastError();
}

}  // namespace iqs
