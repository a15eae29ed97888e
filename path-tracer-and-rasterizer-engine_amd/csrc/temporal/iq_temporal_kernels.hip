// iq_temporal_kernels.hip — temporal reprojection for gfx950 (wave64), lane = pixel: the view kernel (world
// positions of a new view and its history, gathered from the previous view's result) and the resolve kernel (the
// blend with the accumulator plus the BGRA8 encoding). DESIGN.md §11 is the definition these restate; every float
// operation below is written in that section's order and compiled with -ffp-contract=off and correctly rounded
// division and square root.
#include <hip/hip_runtime.h>

#include "post/iq_post_device.hpp"
#include "temporal/iq_temporal.hpp"

namespace iqt {

using namespace iqp;

namespace {

// (x, y, z, 1) times a row-major 4x4 as a row vector: each component a left-to-right sum over the column
// (tests/raster_ref.py dot4; the product with w = 1 is exact, so the last term is the matrix word itself)
__device__ inline float4 dot4_w1(float x, float y, float z, const float* m) {
    return make_float4(((x * m[0] + y * m[4]) + z * m[8]) + m[12], ((x * m[1] + y * m[5]) + z * m[9]) + m[13],
                       ((x * m[2] + y * m[6]) + z * m[10]) + m[14], ((x * m[3] + y * m[7]) + z * m[11]) + m[15]);
}

__device__ inline float4 dot4(const float4& v, const float* m) {
    return make_float4(((v.x * m[0] + v.y * m[4]) + v.z * m[8]) + v.w * m[12], ((v.x * m[1] + v.y * m[5]) + v.z * m[9]) + v.w * m[13],
                       ((v.x * m[2] + v.y * m[6]) + v.z * m[10]) + v.w * m[14],
                       ((v.x * m[3] + v.y * m[7]) + v.z * m[11]) + v.w * m[15]);
}

// Coalesced: reads normal_z and id, writes pos and hist. Gathered at q, the pixel the point fell on in the
// previous view: id, normal_z, pos and out, each read only while the tests before it hold, so a pixel without a
// guide or off the old frame reads nothing. q is inside the old frame by the tests on xs and ys themselves
// (0 <= xs < width as floats, width <= 8192 exact), which is what bounds every gather.
__global__ void __launch_bounds__(kBlockX* kBlockY) iqt_view_kernel(view_params p, const float4* __restrict__ normal_z,
                                                                    const uint32_t* __restrict__ id,
                                                                    float4* __restrict__ pos, float4* __restrict__ hist,
                                                                    const float4* __restrict__ nz_prev,
                                                                    const uint32_t* __restrict__ id_prev,
                                                                    const float4* __restrict__ pos_prev,
                                                                    const float4* __restrict__ out_prev) {
    const uint32_t px = blockIdx.x * kBlockX + threadIdx.x, py = blockIdx.y * kBlockY + threadIdx.y;
    if (px >= p.width || py >= p.height) return;
    const size_t pix = (size_t)py * p.width + px;
    const float4 np = normal_z[pix];
    const uint32_t idp = id[pix];
    const float wf = (float)p.width, hf = (float)p.height;
    const float x = (((float)px + 0.5f) * 2.0f) / wf - 1.0f;
    const float y = 1.0f - (((float)py + 0.5f) * 2.0f) / hf;
    const float4 v = dot4_w1(x, y, np.w, p.inv_proj);
    const float rw = 1.0f / v.w;
    const float4 P = dot4_w1(v.x * rw, v.y * rw, v.z * rw, p.inv_view);
    pos[pix] = P;
    float4 h = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (p.have_prev && idp != kNoPrim) {
        const float4 c = dot4(dot4_w1(P.x, P.y, P.z, p.view_prev), p.proj_prev);
        const float xs = ((c.x / c.w + 1.0f) * wf) * 0.5f;
        const float ys = ((1.0f - c.y / c.w) * hf) * 0.5f;
        if (c.w > 0.0f && xs >= 0.0f && xs < wf && ys >= 0.0f && ys < hf) {      // a NaN fails
            const uint32_t qx = min((uint32_t)floorf(xs), p.width - 1u), qy = min((uint32_t)floorf(ys), p.height - 1u);
            const size_t q = (size_t)qy * p.width + qx;
            if (id_prev[q] == idp) {
                const float4 nq = nz_prev[q];
                if ((np.x * nq.x + np.y * nq.y) + np.z * nq.z >= p.normal_min) {
                    const float4 Pq = pos_prev[q];
                    const float dx = Pq.x - P.x, dy = Pq.y - P.y, dz = Pq.z - P.z;
                    if (fabsf((np.x * dx + np.y * dy) + np.z * dz) <= p.plane_tolerance * c.w) {
                        const float4 o = out_prev[q];
                        if (o.w > 0.0f && finite3(o)) h = make_float4(o.x, o.y, o.z, fminf(o.w, p.max_history));
                    }
                }
            }
        }
    }
    hist[pix] = h;
}

// 16 + 16 bytes in, 16 + 4 out per pixel; the table of §11.
__global__ void __launch_bounds__(kBlockX* kBlockY) iqt_resolve_kernel(uint32_t width, uint32_t height, float nf,
                                                                       const float4* __restrict__ hist,
                                                                       const float4* __restrict__ colour,
                                                                       float4* __restrict__ out,
                                                                       uint32_t* __restrict__ bgra) {
    const uint32_t px = blockIdx.x * kBlockX + threadIdx.x, py = blockIdx.y * kBlockY + threadIdx.y;
    if (px >= width || py >= height) return;
    const size_t pix = (size_t)py * width + px;
    const float4 h = hist[pix];
    const float4 c = colour[pix];
    const bool cf = finite3(c);
    const float m = h.w;
    float4 res;
    if (m > 0.0f) {
        if (nf > 0.0f && cf) {
            const float tot = m + nf;
            res = make_float4((h.x * m + c.x * nf) / tot, (h.y * m + c.y * nf) / tot, (h.z * m + c.z * nf) / tot, tot);
        } else {
            res = h;
        }
    } else if (nf > 0.0f) {
        res = make_float4(c.x, c.y, c.z, cf ? nf : 0.0f);
    } else {
        res = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    out[pix] = res;
    bgra[pix] = encode(res);
}

// The two counts of iqpt_temporal_stats: a ballot per wave, one atomic pair per wave. Run on request only.
__global__ void __launch_bounds__(256) iqt_stats_kernel(uint32_t npix, const uint32_t* __restrict__ id,
                                                        const float4* __restrict__ hist, unsigned long long* counts) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool guided = false, valid = false;
    if (i < npix) {
        guided = id[i] != kNoPrim;
        valid = guided && hist[i].w > 0.0f;
    }
    const unsigned long long g = __ballot(guided), v = __ballot(valid);
    if ((threadIdx.x & 63u) == 0u) {
        if (g) atomicAdd(&counts[0], (unsigned long long)__popcll(g));
        if (v) atomicAdd(&counts[1], (unsigned long long)__popcll(v));
    }
}

}  // namespace

hipError_t launch_view(hipStream_t s, const view_params& p, const view_planes& cur, const view_planes& prev,
                       const void* out, void* hist) {
    iqt_view_kernel<<<grid(p.width, p.height), dim3(kBlockX, kBlockY), 0, s>>>(
        p, static_cast<const float4*>(cur.normal_z), cur.id, static_cast<float4*>(cur.pos), static_cast<float4*>(hist),
        static_cast<const float4*>(prev.normal_z), prev.id, static_cast<const float4*>(prev.pos),
        static_cast<const float4*>(out));
    return hipGetLastError();
}

hipError_t launch_resolve(hipStream_t s, uint32_t width, uint32_t height, float nf, const void* hist, const void* colour,
                          void* out, uint32_t* bgra) {
    iqt_resolve_kernel<<<grid(width, height), dim3(kBlockX, kBlockY), 0, s>>>(
        width, height, nf, static_cast<const float4*>(hist), static_cast<const float4*>(colour), static_cast<float4*>(out), bgra);
    return hipGetLastError();
}

hipError_t launch_stats(hipStream_t s, uint32_t npix, const uint32_t* id, const void* hist, unsigned long long* counts) {
    iqt_stats_kernel<<<dim3((npix + 255u) / 256u), dim3(256), 0, s>>>(npix, id, static_cast<const float4*>(hist), counts);
    return hipGetLastError();
}

}  // namespace iqt
