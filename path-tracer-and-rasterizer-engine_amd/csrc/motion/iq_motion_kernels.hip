// iq_motion_kernels.hip — moving-model reprojection for gfx950 (wave64), lane = pixel: the view kernel (world
// positions of a new view and its history, gathered from the previous view's result through each model's motion
// entry) and the four counts. DESIGN.md §15 is the definition these restate; every float operation below is
// written in that section's order and compiled with -ffp-contract=off and correctly rounded division and square
// root. The resolve is temporal reprojection's own kernel (iqt::launch_resolve).
#include <hip/hip_runtime.h>

#include "motion/iq_motion.hpp"
#include "post/iq_post_device.hpp"

// 0: every lane gathers its own entry (the default: the simpler form, and no slower where it was measured,
// DESIGN.md §15.2); 1: a wave whose guided lanes all have one draw index reads that entry through wave-uniform
// loads and falls back to the per-lane gather otherwise (the A/B library). The bits are the same.
#ifndef IQM_UNIFORM_ENTRY
#define IQM_UNIFORM_ENTRY 0
#endif

namespace iqm {

using namespace iqp;
using iqt::view_params;

namespace {

// (x, y, z, 1) times a row-major 4x4 as a row vector: each component a left-to-right sum over the column
// (tests/raster_ref.py dot4; the product with w = 1 is exact, so the last term is the matrix word itself)
__device__ __forceinline__ float4 dot4_w1(float x, float y, float z, const float* m) {
    return make_float4(((x * m[0] + y * m[4]) + z * m[8]) + m[12], ((x * m[1] + y * m[5]) + z * m[9]) + m[13],
                       ((x * m[2] + y * m[6]) + z * m[10]) + m[14], ((x * m[3] + y * m[7]) + z * m[11]) + m[15]);
}

__device__ __forceinline__ float4 dot4(const float4& v, const float* m) {
    return make_float4(((v.x * m[0] + v.y * m[4]) + v.z * m[8]) + v.w * m[12], ((v.x * m[1] + v.y * m[5]) + v.z * m[9]) + v.w * m[13],
                       ((v.x * m[2] + v.y * m[6]) + v.z * m[10]) + v.w * m[14],
                       ((v.x * m[3] + v.y * m[7]) + v.z * m[11]) + v.w * m[15]);
}

struct prev_view {
    const float4* __restrict__ normal_z;
    const uint32_t* __restrict__ id;
    const float4* __restrict__ pos;
    const float4* __restrict__ out;
};

// The history tap of §11.1 step 2 for the point (X, Y, Z) with normal (nx, ny, nz) and draw index idp: §11's own
// with the pixel's P and n_p, §15.1's with Pm and nm. Gathered at q, the pixel the point fell on in the previous
// view: id, normal_z, pos and out, each read only while the tests before it hold. q is inside the old frame by the
// tests on xs and ys themselves (0 <= xs < width as floats, width <= 8192 exact), which is what bounds every gather.
__device__ __forceinline__ float4 tap(const view_params& p, const prev_view& v, uint32_t idp, float X, float Y, float Z,
                                      float nx, float ny, float nz) {
    float4 h = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float wf = (float)p.width, hf = (float)p.height;
    const float4 c = dot4(dot4_w1(X, Y, Z, p.view_prev), p.proj_prev);
    const float xs = ((c.x / c.w + 1.0f) * wf) * 0.5f;
    const float ys = ((1.0f - c.y / c.w) * hf) * 0.5f;
    if (c.w > 0.0f && xs >= 0.0f && xs < wf && ys >= 0.0f && ys < hf) {      // a NaN fails
        const uint32_t qx = min((uint32_t)floorf(xs), p.width - 1u), qy = min((uint32_t)floorf(ys), p.height - 1u);
        const size_t q = (size_t)qy * p.width + qx;
        if (v.id[q] == idp) {
            const float4 nq = v.normal_z[q];
            if ((nx * nq.x + ny * nq.y) + nz * nq.z >= p.normal_min) {
                const float4 Pq = v.pos[q];
                const float dx = Pq.x - X, dy = Pq.y - Y, dz = Pq.z - Z;
                if (fabsf((nx * dx + ny * dy) + nz * dz) <= p.plane_tolerance * c.w) {
                    const float4 o = v.out[q];
                    if (o.w > 0.0f && finite3(o)) h = make_float4(o.x, o.y, o.z, fminf(o.w, p.max_history));
                }
            }
        }
    }
    return h;
}

// §15.1's moved case: the point and the normal through the entry, then the tap. `e` is wave-uniform (scalar loads
// of its 28 words) or per lane (a gather); the arithmetic, and so the bits, are the same.
__device__ __forceinline__ float4 moved_tap(const view_params& p, const prev_view& v, uint32_t idp, const float4& P,
                                            const float4& np, const iqpt_motion_entry* __restrict__ e) {
    const float* B = e->back;
    const float* N = e->nback;
    const float4 Pm = dot4_w1(P.x, P.y, P.z, B);
    const float mx = (np.x * N[0] + np.y * N[4]) + np.z * N[8];
    const float my = (np.x * N[1] + np.y * N[5]) + np.z * N[9];
    const float mz = (np.x * N[2] + np.y * N[6]) + np.z * N[10];
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (!(fabsf(mx) < 0.00001f && fabsf(my) < 0.00001f && fabsf(mz) < 0.00001f)) {      // §9.6's normalized3
        const float inv = 1.0f / sqrtf((mx * mx + my * my) + mz * mz);
        nx = mx * inv;
        ny = my * inv;
        nz = mz * inv;
    }
    return tap(p, v, idp, Pm.x, Pm.y, Pm.z, nx, ny, nz);
}

__device__ __forceinline__ float4 entry_tap(const view_params& p, const prev_view& v, uint32_t idp, const float4& P,
                                            const float4& np, const iqpt_motion_entry* __restrict__ e) {
    return e->moved ? moved_tap(p, v, idp, P, np, e) : tap(p, v, idp, P.x, P.y, P.z, np.x, np.y, np.z);
}

// Coalesced: reads normal_z and id, writes pos and hist (104 bytes per pixel with the four gathers, as §11's). The
// table is read only by a pixel with a guide whose id is below n, which is tested before any address is formed.
__global__ void __launch_bounds__(kBlockX* kBlockY) iqm_view_kernel(view_params p, const float4* __restrict__ normal_z,
                                                                    const uint32_t* __restrict__ id,
                                                                    float4* __restrict__ pos, float4* __restrict__ hist,
                                                                    prev_view v, const iqpt_motion_entry* __restrict__ table,
                                                                    uint32_t n) {
    const uint32_t px = blockIdx.x * kBlockX + threadIdx.x, py = blockIdx.y * kBlockY + threadIdx.y;
    if (px >= p.width || py >= p.height) return;
    const size_t pix = (size_t)py * p.width + px;
    const float4 np = normal_z[pix];
    const uint32_t idp = id[pix];
    const float wf = (float)p.width, hf = (float)p.height;
    const float x = (((float)px + 0.5f) * 2.0f) / wf - 1.0f;
    const float y = 1.0f - (((float)py + 0.5f) * 2.0f) / hf;
    const float4 vv = dot4_w1(x, y, np.w, p.inv_proj);
    const float rw = 1.0f / vv.w;
    const float4 P = dot4_w1(vv.x * rw, vv.y * rw, vv.z * rw, p.inv_view);
    float4 h = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (p.have_prev && idp != kNoPrim) {
        if (n == 0u) {
            h = tap(p, v, idp, P.x, P.y, P.z, np.x, np.y, np.z);
        } else if (idp < n) {
#if IQM_UNIFORM_ENTRY
            // the first active lane here has a guide and an id below n: d0 is a valid index, and wave-uniform by
            // construction, so the entry's words come through the scalar cache
            const uint32_t d0 = __builtin_amdgcn_readfirstlane(idp);
            if (__ballot(idp != d0) == 0ull) {
                h = entry_tap(p, v, d0, P, np, table + d0);
            } else
#endif
            {
                h = entry_tap(p, v, idp, P, np, table + idp);
            }
        }
    }
    pos[pix] = P;
    hist[pix] = h;
}

// The four counts of iqpt_motion_stats: a ballot per wave, at most four atomics per wave. Run on request only.
__global__ void __launch_bounds__(256) iqm_stats_kernel(uint32_t npix, const uint32_t* __restrict__ id,
                                                        const float4* __restrict__ hist,
                                                        const iqpt_motion_entry* __restrict__ table, uint32_t n,
                                                        unsigned long long* counts) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool guided = false, valid = false, moved = false;
    if (i < npix) {
        const uint32_t d = id[i];
        guided = d != kNoPrim;
        valid = guided && hist[i].w > 0.0f;
        if (guided && d < n) moved = table[d].moved != 0u;
    }
    const unsigned long long g = __ballot(guided), v = __ballot(valid), m = __ballot(moved), mv = __ballot(moved && valid);
    if ((threadIdx.x & 63u) == 0u) {
        if (g) atomicAdd(&counts[0], (unsigned long long)__popcll(g));
        if (v) atomicAdd(&counts[1], (unsigned long long)__popcll(v));
        if (m) atomicAdd(&counts[2], (unsigned long long)__popcll(m));
        if (mv) atomicAdd(&counts[3], (unsigned long long)__popcll(mv));
    }
}

}  // namespace

hipError_t launch_view(hipStream_t s, const view_params& p, const iqt::view_planes& cur, const iqt::view_planes& prev,
                       const void* out, void* hist, const iqpt_motion_entry* table, uint32_t n) {
    const prev_view v{static_cast<const float4*>(prev.normal_z), prev.id, static_cast<const float4*>(prev.pos),
                      static_cast<const float4*>(out)};
    iqm_view_kernel<<<grid(p.width, p.height), dim3(kBlockX, kBlockY), 0, s>>>(
        p, static_cast<const float4*>(cur.normal_z), cur.id, static_cast<float4*>(cur.pos), static_cast<float4*>(hist), v,
        table, n);
    return hipGetLastError();
}

hipError_t launch_stats(hipStream_t s, uint32_t npix, const uint32_t* id, const void* hist, const iqpt_motion_entry* table,
                        uint32_t n, unsigned long long* counts) {
    iqm_stats_kernel<<<dim3((npix + 255u) / 256u), dim3(256), 0, s>>>(npix, id, static_cast<const float4*>(hist), table, n,
                                                                      counts);
    return hipGetLastError();
}

}  // namespace iqm
