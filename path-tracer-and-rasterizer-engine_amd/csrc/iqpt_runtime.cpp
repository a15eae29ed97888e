// iqpt_runtime.cpp — the C ABI of include/iqpt.h over HIP, its core: errors, render contexts (create, destroy,
// camera, packet upload with both BVH builders), the helpers the runtime sources share, sync, reset, readback and
// frame copies, counters and timing. The rest of the ABI is runtime/iq_*.cpp by concern.
//
// Replaces the CUDA side of path_tracer (IoniqRE/path_tracer.cu:48-164, 368-404) and the upload
// half of scene::build_packet / free_packet (IoniqRE/scene.cu:183-264).
#include <mutex>

#include "iq_bvh.hpp"
#include "iq_host_math.hpp"
#include "iq_xorwow.h"
#include "runtime/iq_ctx.hpp"

namespace iqpt {

namespace {
thread_local std::string g_last_error;

std::once_flag g_tables_once;
std::vector<uint32_t> g_tables;  // A^(2^(67+i)), i < 32

const std::vector<uint32_t>& xorwow_tables() {
    std::call_once(g_tables_once, [] {
        g_tables.resize(32 * IQ_XORWOW_MAT_WORDS);
        iq_xorwow_subseq_tables(g_tables.data(), 32);
    });
    return g_tables;
}

}  // namespace

int hip_fail(hipError_t e, const char* what) {
    return fail(IQPT_ERR_HIP, std::string(what) + ": " + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ")");
}

void set_last_error(const std::string& msg) { g_last_error = msg; }
int fail(int status, const std::string& msg) {
    g_last_error = msg;
    return status;
}

}  // namespace iqpt

using namespace iqpt::rt;

namespace iqpt::rt {

int use_device(const iqpt_ctx* c) {
    IQPT_HIP(hipSetDevice(c->device));
    return IQPT_OK;
}

// kOptOverlap: make `stream` wait for the last launch on `stream2`; the next overlapped launch starts a
// new chain (tile_done zeroed on `stream`, no waits).
int join_streams(iqpt_ctx* c) {
    if (c->s2_pending) {
        IQPT_HIP(hipEventRecord(c->ev_s2, c->stream2));
        IQPT_HIP(hipStreamWaitEvent(c->stream, c->ev_s2, 0));
        c->s2_pending = false;
    }
    // pipelined launches: `stream` also waits for the frame copies still reading a frame buffer
    if (c->copy_seq > c->pwaited) {
        IQPT_HIP(hipStreamWaitEvent(c->stream, c->pev[c->copy_seq % iqpt::kPipeRing], 0));
        c->pwaited = c->copy_seq;
    }
    c->pipe = false;
    c->next_on_main = true;
    c->ovl_zero = true;
    c->last_ovl = false;
    c->sky_last = nullptr;             // everything before is ordered on `stream` now
    return IQPT_OK;
}

// Pipelined launches: the frame-copy stream and its two events, created when the first pipelined launch
// ends, so that iqpt_frame_stream names the stream the next copy goes on before any copy was asked for.
int ensure_copy_stream(iqpt_ctx* c) {
    if (!c->stream3 && hipStreamCreateWithFlags(&c->stream3, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        return iqpt::fail(IQPT_ERR_HIP, "frame copy stream");
    }
    return IQPT_OK;
}

// Every entry point but iqpt_render: the device, then the streams joined — the gathers in flight too
// (they read the send buffers and write the caller's frame; a render never waits for them: the copy
// into a send buffer is ordered behind the launch that wrote the frame, on the launch's own stream).
int enter(iqpt_ctx* c) {
    int st = use_device(c);
    if (st) return st;
    if (c->comm_pend) {
        IQPT_HIP(hipStreamWaitEvent(c->stream, c->ev_gend, 0));
        c->comm_pend = false;
    }
    return join_streams(c);
}

}  // namespace iqpt::rt

namespace {

// Words of a BGRA8 frame buffer: the owned pixels, padded to the multi-GPU gather's block once a communicator
// exists (a pipelined launch's buffer is then the gather's send buffer itself)
size_t frame_words(const iqpt_ctx* c) {
    return std::max<size_t>((size_t)c->npix, (size_t)c->comm_stride);
}

void free_scene(iqpt_ctx* c) {
    for (float4_storage** b : {&c->d_tris, &c->d_tri_pairs, &c->d_tri_shade, &c->d_sph, &c->d_sph_pairs, &c->d_mats,
                               &c->d_bvh_nodes, &c->d_bvh_pairs, &c->d_sbvh_nodes, &c->d_sbvh_sph})
        dev_free(*b);
    c->bvh_nnodes = c->bvh_nalways = 0;
    c->sbvh_nnodes = c->sbvh_nalways = 0;
    for (uint32_t** b : {&c->d_tri_mat, &c->d_sph_mat, &c->d_bvh_always, &c->d_sbvh_idx, &c->d_sbvh_always})
        dev_free(*b);
    c->ntri = c->nsph = 0;
    c->cull_valid = false;
    c->tune_stage = 0;
    c->tune_primary = false;
}

// Exact BVH for secondary rays (iq_bvh.hpp) over the world-space triangles `tris` (kTriFloat4 each)
// and the spheres (for the scene box). Fills the host arrays the upload copies to the device.
struct bvh_host {
    std::vector<float4_storage> nodes, pairs;
    std::vector<uint32_t> always;
    float md, gulp;
};
constexpr uint32_t kBvhMinTriangles = 256;

bool build_bvh(const std::vector<float4_storage>& tris, const std::vector<float4_storage>& sph, bvh_host& out) {
    const size_t ntri = tris.size() / iqpt::kTriFloat4;
    if (ntri < kBvhMinTriangles) return false;
    // scene box (exact corners of every triangle in double, spheres' centre +- radius)
    double blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
    std::vector<double> corners(ntri * 9);
    for (size_t k = 0; k < ntri; ++k) {
        const float4_storage* t = &tris[k * iqpt::kTriFloat4];
        const double v0[3] = {t[0].x, t[0].y, t[0].z};
        const double e1[3] = {t[0].w, t[1].x, t[1].y}, e2[3] = {t[1].z, t[1].w, t[2].x};
        for (int a = 0; a < 3; ++a) {
            const double c3[3] = {v0[a], v0[a] + e1[a], v0[a] + e2[a]};
            for (int q = 0; q < 3; ++q) {
                corners[k * 9 + 3 * q + a] = c3[q];
                blo[a] = std::min(blo[a], c3[q]);
                bhi[a] = std::max(bhi[a], c3[q]);
            }
        }
    }
    for (const float4_storage& s4 : sph) {
        const double c[3] = {s4.x, s4.y, s4.z}, r = std::fabs((double)s4.w);
        for (int a = 0; a < 3; ++a) {
            blo[a] = std::min(blo[a], c[a] - r);
            bhi[a] = std::max(bhi[a], c[a] + r);
        }
    }
    double ext = 0.0, maxabs = 0.0;
    for (int a = 0; a < 3; ++a) {
        ext = std::max(ext, bhi[a] - blo[a]);
        maxabs = std::max({maxabs, std::fabs(blo[a]), std::fabs(bhi[a])});
    }
    if (!std::isfinite(ext) || maxabs > 1e9) return false;
    // rays may use the BVH with |d_i| <= md and a finite origin (the bound holds for any origin:
    // it grows with the origin's distance S to the node, iq_bvh.hpp)
    const double Md = 1.001;
    out.md = 1.001f;
    // a box side lo - g rounds to nearest: |error| <= 2^-24 (maxabs + g); the kernel adds gulp and
    // scales g by 1 + 2^-20, which covers it
    double gc_max = 0.0;
    iqbvh::build_input in;
    for (size_t k = 0; k < ntri; ++k) {
        const float4_storage* t = &tris[k * iqpt::kTriFloat4];
        const float e1[3] = {t[0].w, t[1].x, t[1].y}, e2[3] = {t[1].z, t[1].w, t[2].x};
        const iqbvh::tri_coeffs b = iqbvh::triangle_coeffs(e1, e2, Md);
        if (!b.eligible) {
            out.always.push_back((uint32_t)k);
            continue;
        }
        for (int a = 0; a < 3; ++a) {
            const double lo = std::min({corners[k * 9 + a], corners[k * 9 + 3 + a], corners[k * 9 + 6 + a]});
            const double hi = std::max({corners[k * 9 + a], corners[k * 9 + 3 + a], corners[k * 9 + 6 + a]});
            in.lo.push_back(iqbvh::round_down(lo));
            in.hi.push_back(iqbvh::round_up(hi));
            in.centroid.push_back((float)((lo + hi) * 0.5));
        }
        const double co[4] = {b.gR, b.gB, b.tA, b.tB};
        gc_max = std::max(gc_max, b.gC);
        for (double v : co) in.coeff.push_back(iqbvh::round_up(v));
        in.normal.push_back(iqbvh::triangle_normal(e1, e2, Md, b.edet));
        in.edet.push_back(b.edet);
        in.tris.push_back((uint32_t)k);
    }
    // the D-independent part of the growth (gC) is applied as one scene-wide maximum
    out.gulp = iqbvh::round_up(maxabs * 0x1p-22 + gc_max);
    iqbvh::build_output bo;
    iqbvh::build(in, bo);
    // the 64-byte device node (iqpt_internal.hpp kBvhNodeFloat4): a leaf's successor is always the next
    // node, so one word holds the link — skip pointer (inner) or 1 << 31 | first pair << 8 | count (leaf);
    // tA, tB as bf16 rounded up; the cone as A = Nmin cos(beta) (down) and B = Nmin sin(beta) (up), from
    // which the kernel bounds Nmin |d| cos(theta + beta) = |d| cos(theta) A - |d| sin(theta) B
    if (bo.order.size() / 2 >= (1u << 23)) return false;
    for (const iqbvh::node& n : bo.nodes) {
        const uint32_t link = n.first_count ? (0x80000000u | n.first_count) : n.skip;
        const uint32_t tab = (iqbvh::bf16_up_bits(n.tA) << 16) | iqbvh::bf16_up_bits(n.tB);
        float4_storage w[4] = {{n.bmin[0], n.bmin[1], n.bmin[2], 0.0f},
                               {n.bmax[0], n.bmax[1], n.bmax[2], 0.0f},
                               {n.axis[0], n.axis[1], n.axis[2], n.edet},
                               {n.gR, n.gB, 0.0f, 0.0f}};
        std::memcpy(&w[0].w, &link, 4);
        std::memcpy(&w[1].w, &tab, 4);
        if (n.cos_beta > 0.0f && n.nmin > 0.0f) {
            w[3].z = iqbvh::round_down((double)n.cos_beta * (double)n.nmin);
            w[3].w = iqbvh::round_up((double)n.sin_beta * (double)n.nmin);
        }
        for (const float4_storage& v : w) out.nodes.push_back(v);
    }
    // leaf pairs in the kernel's pair layout (iqpt_internal.hpp), padding elements zero; the two
    // packet indices ride in the record's spare last two words (no separate index load per pair)
    const size_t npairs = bo.order.size() / 2;
    out.pairs.assign(npairs * iqpt::kTriPairFloat4, float4_storage{0.0f, 0.0f, 0.0f, 0.0f});
    for (size_t q = 0; q < bo.order.size(); ++q) {
        std::memcpy(&out.pairs[(q / 2) * iqpt::kTriPairFloat4 + 4].z + (q & 1), &bo.order[q], 4);
        if (bo.order[q] == ~0u) continue;
        const float4_storage* t = &tris[(size_t)bo.order[q] * iqpt::kTriFloat4];
        const float f[9] = {t[0].x, t[0].y, t[0].z, t[0].w, t[1].x, t[1].y, t[1].z, t[1].w, t[2].x};
        float* dst = &out.pairs[(q / 2) * iqpt::kTriPairFloat4].x;
        for (int comp = 0; comp < 9; ++comp) dst[2 * comp + (q & 1)] = f[comp];
    }
    return true;
}

// Exact sphere BVH (iq_bvh.hpp) over the world-space spheres (center.xyz, radius): spheres much larger
// than the median stay on the always-tested list. None for few spheres or coordinates beyond 2^60.
struct sbvh_host {
    std::vector<float4_storage> nodes, sph;
    std::vector<uint32_t> idx, always;
    float gulp;
};
constexpr uint32_t kSbvhMinSpheres = 64;
constexpr size_t kSbvhMaxSpheres = size_t(1) << 24;

bool build_sbvh(const std::vector<float4_storage>& sph, sbvh_host& out) {
    const size_t n = sph.size();
    // a leaf packs first << 8 | count (iq_bvh.hpp build_spheres): indices must stay below 2^24
    if (n < kSbvhMinSpheres || n >= kSbvhMaxSpheres) return false;
    std::vector<float> s4(4 * n), radii(n);
    double maxabs = 0.0;
    for (size_t k = 0; k < n; ++k) {
        const float v[4] = {sph[k].x, sph[k].y, sph[k].z, sph[k].w};
        for (int a = 0; a < 4; ++a) {
            if (!std::isfinite(v[a]) || std::fabs(v[a]) > 0x1p60f) return false;
            s4[4 * k + a] = v[a];
        }
        radii[k] = std::fabs(v[3]);
        for (int a = 0; a < 3; ++a) maxabs = std::max(maxabs, std::fabs((double)v[a]) + std::fabs((double)v[3]));
    }
    std::vector<float> sorted(radii);
    std::nth_element(sorted.begin(), sorted.begin() + n / 2, sorted.end());
    const double big = 8.0 * (double)sorted[n / 2];
    std::vector<uint32_t> ids;
    for (size_t k = 0; k < n; ++k) {
        if ((double)radii[k] > big) out.always.push_back((uint32_t)k);
        else ids.push_back((uint32_t)k);
    }
    std::vector<iqbvh::sph_node> nodes;
    std::vector<uint32_t> order;
    iqbvh::build_spheres(s4, ids, nodes, order);
    for (const iqbvh::sph_node& nd : nodes) {
        float4_storage lo, hi;
        lo.x = nd.bmin[0];
        lo.y = nd.bmin[1];
        lo.z = nd.bmin[2];
        std::memcpy(&lo.w, &nd.skip, 4);
        hi.x = nd.bmax[0];
        hi.y = nd.bmax[1];
        hi.z = nd.bmax[2];
        std::memcpy(&hi.w, &nd.first_count, 4);
        out.nodes.push_back(lo);
        out.nodes.push_back(hi);
        out.nodes.push_back(float4_storage{nd.rmin, nd.rmax, 0.0f, 0.0f});
    }
    for (uint32_t k : order) out.sph.push_back(sph[k]);
    out.idx = order;
    // a grown box side lo - g rounds to nearest: |error| <= 2^-24 (maxabs + g), covered by gulp and
    // the kernel's (1 + 2^-16) on g
    out.gulp = iqbvh::round_up(maxabs * 0x1p-22);
    return true;
}

}  // namespace

namespace iqpt::rt {

// Pixel-state planes between device tile-major storage and host compact row-major order
// (iqpt_internal.hpp): a device reorder into a temporary buffer plus one copy. Synchronises.
int fetch_compact(iqpt_ctx* c, const void* dev, uint32_t words, uint32_t planes, void* host) {
    const size_t bytes = (size_t)c->npix * words * planes * sizeof(uint32_t);
    if (bytes == 0) return IQPT_OK;
    void* tmp = nullptr;
    if (hipMalloc(&tmp, bytes) != hipSuccess) return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "readback buffer");
    hipError_t e = (hipError_t)iqpt::launch_relayout(c->stream, static_cast<const uint32_t*>(dev),
                                                      static_cast<uint32_t*>(tmp), c->ncols, c->set.nrows, words,
                                                      planes, true);
    if (e == hipSuccess) e = hipMemcpyAsync(host, tmp, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(tmp);
    return e == hipSuccess ? IQPT_OK : iqpt::hip_fail(e, "readback");
}

int store_compact(iqpt_ctx* c, const void* host, uint32_t words, uint32_t planes, void* dev) {
    const size_t bytes = (size_t)c->npix * words * planes * sizeof(uint32_t);
    if (bytes == 0) return IQPT_OK;
    void* tmp = nullptr;
    if (hipMalloc(&tmp, bytes) != hipSuccess) return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "upload buffer");
    hipError_t e = hipMemcpyAsync(tmp, host, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
        e = (hipError_t)iqpt::launch_relayout(c->stream, static_cast<const uint32_t*>(tmp), static_cast<uint32_t*>(dev),
                                              c->ncols, c->set.nrows, words, planes, false);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(tmp);
    return e == hipSuccess ? IQPT_OK : iqpt::hip_fail(e, "upload");
}

// The sum of the spread ray counters (iqpt_internal.hpp kRaySlots); the streams are synchronised.
int read_rays(iqpt_ctx* c, unsigned long long* total) {
    std::vector<unsigned long long> slots((size_t)iqpt::kRaySlots * iqpt::kRaySlotStride);
    IQPT_HIP(hipMemcpy(slots.data(), c->d_rays, slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long v = 0;
    for (uint32_t k = 0; k < iqpt::kRaySlots; ++k) v += slots[(size_t)k * iqpt::kRaySlotStride];
    *total = v;
    return IQPT_OK;
}

// After the context's streams are synchronised: read the kernels' error word and latch it (see
// iqpt_ctx::dev_err). Returns IQPT_ERR_HIP while an error is latched.
int check_dev_err(iqpt_ctx* c) {
    if (!c->dev_err) {
        uint32_t err = 0;
        IQPT_HIP(hipMemcpy(&err, c->d_ovl_err, sizeof err, hipMemcpyDeviceToHost));
        c->dev_err = err;
    }
    if (!c->dev_err) return IQPT_OK;
    return iqpt::fail(IQPT_ERR_HIP, std::string((c->dev_err & 4u) ? "launch: an XCD's tile list was never taken"
                                                                   : "overlapped launch: a per-tile wait timed out") +
                                        " (pixel state undefined until iqpt_checkpoint_load)");
}

hipEvent_t take_event(iqpt_ctx* c) {
    if (!c->timing_on) return nullptr;
    if (!c->event_pool.empty()) {
        hipEvent_t e = c->event_pool.back();
        c->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

}  // namespace iqpt::rt

extern "C" {

int iqpt_abi_version(void) { return IQPT_ABI_VERSION; }

const char* iqpt_error_string(int status) {
    switch (status) {
    case IQPT_OK: return "IQPT_OK";
    case IQPT_ERR_INVALID_ARG: return "IQPT_ERR_INVALID_ARG";
    case IQPT_ERR_HIP: return "IQPT_ERR_HIP";
    case IQPT_ERR_OUT_OF_MEMORY: return "IQPT_ERR_OUT_OF_MEMORY";
    case IQPT_ERR_NO_DEVICE: return "IQPT_ERR_NO_DEVICE";
    case IQPT_ERR_NOT_READY: return "IQPT_ERR_NOT_READY";
    case IQPT_ERR_UNSUPPORTED: return "IQPT_ERR_UNSUPPORTED";
    default: return "IQPT_ERR_UNKNOWN";
    }
}

const char* iqpt_last_error(void) { return iqpt::g_last_error.c_str(); }

const char* iqpt_kernel_name(void) { return iqpt::render_kernel_name(); }

int iqpt_create(int device, uint32_t width, uint32_t height, const iqpt_pixel_set* pixels, uint64_t seed,
                int max_depth, iqpt_ctx** out) {
    if (!out) return iqpt::fail(IQPT_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (width == 0 || height == 0 || width > 65535 || height > 65535)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "frame must be 1..65535 pixels per side (camera stores uint16)");
    if (max_depth < 1) return iqpt::fail(IQPT_ERR_INVALID_ARG, "max_depth must be >= 1");
    if (max_depth > IQPT_MAX_DEPTH_LIMIT)
        return iqpt::fail(IQPT_ERR_UNSUPPORTED, "max_depth above IQPT_MAX_DEPTH_LIMIT");
    iqpt_pixel_set ps = pixels ? *pixels : iqpt_pixel_set{0, width, 0, 1, height};
    if (ps.x1 <= ps.x0 || ps.x1 > width || ps.nrows == 0 || ps.ystep == 0 ||
        (uint64_t)ps.y0 + (uint64_t)(ps.nrows - 1) * ps.ystep >= height)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "pixel set outside the frame");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return iqpt::fail(IQPT_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= count) return iqpt::fail(IQPT_ERR_NO_DEVICE, "device index out of range");

    iqpt_ctx* c = new iqpt_ctx();
    c->device = device;
    c->width = width;
    c->height = height;
    c->set = ps;
    c->ncols = ps.x1 - ps.x0;
    c->npix = c->ncols * ps.nrows;
    c->seed = seed;
    c->max_depth = max_depth;
    auto cleanup = [&](int st) {
        iqpt_destroy(c);
        return st;
    };
    int st = use_device(c);
    if (st) return cleanup(st);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return cleanup(iqpt::fail(IQPT_ERR_HIP, "hipGetDeviceProperties"));
    c->num_cus = prop.multiProcessorCount;
    c->lds_per_block = (uint32_t)prop.sharedMemPerBlock;
    if (hipDeviceGetAttribute(&c->num_xcc, hipDeviceAttributeNumberOfXccs, device) != hipSuccess) {
        (void)hipGetLastError();
        c->num_xcc = 0;
    }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
        return cleanup(iqpt::fail(IQPT_ERR_HIP, "hipStreamCreate"));
    const size_t n = c->npix;
    if (hipMalloc(&c->d_lin, n * sizeof(float4_storage)) != hipSuccess ||
        hipMalloc(&c->d_bgra, n * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&c->d_rng, 6 * n * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&c->d_rays, iqpt::kRaySlots * iqpt::kRaySlotStride * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&c->d_queue, (4 + iqpt::kOverlapQueueWords) * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&c->d_ovl_err, sizeof(uint32_t)) != hipSuccess)
        return cleanup(iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "device allocation of the frame state failed"));
    c->d_bgra_own = c->d_bgra;
    // path_tracer.cu:134-135: both buffers start at zero
    if (hipMemsetAsync(c->d_lin, 0, n * sizeof(float4_storage), c->stream) != hipSuccess ||
        hipMemsetAsync(c->d_bgra, 0, n * sizeof(uint32_t), c->stream) != hipSuccess ||
        hipMemsetAsync(c->d_rays, 0, iqpt::kRaySlots * iqpt::kRaySlotStride * sizeof(unsigned long long), c->stream) != hipSuccess ||
        hipMemsetAsync(c->d_ovl_err, 0, sizeof(uint32_t), c->stream) != hipSuccess)
        return cleanup(iqpt::fail(IQPT_ERR_HIP, "hipMemsetAsync"));
    // renderer_init_kernel (path_tracer.cu:139): curand_init(seed, pixelid, 0)
    const std::vector<uint32_t>& tables = iqpt::xorwow_tables();
    uint32_t* d_tables = nullptr;
    if (hipMalloc(&d_tables, tables.size() * sizeof(uint32_t)) != hipSuccess)
        return cleanup(iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "jump tables"));
    hipError_t e = hipMemcpyAsync(d_tables, tables.data(), tables.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
    int lst = e == hipSuccess ? iqpt::launch_rng_init(c->stream, width, ps.x0, c->ncols, ps.y0, ps.ystep, ps.nrows,
                                                      seed, d_tables, c->d_rng)
                              : (int)e;
    hipError_t se = hipStreamSynchronize(c->stream);
    (void)hipFree(d_tables);
    if (lst != 0) return cleanup(iqpt::hip_fail((hipError_t)lst, "rng init kernel"));
    if (se != hipSuccess) return cleanup(iqpt::hip_fail(se, "rng init sync"));
    *out = c;
    return IQPT_OK;
}

int iqpt_destroy(iqpt_ctx* c) {
    if (!c) return IQPT_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    if (c->stream3) (void)hipStreamSynchronize(c->stream3);
    free_comm(c);
    free_scene(c);
    dev_free(c->d_lin);
    if (c->d_bgra_own) dev_free(c->d_bgra_own);
    else dev_free(c->d_bgra);                            // (a context whose creation failed half way)
    dev_free(c->d_alt_own);
    for (int i = 0; i < iqpt::kPipeRing; ++i) {
        dev_free(c->d_pring[i]);
        event_free(c->pev[i]);
    }
    dev_free(c->d_rng);
    dev_free(c->d_rays);
    dev_free(c->d_queue);
    for (uint32_t** b : {&c->d_tile_done, &c->d_xcd_order, &c->d_xcd_band, &c->d_ovl_err}) dev_free(*b);
    event_free(c->ev_pre);
    event_free(c->ev_s2);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->stream3) (void)hipStreamDestroy(c->stream3);
    event_free(c->ev_pipe_end);
    free_split(c);
    dev_free(c->d_spec);
    dev_free(c->d_spec_res);
    dev_free(c->d_spec_tl);
    dev_free(c->d_spec_plan);
    for (uint32_t** b : {&c->h_spec_rho, &c->h_spec_plan})
        if (*b) (void)hipHostFree(*b);
    for (hipEvent_t* e : {&c->ev_spec_rho, &c->ev_spec_plan}) event_free(*e);
    dev_free(c->d_stats);
    dev_free(c->d_cull);
    dev_free(c->d_certain);
    dev_free(c->d_sky_tiles);
    event_free(c->ev_sky);
    dev_free(c->d_tile_order);
    dev_free(c->d_list);
    dev_free(c->d_pmask);
    for (auto& tl : c->timed)
        for (hipEvent_t* ev : {&tl.e0, &tl.e1, &tl.e1b}) event_free(*ev);
    for (hipEvent_t& ev : c->event_pool) event_free(ev);
    for (hipEvent_t& ev : c->tune_ev) event_free(ev);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return IQPT_OK;
}

int iqpt_set_camera(iqpt_ctx* c, const iqpt_camera* cam) {
    if (!c || !cam) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (cam->width != c->width || cam->height != c->height)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "camera size differs from the context frame");
    // an interactive loop sets the camera every frame: the same view keeps its tile masks and the
    // camera-ray path decision (only a changed view is binned and timed again)
    if (c->have_camera && std::memcmp(&c->cam, cam, sizeof *cam) == 0) return IQPT_OK;
    c->cam = *cam;   // passed by value to every launch: no device copy to race with
    c->have_camera = true;
    c->cull_valid = false;
    c->tune_stage = 0;              // the faster camera-ray path depends on the view: time it again
    return IQPT_OK;
}

int iqpt_upload_packet(iqpt_ctx* c, const iqpt_packet_desc* pk) {
    if (!c || !pk) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    const uint32_t ntdc = pk->num_drawcalls[IQPT_MESH_TRIANGLES];
    const uint32_t nsdc = pk->num_drawcalls[IQPT_MESH_SPHERES];
    if ((ntdc && !pk->tri_mesh_dcs) || (nsdc && !pk->sphere_dcs) || (pk->num_tri_meshes && !pk->tri_meshes))
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "packet array is NULL");
    // world-space relayout (the ray-independent part of path_tracer.cu:257-270)
    std::vector<float4_storage> tris, shade, sph;
    uint64_t total = 0;
    for (uint32_t i = 0; i < ntdc; ++i) {
        const uint32_t id = pk->tri_mesh_dcs[i].mesh_id;
        if (id >= pk->num_tri_meshes)
            return iqpt::fail(IQPT_ERR_INVALID_ARG, "tri drawcall " + std::to_string(i) + ": mesh_id out of range");
        const iqpt_tri_mesh& m = pk->tri_meshes[id];
        if (m.num_indices % 3 != 0)
            return iqpt::fail(IQPT_ERR_INVALID_ARG, "mesh " + std::to_string(id) + ": num_indices not a multiple of 3");
        if (m.num_indices && (!m.indices || !m.vertices))
            return iqpt::fail(IQPT_ERR_INVALID_ARG, "mesh " + std::to_string(id) + ": NULL arrays");
        total += m.num_indices / 3;
    }
    if (total > 0xffffffffull / 4) return iqpt::fail(IQPT_ERR_INVALID_ARG, "too many triangles");
    // sphere indices, pair counts ((n + 1) / 2) and mask words are 32-bit in the kernels
    if (nsdc > 0xffffffffu / 4) return iqpt::fail(IQPT_ERR_INVALID_ARG, "too many spheres");
    // material table (iqpt.h): indices in range, known types
    if (pk->materials) {
        if ((ntdc && !pk->tri_dc_material) || (nsdc && !pk->sphere_dc_material))
            return iqpt::fail(IQPT_ERR_INVALID_ARG, "material table without per-drawcall indices");
        for (uint32_t i = 0; i < ntdc; ++i)
            if (pk->tri_dc_material[i] >= pk->num_materials)
                return iqpt::fail(IQPT_ERR_INVALID_ARG, "tri drawcall " + std::to_string(i) + ": material out of range");
        for (uint32_t i = 0; i < nsdc; ++i)
            if (pk->sphere_dc_material[i] >= pk->num_materials)
                return iqpt::fail(IQPT_ERR_INVALID_ARG, "sphere drawcall " + std::to_string(i) + ": material out of range");
        for (uint32_t k = 0; k < pk->num_materials; ++k)
            if (pk->materials[k].type != IQPT_MAT_EMISSIVE && pk->materials[k].type != IQPT_MAT_OREN_NAYAR)
                return iqpt::fail(IQPT_ERR_INVALID_ARG, "material " + std::to_string(k) + ": unknown type");
    }
    tris.reserve(total * iqpt::kTriFloat4);
    shade.reserve(total * 3);
    for (uint32_t i = 0; i < ntdc; ++i) {
        const iqpt_tri_mesh_drawcall& dc = pk->tri_mesh_dcs[i];
        const iq::mat4 M = iq::mat4::from(dc.transform);
        const iq::mat4 N = iq::normal_matrix(M);                     // path_tracer.cu:260
        const iqpt_tri_mesh& m = pk->tri_meshes[dc.mesh_id];
        for (uint32_t j = 0; j < m.num_indices; j += 3) {
            const uint32_t ia = m.indices[j], ib = m.indices[j + 1], ic = m.indices[j + 2];
            if (ia >= m.num_vertices || ib >= m.num_vertices || ic >= m.num_vertices)
                return iqpt::fail(IQPT_ERR_INVALID_ARG, "mesh " + std::to_string(dc.mesh_id) + ": index out of range");
            const iqpt_vertex& a = m.vertices[ia];
            const iqpt_vertex& b = m.vertices[ib];
            const iqpt_vertex& cc = m.vertices[ic];
            const iq::vec4 v0 = iq::transformed(iq::load3(a.pos, iq::usage::POINT), M);
            const iq::vec4 v1 = iq::transformed(iq::load3(b.pos, iq::usage::POINT), M);
            const iq::vec4 v2 = iq::transformed(iq::load3(cc.pos, iq::usage::POINT), M);
            const iq::vec4 n0 = iq::transformed(iq::load3(a.normal, iq::usage::DIRECTION), N);
            const iq::vec4 n1 = iq::transformed(iq::load3(b.normal, iq::usage::DIRECTION), N);
            const iq::vec4 n2 = iq::transformed(iq::load3(cc.normal, iq::usage::DIRECTION), N);
            const iq::vec4 e1 = v1 - v0, e2 = v2 - v0;               // shape.cu:65-66
            const iq::vec4 ng = iq::cross3(e1, e2);                  // shape.cu:98
            tris.push_back({v0.x, v0.y, v0.z, e1.x});
            tris.push_back({e1.y, e1.z, e2.x, e2.y});
            tris.push_back({e2.z, 0.0f, 0.0f, 0.0f});
            shade.push_back({n0.x, n0.y, n0.z, ng.x});
            shade.push_back({n1.x, n1.y, n1.z, ng.y});
            shade.push_back({n2.x, n2.y, n2.z, ng.z});
        }
    }
    for (uint32_t i = 0; i < nsdc; ++i) {
        const iqpt_sphere_drawcall& s = pk->sphere_dcs[i];
        sph.push_back({s.center[0], s.center[1], s.center[2], s.radius});
    }
    // material records: (albedo.rgb, type bits), (strength | sigma, A, B, 0) with the Oren-Nayar
    // constants of material.cu:22-24 evaluated here by the same IEEE operations (sigma clamped to
    // [0, 1] as the oren_nayar constructor does, material.h:25-29)
    std::vector<float4_storage> mats;
    std::vector<uint32_t> tri_mat, sph_mat;
    if (pk->materials) {
        for (uint32_t k = 0; k < pk->num_materials; ++k) {
            const iqpt_material& m = pk->materials[k];
            float tbits;
            std::memcpy(&tbits, &m.type, 4);
            mats.push_back({m.albedo[0], m.albedo[1], m.albedo[2], tbits});
            if (m.type == IQPT_MAT_EMISSIVE) {
                mats.push_back({m.param, 0.0f, 0.0f, 0.0f});
            } else {
                const float sigma = m.param < 0.0f ? 0.0f : (m.param > 1.0f ? 1.0f : m.param);
                const float sigma2 = sigma * sigma;
                const float A = 1.0f - 0.5f * sigma2 / (sigma2 + 0.33f);
                const float B = 0.45f * sigma2 / (sigma2 + 0.09f);
                mats.push_back({sigma, A, B, 0.0f});
            }
        }
        for (uint32_t i = 0; i < ntdc; ++i) {
            const iqpt_tri_mesh& m = pk->tri_meshes[pk->tri_mesh_dcs[i].mesh_id];
            tri_mat.insert(tri_mat.end(), m.num_indices / 3, pk->tri_dc_material[i]);
        }
        sph_mat.assign(pk->sphere_dc_material, pk->sphere_dc_material + nsdc);
    }
    // kOptFastDiv (iq_fastdiv.h): iq_rcp is exact for |x| in [2^-126, 2^126) and for 0, inf, NaN.
    // Möller–Trumbore determinants are |e1 . (dir x e2)| <= |e1| |e2| (|dir| = 1) < 2^126 when every
    // finite edge component is within 2^60 (a non-finite component makes det inf or NaN), and sphere
    // radii must be 0, non-finite or in [2^-126, 2^126).
    bool fast_rcp_ok = true;
    auto big = [](float v) { return std::isfinite(v) && std::fabs(v) > 0x1p60f; };
    for (uint64_t k = 0; k < total && fast_rcp_ok; ++k) {
        const float4_storage* t = &tris[k * iqpt::kTriFloat4];
        fast_rcp_ok = !(big(t[0].w) || big(t[1].x) || big(t[1].y) || big(t[1].z) || big(t[1].w) || big(t[2].x));
    }
    for (const float4_storage& s : sph) {
        const float r = std::fabs(s.w);
        if (std::isfinite(r) && r != 0.0f && (r < 0x1p-126f || r >= 0x1p126f)) fast_rcp_ok = false;
    }
    // pair layouts (iqpt_internal.hpp): SoA inside each pair of consecutive primitives
    std::vector<float4_storage> tri_pairs, sph_pairs;
    const size_t ntp = (total + 1) / 2, nsp = ((size_t)nsdc + 1) / 2;
    tri_pairs.resize(ntp * iqpt::kTriPairFloat4, float4_storage{0.0f, 0.0f, 0.0f, 0.0f});
    for (size_t k = 0; k < total; ++k) {
        const float4_storage* t = &tris[k * iqpt::kTriFloat4];
        const float f[9] = {t[0].x, t[0].y, t[0].z, t[0].w, t[1].x, t[1].y, t[1].z, t[1].w, t[2].x};
        float* dst = &tri_pairs[(k / 2) * iqpt::kTriPairFloat4].x;     // 20 floats, component c at 2c + (k & 1)
        for (int comp = 0; comp < 9; ++comp) dst[2 * comp + (k & 1)] = f[comp];
    }
    sph_pairs.resize(nsp * iqpt::kSphPairFloat4, float4_storage{0.0f, 0.0f, 0.0f, 0.0f});
    for (size_t k = 0; k < nsdc; ++k) {
        const float f[4] = {sph[k].x, sph[k].y, sph[k].z, sph[k].w};
        float* dst = &sph_pairs[(k / 2) * iqpt::kSphPairFloat4].x;
        for (int comp = 0; comp < 4; ++comp) dst[2 * comp + (k & 1)] = f[comp];
    }
    int st = enter(c);
    if (st) return st;
    IQPT_HIP(hipStreamSynchronize(c->stream));   // a render in flight may still read the old scene
    free_scene(c);
    c->have_packet = false;
    auto upload = [&](const std::vector<float4_storage>& v, float4_storage** dst) -> int {
        if (v.empty()) return IQPT_OK;
        if (hipMalloc(dst, v.size() * sizeof(float4_storage)) != hipSuccess)
            return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "scene allocation");
        IQPT_HIP(hipMemcpy(*dst, v.data(), v.size() * sizeof(float4_storage), hipMemcpyHostToDevice));
        return IQPT_OK;
    };
    bvh_host bvh;
    const bool have_bvh = build_bvh(tris, sph, bvh);
    sbvh_host sbvh;
    const bool have_sbvh = build_sbvh(sph, sbvh);
    auto upload_u32 = [&](const std::vector<uint32_t>& v, uint32_t** dst) -> int {
        if (v.empty()) return IQPT_OK;
        if (hipMalloc(dst, v.size() * sizeof(uint32_t)) != hipSuccess)
            return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "material index allocation");
        IQPT_HIP(hipMemcpy(*dst, v.data(), v.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        return IQPT_OK;
    };
    if ((st = upload(tris, &c->d_tris)) || (st = upload(tri_pairs, &c->d_tri_pairs)) ||
        (st = upload(shade, &c->d_tri_shade)) || (st = upload(sph, &c->d_sph)) ||
        (st = upload(sph_pairs, &c->d_sph_pairs)) || (st = upload(mats, &c->d_mats)) ||
        (st = upload_u32(tri_mat, &c->d_tri_mat)) || (st = upload_u32(sph_mat, &c->d_sph_mat)) ||
        (have_bvh && ((st = upload(bvh.nodes, &c->d_bvh_nodes)) || (st = upload(bvh.pairs, &c->d_bvh_pairs)) ||
                      (st = upload_u32(bvh.always, &c->d_bvh_always)))) ||
        (have_sbvh && ((st = upload(sbvh.nodes, &c->d_sbvh_nodes)) || (st = upload(sbvh.sph, &c->d_sbvh_sph)) ||
                       (st = upload_u32(sbvh.idx, &c->d_sbvh_idx)) ||
                       (st = upload_u32(sbvh.always, &c->d_sbvh_always))))) {
        free_scene(c);
        return st;
    }
    if (have_sbvh) {
        c->sbvh_nnodes = (uint32_t)(sbvh.nodes.size() / iqpt::kSphNodeFloat4);
        c->sbvh_nalways = (uint32_t)sbvh.always.size();
        c->sbvh_gulp = sbvh.gulp;
    }
    if (have_bvh) {
        c->bvh_nnodes = (uint32_t)(bvh.nodes.size() / iqpt::kBvhNodeFloat4);
        c->bvh_nalways = (uint32_t)bvh.always.size();
        c->bvh_md = bvh.md;
        c->bvh_gulp = bvh.gulp;
    }
    c->ntri = (uint32_t)total;
    c->nsph = nsdc;
    c->h_sph = sph;
    c->fast_rcp_ok = fast_rcp_ok;
    c->have_packet = true;
    return IQPT_OK;
}

int iqpt_sync(iqpt_ctx* c) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    int st = enter(c);
    if (st) return st;
    IQPT_HIP(hipStreamSynchronize(c->stream));
    // a per-tile wait that gave up or a chain wave past its bound (never expected) leaves the frame
    // undefined: report it (and keep reporting it, iqpt_ctx::dev_err)
    return check_dev_err(c);
}

int iqpt_reset(iqpt_ctx* c) {                                       // path_tracer.cu:394-400
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    int st = enter(c);
    if (st) return st;
    IQPT_HIP(hipStreamSynchronize(c->stream));
    IQPT_HIP(hipMemsetAsync(c->d_bgra, 0, (size_t)c->npix * sizeof(uint32_t), c->stream));
    IQPT_HIP(hipStreamSynchronize(c->stream));
    c->frame = 0;
    return IQPT_OK;
}

int iqpt_read(iqpt_ctx* c, float* lin_rgba, uint8_t* bgra) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    int st = enter(c);
    if (st) return st;
    if (lin_rgba && (st = fetch_compact(c, c->d_lin, 4, 1, lin_rgba)) != IQPT_OK) return st;
    // the BGRA8 frame is stored in compact order already (tile_to_compact)
    if (bgra) IQPT_HIP(hipMemcpyAsync(bgra, c->d_bgra, (size_t)c->npix * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                      c->stream));
    IQPT_HIP(hipStreamSynchronize(c->stream));
    return check_dev_err(c);
}

int iqpt_read_rng(iqpt_ctx* c, uint32_t* states) {
    if (!c || !states) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    int st = enter(c);
    if (st) return st;
    std::vector<uint32_t> planes((size_t)c->npix * 6);
    if ((st = fetch_compact(c, c->d_rng, 1, 6, planes.data())) != IQPT_OK) return st;
    if ((st = check_dev_err(c)) != IQPT_OK) return st;
    for (size_t p = 0; p < c->npix; ++p)
        for (int k = 0; k < 6; ++k) states[p * 6 + k] = planes[(size_t)k * c->npix + p];
    return IQPT_OK;
}

int iqpt_copy_accum_device(iqpt_ctx* c, void* dst_device, size_t bytes) {
    if (!c || !dst_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (bytes < (size_t)c->npix * sizeof(float4_storage)) return iqpt::fail(IQPT_ERR_INVALID_ARG, "destination too small");
    int st = enter(c);
    if (st) return st;
    const int le = iqpt::launch_relayout(c->stream, reinterpret_cast<const uint32_t*>(c->d_lin),
                                         static_cast<uint32_t*>(dst_device), c->ncols, c->set.nrows, 4, 1, true);
    if (le != 0) return iqpt::hip_fail((hipError_t)le, "accumulator reorder");
    IQPT_HIP(hipStreamSynchronize(c->stream));
    return check_dev_err(c);
}

int iqpt_num_pixels(const iqpt_ctx* c, uint64_t* npix) {
    if (!c || !npix) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    *npix = c->npix;
    return IQPT_OK;
}

int iqpt_frame_count(const iqpt_ctx* c, uint64_t* frames) {
    if (!c || !frames) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    *frames = c->frame;
    return IQPT_OK;
}

int iqpt_rays_traced(iqpt_ctx* c, uint64_t* rays) {
    if (!c || !rays) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    int st = enter(c);
    if (st) return st;
    IQPT_HIP(hipStreamSynchronize(c->stream));
    unsigned long long v = 0;
    if ((st = read_rays(c, &v)) != IQPT_OK) return st;
    *rays = v;
    return IQPT_OK;
}

int iqpt_kernel_time(iqpt_ctx* c, double* total_ms, uint64_t* launches) {
    if (!c || !total_ms || !launches) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    int st = enter(c);
    if (st) return st;
    IQPT_HIP(hipStreamSynchronize(c->stream));
    c->end1 = c->end2 = nullptr;        // (the events go back to the pool)
    double sum = 0.0, span = 0.0;
    for (auto& tl : c->timed) {
        float ms = 0.0f, end = 0.0f;
        IQPT_HIP(hipEventElapsedTime(&ms, tl.e0, tl.e1));
        // span: from the first launch's start to the latest end (launches on two streams overlap)
        IQPT_HIP(hipEventElapsedTime(&end, c->timed.front().e0, tl.e1));
        if (tl.e1b) {
            float ms2 = 0.0f, end2 = 0.0f;
            IQPT_HIP(hipEventElapsedTime(&ms2, tl.e0, tl.e1b));
            IQPT_HIP(hipEventElapsedTime(&end2, c->timed.front().e0, tl.e1b));
            ms = std::max(ms, ms2);
            end = std::max(end, end2);
            c->event_pool.push_back(tl.e1b);
        }
        sum += ms;
        span = std::max(span, (double)end);
        c->event_pool.push_back(tl.e0);
        c->event_pool.push_back(tl.e1);
    }
    c->last_span_ms = span;
    *total_ms = sum;
    *launches = c->timed.size();
    c->timed.clear();
    return IQPT_OK;
}

int iqpt_copy_frame_device(iqpt_ctx* c, void* dst_device, size_t bytes) {
    if (!c || !dst_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (bytes < (size_t)c->npix * sizeof(uint32_t)) return iqpt::fail(IQPT_ERR_INVALID_ARG, "destination too small");
    int st = enter(c);
    if (st) return st;
    IQPT_HIP(hipMemcpyAsync(dst_device, c->d_bgra, (size_t)c->npix * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                            c->stream));                    // compact order already
    IQPT_HIP(hipStreamSynchronize(c->stream));
    return check_dev_err(c);
}

// The stream-ordered frame copy (iqpt_copy_frame_device_async, the gather's send copy): the BGRA8 frame in
// compact order into dst, behind every render issued so far; `wait` (if not null) is waited for on the copy's
// stream first; *used = that stream.
// Pipelined launches, from the first copy or gather behind one on: the ring of frame buffers the launches write
// in turn (each of frame_words(c): the multi-GPU gather sends a launch's buffer as it is).
int ensure_ring(iqpt_ctx* c) {
    if (c->pring_on) return IQPT_OK;
    for (int i = 0; i < iqpt::kPipeRing; ++i) {
        if ((!c->d_pring[i] && hipMalloc(&c->d_pring[i], frame_words(c) * sizeof(uint32_t)) != hipSuccess) ||
            (!c->pev[i] && hipEventCreateWithFlags(&c->pev[i], hipEventDisableTiming) != hipSuccess)) {
            (void)hipGetLastError();
            return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "frame buffers for pipelined copies");
        }
        c->pseq[i] = 0;
    }
    c->pidx = iqpt::kPipeRing - 1;     // the next launch writes d_pring[0]
    c->pring_on = true;
    return IQPT_OK;
}

int copy_frame_async(iqpt_ctx* c, uint32_t* dst, hipEvent_t wait, hipStream_t* used) {
    // no synchronisation here: an error the kernels raise for this launch is reported by the next
    // synchronising call (iqpt_sync, iqpt_read, ...); one already latched fails the copy now
    if (c->dev_err) return check_dev_err(c);
    int st = IQPT_OK;
    hipStream_t cs = c->stream;
    if (c->pipe) {
        // pipelined spec launches: the copy on stream3 behind both kernels of the last launch; from here on
        // the launches write the ring of frame buffers in turn
        if ((st = ensure_ring(c)) != IQPT_OK) return st;
        if ((st = ensure_copy_stream(c)) != IQPT_OK) return st;
        // a gather in flight read an earlier ring buffer: keep the ring's reuse events in one order
        if (c->comm_pend) IQPT_HIP(hipStreamWaitEvent(c->stream3, c->ev_gend, 0));
        if (!c->end1) IQPT_HIP(hipEventRecord(c->ev_pipe_end, c->stream));
        if (!c->end2) IQPT_HIP(hipEventRecord(c->ev_s2, c->stream2));
        IQPT_HIP(hipStreamWaitEvent(c->stream3, c->end1 ? c->end1 : c->ev_pipe_end, 0));
        IQPT_HIP(hipStreamWaitEvent(c->stream3, c->end2 ? c->end2 : c->ev_s2, 0));
        if (wait) IQPT_HIP(hipStreamWaitEvent(c->stream3, wait, 0));
        IQPT_HIP(hipMemcpyAsync(dst, c->d_bgra, (size_t)c->npix * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream3));
        c->copy_seq += 1;
        IQPT_HIP(hipEventRecord(c->pev[c->copy_seq % iqpt::kPipeRing], c->stream3));
        if (c->d_bgra == c->d_pring[c->pidx]) c->pseq[c->pidx] = c->copy_seq;
        *used = c->stream3;
        return IQPT_OK;
    }
    if (c->last_ovl && c->last_ls) {
        // overlapped launches in flight: copy on the last launch's stream without joining, so the next
        // launch still overlaps this one (from here on overlapped launches alternate two frame buffers)
        if (!c->d_bgra_alt) {
            if (hipMalloc(&c->d_bgra_alt, frame_words(c) * sizeof(uint32_t)) != hipSuccess) {
                (void)hipGetLastError();
                c->d_bgra_alt = nullptr;
                return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "second frame buffer for overlapped copies");
            }
            c->d_alt_own = c->d_bgra_alt;
        }
        cs = c->last_ls;
        if (cs == c->stream2) c->s2_pending = true;
    } else if ((st = join_streams(c)) != IQPT_OK) {
        return st;
    }
    if (wait) IQPT_HIP(hipStreamWaitEvent(cs, wait, 0));
    IQPT_HIP(hipMemcpyAsync(dst, c->d_bgra, (size_t)c->npix * sizeof(uint32_t), hipMemcpyDeviceToDevice, cs));
    *used = cs;
    return IQPT_OK;
}

int iqpt_copy_frame_device_async(iqpt_ctx* c, void* dst_device, size_t bytes) {
    if (!c || !dst_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (bytes < (size_t)c->npix * sizeof(uint32_t)) return iqpt::fail(IQPT_ERR_INVALID_ARG, "destination too small");
    int st = use_device(c);
    if (st) return st;
    hipStream_t used = nullptr;
    return copy_frame_async(c, static_cast<uint32_t*>(dst_device), nullptr, &used);
}

int iqpt_frame_stream(iqpt_ctx* c, void** stream) {
    if (!c || !stream) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    // pipelined launches: the copy stream exists from the launch's end on (pipe_end), so the stream named
    // here is the one the next copy goes on (it used to appear only at the first copy)
    if (c->pipe) {
        int st = use_device(c);
        if (st) return st;
        if ((st = ensure_copy_stream(c)) != IQPT_OK) return st;
    }
    *stream = (void*)(c->pipe ? c->stream3 : ((c->last_ovl && c->last_ls) ? c->last_ls : c->stream));
    return IQPT_OK;
}

int iqpt_stream(iqpt_ctx* c, void** stream) {
    if (!c || !stream) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    int st = enter(c);
    if (st) return st;
    *stream = (void*)c->stream;
    return IQPT_OK;
}

int iqpt_prepare(iqpt_ctx* c) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    if (!c->have_camera || !c->have_packet) return iqpt::fail(IQPT_ERR_NOT_READY, "camera and packet must be set");
    int st = enter(c);
    if (st) return st;
    if ((c->opt & iqpt::kOptPair) && (c->opt & iqpt::kOptCull) && (c->ntri + c->nsph) > 0 && !c->cull_valid &&
        (st = build_cull(c)) != IQPT_OK)
        return st;
    IQPT_HIP(hipStreamSynchronize(c->stream));
    return IQPT_OK;
}

int iqpt_kernel_span(const iqpt_ctx* c, double* span_ms) {
    if (!c || !span_ms) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    *span_ms = c->last_span_ms;
    return IQPT_OK;
}
int iqpt_set_overlap(iqpt_ctx* c, int mode) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    if (mode != IQPT_OVERLAP_OFF && mode != IQPT_OVERLAP_AUTO)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "overlap mode must be IQPT_OVERLAP_OFF or _AUTO");
    int st = enter(c);
    if (st) return st;
    c->overlap_mode = mode;
    return IQPT_OK;
}
int iqpt_set_split(iqpt_ctx* c, int mode) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    if (mode == IQPT_SPLIT_CHAIN || mode == IQPT_SPLIT_FAN)
        return iqpt::fail(IQPT_ERR_UNSUPPORTED, "CHAIN and FAN launches were archived in round 6 (branch round6-ab-archive)");
    if (mode != IQPT_SPLIT_AUTO && mode != IQPT_SPLIT_OFF && mode != IQPT_SPLIT_ON && mode != IQPT_SPLIT_SPEC)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "split mode must be IQPT_SPLIT_AUTO, _OFF, _ON or _SPEC");
    c->split_mode = mode;
    return IQPT_OK;
}

int iqpt_write_ppm(const char* path, uint32_t width, uint32_t height, const uint8_t* bgra) {
    if (!path || !bgra || !width || !height) return iqpt::fail(IQPT_ERR_INVALID_ARG, "bad PPM arguments");
    FILE* f = std::fopen(path, "wb");
    if (!f) return iqpt::fail(IQPT_ERR_INVALID_ARG, std::string("cannot open ") + path);
    std::fprintf(f, "P6\n%u %u\n255\n", width, height);
    std::vector<uint8_t> row((size_t)width * 3);
    for (uint32_t y = 0; y < height; ++y) {
        const uint8_t* src = bgra + (size_t)y * width * 4;
        for (uint32_t x = 0; x < width; ++x) {
            row[x * 3 + 0] = src[x * 4 + 2];
            row[x * 3 + 1] = src[x * 4 + 1];
            row[x * 3 + 2] = src[x * 4 + 0];
        }
        std::fwrite(row.data(), 1, row.size(), f);
    }
    std::fclose(f);
    return IQPT_OK;
}

}  // extern "C"
