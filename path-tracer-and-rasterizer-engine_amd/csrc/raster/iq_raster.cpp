// iq_raster.cpp — the iqpt_raster_* C ABI (include/raster/iqpt_raster.h): device buffers, scene upload and
// the draw sequence vertex -> setup -> (counter readback) -> bin -> sort -> tiles on the rasterizer's own
// stream. The kernels are iq_raster_kernels.hip; the pipeline is DESIGN.md §9.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "iq_host_math.hpp"
#include "post/iq_post.hpp"
#include "raster/iq_raster.hpp"
#include "raster/iqpt_raster.h"

namespace {

// a device buffer that only grows
struct dbuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t reserve(size_t want) {
        if (want <= bytes) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        const hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) bytes = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// what a draw consumes: draws, their prefix ends, the index pool and the transformed vertices
struct geometry {
    dbuf draws, vend, tend, indices, mesh_verts, clip, wn;
    uint32_t ndraws = 0, nverts = 0, ntris = 0;
    bool transformed = false;     // clip / wn hold the current camera's vertices
    void release() {
        for (dbuf* b : {&draws, &vend, &tend, &indices, &mesh_verts, &clip, &wn}) b->release();
    }
};

// what a tile kernel consumes: the set-up records, the sorted (tile, record) pairs ([1] after the sort) and the
// tiles' ranges. A draw and a G-buffer pass each keep their own, so neither disturbs the other's.
struct lists {
    dbuf recs, keys[2], vals[2], ranges;
    void release() {
        for (dbuf* b : {&recs, &keys[0], &keys[1], &vals[0], &vals[1], &ranges}) b->release();
    }
};

constexpr int kEvents = 6;

}  // namespace

struct iqpt_raster {
    int device = 0;
    hipStream_t stream = nullptr;
    iqr::frame_params fp{};
    bool have_camera = false, have_scene = false, have_frame = false;
    dbuf camera;                  // view[16], projection[16]
    iqpt_camera host_camera{};    // the camera as it was given (iqr::current_camera)
    geometry scene, direct;       // the uploaded scene; the vertices of the last draw_clip
    dbuf cnt, frame, depth_samples, prim_samples, sort_temp;
    lists draw_lists;             // of the last draw (iqpt_raster_read re-runs its tile kernel over them)
    lists guide_lists;            // of the G-buffer pass
    dbuf guide_nz, guide_id;      // the G-buffer: float4 (n, z) and the draw index per pixel
    bool have_gbuffer = false;    // guide_* hold the uploaded scene through the current camera
    hipEvent_t guide_ev[2] = {};
    bool guide_pending = false;
    double guide_ms = 0.0;
    uint64_t guide_passes = 0;
    iqr::counters* host_cnt = nullptr;    // pinned
    uint32_t last_nrec = 0, last_npairs = 0, last_ntris = 0;
    hipEvent_t ev[kEvents] = {};
    bool pending = false;         // the events of the last draw have not been added up yet
    double total_ms = 0.0, stage_ms[5] = {};
    uint64_t draws = 0;
};

namespace {

int set_device(iqpt_raster* r) {
    IQPT_HIP(hipSetDevice(r->device));
    return IQPT_OK;
}

int collect(iqpt_raster* r) {
    if (!r->pending) return IQPT_OK;
    IQPT_HIP(hipEventSynchronize(r->ev[kEvents - 1]));
    float ms = 0.0f;
    for (int k = 0; k < 5; ++k) {
        IQPT_HIP(hipEventElapsedTime(&ms, r->ev[k], r->ev[k + 1]));
        r->stage_ms[k] += ms;
    }
    IQPT_HIP(hipEventElapsedTime(&ms, r->ev[0], r->ev[kEvents - 1]));
    r->total_ms += ms;
    r->draws += 1;
    r->pending = false;
    return IQPT_OK;
}

// the same for the last G-buffer pass
int collect_guide(iqpt_raster* r) {
    if (!r->guide_pending) return IQPT_OK;
    IQPT_HIP(hipEventSynchronize(r->guide_ev[1]));
    float ms = 0.0f;
    IQPT_HIP(hipEventElapsedTime(&ms, r->guide_ev[0], r->guide_ev[1]));
    r->guide_ms += ms;
    r->guide_pending = false;
    return IQPT_OK;
}

int upload(dbuf& b, const void* src, size_t bytes, hipStream_t s) {
    IQPT_HIP(b.reserve(std::max<size_t>(bytes, 16)));
    if (bytes) IQPT_HIP(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s));
    return IQPT_OK;
}

// Setup, binning, sort and tile ranges of geometry g into the lists l, on the rasterizer's stream. guide: the
// G-buffer's doubled index list, whose submission indices run to 2 ntris. ev (may be NULL): two
// events, recorded after the setup and after the binning.
int build_lists(iqpt_raster* r, geometry& g, const iqr::frame_params& fp, bool guide, lists& l, hipEvent_t* ev,
                uint32_t& nrec, uint32_t& npairs) {
    hipStream_t s = r->stream;
    const uint32_t nsub = guide ? 2 * g.ntris : g.ntris;
    // setup: records and pair positions are claimed with two counters; a record buffer that proves too small
    // is grown to the count the pass reported and the pass is redone (never a silent limit)
    nrec = npairs = 0;
    if (g.ntris) {
        size_t cap = std::max<size_t>(l.recs.bytes / sizeof(iqr::setup_rec), 1024);
        for (int attempt = 0;; ++attempt) {
            IQPT_HIP(l.recs.reserve(cap * sizeof(iqr::setup_rec)));
            IQPT_HIP(hipMemsetAsync(r->cnt.p, 0, sizeof(iqr::counters), s));
            IQPT_HIP((guide ? iqr::launch_setup_guide : iqr::launch_setup)(
                s, fp, g.draws.as<iqr::draw_rec>(), g.ndraws, g.tend.as<uint32_t>(), g.ntris, g.indices.as<uint32_t>(),
                g.clip.as<float>(), g.wn.as<float>(), l.recs.as<iqr::setup_rec>(),
                (uint32_t)std::min<size_t>(cap, 0xffffffffu), r->cnt.as<iqr::counters>()));
            IQPT_HIP(hipMemcpyAsync(r->host_cnt, r->cnt.p, sizeof(iqr::counters), hipMemcpyDeviceToHost, s));
            IQPT_HIP(hipStreamSynchronize(s));
            if (r->host_cnt->npairs >= 0xffffffffull || r->host_cnt->nrec >= 0xffffffffull)
                return iqpt::fail(IQPT_ERR_UNSUPPORTED, "more than 2^32 (tile, triangle) pairs in one frame");
            if (r->host_cnt->nrec <= cap) break;
            if (attempt) return iqpt::fail(IQPT_ERR_HIP, "setup record count changed between passes");
            cap = (size_t)r->host_cnt->nrec;
        }
        nrec = (uint32_t)r->host_cnt->nrec;
        npairs = (uint32_t)r->host_cnt->npairs;
    }
    if (ev) IQPT_HIP(hipEventRecord(ev[0], s));

    const int in = 0, out = 1;
    // sort key: tile << key_bits | (submission index << 3 | piece), key_bits just wide enough for this draw
    unsigned key_bits = iqr::kPieceBits + 1;
    while ((1ull << key_bits) < ((unsigned long long)nsub << iqr::kPieceBits)) ++key_bits;
    if (npairs) {
        for (int k = 0; k < 2; ++k) {
            IQPT_HIP(l.keys[k].reserve((size_t)npairs * sizeof(unsigned long long)));
            IQPT_HIP(l.vals[k].reserve((size_t)npairs * sizeof(uint32_t)));
        }
        IQPT_HIP(iqr::launch_bin(s, fp, l.recs.as<iqr::setup_rec>(), nrec, key_bits, l.keys[in].as<unsigned long long>(),
                                l.vals[in].as<uint32_t>()));
    }
    if (ev) IQPT_HIP(hipEventRecord(ev[1], s));
    if (npairs) {
        unsigned tile_bits = 1;
        while ((1ull << tile_bits) < (unsigned long long)fp.ntx * fp.nty) ++tile_bits;
        const unsigned end_bit = key_bits + tile_bits;
        size_t need = 0;
        IQPT_HIP(iqr::sort_pairs(s, nullptr, need, l.keys[in].as<unsigned long long>(),
                                l.keys[out].as<unsigned long long>(), l.vals[in].as<uint32_t>(),
                                l.vals[out].as<uint32_t>(), npairs, end_bit));
        IQPT_HIP(r->sort_temp.reserve(std::max<size_t>(need, 16)));
        need = r->sort_temp.bytes;
        IQPT_HIP(iqr::sort_pairs(s, r->sort_temp.p, need, l.keys[in].as<unsigned long long>(),
                                l.keys[out].as<unsigned long long>(), l.vals[in].as<uint32_t>(),
                                l.vals[out].as<uint32_t>(), npairs, end_bit));
    }
    IQPT_HIP(iqr::launch_ranges(s, fp, l.keys[out].as<unsigned long long>(), npairs, key_bits, l.ranges.as<uint32_t>()));
    return IQPT_OK;
}

int run_draw(iqpt_raster* r, geometry& g, bool vertex_stage) {
    if (int st = set_device(r)) return st;
    if (int st = collect(r)) return st;
    hipStream_t s = r->stream;
    const iqr::frame_params& fp = r->fp;
    IQPT_HIP(hipEventRecord(r->ev[0], s));
    if (vertex_stage && !g.transformed) {
        IQPT_HIP(iqr::launch_vertex(s, g.draws.as<iqr::draw_rec>(), g.ndraws, g.vend.as<uint32_t>(), g.nverts,
                                   g.mesh_verts.as<float>(), r->camera.as<float>(), r->camera.as<float>() + 16,
                                   g.clip.as<float>(), g.wn.as<float>()));
        g.transformed = true;
    }
    IQPT_HIP(hipEventRecord(r->ev[1], s));

    uint32_t nrec = 0, npairs = 0;
    if (int st = build_lists(r, g, fp, false, r->draw_lists, r->ev + 2, nrec, npairs)) return st;
    IQPT_HIP(hipEventRecord(r->ev[4], s));
    const lists& l = r->draw_lists;
    IQPT_HIP(iqr::launch_tiles(s, fp, l.recs.as<iqr::setup_rec>(), l.vals[1].as<uint32_t>(), l.ranges.as<uint32_t>(),
                              r->frame.as<uint32_t>(), nullptr, nullptr));
    IQPT_HIP(hipEventRecord(r->ev[5], s));
    r->pending = true;
    r->have_frame = true;
    r->last_nrec = nrec;
    r->last_npairs = npairs;
    r->last_ntris = g.ntris;
    return IQPT_OK;
}

}  // namespace

extern "C" {

int iqpt_raster_create(int device, uint32_t width, uint32_t height, uint32_t samples, iqpt_raster** out) {
    if (!out) return iqpt::fail(IQPT_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (width == 0 || height == 0 || width > IQPT_RASTER_MAX_DIM || height > IQPT_RASTER_MAX_DIM)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "frame size must be 1..8192 in each dimension");
    if (samples != 1 && samples != 4) return iqpt::fail(IQPT_ERR_INVALID_ARG, "samples must be 1 or 4");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return iqpt::fail(IQPT_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= count) return iqpt::fail(IQPT_ERR_NO_DEVICE, "device index out of range");

    iqpt_raster* r = new iqpt_raster();
    r->device = device;
    r->fp.width = width;
    r->fp.height = height;
    r->fp.samples = samples;
    r->fp.ntx = (width + iqr::kTile - 1) / iqr::kTile;
    r->fp.nty = (height + iqr::kTile - 1) / iqr::kTile;
    auto fail_with = [&](hipError_t e, const char* what) {
        const int st = iqpt::hip_fail(e, what);
        iqpt_raster_destroy(r);
        return st;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return fail_with(e, "hipSetDevice");
    if ((e = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking)) != hipSuccess) return fail_with(e, "hipStreamCreate");
    for (int k = 0; k < kEvents; ++k)
        if ((e = hipEventCreate(&r->ev[k])) != hipSuccess) return fail_with(e, "hipEventCreate");
    if ((e = hipHostMalloc((void**)&r->host_cnt, sizeof(iqr::counters), hipHostMallocDefault)) != hipSuccess)
        return fail_with(e, "hipHostMalloc");
    if ((e = r->cnt.reserve(sizeof(iqr::counters))) != hipSuccess) return fail_with(e, "hipMalloc(counters)");
    if ((e = r->camera.reserve(32 * sizeof(float))) != hipSuccess) return fail_with(e, "hipMalloc(camera)");
    if ((e = r->frame.reserve((size_t)width * height * 4)) != hipSuccess) return fail_with(e, "hipMalloc(frame)");
    for (lists* l : {&r->draw_lists, &r->guide_lists})
        if ((e = l->ranges.reserve((size_t)r->fp.ntx * r->fp.nty * 8)) != hipSuccess) return fail_with(e, "hipMalloc(ranges)");
    for (hipEvent_t& ev : r->guide_ev)
        if ((e = hipEventCreate(&ev)) != hipSuccess) return fail_with(e, "hipEventCreate");
    *out = r;
    return IQPT_OK;
}

int iqpt_raster_destroy(iqpt_raster* r) {
    if (!r) return IQPT_OK;
    (void)hipSetDevice(r->device);
    if (r->stream) (void)hipStreamSynchronize(r->stream);
    r->scene.release();
    r->direct.release();
    r->draw_lists.release();
    r->guide_lists.release();
    for (dbuf* b : {&r->camera, &r->cnt, &r->frame, &r->depth_samples, &r->prim_samples, &r->sort_temp, &r->guide_nz,
                    &r->guide_id})
        b->release();
    for (hipEvent_t ev : r->guide_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (r->host_cnt) (void)hipHostFree(r->host_cnt);
    for (hipEvent_t ev : r->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (r->stream) (void)hipStreamDestroy(r->stream);
    delete r;
    return IQPT_OK;
}

int iqpt_raster_set_camera(iqpt_raster* r, const iqpt_camera* cam) {
    if (!r || !cam) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (cam->width != r->fp.width || cam->height != r->fp.height)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "camera size differs from the frame's");
    if (int st = set_device(r)) return st;
    float m[32];
    std::memcpy(m, cam->view, 64);
    std::memcpy(m + 16, cam->projection, 64);
    // ordered behind the draws in flight; m is on the stack, so the copy is finished before returning
    IQPT_HIP(hipMemcpyAsync(r->camera.p, m, sizeof m, hipMemcpyHostToDevice, r->stream));
    IQPT_HIP(hipStreamSynchronize(r->stream));
    r->host_camera = *cam;
    r->have_camera = true;
    r->scene.transformed = false;
    r->have_gbuffer = false;
    return IQPT_OK;
}

int iqpt_raster_upload_scene(iqpt_raster* r, const iqpt_scene* scene) {
    if (!r || !scene) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    uint32_t n = 0;
    if (int st = iqpt_scene_draw_list(scene, nullptr, 0, &n)) return st;
    std::vector<iqpt_draw_item> items(n);
    if (n)
        if (int st = iqpt_scene_draw_list(scene, items.data(), n, &n)) return st;

    // one copy of every distinct mesh in the pools; one draw record per model
    std::vector<float> verts;
    std::vector<uint32_t> indices, vend, tend;
    std::vector<iqr::draw_rec> draws;
    struct pooled { const iqpt_vertex* v; uint32_t vbase, ibase; };
    std::vector<pooled> pool;
    uint64_t nverts = 0, ntris = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const iqpt_draw_item& it = items[i];
        if (it.num_indices % 3) return iqpt::fail(IQPT_ERR_INVALID_ARG, "model " + std::to_string(i) + ": index count is not a multiple of 3");
        if (it.num_indices == 0 || it.num_vertices == 0) continue;      // an empty mesh draws nothing
        const pooled* found = nullptr;
        for (const pooled& p : pool)
            if (p.v == it.vertices) found = &p;
        if (!found) {
            for (uint32_t k = 0; k < it.num_indices; ++k)
                if (it.indices[k] >= it.num_vertices)
                    return iqpt::fail(IQPT_ERR_INVALID_ARG, "model " + std::to_string(i) + ": index out of range");
            pool.push_back({it.vertices, (uint32_t)(verts.size() / 6), (uint32_t)indices.size()});
            const float* f = reinterpret_cast<const float*>(it.vertices);
            verts.insert(verts.end(), f, f + 6 * (size_t)it.num_vertices);
            indices.insert(indices.end(), it.indices, it.indices + it.num_indices);
            found = &pool.back();
        }
        iqr::draw_rec d{};
        std::memcpy(d.model, it.transform, sizeof d.model);
        const iq::mat4 N = iq::normal_matrix(iq::mat4::from(it.transform));      // path_tracer.cu:260
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 4; ++b) d.normal[a * 4 + b] = N.m[a][b];
        d.albedo[0] = it.albedo[0]; d.albedo[1] = it.albedo[1]; d.albedo[2] = it.albedo[2]; d.albedo[3] = 1.0f;
        d.vbase = (uint32_t)nverts;
        d.src_vbase = found->vbase;
        d.ibase = found->ibase;
        d.tbase = (uint32_t)ntris;
        d.item = i;
        nverts += it.num_vertices;
        ntris += it.num_indices / 3;
        if (ntris >= iqr::kMaxTriangles || nverts >= 0x7fffffffu)
            return iqpt::fail(IQPT_ERR_UNSUPPORTED, "more than 2^28 triangles in one frame");
        draws.push_back(d);
        vend.push_back((uint32_t)nverts);
        tend.push_back((uint32_t)ntris);
    }

    if (int st = set_device(r)) return st;
    IQPT_HIP(hipStreamSynchronize(r->stream));
    geometry& g = r->scene;
    hipStream_t s = r->stream;
    if (int st = upload(g.draws, draws.data(), draws.size() * sizeof(iqr::draw_rec), s)) return st;
    if (int st = upload(g.vend, vend.data(), vend.size() * 4, s)) return st;
    if (int st = upload(g.tend, tend.data(), tend.size() * 4, s)) return st;
    if (int st = upload(g.indices, indices.data(), indices.size() * 4, s)) return st;
    if (int st = upload(g.mesh_verts, verts.data(), verts.size() * 4, s)) return st;
    IQPT_HIP(g.clip.reserve(std::max<size_t>((size_t)nverts * 16, 16)));
    IQPT_HIP(g.wn.reserve(std::max<size_t>((size_t)nverts * 16, 16)));
    IQPT_HIP(hipStreamSynchronize(s));              // the host vectors go out of scope
    g.ndraws = (uint32_t)draws.size();
    g.nverts = (uint32_t)nverts;
    g.ntris = (uint32_t)ntris;
    g.transformed = false;
    r->have_scene = true;
    r->have_gbuffer = false;
    return IQPT_OK;
}

int iqpt_raster_draw(iqpt_raster* r) {
    if (!r) return iqpt::fail(IQPT_ERR_INVALID_ARG, "rasterizer is NULL");
    if (!r->have_camera || !r->have_scene) return iqpt::fail(IQPT_ERR_NOT_READY, "draw before set_camera / upload_scene");
    return run_draw(r, r->scene, true);
}

int iqpt_raster_draw_clip(iqpt_raster* r, const float* clip_xyzw, const float* normals, uint32_t nverts,
                          const uint32_t* indices, uint32_t nindices) {
    if (!r) return iqpt::fail(IQPT_ERR_INVALID_ARG, "rasterizer is NULL");
    if ((nverts && (!clip_xyzw || !normals)) || (nindices && !indices))
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL vertex / index array");
    if (nindices % 3) return iqpt::fail(IQPT_ERR_INVALID_ARG, "index count is not a multiple of 3");
    if (nindices / 3 >= iqr::kMaxTriangles) return iqpt::fail(IQPT_ERR_UNSUPPORTED, "more than 2^28 triangles in one frame");
    for (uint32_t k = 0; k < nindices; ++k)
        if (indices[k] >= nverts) return iqpt::fail(IQPT_ERR_INVALID_ARG, "index out of range");
    if (int st = set_device(r)) return st;
    IQPT_HIP(hipStreamSynchronize(r->stream));
    std::vector<float> c4((size_t)nverts * 4), n4((size_t)nverts * 4, 0.0f);
    if (nverts) std::memcpy(c4.data(), clip_xyzw, c4.size() * 4);
    for (uint32_t i = 0; i < nverts; ++i)
        for (int k = 0; k < 3; ++k) n4[(size_t)i * 4 + k] = normals[(size_t)i * 3 + k];
    iqr::draw_rec d{};
    d.albedo[0] = 1.0f; d.albedo[3] = 1.0f;                                       // pixel_shader.hlsl: albedo
    const uint32_t ntris = nindices / 3;
    geometry& g = r->direct;
    hipStream_t s = r->stream;
    if (int st = upload(g.draws, &d, sizeof d, s)) return st;
    if (int st = upload(g.vend, &nverts, 4, s)) return st;
    if (int st = upload(g.tend, &ntris, 4, s)) return st;
    if (int st = upload(g.indices, indices, (size_t)nindices * 4, s)) return st;
    if (int st = upload(g.clip, c4.data(), c4.size() * 4, s)) return st;
    if (int st = upload(g.wn, n4.data(), n4.size() * 4, s)) return st;
    IQPT_HIP(hipStreamSynchronize(s));
    g.ndraws = 1;
    g.nverts = nverts;
    g.ntris = ntris;
    return run_draw(r, g, false);
}

int iqpt_raster_read(iqpt_raster* r, uint8_t* bgra, float* depth_samples, uint32_t* prim_samples) {
    if (!r) return iqpt::fail(IQPT_ERR_INVALID_ARG, "rasterizer is NULL");
    if (!r->have_frame) return iqpt::fail(IQPT_ERR_NOT_READY, "read before the first draw");
    if (int st = set_device(r)) return st;
    hipStream_t s = r->stream;
    const size_t npix = (size_t)r->fp.width * r->fp.height, nsamp = npix * r->fp.samples;
    if (depth_samples || prim_samples) {
        // the tile kernel of the last draw again, over the same sorted lists, with the per-sample outputs on
        IQPT_HIP(r->depth_samples.reserve(nsamp * 4));
        IQPT_HIP(r->prim_samples.reserve(nsamp * 4));
        const lists& l = r->draw_lists;
        IQPT_HIP(iqr::launch_tiles(s, r->fp, l.recs.as<iqr::setup_rec>(), l.vals[1].as<uint32_t>(),
                                  l.ranges.as<uint32_t>(), r->frame.as<uint32_t>(), r->depth_samples.as<float>(),
                                  r->prim_samples.as<uint32_t>()));
        if (depth_samples) IQPT_HIP(hipMemcpyAsync(depth_samples, r->depth_samples.p, nsamp * 4, hipMemcpyDeviceToHost, s));
        if (prim_samples) IQPT_HIP(hipMemcpyAsync(prim_samples, r->prim_samples.p, nsamp * 4, hipMemcpyDeviceToHost, s));
    }
    if (bgra) IQPT_HIP(hipMemcpyAsync(bgra, r->frame.p, npix * 4, hipMemcpyDeviceToHost, s));
    IQPT_HIP(hipStreamSynchronize(s));
    return IQPT_OK;
}

int iqpt_raster_copy_frame_device(iqpt_raster* r, void* dst_device, size_t bytes) {
    if (!r || !dst_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (!r->have_frame) return iqpt::fail(IQPT_ERR_NOT_READY, "copy before the first draw");
    if (bytes != (size_t)r->fp.width * r->fp.height * 4) return iqpt::fail(IQPT_ERR_INVALID_ARG, "bytes must be width*height*4");
    if (int st = set_device(r)) return st;
    IQPT_HIP(hipMemcpyAsync(dst_device, r->frame.p, bytes, hipMemcpyDeviceToDevice, r->stream));
    IQPT_HIP(hipStreamSynchronize(r->stream));
    return IQPT_OK;
}

int iqpt_raster_sync(iqpt_raster* r) {
    if (!r) return iqpt::fail(IQPT_ERR_INVALID_ARG, "rasterizer is NULL");
    if (int st = set_device(r)) return st;
    IQPT_HIP(hipStreamSynchronize(r->stream));
    return IQPT_OK;
}

int iqpt_raster_time(iqpt_raster* r, double* total_ms, uint64_t* draws) {
    if (!r || !total_ms || !draws) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = set_device(r)) return st;
    if (int st = collect(r)) return st;
    *total_ms = r->total_ms;
    *draws = r->draws;
    r->total_ms = 0.0;
    r->draws = 0;
    for (double& v : r->stage_ms) v = 0.0;
    return IQPT_OK;
}

int iqpt_raster_stage_time(iqpt_raster* r, double stage_ms[5]) {
    if (!r || !stage_ms) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = set_device(r)) return st;
    if (int st = collect(r)) return st;
    for (int k = 0; k < 5; ++k) stage_ms[k] = r->stage_ms[k];
    return IQPT_OK;
}

int iqpt_raster_stats(iqpt_raster* r, uint64_t counts[3]) {
    if (!r || !counts) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    counts[0] = r->last_ntris;
    counts[1] = r->last_nrec;
    counts[2] = r->last_npairs;
    return IQPT_OK;
}

// ---------------------------------------------------------------------------------------------- G-buffer
int iqpt_raster_gbuffer(iqpt_raster* r) {
    if (!r) return iqpt::fail(IQPT_ERR_INVALID_ARG, "rasterizer is NULL");
    if (!r->have_camera || !r->have_scene) return iqpt::fail(IQPT_ERR_NOT_READY, "gbuffer before set_camera / upload_scene");
    if (r->have_gbuffer) return IQPT_OK;       // kept until the camera or the scene changes
    geometry& g = r->scene;
    if (2ull * g.ntris >= iqr::kMaxTriangles)
        return iqpt::fail(IQPT_ERR_UNSUPPORTED, "more than 2^27 triangles in a G-buffer pass (every one is submitted twice)");
    if (int st = set_device(r)) return st;
    if (int st = collect_guide(r)) return st;
    hipStream_t s = r->stream;
    const size_t npix = (size_t)r->fp.width * r->fp.height;
    IQPT_HIP(r->guide_nz.reserve(npix * 16));
    IQPT_HIP(r->guide_id.reserve(npix * 4));
    iqr::frame_params fp = r->fp;
    fp.samples = 1;                            // one sample per pixel, whatever the rasterizer's own count
    IQPT_HIP(hipEventRecord(r->guide_ev[0], s));
    if (!g.transformed) {
        IQPT_HIP(iqr::launch_vertex(s, g.draws.as<iqr::draw_rec>(), g.ndraws, g.vend.as<uint32_t>(), g.nverts,
                                   g.mesh_verts.as<float>(), r->camera.as<float>(), r->camera.as<float>() + 16,
                                   g.clip.as<float>(), g.wn.as<float>()));
        g.transformed = true;
    }
    uint32_t nrec = 0, npairs = 0;
    lists& l = r->guide_lists;
    if (int st = build_lists(r, g, fp, true, l, nullptr, nrec, npairs)) return st;
    IQPT_HIP(iqr::launch_guide_tiles(s, fp, l.recs.as<iqr::setup_rec>(), l.vals[1].as<uint32_t>(), l.ranges.as<uint32_t>(),
                                    r->guide_nz.p, r->guide_id.as<uint32_t>()));
    IQPT_HIP(hipEventRecord(r->guide_ev[1], s));
    r->guide_pending = true;
    r->guide_passes += 1;
    r->have_gbuffer = true;
    return IQPT_OK;
}

int iqpt_raster_read_gbuffer(iqpt_raster* r, float* normal_z, uint32_t* id) {
    if (!r) return iqpt::fail(IQPT_ERR_INVALID_ARG, "rasterizer is NULL");
    if (!r->have_gbuffer) return iqpt::fail(IQPT_ERR_NOT_READY, "read_gbuffer without a G-buffer of the current camera and scene");
    if (int st = set_device(r)) return st;
    const size_t npix = (size_t)r->fp.width * r->fp.height;
    if (normal_z) IQPT_HIP(hipMemcpyAsync(normal_z, r->guide_nz.p, npix * 16, hipMemcpyDeviceToHost, r->stream));
    if (id) IQPT_HIP(hipMemcpyAsync(id, r->guide_id.p, npix * 4, hipMemcpyDeviceToHost, r->stream));
    IQPT_HIP(hipStreamSynchronize(r->stream));
    return IQPT_OK;
}

int iqpt_raster_gbuffer_device(iqpt_raster* r, const void** normal_z, const void** id) {
    if (!r || !normal_z || !id) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (!r->have_gbuffer) return iqpt::fail(IQPT_ERR_NOT_READY, "gbuffer_device without a G-buffer of the current camera and scene");
    if (int st = set_device(r)) return st;
    IQPT_HIP(hipStreamSynchronize(r->stream));  // the caller reads them on a stream of its own
    *normal_z = r->guide_nz.p;
    *id = r->guide_id.p;
    return IQPT_OK;
}

int iqpt_raster_gbuffer_time(iqpt_raster* r, double* total_ms, uint64_t* passes) {
    if (!r || !total_ms || !passes) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = set_device(r)) return st;
    if (int st = collect_guide(r)) return st;
    *total_ms = r->guide_ms;
    *passes = r->guide_passes;
    r->guide_ms = 0.0;
    r->guide_passes = 0;
    return IQPT_OK;
}

}  // extern "C"

void iqr::frame_size(const iqpt_raster* r, uint32_t* width, uint32_t* height) {
    *width = r->fp.width;
    *height = r->fp.height;
}

const iqpt_camera* iqr::current_camera(const iqpt_raster* r) { return r->have_camera ? &r->host_camera : nullptr; }
