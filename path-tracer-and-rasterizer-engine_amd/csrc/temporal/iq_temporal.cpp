// iq_temporal.cpp — the iqpt_temporal_* C ABI (include/temporal/iqpt_temporal.h): the two sets of view planes
// that swap at every begin_view, the history and the result, one kernel launch per begin_view and per resolve
// on the object's own stream, readback, timing and the counts. The kernels are iq_temporal_kernels.hip; the
// definition is DESIGN.md §11.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "post/iq_post.hpp"
#include "temporal/iq_temporal.hpp"
#include "temporal/iqpt_temporal.h"

namespace {

// DESIGN.md §11 "Defaults": starting values, not measured
constexpr iqpt_temporal_params kDefaults = {0.9f, 0.01f, 256u};

}  // namespace

int iqt::check_params(const iqpt_temporal_params& p) {
    if (!std::isfinite(p.normal_min)) return iqpt::fail(IQPT_ERR_INVALID_ARG, "normal_min must be finite");
    if (!(p.plane_tolerance >= 0.0f)) return iqpt::fail(IQPT_ERR_INVALID_ARG, "plane_tolerance must be >= 0");
    if (p.max_history < 1u || p.max_history > IQPT_TEMPORAL_MAX_HISTORY)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "max_history must be 1..2^24");
    return IQPT_OK;
}

struct iqpt_temporal : iqp::frame {
    iqpt_temporal_params params = kDefaults;
    iqt::view_planes planes[2] = {};   // planes[cur] is the current view's, the other one the previous view's
    int cur = 0;
    void* hist = nullptr;              // npix float4: the current view's history
    void* out = nullptr;               // npix float4: the last result
    uint32_t* bgra = nullptr;          // npix
    void* input = nullptr;             // npix float4: a host colour, or the accumulator resolve_ctx takes
    unsigned long long* counts = nullptr;   // 2, device
    iqpt_camera camera{};              // the current view's
    bool have_view = false, have_result = false;
    iqp::event_timer view_t, resolve_t;     // each one stage: ev[0] before the kernel, ev[1] after it
};

namespace {

// the planes of the new view are in planes[1 - cur] already (copied on the stream): positions, history, swap
int begin(iqpt_temporal* t, const iqpt_camera& cam) {
    if (int st = t->view_t.collect()) return st;
    iqt::view_params p{};
    p.width = t->width;
    p.height = t->height;
    p.have_prev = t->have_view && t->have_result ? 1u : 0u;
    p.normal_min = t->params.normal_min;
    p.plane_tolerance = t->params.plane_tolerance;
    p.max_history = (float)t->params.max_history;
    std::memcpy(p.inv_proj, cam.inv_proj, sizeof p.inv_proj);
    std::memcpy(p.inv_view, cam.inv_view, sizeof p.inv_view);
    std::memcpy(p.view_prev, t->camera.view, sizeof p.view_prev);
    std::memcpy(p.proj_prev, t->camera.projection, sizeof p.proj_prev);
    const int next = 1 - t->cur;
    IQPT_HIP(hipEventRecord(t->view_t.ev[0], t->stream));
    IQPT_HIP(iqt::launch_view(t->stream, p, t->planes[next], t->planes[t->cur], t->out, t->hist));
    IQPT_HIP(hipEventRecord(t->view_t.ev[1], t->stream));
    t->view_t.recorded = 2;
    t->cur = next;
    t->camera = cam;
    t->have_view = true;
    t->have_result = false;
    return IQPT_OK;
}

int begin_planes(iqpt_temporal* t, const iqpt_camera* cam, const void* normal_z, const void* id, hipMemcpyKind kind) {
    if (int st = iqp::check_camera(*t, cam)) return st;
    if (int st = iqp::set_device(*t)) return st;
    const iqt::view_planes& v = t->planes[1 - t->cur];
    if (int st = iqp::copy_guides(*t, v.normal_z, v.id, normal_z, id, kind)) return st;
    return begin(t, *cam);
}

int resolve(iqpt_temporal* t, const void* colour_device, uint64_t n) {
    if (!t->have_view) return iqpt::fail(IQPT_ERR_NOT_READY, "resolve before the first begin_view");
    if (int st = t->resolve_t.collect()) return st;
    const float nf = (float)(n > IQPT_TEMPORAL_MAX_HISTORY ? (uint64_t)IQPT_TEMPORAL_MAX_HISTORY : n);
    IQPT_HIP(hipEventRecord(t->resolve_t.ev[0], t->stream));
    IQPT_HIP(iqt::launch_resolve(t->stream, t->width, t->height, nf, t->hist, colour_device, t->out, t->bgra));
    IQPT_HIP(hipEventRecord(t->resolve_t.ev[1], t->stream));
    t->resolve_t.recorded = 2;
    t->have_result = true;
    return IQPT_OK;
}

}  // namespace

extern "C" {

int iqpt_temporal_default_params(iqpt_temporal_params* out) {
    if (!out) return iqpt::fail(IQPT_ERR_INVALID_ARG, "out is NULL");
    *out = kDefaults;
    return IQPT_OK;
}

int iqpt_temporal_create(int device, uint32_t width, uint32_t height, iqpt_temporal** out) {
    return iqp::frame_create(device, width, height, out, iqpt_temporal_destroy, [](iqpt_temporal* t) {
        if (int st = t->view_t.create(2)) return st;
        if (int st = t->resolve_t.create(2)) return st;
        const size_t n = t->npix();
        iqt::view_planes *a = &t->planes[0], *b = &t->planes[1];
        return iqp::frame_alloc(*t, {{&a->normal_z, n * 16, "hipMalloc(normal_z)"},
                                     {(void**)&a->id, n * 4, "hipMalloc(id)"},
                                     {&a->pos, n * 16, "hipMalloc(pos)"},
                                     {&b->normal_z, n * 16, "hipMalloc(normal_z)"},
                                     {(void**)&b->id, n * 4, "hipMalloc(id)"},
                                     {&b->pos, n * 16, "hipMalloc(pos)"},
                                     {&t->hist, n * 16, "hipMalloc(hist)"},
                                     {&t->out, n * 16, "hipMalloc(out)"},
                                     {(void**)&t->bgra, n * 4, "hipMalloc(bgra)"},
                                     {&t->input, n * 16, "hipMalloc(input)"},
                                     {(void**)&t->counts, 2 * sizeof(unsigned long long), "hipMalloc(counts)"}});
    });
}

int iqpt_temporal_destroy(iqpt_temporal* t) {
    if (!t) return IQPT_OK;
    iqp::frame_close(*t, {&t->view_t, &t->resolve_t});
    delete t;
    return IQPT_OK;
}

int iqpt_temporal_set_params(iqpt_temporal* t, const iqpt_temporal_params* p) {
    if (!p) return iqpt::fail(IQPT_ERR_INVALID_ARG, "params is NULL");
    if (int st = iqt::check_params(*p)) return st;
    if (!t) return iqpt::fail(IQPT_ERR_INVALID_ARG, "temporal object is NULL");
    t->params = *p;
    return IQPT_OK;
}

int iqpt_temporal_begin_view(iqpt_temporal* t, const iqpt_camera* cam, const float* normal_z, const uint32_t* id) {
    if (!t || !cam || !normal_z || !id) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    return begin_planes(t, cam, normal_z, id, hipMemcpyHostToDevice);
}

int iqpt_temporal_begin_view_device(iqpt_temporal* t, const iqpt_camera* cam, const void* normal_z_device,
                                    const void* id_device) {
    if (!t || !cam || !normal_z_device || !id_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    return begin_planes(t, cam, normal_z_device, id_device, hipMemcpyDeviceToDevice);
}

int iqpt_temporal_begin_view_raster(iqpt_temporal* t, iqpt_raster* r) {
    if (!t || !r) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    const iqpt_camera* cam = nullptr;
    const void *nz = nullptr, *id = nullptr;
    if (int st = iqp::raster_view(*t, r, "the object's", &cam, &nz, &id)) return st;
    return iqpt_temporal_begin_view_device(t, cam, nz, id);
}

int iqpt_temporal_clear(iqpt_temporal* t) {
    if (!t) return iqpt::fail(IQPT_ERR_INVALID_ARG, "temporal object is NULL");
    t->have_view = false;
    t->have_result = false;
    return IQPT_OK;
}

int iqpt_temporal_resolve(iqpt_temporal* t, const float* colour, uint64_t n) {
    if (!t || !colour) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (!t->have_view) return iqpt::fail(IQPT_ERR_NOT_READY, "resolve before the first begin_view");
    if (int st = iqp::set_device(*t)) return st;
    IQPT_HIP(hipMemcpyAsync(t->input, colour, t->npix() * 16, hipMemcpyHostToDevice, t->stream));
    IQPT_HIP(hipStreamSynchronize(t->stream));      // the caller's array may go away
    return resolve(t, t->input, n);
}

int iqpt_temporal_resolve_device(iqpt_temporal* t, const void* colour_device, uint64_t n) {
    if (!t || !colour_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = iqp::set_device(*t)) return st;
    return resolve(t, colour_device, n);
}

int iqpt_temporal_resolve_ctx(iqpt_temporal* t, iqpt_ctx* ctx) {
    if (!t || !ctx) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    uint64_t npix = 0, frames = 0;
    if (int st = iqpt_num_pixels(ctx, &npix)) return st;
    if (npix != t->npix()) return iqpt::fail(IQPT_ERR_INVALID_ARG, "the context does not own a whole frame of the object's size");
    if (!t->have_view) return iqpt::fail(IQPT_ERR_NOT_READY, "resolve before the first begin_view");
    if (int st = iqp::set_device(*t)) return st;
    IQPT_HIP(hipStreamSynchronize(t->stream));      // a resolve in flight may still read t->input
    if (int st = iqpt_copy_accum_device(ctx, t->input, t->npix() * 16)) return st;
    if (int st = iqpt_frame_count(ctx, &frames)) return st;
    return resolve(t, t->input, frames);
}

int iqpt_temporal_read(iqpt_temporal* t, float* lin_rgba, uint8_t* bgra) {
    if (!t) return iqpt::fail(IQPT_ERR_INVALID_ARG, "temporal object is NULL");
    if (!t->have_result) return iqpt::fail(IQPT_ERR_NOT_READY, "read before a resolve of the current view");
    return iqp::read_planes(*t, lin_rgba, t->out, bgra, t->bgra);
}

int iqpt_temporal_output_device(iqpt_temporal* t, const void** out_device) {
    if (!t || !out_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    *out_device = t->out;
    return IQPT_OK;
}

int iqpt_temporal_copy_frame_device(iqpt_temporal* t, void* dst_device, size_t bytes) {
    if (!t || !dst_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (!t->have_result) return iqpt::fail(IQPT_ERR_NOT_READY, "copy before a resolve of the current view");
    return iqp::copy_bgra(*t, t->bgra, dst_device, bytes);
}

int iqpt_temporal_sync(iqpt_temporal* t) {
    if (!t) return iqpt::fail(IQPT_ERR_INVALID_ARG, "temporal object is NULL");
    if (int st = iqp::set_device(*t)) return st;
    IQPT_HIP(hipStreamSynchronize(t->stream));
    return IQPT_OK;
}

int iqpt_temporal_time(iqpt_temporal* t, double* view_ms, uint64_t* views, double* resolve_ms, uint64_t* resolves) {
    if (!t || !view_ms || !views || !resolve_ms || !resolves) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = iqp::set_device(*t)) return st;
    if (int st = t->view_t.collect()) return st;
    if (int st = t->resolve_t.collect()) return st;
    *view_ms = t->view_t.ms[0];
    *views = t->view_t.runs;
    *resolve_ms = t->resolve_t.ms[0];
    *resolves = t->resolve_t.runs;
    t->view_t.reset();
    t->resolve_t.reset();
    return IQPT_OK;
}

int iqpt_temporal_stats(iqpt_temporal* t, uint64_t* guided, uint64_t* valid) {
    if (!t || !guided || !valid) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (!t->have_view) return iqpt::fail(IQPT_ERR_NOT_READY, "stats before the first begin_view");
    if (int st = iqp::set_device(*t)) return st;
    unsigned long long host[2] = {0, 0};
    IQPT_HIP(hipMemsetAsync(t->counts, 0, sizeof host, t->stream));
    IQPT_HIP(iqt::launch_stats(t->stream, (uint32_t)t->npix(), t->planes[t->cur].id, t->hist, t->counts));
    IQPT_HIP(hipMemcpyAsync(host, t->counts, sizeof host, hipMemcpyDeviceToHost, t->stream));
    IQPT_HIP(hipStreamSynchronize(t->stream));
    *guided = host[0];
    *valid = host[1];
    return IQPT_OK;
}

}  // extern "C"
