// iq_temporal.cpp — the iqpt_temporal_* C ABI (include/temporal/iqpt_temporal.h): the two sets of view planes
// that swap at every begin_view, the history and the result, one kernel launch per begin_view and per resolve
// on the object's own stream, readback, timing and the counts. The kernels are iq_temporal_kernels.hip; the
// definition is DESIGN.md §11.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "iqpt_internal.hpp"
#include "raster/iq_raster.hpp"
#include "temporal/iq_temporal.hpp"
#include "temporal/iqpt_temporal.h"

namespace {

int hip_fail(hipError_t e, const char* what) {
    return iqpt::fail(IQPT_ERR_HIP, std::string(what) + ": " + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ")");
}

#define IQT_HIP(call)                                        \
    do {                                                     \
        hipError_t e_ = (call);                              \
        if (e_ != hipSuccess) return hip_fail(e_, #call);    \
    } while (0)

// DESIGN.md §11 "Defaults": starting values, not measured
constexpr iqpt_temporal_params kDefaults = {0.9f, 0.01f, 256u};

int check_params(const iqpt_temporal_params& p) {
    if (!std::isfinite(p.normal_min)) return iqpt::fail(IQPT_ERR_INVALID_ARG, "normal_min must be finite");
    if (!(p.plane_tolerance >= 0.0f)) return iqpt::fail(IQPT_ERR_INVALID_ARG, "plane_tolerance must be >= 0");
    if (p.max_history < 1u || p.max_history > IQPT_TEMPORAL_MAX_HISTORY)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "max_history must be 1..2^24");
    return IQPT_OK;
}

// one kind of kernel's events: the last launch's pair and the sums since iqpt_temporal_time
struct timer {
    hipEvent_t ev[2] = {};
    bool pending = false;
    double ms = 0.0;
    uint64_t count = 0;
};

}  // namespace

struct iqpt_temporal {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t width = 0, height = 0;
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
    timer view_t, resolve_t;
    size_t npix() const { return (size_t)width * height; }
};

namespace {

int set_device(iqpt_temporal* t) {
    IQT_HIP(hipSetDevice(t->device));
    return IQPT_OK;
}

int collect(timer& tm) {
    if (!tm.pending) return IQPT_OK;
    IQT_HIP(hipEventSynchronize(tm.ev[1]));
    float ms = 0.0f;
    IQT_HIP(hipEventElapsedTime(&ms, tm.ev[0], tm.ev[1]));
    tm.ms += ms;
    tm.count += 1;
    tm.pending = false;
    return IQPT_OK;
}

// the planes of the new view are in planes[1 - cur] already (copied on the stream): positions, history, swap
int begin(iqpt_temporal* t, const iqpt_camera& cam) {
    if (int st = collect(t->view_t)) return st;
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
    IQT_HIP(hipEventRecord(t->view_t.ev[0], t->stream));
    IQT_HIP(iqt::launch_view(t->stream, p, t->planes[next], t->planes[t->cur], t->out, t->hist));
    IQT_HIP(hipEventRecord(t->view_t.ev[1], t->stream));
    t->view_t.pending = true;
    t->cur = next;
    t->camera = cam;
    t->have_view = true;
    t->have_result = false;
    return IQPT_OK;
}

int check_camera(const iqpt_temporal* t, const iqpt_camera* cam) {
    if (cam->width != t->width || cam->height != t->height)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "camera size differs from the frame's");
    return IQPT_OK;
}

int resolve(iqpt_temporal* t, const void* colour_device, uint64_t n) {
    if (!t->have_view) return iqpt::fail(IQPT_ERR_NOT_READY, "resolve before the first begin_view");
    if (int st = collect(t->resolve_t)) return st;
    const float nf = (float)(n > IQPT_TEMPORAL_MAX_HISTORY ? (uint64_t)IQPT_TEMPORAL_MAX_HISTORY : n);
    IQT_HIP(hipEventRecord(t->resolve_t.ev[0], t->stream));
    IQT_HIP(iqt::launch_resolve(t->stream, t->width, t->height, nf, t->hist, colour_device, t->out, t->bgra));
    IQT_HIP(hipEventRecord(t->resolve_t.ev[1], t->stream));
    t->resolve_t.pending = true;
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
    if (!out) return iqpt::fail(IQPT_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (width == 0 || height == 0 || width > IQPT_RASTER_MAX_DIM || height > IQPT_RASTER_MAX_DIM)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "frame size must be 1..8192 in each dimension");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return iqpt::fail(IQPT_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= count) return iqpt::fail(IQPT_ERR_NO_DEVICE, "device index out of range");

    iqpt_temporal* t = new iqpt_temporal();
    t->device = device;
    t->width = width;
    t->height = height;
    auto fail_with = [&](hipError_t e, const char* what) {
        const int st = hip_fail(e, what);
        iqpt_temporal_destroy(t);
        return st;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return fail_with(e, "hipSetDevice");
    if ((e = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking)) != hipSuccess) return fail_with(e, "hipStreamCreate");
    for (timer* tm : {&t->view_t, &t->resolve_t})
        for (hipEvent_t& ev : tm->ev)
            if ((e = hipEventCreate(&ev)) != hipSuccess) return fail_with(e, "hipEventCreate");
    const size_t n = t->npix();
    for (iqt::view_planes& v : t->planes) {
        if ((e = hipMalloc(&v.normal_z, n * 16)) != hipSuccess) return fail_with(e, "hipMalloc(normal_z)");
        if ((e = hipMalloc((void**)&v.id, n * 4)) != hipSuccess) return fail_with(e, "hipMalloc(id)");
        if ((e = hipMalloc(&v.pos, n * 16)) != hipSuccess) return fail_with(e, "hipMalloc(pos)");
    }
    if ((e = hipMalloc(&t->hist, n * 16)) != hipSuccess) return fail_with(e, "hipMalloc(hist)");
    if ((e = hipMalloc(&t->out, n * 16)) != hipSuccess) return fail_with(e, "hipMalloc(out)");
    if ((e = hipMalloc((void**)&t->bgra, n * 4)) != hipSuccess) return fail_with(e, "hipMalloc(bgra)");
    if ((e = hipMalloc(&t->input, n * 16)) != hipSuccess) return fail_with(e, "hipMalloc(input)");
    if ((e = hipMalloc((void**)&t->counts, 2 * sizeof(unsigned long long))) != hipSuccess) return fail_with(e, "hipMalloc(counts)");
    *out = t;
    return IQPT_OK;
}

int iqpt_temporal_destroy(iqpt_temporal* t) {
    if (!t) return IQPT_OK;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    for (iqt::view_planes& v : t->planes)
        for (void* p : {v.normal_z, (void*)v.id, v.pos})
            if (p) (void)hipFree(p);
    for (void* p : {t->hist, t->out, (void*)t->bgra, t->input, (void*)t->counts})
        if (p) (void)hipFree(p);
    for (timer* tm : {&t->view_t, &t->resolve_t})
        for (hipEvent_t ev : tm->ev)
            if (ev) (void)hipEventDestroy(ev);
    if (t->stream) (void)hipStreamDestroy(t->stream);
    delete t;
    return IQPT_OK;
}

int iqpt_temporal_set_params(iqpt_temporal* t, const iqpt_temporal_params* p) {
    if (!p) return iqpt::fail(IQPT_ERR_INVALID_ARG, "params is NULL");
    if (int st = check_params(*p)) return st;
    if (!t) return iqpt::fail(IQPT_ERR_INVALID_ARG, "temporal object is NULL");
    t->params = *p;
    return IQPT_OK;
}

int iqpt_temporal_begin_view(iqpt_temporal* t, const iqpt_camera* cam, const float* normal_z, const uint32_t* id) {
    if (!t || !cam || !normal_z || !id) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = check_camera(t, cam)) return st;
    if (int st = set_device(t)) return st;
    const iqt::view_planes& v = t->planes[1 - t->cur];
    IQT_HIP(hipMemcpyAsync(v.normal_z, normal_z, t->npix() * 16, hipMemcpyHostToDevice, t->stream));
    IQT_HIP(hipMemcpyAsync(v.id, id, t->npix() * 4, hipMemcpyHostToDevice, t->stream));
    IQT_HIP(hipStreamSynchronize(t->stream));      // the caller's arrays may go away
    return begin(t, *cam);
}

int iqpt_temporal_begin_view_device(iqpt_temporal* t, const iqpt_camera* cam, const void* normal_z_device,
                                    const void* id_device) {
    if (!t || !cam || !normal_z_device || !id_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = check_camera(t, cam)) return st;
    if (int st = set_device(t)) return st;
    const iqt::view_planes& v = t->planes[1 - t->cur];
    IQT_HIP(hipMemcpyAsync(v.normal_z, normal_z_device, t->npix() * 16, hipMemcpyDeviceToDevice, t->stream));
    IQT_HIP(hipMemcpyAsync(v.id, id_device, t->npix() * 4, hipMemcpyDeviceToDevice, t->stream));
    IQT_HIP(hipStreamSynchronize(t->stream));      // the caller's planes may change (the G-buffer of the next camera)
    return begin(t, *cam);
}

int iqpt_temporal_begin_view_raster(iqpt_temporal* t, iqpt_raster* r) {
    if (!t || !r) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    uint32_t rw = 0, rh = 0;
    iqr::frame_size(r, &rw, &rh);
    if (rw != t->width || rh != t->height) return iqpt::fail(IQPT_ERR_INVALID_ARG, "the rasterizer's frame size differs from the object's");
    const iqpt_camera* cam = iqr::current_camera(r);
    if (!cam) return iqpt::fail(IQPT_ERR_NOT_READY, "begin_view_raster before the rasterizer's set_camera");
    if (int st = iqpt_raster_gbuffer(r)) return st;
    const void *nz = nullptr, *id = nullptr;
    if (int st = iqpt_raster_gbuffer_device(r, &nz, &id)) return st;
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
    if (int st = set_device(t)) return st;
    IQT_HIP(hipMemcpyAsync(t->input, colour, t->npix() * 16, hipMemcpyHostToDevice, t->stream));
    IQT_HIP(hipStreamSynchronize(t->stream));      // the caller's array may go away
    return resolve(t, t->input, n);
}

int iqpt_temporal_resolve_device(iqpt_temporal* t, const void* colour_device, uint64_t n) {
    if (!t || !colour_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = set_device(t)) return st;
    return resolve(t, colour_device, n);
}

int iqpt_temporal_resolve_ctx(iqpt_temporal* t, iqpt_ctx* ctx) {
    if (!t || !ctx) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    uint64_t npix = 0, frames = 0;
    if (int st = iqpt_num_pixels(ctx, &npix)) return st;
    if (npix != t->npix()) return iqpt::fail(IQPT_ERR_INVALID_ARG, "the context does not own a whole frame of the object's size");
    if (!t->have_view) return iqpt::fail(IQPT_ERR_NOT_READY, "resolve before the first begin_view");
    if (int st = set_device(t)) return st;
    IQT_HIP(hipStreamSynchronize(t->stream));      // a resolve in flight may still read t->input
    if (int st = iqpt_copy_accum_device(ctx, t->input, t->npix() * 16)) return st;
    if (int st = iqpt_frame_count(ctx, &frames)) return st;
    return resolve(t, t->input, frames);
}

int iqpt_temporal_read(iqpt_temporal* t, float* lin_rgba, uint8_t* bgra) {
    if (!t) return iqpt::fail(IQPT_ERR_INVALID_ARG, "temporal object is NULL");
    if (!t->have_result) return iqpt::fail(IQPT_ERR_NOT_READY, "read before a resolve of the current view");
    if (int st = set_device(t)) return st;
    if (lin_rgba) IQT_HIP(hipMemcpyAsync(lin_rgba, t->out, t->npix() * 16, hipMemcpyDeviceToHost, t->stream));
    if (bgra) IQT_HIP(hipMemcpyAsync(bgra, t->bgra, t->npix() * 4, hipMemcpyDeviceToHost, t->stream));
    IQT_HIP(hipStreamSynchronize(t->stream));
    return IQPT_OK;
}

int iqpt_temporal_output_device(iqpt_temporal* t, const void** out_device) {
    if (!t || !out_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    *out_device = t->out;
    return IQPT_OK;
}

int iqpt_temporal_copy_frame_device(iqpt_temporal* t, void* dst_device, size_t bytes) {
    if (!t || !dst_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (!t->have_result) return iqpt::fail(IQPT_ERR_NOT_READY, "copy before a resolve of the current view");
    if (bytes != t->npix() * 4) return iqpt::fail(IQPT_ERR_INVALID_ARG, "bytes must be width*height*4");
    if (int st = set_device(t)) return st;
    IQT_HIP(hipMemcpyAsync(dst_device, t->bgra, bytes, hipMemcpyDeviceToDevice, t->stream));
    IQT_HIP(hipStreamSynchronize(t->stream));
    return IQPT_OK;
}

int iqpt_temporal_sync(iqpt_temporal* t) {
    if (!t) return iqpt::fail(IQPT_ERR_INVALID_ARG, "temporal object is NULL");
    if (int st = set_device(t)) return st;
    IQT_HIP(hipStreamSynchronize(t->stream));
    return IQPT_OK;
}

int iqpt_temporal_time(iqpt_temporal* t, double* view_ms, uint64_t* views, double* resolve_ms, uint64_t* resolves) {
    if (!t || !view_ms || !views || !resolve_ms || !resolves) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = set_device(t)) return st;
    if (int st = collect(t->view_t)) return st;
    if (int st = collect(t->resolve_t)) return st;
    *view_ms = t->view_t.ms;
    *views = t->view_t.count;
    *resolve_ms = t->resolve_t.ms;
    *resolves = t->resolve_t.count;
    t->view_t.ms = t->resolve_t.ms = 0.0;
    t->view_t.count = t->resolve_t.count = 0;
    return IQPT_OK;
}

int iqpt_temporal_stats(iqpt_temporal* t, uint64_t* guided, uint64_t* valid) {
    if (!t || !guided || !valid) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (!t->have_view) return iqpt::fail(IQPT_ERR_NOT_READY, "stats before the first begin_view");
    if (int st = set_device(t)) return st;
    unsigned long long host[2] = {0, 0};
    IQT_HIP(hipMemsetAsync(t->counts, 0, sizeof host, t->stream));
    IQT_HIP(iqt::launch_stats(t->stream, (uint32_t)t->npix(), t->planes[t->cur].id, t->hist, t->counts));
    IQT_HIP(hipMemcpyAsync(host, t->counts, sizeof host, hipMemcpyDeviceToHost, t->stream));
    IQT_HIP(hipStreamSynchronize(t->stream));
    *guided = host[0];
    *valid = host[1];
    return IQPT_OK;
}

}  // extern "C"
