// iq_svgf.cpp — the iqpt_svgf_* C ABI (include/svgf/iqpt_svgf.h): two iqpt_temporal objects driven through their
// public C ABI (the colour history and the moments history), the guide planes kept for the filter, and per
// resolve the moments kernel, both histories' resolves, the variance kernel and one launch per level on the
// object's own stream; readback, timing and the counts. The kernels are iq_svgf_kernels.hip; the definition is
// DESIGN.md §12.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "iqpt_internal.hpp"
#include "raster/iq_raster.hpp"
#include "svgf/iq_svgf.hpp"
#include "svgf/iqpt_svgf.h"

namespace {

int hip_fail(hipError_t e, const char* what) {
    return iqpt::fail(IQPT_ERR_HIP, std::string(what) + ": " + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ")");
}

#define IQS_HIP(call)                                        \
    do {                                                     \
        hipError_t e_ = (call);                              \
        if (e_ != hipSuccess) return hip_fail(e_, #call);    \
    } while (0)

constexpr int kMaxLevels = IQPT_SVGF_MAX_LEVELS;
// DESIGN.md §12.5 "Defaults": §11's three temporal values (not measured), §10.5's q and s_z, and the lowest mean
// RMSE ratio of tools/svgf_sweep.py's grid for min_history, levels, colour_sigma and variance_floor
constexpr iqpt_svgf_params kDefaults = {0.9f, 0.01f, 256u, 2u, 4u, 5u, 1024.0f, 8.0f, 0.01f};

int check_params(const iqpt_svgf_params& p) {
    if (!std::isfinite(p.normal_min)) return iqpt::fail(IQPT_ERR_INVALID_ARG, "normal_min must be finite");
    if (!(p.plane_tolerance >= 0.0f)) return iqpt::fail(IQPT_ERR_INVALID_ARG, "plane_tolerance must be >= 0");
    if (p.max_history < 1u || p.max_history > IQPT_TEMPORAL_MAX_HISTORY)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "max_history must be 1..2^24");
    if (p.min_history < 1u || p.min_history > IQPT_TEMPORAL_MAX_HISTORY)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "min_history must be 1..2^24");
    if (p.levels > IQPT_SVGF_MAX_LEVELS) return iqpt::fail(IQPT_ERR_INVALID_ARG, "levels must be 0..8");
    if (p.normal_squarings > IQPT_SVGF_MAX_SQUARINGS) return iqpt::fail(IQPT_ERR_INVALID_ARG, "normal_squarings must be 0..7");
    if (!std::isfinite(p.depth_sharpness) || !(p.depth_sharpness >= 0.0f))
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "depth_sharpness must be finite and >= 0");
    if (!std::isfinite(p.colour_sigma) || !(p.colour_sigma >= 0.0f))
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "colour_sigma must be finite and >= 0");
    if (!std::isfinite(p.variance_floor) || !(p.variance_floor > 0.0f))
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "variance_floor must be finite and > 0");
    return IQPT_OK;
}

}  // namespace

struct iqpt_svgf {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t width = 0, height = 0;
    iqpt_svgf_params params = kDefaults;
    iqpt_temporal* colour_t = nullptr;     // §11 unchanged
    iqpt_temporal* moments_t = nullptr;    // the same camera, planes and n, fed (L, L L, +0, +0)
    void* normal_z = nullptr;              // npix float4: the current view's guides, for the filter
    uint32_t* id = nullptr;                // npix
    void* input = nullptr;                 // npix float4: a host colour, or the accumulator resolve_ctx takes
    void* moments = nullptr;               // npix float4: M of the colour being resolved
    void* c0 = nullptr;                    // npix float4: (o.xyz, v)
    void* colour[2] = {};                  // npix float4 each: the levels ping-pong between them
    uint32_t* bgra = nullptr;              // npix
    uint32_t* spatial = nullptr;           // one per block, device: the spatial-estimate counts of the last resolve
    const void* result = nullptr;          // c0 or one of colour[]
    bool have_view = false, have_result = false;
    hipEvent_t ev_moments[2] = {};
    hipEvent_t ev[kMaxLevels + 2] = {};    // before the variance kernel, after it, after every level
    uint32_t pending_levels = 0;
    bool pending = false;                  // the events of the last resolve have not been added up yet
    double moments_ms = 0.0, variance_ms = 0.0, level_ms[kMaxLevels] = {};
    uint64_t resolves = 0;
    size_t npix() const { return (size_t)width * height; }
};

namespace {

int set_device(iqpt_svgf* s) {
    IQS_HIP(hipSetDevice(s->device));
    return IQPT_OK;
}

int collect(iqpt_svgf* s) {
    if (!s->pending) return IQPT_OK;
    IQS_HIP(hipEventSynchronize(s->ev[1 + s->pending_levels]));
    float ms = 0.0f;
    IQS_HIP(hipEventElapsedTime(&ms, s->ev_moments[0], s->ev_moments[1]));
    s->moments_ms += ms;
    IQS_HIP(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
    s->variance_ms += ms;
    for (uint32_t k = 0; k < s->pending_levels; ++k) {
        IQS_HIP(hipEventElapsedTime(&ms, s->ev[1 + k], s->ev[2 + k]));
        s->level_ms[k] += ms;
    }
    s->resolves += 1;
    s->pending = false;
    return IQPT_OK;
}

int check_camera(const iqpt_svgf* s, const iqpt_camera* cam) {
    if (cam->width != s->width || cam->height != s->height)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "camera size differs from the frame's");
    return IQPT_OK;
}

// the new view's planes are in s->normal_z / s->id already: both histories take them from there
int begin(iqpt_svgf* s, const iqpt_camera* cam) {
    s->have_view = false;
    s->have_result = false;
    if (int st = iqpt_temporal_begin_view_device(s->colour_t, cam, s->normal_z, s->id)) return st;
    if (int st = iqpt_temporal_begin_view_device(s->moments_t, cam, s->normal_z, s->id)) return st;
    s->have_view = true;
    return IQPT_OK;
}

int resolve(iqpt_svgf* s, const void* colour_device, uint64_t n) {
    if (!s->have_view) return iqpt::fail(IQPT_ERR_NOT_READY, "resolve before the first begin_view");
    if (int st = collect(s)) return st;
    hipStream_t q = s->stream;
    const iqpt_svgf_params& p = s->params;
    // M on the object's stream, waited for: the moments history reads it on a stream of its own
    IQS_HIP(hipEventRecord(s->ev_moments[0], q));
    IQS_HIP(iqs::launch_moments(q, (uint32_t)s->npix(), colour_device, s->moments));
    IQS_HIP(hipEventRecord(s->ev_moments[1], q));
    IQS_HIP(hipStreamSynchronize(q));
    if (int st = iqpt_temporal_resolve_device(s->colour_t, colour_device, n)) return st;
    if (int st = iqpt_temporal_resolve_device(s->moments_t, s->moments, n)) return st;
    const void *o = nullptr, *mu = nullptr;
    if (int st = iqpt_temporal_output_device(s->colour_t, &o)) return st;
    if (int st = iqpt_temporal_output_device(s->moments_t, &mu)) return st;
    if (int st = iqpt_temporal_sync(s->colour_t)) return st;
    if (int st = iqpt_temporal_sync(s->moments_t)) return st;

    const float nf = (float)(n > IQPT_TEMPORAL_MAX_HISTORY ? (uint64_t)IQPT_TEMPORAL_MAX_HISTORY : n);
    iqs::variance_params vp;
    vp.width = s->width;
    vp.height = s->height;
    vp.ne = std::fmax(nf, 1.0f);
    vp.min_weight = (float)p.min_history * vp.ne;
    IQS_HIP(hipEventRecord(s->ev[0], q));
    IQS_HIP(iqs::launch_variance(q, vp, o, mu, s->id, s->c0, s->spatial));
    IQS_HIP(hipEventRecord(s->ev[1], q));
    s->result = s->c0;
    if (p.levels == 0) {
        IQS_HIP(iqs::launch_encode(q, s->width, s->height, s->c0, s->bgra));
        IQS_HIP(hipEventRecord(s->ev[2], q));
    }
    const void* in = s->c0;
    for (uint32_t i = 0; i < p.levels; ++i) {
        iqs::level_params lp;
        lp.width = s->width;
        lp.height = s->height;
        lp.step = 1 << i;
        lp.squarings = p.normal_squarings;
        lp.depth_sharpness = p.depth_sharpness;
        lp.sigma2 = p.colour_sigma * p.colour_sigma;
        lp.variance_floor = p.variance_floor;
        void* out = s->colour[i & 1u];
        IQS_HIP(iqs::launch_level(q, lp, in, s->normal_z, s->id, out, i + 1 == p.levels ? s->bgra : nullptr));
        IQS_HIP(hipEventRecord(s->ev[2 + i], q));
        in = out;
        s->result = out;
    }
    s->pending_levels = p.levels ? p.levels : 1u;
    s->pending = true;
    s->have_result = true;
    return IQPT_OK;
}

}  // namespace

extern "C" {

int iqpt_svgf_default_params(iqpt_svgf_params* out) {
    if (!out) return iqpt::fail(IQPT_ERR_INVALID_ARG, "out is NULL");
    *out = kDefaults;
    return IQPT_OK;
}

int iqpt_svgf_create(int device, uint32_t width, uint32_t height, iqpt_svgf** out) {
    if (!out) return iqpt::fail(IQPT_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (width == 0 || height == 0 || width > IQPT_RASTER_MAX_DIM || height > IQPT_RASTER_MAX_DIM)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "frame size must be 1..8192 in each dimension");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return iqpt::fail(IQPT_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= count) return iqpt::fail(IQPT_ERR_NO_DEVICE, "device index out of range");

    iqpt_svgf* s = new iqpt_svgf();
    s->device = device;
    s->width = width;
    s->height = height;
    auto fail_with = [&](hipError_t e, const char* what) {
        const int st = hip_fail(e, what);
        iqpt_svgf_destroy(s);
        return st;
    };
    auto fail_status = [&](int st) {
        const std::string detail = iqpt_last_error();      // destroy must not lose it
        iqpt_svgf_destroy(s);
        return iqpt::fail(st, detail);
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return fail_with(e, "hipSetDevice");
    if ((e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking)) != hipSuccess) return fail_with(e, "hipStreamCreate");
    for (hipEvent_t& ev : s->ev_moments)
        if ((e = hipEventCreate(&ev)) != hipSuccess) return fail_with(e, "hipEventCreate");
    for (hipEvent_t& ev : s->ev)
        if ((e = hipEventCreate(&ev)) != hipSuccess) return fail_with(e, "hipEventCreate");
    if (int st = iqpt_temporal_create(device, width, height, &s->colour_t)) return fail_status(st);
    if (int st = iqpt_temporal_create(device, width, height, &s->moments_t)) return fail_status(st);
    const size_t n = s->npix();
    if ((e = hipMalloc(&s->normal_z, n * 16)) != hipSuccess) return fail_with(e, "hipMalloc(normal_z)");
    if ((e = hipMalloc((void**)&s->id, n * 4)) != hipSuccess) return fail_with(e, "hipMalloc(id)");
    if ((e = hipMalloc(&s->input, n * 16)) != hipSuccess) return fail_with(e, "hipMalloc(input)");
    if ((e = hipMalloc(&s->moments, n * 16)) != hipSuccess) return fail_with(e, "hipMalloc(moments)");
    if ((e = hipMalloc(&s->c0, n * 16)) != hipSuccess) return fail_with(e, "hipMalloc(c0)");
    if ((e = hipMalloc(&s->colour[0], n * 16)) != hipSuccess) return fail_with(e, "hipMalloc(colour)");
    if ((e = hipMalloc(&s->colour[1], n * 16)) != hipSuccess) return fail_with(e, "hipMalloc(colour)");
    if ((e = hipMalloc((void**)&s->bgra, n * 4)) != hipSuccess) return fail_with(e, "hipMalloc(bgra)");
    if ((e = hipMalloc((void**)&s->spatial, iqs::num_blocks(width, height) * 4)) != hipSuccess) return fail_with(e, "hipMalloc(spatial)");
    iqpt_temporal_params tp = {kDefaults.normal_min, kDefaults.plane_tolerance, kDefaults.max_history};
    if (int st = iqpt_temporal_set_params(s->colour_t, &tp)) return fail_status(st);
    if (int st = iqpt_temporal_set_params(s->moments_t, &tp)) return fail_status(st);
    *out = s;
    return IQPT_OK;
}

int iqpt_svgf_destroy(iqpt_svgf* s) {
    if (!s) return IQPT_OK;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    (void)iqpt_temporal_destroy(s->colour_t);
    (void)iqpt_temporal_destroy(s->moments_t);
    for (void* p : {s->normal_z, (void*)s->id, s->input, s->moments, s->c0, s->colour[0], s->colour[1], (void*)s->bgra,
                    (void*)s->spatial})
        if (p) (void)hipFree(p);
    for (hipEvent_t ev : s->ev_moments)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : s->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
    return IQPT_OK;
}

int iqpt_svgf_set_params(iqpt_svgf* s, const iqpt_svgf_params* p) {
    if (!p) return iqpt::fail(IQPT_ERR_INVALID_ARG, "params is NULL");
    if (int st = check_params(*p)) return st;
    if (!s) return iqpt::fail(IQPT_ERR_INVALID_ARG, "svgf object is NULL");
    const iqpt_temporal_params tp = {p->normal_min, p->plane_tolerance, p->max_history};
    if (int st = iqpt_temporal_set_params(s->colour_t, &tp)) return st;
    if (int st = iqpt_temporal_set_params(s->moments_t, &tp)) return st;
    s->params = *p;
    return IQPT_OK;
}

int iqpt_svgf_begin_view(iqpt_svgf* s, const iqpt_camera* cam, const float* normal_z, const uint32_t* id) {
    if (!s || !cam || !normal_z || !id) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = check_camera(s, cam)) return st;
    if (int st = set_device(s)) return st;
    IQS_HIP(hipStreamSynchronize(s->stream));      // levels in flight may still read the old planes
    IQS_HIP(hipMemcpyAsync(s->normal_z, normal_z, s->npix() * 16, hipMemcpyHostToDevice, s->stream));
    IQS_HIP(hipMemcpyAsync(s->id, id, s->npix() * 4, hipMemcpyHostToDevice, s->stream));
    IQS_HIP(hipStreamSynchronize(s->stream));      // the caller's arrays may go away
    return begin(s, cam);
}

int iqpt_svgf_begin_view_device(iqpt_svgf* s, const iqpt_camera* cam, const void* normal_z_device, const void* id_device) {
    if (!s || !cam || !normal_z_device || !id_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = check_camera(s, cam)) return st;
    if (int st = set_device(s)) return st;
    IQS_HIP(hipStreamSynchronize(s->stream));
    IQS_HIP(hipMemcpyAsync(s->normal_z, normal_z_device, s->npix() * 16, hipMemcpyDeviceToDevice, s->stream));
    IQS_HIP(hipMemcpyAsync(s->id, id_device, s->npix() * 4, hipMemcpyDeviceToDevice, s->stream));
    IQS_HIP(hipStreamSynchronize(s->stream));      // the caller's planes may change (the G-buffer of the next camera)
    return begin(s, cam);
}

int iqpt_svgf_begin_view_raster(iqpt_svgf* s, iqpt_raster* r) {
    if (!s || !r) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    uint32_t rw = 0, rh = 0;
    iqr::frame_size(r, &rw, &rh);
    if (rw != s->width || rh != s->height) return iqpt::fail(IQPT_ERR_INVALID_ARG, "the rasterizer's frame size differs from the object's");
    const iqpt_camera* cam = iqr::current_camera(r);
    if (!cam) return iqpt::fail(IQPT_ERR_NOT_READY, "begin_view_raster before the rasterizer's set_camera");
    if (int st = iqpt_raster_gbuffer(r)) return st;
    const void *nz = nullptr, *id = nullptr;
    if (int st = iqpt_raster_gbuffer_device(r, &nz, &id)) return st;
    return iqpt_svgf_begin_view_device(s, cam, nz, id);
}

int iqpt_svgf_clear(iqpt_svgf* s) {
    if (!s) return iqpt::fail(IQPT_ERR_INVALID_ARG, "svgf object is NULL");
    if (int st = iqpt_temporal_clear(s->colour_t)) return st;
    if (int st = iqpt_temporal_clear(s->moments_t)) return st;
    s->have_view = false;
    s->have_result = false;
    return IQPT_OK;
}

int iqpt_svgf_resolve(iqpt_svgf* s, const float* colour, uint64_t n) {
    if (!s || !colour) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (!s->have_view) return iqpt::fail(IQPT_ERR_NOT_READY, "resolve before the first begin_view");
    if (int st = set_device(s)) return st;
    IQS_HIP(hipMemcpyAsync(s->input, colour, s->npix() * 16, hipMemcpyHostToDevice, s->stream));
    IQS_HIP(hipStreamSynchronize(s->stream));      // the caller's array may go away
    return resolve(s, s->input, n);
}

int iqpt_svgf_resolve_device(iqpt_svgf* s, const void* colour_device, uint64_t n) {
    if (!s || !colour_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = set_device(s)) return st;
    return resolve(s, colour_device, n);
}

int iqpt_svgf_resolve_ctx(iqpt_svgf* s, iqpt_ctx* ctx) {
    if (!s || !ctx) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    uint64_t npix = 0, frames = 0;
    if (int st = iqpt_num_pixels(ctx, &npix)) return st;
    if (npix != s->npix()) return iqpt::fail(IQPT_ERR_INVALID_ARG, "the context does not own a whole frame of the object's size");
    if (!s->have_view) return iqpt::fail(IQPT_ERR_NOT_READY, "resolve before the first begin_view");
    if (int st = set_device(s)) return st;
    if (int st = iqpt_copy_accum_device(ctx, s->input, s->npix() * 16)) return st;
    if (int st = iqpt_frame_count(ctx, &frames)) return st;
    return resolve(s, s->input, frames);
}

int iqpt_svgf_read(iqpt_svgf* s, float* lin_rgba, uint8_t* bgra) {
    if (!s) return iqpt::fail(IQPT_ERR_INVALID_ARG, "svgf object is NULL");
    if (!s->have_result) return iqpt::fail(IQPT_ERR_NOT_READY, "read before a resolve of the current view");
    if (int st = set_device(s)) return st;
    if (lin_rgba) IQS_HIP(hipMemcpyAsync(lin_rgba, s->result, s->npix() * 16, hipMemcpyDeviceToHost, s->stream));
    if (bgra) IQS_HIP(hipMemcpyAsync(bgra, s->bgra, s->npix() * 4, hipMemcpyDeviceToHost, s->stream));
    IQS_HIP(hipStreamSynchronize(s->stream));
    return IQPT_OK;
}

int iqpt_svgf_read_stages(iqpt_svgf* s, float* temporal_rgba, float* variance_rgba) {
    if (!s) return iqpt::fail(IQPT_ERR_INVALID_ARG, "svgf object is NULL");
    if (!s->have_result) return iqpt::fail(IQPT_ERR_NOT_READY, "read before a resolve of the current view");
    if (int st = set_device(s)) return st;
    if (temporal_rgba)
        if (int st = iqpt_temporal_read(s->colour_t, temporal_rgba, nullptr)) return st;
    if (variance_rgba) IQS_HIP(hipMemcpyAsync(variance_rgba, s->c0, s->npix() * 16, hipMemcpyDeviceToHost, s->stream));
    IQS_HIP(hipStreamSynchronize(s->stream));
    return IQPT_OK;
}

int iqpt_svgf_copy_frame_device(iqpt_svgf* s, void* dst_device, size_t bytes) {
    if (!s || !dst_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (!s->have_result) return iqpt::fail(IQPT_ERR_NOT_READY, "copy before a resolve of the current view");
    if (bytes != s->npix() * 4) return iqpt::fail(IQPT_ERR_INVALID_ARG, "bytes must be width*height*4");
    if (int st = set_device(s)) return st;
    IQS_HIP(hipMemcpyAsync(dst_device, s->bgra, bytes, hipMemcpyDeviceToDevice, s->stream));
    IQS_HIP(hipStreamSynchronize(s->stream));
    return IQPT_OK;
}

int iqpt_svgf_sync(iqpt_svgf* s) {
    if (!s) return iqpt::fail(IQPT_ERR_INVALID_ARG, "svgf object is NULL");
    if (int st = set_device(s)) return st;
    if (int st = iqpt_temporal_sync(s->colour_t)) return st;
    if (int st = iqpt_temporal_sync(s->moments_t)) return st;
    IQS_HIP(hipStreamSynchronize(s->stream));
    return IQPT_OK;
}

int iqpt_svgf_time(iqpt_svgf* s, double* moments_ms, double* variance_ms, double* level_ms, uint64_t* resolves,
                   double* view_ms, double* history_resolve_ms) {
    if (!s || !moments_ms || !variance_ms || !resolves) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = set_device(s)) return st;
    if (int st = collect(s)) return st;
    iqpt_temporal* both[2] = {s->colour_t, s->moments_t};
    for (int k = 0; k < 2; ++k) {
        double vms = 0.0, rms = 0.0;
        uint64_t nv = 0, nr = 0;
        if (int st = iqpt_temporal_time(both[k], &vms, &nv, &rms, &nr)) return st;
        if (view_ms) view_ms[k] = vms;
        if (history_resolve_ms) history_resolve_ms[k] = rms;
    }
    *moments_ms = s->moments_ms;
    *variance_ms = s->variance_ms;
    *resolves = s->resolves;
    for (int k = 0; k < kMaxLevels; ++k) {
        if (level_ms) level_ms[k] = s->level_ms[k];
        s->level_ms[k] = 0.0;
    }
    s->moments_ms = s->variance_ms = 0.0;
    s->resolves = 0;
    return IQPT_OK;
}

int iqpt_svgf_stats(iqpt_svgf* s, uint64_t* guided, uint64_t* valid, uint64_t* spatial) {
    if (!s || !guided || !valid || !spatial) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (!s->have_view) return iqpt::fail(IQPT_ERR_NOT_READY, "stats before the first begin_view");
    if (int st = set_device(s)) return st;
    if (int st = iqpt_temporal_stats(s->colour_t, guided, valid)) return st;
    uint64_t sum = 0;
    if (s->have_result) {
        std::vector<uint32_t> host(iqs::num_blocks(s->width, s->height));
        IQS_HIP(hipMemcpyAsync(host.data(), s->spatial, host.size() * 4, hipMemcpyDeviceToHost, s->stream));
        IQS_HIP(hipStreamSynchronize(s->stream));
        for (uint32_t c : host) sum += c;
    }
    *spatial = sum;
    return IQPT_OK;
}

}  // extern "C"
