// iq_svgf.cpp — the iqpt_svgf_* C ABI (include/svgf/iqpt_svgf.h): two iqpt_temporal objects driven through their
// public C ABI (the colour history and the moments history), the guide planes kept for the filter, and per
// resolve the moments kernel, both histories' resolves, the variance kernel and one launch per level on the
// object's own stream; readback, timing and the counts. The kernels are iq_svgf_kernels.hip; the definition is
// DESIGN.md §12.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "post/iq_post.hpp"
#include "svgf/iq_svgf.hpp"
#include "svgf/iqpt_svgf.h"
#include "temporal/iq_temporal.hpp"

namespace {

constexpr int kMaxLevels = IQPT_SVGF_MAX_LEVELS;
// DESIGN.md §12.5 "Defaults": §11's three temporal values (not measured), §10.5's q and s_z, and the lowest mean
// RMSE ratio of tools/svgf_sweep.py's grid for min_history, levels, colour_sigma and variance_floor
constexpr iqpt_svgf_params kDefaults = {0.9f, 0.01f, 256u, 2u, 4u, 5u, 1024.0f, 8.0f, 0.01f};

int check_params(const iqpt_svgf_params& p) {
    if (int st = iqt::check_params({p.normal_min, p.plane_tolerance, p.max_history})) return st;
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

struct iqpt_svgf : iqp::frame {
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
    iqp::event_timer moments_tm;           // ev[0], ev[1] around the moments kernel
    // ev[0], ev[1] around the variance kernel, ev[2 + i] after level i (or after the encoding, levels = 0)
    iqp::event_timer chain_tm;
};
static_assert(kMaxLevels + 2 <= iqp::event_timer::kMaxEvents, "an event after every level");

namespace {

// the chain's last event is the stream's last, so the moments kernel's pair needs no wait of its own
int collect(iqpt_svgf* s) {
    if (int st = s->chain_tm.collect()) return st;
    return s->moments_tm.collect(false);
}

}  // namespace

namespace {

// the new view's planes are in s->normal_z / s->id already: both histories take them from there
int begin(iqpt_svgf* s, const iqpt_camera* cam) {
    s->have_view = false;
    s->have_result = false;
    if (int st = iqpt_temporal_begin_view_device(s->colour_t, cam, s->normal_z, s->id)) return st;
    if (int st = iqpt_temporal_begin_view_device(s->moments_t, cam, s->normal_z, s->id)) return st;
    s->have_view = true;
    return IQPT_OK;
}

int begin_planes(iqpt_svgf* s, const iqpt_camera* cam, const void* normal_z, const void* id, hipMemcpyKind kind) {
    if (int st = iqp::check_camera(*s, cam)) return st;
    if (int st = iqp::set_device(*s)) return st;
    IQPT_HIP(hipStreamSynchronize(s->stream));      // levels in flight may still read the old planes
    if (int st = iqp::copy_guides(*s, s->normal_z, s->id, normal_z, id, kind)) return st;
    return begin(s, cam);
}

int resolve(iqpt_svgf* s, const void* colour_device, uint64_t n) {
    if (!s->have_view) return iqpt::fail(IQPT_ERR_NOT_READY, "resolve before the first begin_view");
    if (int st = collect(s)) return st;
    hipStream_t q = s->stream;
    const iqpt_svgf_params& p = s->params;
    // M on the object's stream, waited for: the moments history reads it on a stream of its own
    IQPT_HIP(hipEventRecord(s->moments_tm.ev[0], q));
    IQPT_HIP(iqs::launch_moments(q, (uint32_t)s->npix(), colour_device, s->moments));
    IQPT_HIP(hipEventRecord(s->moments_tm.ev[1], q));
    IQPT_HIP(hipStreamSynchronize(q));
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
    IQPT_HIP(hipEventRecord(s->chain_tm.ev[0], q));
    IQPT_HIP(iqs::launch_variance(q, vp, o, mu, s->id, s->c0, s->spatial));
    IQPT_HIP(hipEventRecord(s->chain_tm.ev[1], q));
    s->result = s->c0;
    if (p.levels == 0) {
        IQPT_HIP(iqp::launch_encode(q, s->width, s->height, s->c0, s->bgra));
        IQPT_HIP(hipEventRecord(s->chain_tm.ev[2], q));
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
        IQPT_HIP(iqs::launch_level(q, lp, in, s->normal_z, s->id, out, i + 1 == p.levels ? s->bgra : nullptr));
        IQPT_HIP(hipEventRecord(s->chain_tm.ev[2 + i], q));
        in = out;
        s->result = out;
    }
    s->moments_tm.recorded = 2;
    s->chain_tm.recorded = 2 + (int)(p.levels ? p.levels : 1u);
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
    return iqp::frame_create(device, width, height, out, iqpt_svgf_destroy, [](iqpt_svgf* s) {
        if (int st = s->moments_tm.create(2)) return st;
        if (int st = s->chain_tm.create(kMaxLevels + 2)) return st;
        if (int st = iqpt_temporal_create(s->device, s->width, s->height, &s->colour_t)) return st;
        if (int st = iqpt_temporal_create(s->device, s->width, s->height, &s->moments_t)) return st;
        const size_t n = s->npix();
        if (int st = iqp::frame_alloc(*s, {{&s->normal_z, n * 16, "hipMalloc(normal_z)"},
                                           {(void**)&s->id, n * 4, "hipMalloc(id)"},
                                           {&s->input, n * 16, "hipMalloc(input)"},
                                           {&s->moments, n * 16, "hipMalloc(moments)"},
                                           {&s->c0, n * 16, "hipMalloc(c0)"},
                                           {&s->colour[0], n * 16, "hipMalloc(colour)"},
                                           {&s->colour[1], n * 16, "hipMalloc(colour)"},
                                           {(void**)&s->bgra, n * 4, "hipMalloc(bgra)"},
                                           {(void**)&s->spatial, iqp::num_blocks(s->width, s->height) * 4, "hipMalloc(spatial)"}}))
            return st;
        const iqpt_temporal_params tp = {kDefaults.normal_min, kDefaults.plane_tolerance, kDefaults.max_history};
        if (int st = iqpt_temporal_set_params(s->colour_t, &tp)) return st;
        return iqpt_temporal_set_params(s->moments_t, &tp);
    });
}

// The object's own stream first: its variance kernel reads both histories' results. Nothing of theirs reads this
// object's buffers by then (resolve waits for both), so they go after it.
int iqpt_svgf_destroy(iqpt_svgf* s) {
    if (!s) return IQPT_OK;
    iqp::frame_close(*s, {&s->moments_tm, &s->chain_tm});
    (void)iqpt_temporal_destroy(s->colour_t);
    (void)iqpt_temporal_destroy(s->moments_t);
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
    return begin_planes(s, cam, normal_z, id, hipMemcpyHostToDevice);
}

int iqpt_svgf_begin_view_device(iqpt_svgf* s, const iqpt_camera* cam, const void* normal_z_device, const void* id_device) {
    if (!s || !cam || !normal_z_device || !id_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    return begin_planes(s, cam, normal_z_device, id_device, hipMemcpyDeviceToDevice);
}

int iqpt_svgf_begin_view_raster(iqpt_svgf* s, iqpt_raster* r) {
    if (!s || !r) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    const iqpt_camera* cam = nullptr;
    const void *nz = nullptr, *id = nullptr;
    if (int st = iqp::raster_view(*s, r, "the object's", &cam, &nz, &id)) return st;
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
    if (int st = iqp::set_device(*s)) return st;
    IQPT_HIP(hipMemcpyAsync(s->input, colour, s->npix() * 16, hipMemcpyHostToDevice, s->stream));
    IQPT_HIP(hipStreamSynchronize(s->stream));      // the caller's array may go away
    return resolve(s, s->input, n);
}

int iqpt_svgf_resolve_device(iqpt_svgf* s, const void* colour_device, uint64_t n) {
    if (!s || !colour_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = iqp::set_device(*s)) return st;
    return resolve(s, colour_device, n);
}

int iqpt_svgf_resolve_ctx(iqpt_svgf* s, iqpt_ctx* ctx) {
    if (!s || !ctx) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    uint64_t npix = 0, frames = 0;
    if (int st = iqpt_num_pixels(ctx, &npix)) return st;
    if (npix != s->npix()) return iqpt::fail(IQPT_ERR_INVALID_ARG, "the context does not own a whole frame of the object's size");
    if (!s->have_view) return iqpt::fail(IQPT_ERR_NOT_READY, "resolve before the first begin_view");
    if (int st = iqp::set_device(*s)) return st;
    if (int st = iqpt_copy_accum_device(ctx, s->input, s->npix() * 16)) return st;
    if (int st = iqpt_frame_count(ctx, &frames)) return st;
    return resolve(s, s->input, frames);
}

int iqpt_svgf_read(iqpt_svgf* s, float* lin_rgba, uint8_t* bgra) {
    if (!s) return iqpt::fail(IQPT_ERR_INVALID_ARG, "svgf object is NULL");
    if (!s->have_result) return iqpt::fail(IQPT_ERR_NOT_READY, "read before a resolve of the current view");
    return iqp::read_planes(*s, lin_rgba, s->result, bgra, s->bgra);
}

int iqpt_svgf_read_stages(iqpt_svgf* s, float* temporal_rgba, float* variance_rgba) {
    if (!s) return iqpt::fail(IQPT_ERR_INVALID_ARG, "svgf object is NULL");
    if (!s->have_result) return iqpt::fail(IQPT_ERR_NOT_READY, "read before a resolve of the current view");
    if (int st = iqp::set_device(*s)) return st;
    if (temporal_rgba)
        if (int st = iqpt_temporal_read(s->colour_t, temporal_rgba, nullptr)) return st;
    if (variance_rgba) IQPT_HIP(hipMemcpyAsync(variance_rgba, s->c0, s->npix() * 16, hipMemcpyDeviceToHost, s->stream));
    IQPT_HIP(hipStreamSynchronize(s->stream));
    return IQPT_OK;
}

int iqpt_svgf_copy_frame_device(iqpt_svgf* s, void* dst_device, size_t bytes) {
    if (!s || !dst_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (!s->have_result) return iqpt::fail(IQPT_ERR_NOT_READY, "copy before a resolve of the current view");
    return iqp::copy_bgra(*s, s->bgra, dst_device, bytes);
}

int iqpt_svgf_sync(iqpt_svgf* s) {
    if (!s) return iqpt::fail(IQPT_ERR_INVALID_ARG, "svgf object is NULL");
    if (int st = iqp::set_device(*s)) return st;
    if (int st = iqpt_temporal_sync(s->colour_t)) return st;
    if (int st = iqpt_temporal_sync(s->moments_t)) return st;
    IQPT_HIP(hipStreamSynchronize(s->stream));
    return IQPT_OK;
}

int iqpt_svgf_time(iqpt_svgf* s, double* moments_ms, double* variance_ms, double* level_ms, uint64_t* resolves,
                   double* view_ms, double* history_resolve_ms) {
    if (!s || !moments_ms || !variance_ms || !resolves) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = iqp::set_device(*s)) return st;
    if (int st = collect(s)) return st;
    iqpt_temporal* both[2] = {s->colour_t, s->moments_t};
    for (int k = 0; k < 2; ++k) {
        double vms = 0.0, rms = 0.0;
        uint64_t nv = 0, nr = 0;
        if (int st = iqpt_temporal_time(both[k], &vms, &nv, &rms, &nr)) return st;
        if (view_ms) view_ms[k] = vms;
        if (history_resolve_ms) history_resolve_ms[k] = rms;
    }
    *moments_ms = s->moments_tm.ms[0];
    *variance_ms = s->chain_tm.ms[0];
    *resolves = s->chain_tm.runs;
    for (int k = 0; k < kMaxLevels; ++k)
        if (level_ms) level_ms[k] = s->chain_tm.ms[1 + k];
    s->moments_tm.reset();
    s->chain_tm.reset();
    return IQPT_OK;
}

int iqpt_svgf_stats(iqpt_svgf* s, uint64_t* guided, uint64_t* valid, uint64_t* spatial) {
    if (!s || !guided || !valid || !spatial) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (!s->have_view) return iqpt::fail(IQPT_ERR_NOT_READY, "stats before the first begin_view");
    if (int st = iqp::set_device(*s)) return st;
    if (int st = iqpt_temporal_stats(s->colour_t, guided, valid)) return st;
    uint64_t sum = 0;
    if (s->have_result) {
        std::vector<uint32_t> host(iqp::num_blocks(s->width, s->height));
        IQPT_HIP(hipMemcpyAsync(host.data(), s->spatial, host.size() * 4, hipMemcpyDeviceToHost, s->stream));
        IQPT_HIP(hipStreamSynchronize(s->stream));
        for (uint32_t c : host) sum += c;
    }
    *spatial = sum;
    return IQPT_OK;
}

}  // extern "C"
