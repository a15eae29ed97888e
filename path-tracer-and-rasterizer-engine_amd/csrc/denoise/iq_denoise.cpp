// iq_denoise.cpp — the iqpt_denoise_* C ABI (include/denoise/iqpt_denoise.h): the guide and colour buffers, one
// kernel launch per à-trous level on the denoiser's own stream, readback and timing. The kernels are
// iq_denoise_kernels.hip; the filter is DESIGN.md §10.
#include <hip/hip_runtime.h>

#include "denoise/iq_denoise.hpp"
#include "denoise/iqpt_denoise.h"
#include "post/iq_post.hpp"

namespace {

constexpr int kMaxLevels = IQPT_DENOISE_MAX_LEVELS;
// DESIGN.md §10.5 "Defaults": the lowest mean RMSE ratio of tools/denoise_sweep.py's grid
constexpr iqpt_denoise_params kDefaults = {4u, 5u, 1024.0f, 1.0f};

int check_params(const iqpt_denoise_params& p) {
    if (p.levels > IQPT_DENOISE_MAX_LEVELS) return iqpt::fail(IQPT_ERR_INVALID_ARG, "levels must be 0..8");
    if (p.normal_squarings > IQPT_DENOISE_MAX_SQUARINGS) return iqpt::fail(IQPT_ERR_INVALID_ARG, "normal_squarings must be 0..7");
    if (!(p.depth_sharpness >= 0.0f) || !(p.colour_sharpness >= 0.0f))
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "sharpnesses must be >= 0");
    return IQPT_OK;
}

}  // namespace

struct iqpt_denoise : iqp::frame {
    iqpt_denoise_params params = kDefaults;
    void* normal_z = nullptr;          // npix float4
    uint32_t* id = nullptr;            // npix
    void* input = nullptr;             // npix float4: a host colour, or the accumulator iqpt_denoise_frame takes
    void* colour[2] = {};              // npix float4 each: the levels ping-pong between them
    uint32_t* bgra = nullptr;          // npix
    bool have_guides = false;
    int result = -1;                   // which of colour[] holds the last result
    iqp::event_timer timer;            // ev[0] before the first level, ev[i + 1] after level i
};

namespace {

int set_guides(iqpt_denoise* d, const void* normal_z, const void* id, hipMemcpyKind kind) {
    if (int st = iqp::set_device(*d)) return st;
    if (int st = iqp::copy_guides(*d, d->normal_z, d->id, normal_z, id, kind)) return st;
    d->have_guides = true;
    return IQPT_OK;
}

int run(iqpt_denoise* d, const void* colour_device) {
    if (!d->have_guides) return iqpt::fail(IQPT_ERR_NOT_READY, "run before the guides were set");
    if (int st = d->timer.collect()) return st;
    hipStream_t s = d->stream;
    const iqpt_denoise_params& p = d->params;
    const float sc2 = p.colour_sharpness * p.colour_sharpness;
    IQPT_HIP(hipEventRecord(d->timer.ev[0], s));
    if (p.levels == 0) {
        IQPT_HIP(hipMemcpyAsync(d->colour[0], colour_device, d->npix() * 16, hipMemcpyDeviceToDevice, s));
        IQPT_HIP(iqp::launch_encode(s, d->width, d->height, d->colour[0], d->bgra));
        d->result = 0;
    }
    const void* in = colour_device;
    for (uint32_t i = 0; i < p.levels; ++i) {
        iqd::level_params lp;
        lp.width = d->width;
        lp.height = d->height;
        lp.step = 1 << i;
        lp.squarings = p.normal_squarings;
        lp.depth_sharpness = p.depth_sharpness;
        lp.colour_scale = sc2 * (float)(1u << (2 * i));
        const int o = (int)(i & 1u);
        IQPT_HIP(iqd::launch_level(s, lp, in, d->normal_z, d->id, d->colour[o], i + 1 == p.levels ? d->bgra : nullptr));
        IQPT_HIP(hipEventRecord(d->timer.ev[i + 1], s));
        in = d->colour[o];
        d->result = o;
    }
    d->timer.recorded = (int)p.levels + 1;
    return IQPT_OK;
}

}  // namespace

extern "C" {

int iqpt_denoise_default_params(iqpt_denoise_params* out) {
    if (!out) return iqpt::fail(IQPT_ERR_INVALID_ARG, "out is NULL");
    *out = kDefaults;
    return IQPT_OK;
}

int iqpt_denoise_create(int device, uint32_t width, uint32_t height, iqpt_denoise** out) {
    return iqp::frame_create(device, width, height, out, iqpt_denoise_destroy, [](iqpt_denoise* d) {
        if (int st = d->timer.create(kMaxLevels + 1)) return st;
        const size_t n = d->npix();
        return iqp::frame_alloc(*d, {{&d->normal_z, n * 16, "hipMalloc(normal_z)"},
                                     {(void**)&d->id, n * 4, "hipMalloc(id)"},
                                     {&d->input, n * 16, "hipMalloc(input)"},
                                     {&d->colour[0], n * 16, "hipMalloc(colour)"},
                                     {&d->colour[1], n * 16, "hipMalloc(colour)"},
                                     {(void**)&d->bgra, n * 4, "hipMalloc(bgra)"}});
    });
}

int iqpt_denoise_destroy(iqpt_denoise* d) {
    if (!d) return IQPT_OK;
    iqp::frame_close(*d, {&d->timer});
    delete d;
    return IQPT_OK;
}

int iqpt_denoise_set_params(iqpt_denoise* d, const iqpt_denoise_params* p) {
    if (!p) return iqpt::fail(IQPT_ERR_INVALID_ARG, "params is NULL");
    if (int st = check_params(*p)) return st;
    if (!d) return iqpt::fail(IQPT_ERR_INVALID_ARG, "denoiser is NULL");
    d->params = *p;
    return IQPT_OK;
}

int iqpt_denoise_set_guides(iqpt_denoise* d, const float* normal_z, const uint32_t* id) {
    if (!d || !normal_z || !id) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    return set_guides(d, normal_z, id, hipMemcpyHostToDevice);
}

int iqpt_denoise_set_guides_device(iqpt_denoise* d, const void* normal_z_device, const void* id_device) {
    if (!d || !normal_z_device || !id_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    return set_guides(d, normal_z_device, id_device, hipMemcpyDeviceToDevice);
}

int iqpt_denoise_run(iqpt_denoise* d, const float* colour) {
    if (!d || !colour) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = iqp::set_device(*d)) return st;
    IQPT_HIP(hipMemcpyAsync(d->input, colour, d->npix() * 16, hipMemcpyHostToDevice, d->stream));
    IQPT_HIP(hipStreamSynchronize(d->stream));      // the caller's array may go away
    return run(d, d->input);
}

int iqpt_denoise_run_device(iqpt_denoise* d, const void* colour_device) {
    if (!d || !colour_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = iqp::set_device(*d)) return st;
    return run(d, colour_device);
}

int iqpt_denoise_frame(iqpt_denoise* d, iqpt_ctx* ctx, iqpt_raster* r) {
    if (!d || !ctx || !r) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    uint64_t npix = 0;
    if (int st = iqpt_num_pixels(ctx, &npix)) return st;
    if (npix != d->npix()) return iqpt::fail(IQPT_ERR_INVALID_ARG, "the context does not own a whole frame of the denoiser's size");
    const void *nz = nullptr, *id = nullptr;
    if (int st = iqp::raster_view(*d, r, "the denoiser's", nullptr, &nz, &id)) return st;
    if (int st = iqp::set_device(*d)) return st;
    IQPT_HIP(hipStreamSynchronize(d->stream));      // a run in flight may still read d->input
    if (int st = iqpt_copy_accum_device(ctx, d->input, d->npix() * 16)) return st;
    if (int st = iqpt_denoise_set_guides_device(d, nz, id)) return st;
    return run(d, d->input);
}

int iqpt_denoise_read(iqpt_denoise* d, float* lin_rgba, uint8_t* bgra) {
    if (!d) return iqpt::fail(IQPT_ERR_INVALID_ARG, "denoiser is NULL");
    if (d->result < 0) return iqpt::fail(IQPT_ERR_NOT_READY, "read before the first run");
    return iqp::read_planes(*d, lin_rgba, d->colour[d->result], bgra, d->bgra);
}

int iqpt_denoise_copy_frame_device(iqpt_denoise* d, void* dst_device, size_t bytes) {
    if (!d || !dst_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (d->result < 0) return iqpt::fail(IQPT_ERR_NOT_READY, "copy before the first run");
    return iqp::copy_bgra(*d, d->bgra, dst_device, bytes);
}

int iqpt_denoise_sync(iqpt_denoise* d) {
    if (!d) return iqpt::fail(IQPT_ERR_INVALID_ARG, "denoiser is NULL");
    if (int st = iqp::set_device(*d)) return st;
    IQPT_HIP(hipStreamSynchronize(d->stream));
    return IQPT_OK;
}

int iqpt_denoise_time(iqpt_denoise* d, double* total_ms, double* level_ms, uint64_t* runs) {
    if (!d || !total_ms || !runs) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = iqp::set_device(*d)) return st;
    if (int st = d->timer.collect()) return st;
    *total_ms = d->timer.total_ms;
    *runs = d->timer.runs;
    for (int k = 0; k < kMaxLevels; ++k)
        if (level_ms) level_ms[k] = d->timer.ms[k];
    d->timer.reset();
    return IQPT_OK;
}

}  // extern "C"
