// iq_upscale.cpp — the iqpt_upscale_* C ABI (include/upscale/iqpt_upscale.h): the guide and colour buffers of
// both sizes, one kernel launch per run on the upscaler's own stream, readback, class counts on request and
// timing. The kernels are iq_upscale_kernels.hip; the definition is DESIGN.md §14.
#include <hip/hip_runtime.h>

#include <cstring>

#include "post/iq_post.hpp"
#include "upscale/iq_upscale.hpp"
#include "upscale/iqpt_upscale.h"

namespace {

// the denoiser's q and s_z; not measured for this stage
constexpr iqpt_upscale_params kDefaults = {5u, 1024.0f};

int check_params(const iqpt_upscale_params& p) {
    if (p.normal_squarings > IQPT_UPSCALE_MAX_SQUARINGS) return iqpt::fail(IQPT_ERR_INVALID_ARG, "normal_squarings must be 0..7");
    if (!(p.depth_sharpness >= 0.0f)) return iqpt::fail(IQPT_ERR_INVALID_ARG, "depth_sharpness must be >= 0");
    return IQPT_OK;
}

}  // namespace

// The frame the object is is the hi one; `lo` is the same device and stream with the lo size (it owns nothing).
struct iqpt_upscale : iqp::frame {
    iqpt_upscale_params params = kDefaults;
    iqp::frame lo;
    uint32_t factor = 0;
    void* normal_z_lo = nullptr;       // lo npix float4
    uint32_t* id_lo = nullptr;         // lo npix
    void* normal_z_hi = nullptr;       // npix float4
    uint32_t* id_hi = nullptr;         // npix
    void* input = nullptr;             // lo npix float4: a host colour, or the accumulator iqpt_upscale_frame takes
    void* out = nullptr;               // npix float4
    uint32_t* bgra = nullptr;          // npix
    unsigned long long* counts = nullptr;   // guided, widened, unguided: filled by iqpt_upscale_stats
    bool have_guides = false;
    bool have_result = false;
    iqp::event_timer timer;            // ev[0] before the kernel, ev[1] after it
};

namespace {

int set_guides(iqpt_upscale* u, const void* normal_z_lo, const void* id_lo, const void* normal_z_hi, const void* id_hi,
               hipMemcpyKind kind) {
    if (int st = iqp::set_device(*u)) return st;
    if (int st = iqp::copy_guides(u->lo, u->normal_z_lo, u->id_lo, normal_z_lo, id_lo, kind)) return st;
    if (int st = iqp::copy_guides(*u, u->normal_z_hi, u->id_hi, normal_z_hi, id_hi, kind)) return st;
    u->have_guides = true;
    return IQPT_OK;
}

int run(iqpt_upscale* u, const void* colour_lo_device) {
    if (!u->have_guides) return iqpt::fail(IQPT_ERR_NOT_READY, "run before the guides were set");
    if (int st = u->timer.collect()) return st;
    hipStream_t s = u->stream;
    iqu::run_params p;
    p.width = u->width;
    p.height = u->height;
    p.lo_width = u->lo.width;
    p.lo_height = u->lo.height;
    p.factor = u->factor;
    p.squarings = u->params.normal_squarings;
    p.depth_sharpness = u->params.depth_sharpness;
    const iqu::run_planes g = {colour_lo_device, u->normal_z_lo, u->id_lo, u->normal_z_hi, u->id_hi};
    IQPT_HIP(hipEventRecord(u->timer.ev[0], s));
    IQPT_HIP(iqu::launch_upscale(s, p, g, u->out, u->bgra));
    IQPT_HIP(hipEventRecord(u->timer.ev[1], s));
    u->timer.recorded = 2;
    u->have_result = true;
    return IQPT_OK;
}

}  // namespace

extern "C" {

int iqpt_upscale_default_params(iqpt_upscale_params* out) {
    if (!out) return iqpt::fail(IQPT_ERR_INVALID_ARG, "out is NULL");
    *out = kDefaults;
    return IQPT_OK;
}

int iqpt_upscale_create(int device, uint32_t width, uint32_t height, uint32_t factor, iqpt_upscale** out) {
    if (out) *out = nullptr;
    if (factor < IQPT_UPSCALE_MIN_FACTOR || factor > IQPT_UPSCALE_MAX_FACTOR)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "factor must be 2, 3 or 4");
    if (width % factor != 0 || height % factor != 0)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "width and height must be multiples of factor");
    return iqp::frame_create(device, width, height, out, iqpt_upscale_destroy, [factor](iqpt_upscale* u) {
        u->factor = factor;
        u->lo.device = u->device;
        u->lo.stream = u->stream;
        u->lo.width = u->width / factor;
        u->lo.height = u->height / factor;
        if (int st = u->timer.create(2)) return st;
        const size_t n = u->npix(), nlo = u->lo.npix();
        return iqp::frame_alloc(*u, {{&u->normal_z_lo, nlo * 16, "hipMalloc(normal_z_lo)"},
                                     {(void**)&u->id_lo, nlo * 4, "hipMalloc(id_lo)"},
                                     {&u->normal_z_hi, n * 16, "hipMalloc(normal_z_hi)"},
                                     {(void**)&u->id_hi, n * 4, "hipMalloc(id_hi)"},
                                     {&u->input, nlo * 16, "hipMalloc(input)"},
                                     {&u->out, n * 16, "hipMalloc(out)"},
                                     {(void**)&u->bgra, n * 4, "hipMalloc(bgra)"},
                                     {(void**)&u->counts, 3 * sizeof(unsigned long long), "hipMalloc(counts)"}});
    });
}

int iqpt_upscale_destroy(iqpt_upscale* u) {
    if (!u) return IQPT_OK;
    iqp::frame_close(*u, {&u->timer});
    delete u;
    return IQPT_OK;
}

int iqpt_upscale_set_params(iqpt_upscale* u, const iqpt_upscale_params* p) {
    if (!p) return iqpt::fail(IQPT_ERR_INVALID_ARG, "params is NULL");
    if (int st = check_params(*p)) return st;
    if (!u) return iqpt::fail(IQPT_ERR_INVALID_ARG, "upscaler is NULL");
    u->params = *p;
    return IQPT_OK;
}

int iqpt_upscale_set_guides(iqpt_upscale* u, const float* normal_z_lo, const uint32_t* id_lo, const float* normal_z_hi,
                            const uint32_t* id_hi) {
    if (!u || !normal_z_lo || !id_lo || !normal_z_hi || !id_hi) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    return set_guides(u, normal_z_lo, id_lo, normal_z_hi, id_hi, hipMemcpyHostToDevice);
}

int iqpt_upscale_set_guides_device(iqpt_upscale* u, const void* normal_z_lo_device, const void* id_lo_device,
                                   const void* normal_z_hi_device, const void* id_hi_device) {
    if (!u || !normal_z_lo_device || !id_lo_device || !normal_z_hi_device || !id_hi_device)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    return set_guides(u, normal_z_lo_device, id_lo_device, normal_z_hi_device, id_hi_device, hipMemcpyDeviceToDevice);
}

int iqpt_upscale_run(iqpt_upscale* u, const float* colour_lo) {
    if (!u || !colour_lo) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = iqp::set_device(*u)) return st;
    IQPT_HIP(hipMemcpyAsync(u->input, colour_lo, u->lo.npix() * 16, hipMemcpyHostToDevice, u->stream));
    IQPT_HIP(hipStreamSynchronize(u->stream));      // the caller's array may go away
    return run(u, u->input);
}

int iqpt_upscale_run_device(iqpt_upscale* u, const void* colour_lo_device) {
    if (!u || !colour_lo_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = iqp::set_device(*u)) return st;
    return run(u, colour_lo_device);
}

int iqpt_upscale_frame(iqpt_upscale* u, iqpt_ctx* ctx, iqpt_raster* r_lo, iqpt_raster* r_hi) {
    if (!u || !ctx || !r_lo || !r_hi) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    uint64_t npix = 0;
    if (int st = iqpt_num_pixels(ctx, &npix)) return st;
    if (npix != u->lo.npix()) return iqpt::fail(IQPT_ERR_INVALID_ARG, "the context does not own a whole frame of the upscaler's lo size");
    const iqpt_camera *cam_lo = nullptr, *cam_hi = nullptr;
    const void *nz_lo = nullptr, *id_lo = nullptr, *nz_hi = nullptr, *id_hi = nullptr;
    if (int st = iqp::raster_view(u->lo, r_lo, "the upscaler's lo size", &cam_lo, &nz_lo, &id_lo)) return st;
    if (int st = iqp::raster_view(*u, r_hi, "the upscaler's", &cam_hi, &nz_hi, &id_hi)) return st;
    if (std::memcmp(cam_lo->view, cam_hi->view, sizeof cam_lo->view) != 0 ||
        std::memcmp(cam_lo->projection, cam_hi->projection, sizeof cam_lo->projection) != 0)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "the two rasterizers' cameras differ in view or projection");
    if (int st = iqp::set_device(*u)) return st;
    IQPT_HIP(hipStreamSynchronize(u->stream));      // a run in flight may still read u->input
    if (int st = iqpt_copy_accum_device(ctx, u->input, u->lo.npix() * 16)) return st;
    if (int st = iqpt_upscale_set_guides_device(u, nz_lo, id_lo, nz_hi, id_hi)) return st;
    return run(u, u->input);
}

int iqpt_upscale_read(iqpt_upscale* u, float* lin_rgba, uint8_t* bgra) {
    if (!u) return iqpt::fail(IQPT_ERR_INVALID_ARG, "upscaler is NULL");
    if (!u->have_result) return iqpt::fail(IQPT_ERR_NOT_READY, "read before the first run");
    return iqp::read_planes(*u, lin_rgba, u->out, bgra, u->bgra);
}

int iqpt_upscale_output_device(iqpt_upscale* u, const void** lin_device) {
    if (!u || !lin_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (!u->have_result) return iqpt::fail(IQPT_ERR_NOT_READY, "output before the first run");
    if (int st = iqp::set_device(*u)) return st;
    IQPT_HIP(hipStreamSynchronize(u->stream));      // its reader runs on another stream
    *lin_device = u->out;
    return IQPT_OK;
}

int iqpt_upscale_copy_frame_device(iqpt_upscale* u, void* dst_device, size_t bytes) {
    if (!u || !dst_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (!u->have_result) return iqpt::fail(IQPT_ERR_NOT_READY, "copy before the first run");
    return iqp::copy_bgra(*u, u->bgra, dst_device, bytes);
}

int iqpt_upscale_sync(iqpt_upscale* u) {
    if (!u) return iqpt::fail(IQPT_ERR_INVALID_ARG, "upscaler is NULL");
    if (int st = iqp::set_device(*u)) return st;
    IQPT_HIP(hipStreamSynchronize(u->stream));
    return IQPT_OK;
}

int iqpt_upscale_time(iqpt_upscale* u, double* total_ms, uint64_t* runs) {
    if (!u || !total_ms || !runs) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = iqp::set_device(*u)) return st;
    if (int st = u->timer.collect()) return st;
    *total_ms = u->timer.total_ms;
    *runs = u->timer.runs;
    u->timer.reset();
    return IQPT_OK;
}

int iqpt_upscale_stats(iqpt_upscale* u, uint64_t* guided, uint64_t* widened, uint64_t* unguided) {
    if (!u) return iqpt::fail(IQPT_ERR_INVALID_ARG, "upscaler is NULL");
    if (!u->have_result) return iqpt::fail(IQPT_ERR_NOT_READY, "stats before the first run");
    if (int st = iqp::set_device(*u)) return st;
    unsigned long long host[3] = {0, 0, 0};
    IQPT_HIP(hipMemsetAsync(u->counts, 0, sizeof host, u->stream));
    IQPT_HIP(iqu::launch_stats(u->stream, u->width, u->height, u->out, u->counts));
    IQPT_HIP(hipMemcpyAsync(host, u->counts, sizeof host, hipMemcpyDeviceToHost, u->stream));
    IQPT_HIP(hipStreamSynchronize(u->stream));
    if (guided) *guided = host[0];
    if (widened) *widened = host[1];
    if (unguided) *unguided = host[2];
    return IQPT_OK;
}

}  // extern "C"
