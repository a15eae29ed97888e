// iq_denoise.cpp — the iqpt_denoise_* C ABI (include/denoise/iqpt_denoise.h): the guide and colour buffers, one
// kernel launch per à-trous level on the denoiser's own stream, readback and timing. The kernels are
// iq_denoise_kernels.hip; the filter is DESIGN.md §10.
#include <hip/hip_runtime.h>

#include <string>

#include "denoise/iq_denoise.hpp"
#include "denoise/iqpt_denoise.h"
#include "iqpt_internal.hpp"
#include "raster/iq_raster.hpp"

namespace {

int hip_fail(hipError_t e, const char* what) {
    return iqpt::fail(IQPT_ERR_HIP, std::string(what) + ": " + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ")");
}

#define IQD_HIP(call)                                        \
    do {                                                     \
        hipError_t e_ = (call);                              \
        if (e_ != hipSuccess) return hip_fail(e_, #call);    \
    } while (0)

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

struct iqpt_denoise {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t width = 0, height = 0;
    iqpt_denoise_params params = kDefaults;
    void* normal_z = nullptr;          // npix float4
    uint32_t* id = nullptr;            // npix
    void* input = nullptr;             // npix float4: a host colour, or the accumulator iqpt_denoise_frame takes
    void* colour[2] = {};              // npix float4 each: the levels ping-pong between them
    uint32_t* bgra = nullptr;          // npix
    bool have_guides = false;
    int result = -1;                   // which of colour[] holds the last result
    hipEvent_t ev[kMaxLevels + 1] = {};
    uint32_t pending_levels = 0;
    bool pending = false;              // the events of the last run have not been added up yet
    double total_ms = 0.0, level_ms[kMaxLevels] = {};
    uint64_t runs = 0;
    size_t npix() const { return (size_t)width * height; }
};

namespace {

int set_device(iqpt_denoise* d) {
    IQD_HIP(hipSetDevice(d->device));
    return IQPT_OK;
}

int collect(iqpt_denoise* d) {
    if (!d->pending) return IQPT_OK;
    IQD_HIP(hipEventSynchronize(d->ev[d->pending_levels]));
    float ms = 0.0f;
    for (uint32_t k = 0; k < d->pending_levels; ++k) {
        IQD_HIP(hipEventElapsedTime(&ms, d->ev[k], d->ev[k + 1]));
        d->level_ms[k] += ms;
    }
    if (d->pending_levels) {
        IQD_HIP(hipEventElapsedTime(&ms, d->ev[0], d->ev[d->pending_levels]));
        d->total_ms += ms;
    }
    d->runs += 1;
    d->pending = false;
    return IQPT_OK;
}

int run(iqpt_denoise* d, const void* colour_device) {
    if (!d->have_guides) return iqpt::fail(IQPT_ERR_NOT_READY, "run before the guides were set");
    if (int st = collect(d)) return st;
    hipStream_t s = d->stream;
    const iqpt_denoise_params& p = d->params;
    const float sc2 = p.colour_sharpness * p.colour_sharpness;
    IQD_HIP(hipEventRecord(d->ev[0], s));
    if (p.levels == 0) {
        IQD_HIP(hipMemcpyAsync(d->colour[0], colour_device, d->npix() * 16, hipMemcpyDeviceToDevice, s));
        IQD_HIP(iqd::launch_encode(s, d->width, d->height, d->colour[0], d->bgra));
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
        IQD_HIP(iqd::launch_level(s, lp, in, d->normal_z, d->id, d->colour[o], i + 1 == p.levels ? d->bgra : nullptr));
        IQD_HIP(hipEventRecord(d->ev[i + 1], s));
        in = d->colour[o];
        d->result = o;
    }
    d->pending_levels = p.levels;
    d->pending = true;
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
    if (!out) return iqpt::fail(IQPT_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (width == 0 || height == 0 || width > IQPT_RASTER_MAX_DIM || height > IQPT_RASTER_MAX_DIM)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "frame size must be 1..8192 in each dimension");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return iqpt::fail(IQPT_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= count) return iqpt::fail(IQPT_ERR_NO_DEVICE, "device index out of range");

    iqpt_denoise* d = new iqpt_denoise();
    d->device = device;
    d->width = width;
    d->height = height;
    auto fail_with = [&](hipError_t e, const char* what) {
        const int st = hip_fail(e, what);
        iqpt_denoise_destroy(d);
        return st;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return fail_with(e, "hipSetDevice");
    if ((e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking)) != hipSuccess) return fail_with(e, "hipStreamCreate");
    for (hipEvent_t& ev : d->ev)
        if ((e = hipEventCreate(&ev)) != hipSuccess) return fail_with(e, "hipEventCreate");
    const size_t n = d->npix();
    if ((e = hipMalloc(&d->normal_z, n * 16)) != hipSuccess) return fail_with(e, "hipMalloc(normal_z)");
    if ((e = hipMalloc((void**)&d->id, n * 4)) != hipSuccess) return fail_with(e, "hipMalloc(id)");
    if ((e = hipMalloc(&d->input, n * 16)) != hipSuccess) return fail_with(e, "hipMalloc(input)");
    if ((e = hipMalloc(&d->colour[0], n * 16)) != hipSuccess) return fail_with(e, "hipMalloc(colour)");
    if ((e = hipMalloc(&d->colour[1], n * 16)) != hipSuccess) return fail_with(e, "hipMalloc(colour)");
    if ((e = hipMalloc((void**)&d->bgra, n * 4)) != hipSuccess) return fail_with(e, "hipMalloc(bgra)");
    *out = d;
    return IQPT_OK;
}

int iqpt_denoise_destroy(iqpt_denoise* d) {
    if (!d) return IQPT_OK;
    (void)hipSetDevice(d->device);
    if (d->stream) (void)hipStreamSynchronize(d->stream);
    for (void* p : {d->normal_z, (void*)d->id, d->input, d->colour[0], d->colour[1], (void*)d->bgra})
        if (p) (void)hipFree(p);
    for (hipEvent_t ev : d->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (d->stream) (void)hipStreamDestroy(d->stream);
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
    if (int st = set_device(d)) return st;
    IQD_HIP(hipMemcpyAsync(d->normal_z, normal_z, d->npix() * 16, hipMemcpyHostToDevice, d->stream));
    IQD_HIP(hipMemcpyAsync(d->id, id, d->npix() * 4, hipMemcpyHostToDevice, d->stream));
    IQD_HIP(hipStreamSynchronize(d->stream));
    d->have_guides = true;
    return IQPT_OK;
}

int iqpt_denoise_set_guides_device(iqpt_denoise* d, const void* normal_z_device, const void* id_device) {
    if (!d || !normal_z_device || !id_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = set_device(d)) return st;
    IQD_HIP(hipMemcpyAsync(d->normal_z, normal_z_device, d->npix() * 16, hipMemcpyDeviceToDevice, d->stream));
    IQD_HIP(hipMemcpyAsync(d->id, id_device, d->npix() * 4, hipMemcpyDeviceToDevice, d->stream));
    IQD_HIP(hipStreamSynchronize(d->stream));
    d->have_guides = true;
    return IQPT_OK;
}

int iqpt_denoise_run(iqpt_denoise* d, const float* colour) {
    if (!d || !colour) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = set_device(d)) return st;
    IQD_HIP(hipMemcpyAsync(d->input, colour, d->npix() * 16, hipMemcpyHostToDevice, d->stream));
    IQD_HIP(hipStreamSynchronize(d->stream));      // the caller's array may go away
    return run(d, d->input);
}

int iqpt_denoise_run_device(iqpt_denoise* d, const void* colour_device) {
    if (!d || !colour_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = set_device(d)) return st;
    return run(d, colour_device);
}

int iqpt_denoise_frame(iqpt_denoise* d, iqpt_ctx* ctx, iqpt_raster* r) {
    if (!d || !ctx || !r) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    uint64_t npix = 0;
    if (int st = iqpt_num_pixels(ctx, &npix)) return st;
    if (npix != d->npix()) return iqpt::fail(IQPT_ERR_INVALID_ARG, "the context does not own a whole frame of the denoiser's size");
    uint32_t rw = 0, rh = 0;
    iqr::frame_size(r, &rw, &rh);
    if (rw != d->width || rh != d->height) return iqpt::fail(IQPT_ERR_INVALID_ARG, "the rasterizer's frame size differs from the denoiser's");
    if (int st = set_device(d)) return st;
    IQD_HIP(hipStreamSynchronize(d->stream));      // a run in flight may still read d->input
    if (int st = iqpt_copy_accum_device(ctx, d->input, d->npix() * 16)) return st;
    if (int st = iqpt_raster_gbuffer(r)) return st;
    const void *nz = nullptr, *id = nullptr;
    if (int st = iqpt_raster_gbuffer_device(r, &nz, &id)) return st;
    if (int st = iqpt_denoise_set_guides_device(d, nz, id)) return st;
    return run(d, d->input);
}

int iqpt_denoise_read(iqpt_denoise* d, float* lin_rgba, uint8_t* bgra) {
    if (!d) return iqpt::fail(IQPT_ERR_INVALID_ARG, "denoiser is NULL");
    if (d->result < 0) return iqpt::fail(IQPT_ERR_NOT_READY, "read before the first run");
    if (int st = set_device(d)) return st;
    if (lin_rgba) IQD_HIP(hipMemcpyAsync(lin_rgba, d->colour[d->result], d->npix() * 16, hipMemcpyDeviceToHost, d->stream));
    if (bgra) IQD_HIP(hipMemcpyAsync(bgra, d->bgra, d->npix() * 4, hipMemcpyDeviceToHost, d->stream));
    IQD_HIP(hipStreamSynchronize(d->stream));
    return IQPT_OK;
}

int iqpt_denoise_copy_frame_device(iqpt_denoise* d, void* dst_device, size_t bytes) {
    if (!d || !dst_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (d->result < 0) return iqpt::fail(IQPT_ERR_NOT_READY, "copy before the first run");
    if (bytes != d->npix() * 4) return iqpt::fail(IQPT_ERR_INVALID_ARG, "bytes must be width*height*4");
    if (int st = set_device(d)) return st;
    IQD_HIP(hipMemcpyAsync(dst_device, d->bgra, bytes, hipMemcpyDeviceToDevice, d->stream));
    IQD_HIP(hipStreamSynchronize(d->stream));
    return IQPT_OK;
}

int iqpt_denoise_sync(iqpt_denoise* d) {
    if (!d) return iqpt::fail(IQPT_ERR_INVALID_ARG, "denoiser is NULL");
    if (int st = set_device(d)) return st;
    IQD_HIP(hipStreamSynchronize(d->stream));
    return IQPT_OK;
}

int iqpt_denoise_time(iqpt_denoise* d, double* total_ms, double* level_ms, uint64_t* runs) {
    if (!d || !total_ms || !runs) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = set_device(d)) return st;
    if (int st = collect(d)) return st;
    *total_ms = d->total_ms;
    *runs = d->runs;
    for (int k = 0; k < kMaxLevels; ++k) {
        if (level_ms) level_ms[k] = d->level_ms[k];
        d->level_ms[k] = 0.0;
    }
    d->total_ms = 0.0;
    d->runs = 0;
    return IQPT_OK;
}

}  // extern "C"
