// iq_post.cpp — the host code the frame-sized post-process objects share (post/iq_post.hpp): creation and
// destruction, the copies in and out, the rasterizer's view and the event timer.
#include "post/iq_post.hpp"

#include <hip/hip_runtime.h>

#include "raster/iq_raster.hpp"
#include "raster/iqpt_raster.h"

namespace iqp {

int event_timer::create(int events) {
    for (int k = 0; k < events; ++k) IQPT_HIP(hipEventCreate(&ev[k]));
    return IQPT_OK;
}

void event_timer::destroy() {
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
}

int event_timer::collect(bool wait) {
    if (!recorded) return IQPT_OK;
    const int last = recorded - 1;
    if (wait) IQPT_HIP(hipEventSynchronize(ev[last]));
    float t = 0.0f;
    for (int k = 0; k < last; ++k) {
        IQPT_HIP(hipEventElapsedTime(&t, ev[k], ev[k + 1]));
        ms[k] += t;
    }
    if (last > 1) IQPT_HIP(hipEventElapsedTime(&t, ev[0], ev[last]));      // one stage: t is that interval already
    if (last) total_ms += t;
    runs += 1;
    recorded = 0;
    return IQPT_OK;
}

void event_timer::reset() {
    for (double& m : ms) m = 0.0;
    total_ms = 0.0;
    runs = 0;
}

int frame_check(int device, uint32_t width, uint32_t height) {
    if (width == 0 || height == 0 || width > IQPT_RASTER_MAX_DIM || height > IQPT_RASTER_MAX_DIM)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "frame size must be 1..8192 in each dimension");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return iqpt::fail(IQPT_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= count) return iqpt::fail(IQPT_ERR_NO_DEVICE, "device index out of range");
    return IQPT_OK;
}

int frame_open(frame& f, int device, uint32_t width, uint32_t height) {
    f.device = device;
    f.width = width;
    f.height = height;
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return iqpt::hip_fail(e, "hipSetDevice");
    if ((e = hipStreamCreateWithFlags(&f.stream, hipStreamNonBlocking)) != hipSuccess)
        return iqpt::hip_fail(e, "hipStreamCreate");
    return IQPT_OK;
}

int frame_alloc(frame& f, std::initializer_list<buffer_spec> specs) {
    for (const buffer_spec& b : specs) {
        const hipError_t e = hipMalloc(b.p, b.bytes);
        if (e != hipSuccess) return iqpt::hip_fail(e, b.what);
        f.buffers.push_back(*b.p);
    }
    return IQPT_OK;
}

void frame_close(frame& f, std::initializer_list<event_timer*> timers) {
    (void)hipSetDevice(f.device);
    if (f.stream) (void)hipStreamSynchronize(f.stream);
    for (void* p : f.buffers) (void)hipFree(p);
    for (event_timer* t : timers) t->destroy();
    if (f.stream) (void)hipStreamDestroy(f.stream);
}

int set_device(const frame& f) {
    IQPT_HIP(hipSetDevice(f.device));
    return IQPT_OK;
}

int check_camera(const frame& f, const iqpt_camera* cam) {
    if (cam->width != f.width || cam->height != f.height)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "camera size differs from the frame's");
    return IQPT_OK;
}

int copy_guides(const frame& f, void* normal_z_dst, uint32_t* id_dst, const void* normal_z, const void* id,
                hipMemcpyKind kind) {
    IQPT_HIP(hipMemcpyAsync(normal_z_dst, normal_z, f.npix() * 16, kind, f.stream));
    IQPT_HIP(hipMemcpyAsync(id_dst, id, f.npix() * 4, kind, f.stream));
    IQPT_HIP(hipStreamSynchronize(f.stream));
    return IQPT_OK;
}

int raster_view(const frame& f, iqpt_raster* r, const char* whose, const iqpt_camera** cam, const void** normal_z,
                const void** id) {
    uint32_t rw = 0, rh = 0;
    iqr::frame_size(r, &rw, &rh);
    if (rw != f.width || rh != f.height)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, std::string("the rasterizer's frame size differs from ") + whose);
    if (cam) {
        *cam = iqr::current_camera(r);
        if (!*cam) return iqpt::fail(IQPT_ERR_NOT_READY, "begin_view_raster before the rasterizer's set_camera");
    }
    if (int st = iqpt_raster_gbuffer(r)) return st;
    return iqpt_raster_gbuffer_device(r, normal_z, id);
}

int read_planes(const frame& f, float* lin_rgba, const void* lin_device, uint8_t* bgra, const uint32_t* bgra_device) {
    if (int st = set_device(f)) return st;
    if (lin_rgba) IQPT_HIP(hipMemcpyAsync(lin_rgba, lin_device, f.npix() * 16, hipMemcpyDeviceToHost, f.stream));
    if (bgra) IQPT_HIP(hipMemcpyAsync(bgra, bgra_device, f.npix() * 4, hipMemcpyDeviceToHost, f.stream));
    IQPT_HIP(hipStreamSynchronize(f.stream));
    return IQPT_OK;
}

int copy_bgra(const frame& f, const uint32_t* bgra_device, void* dst_device, size_t bytes) {
    if (bytes != f.npix() * 4) return iqpt::fail(IQPT_ERR_INVALID_ARG, "bytes must be width*height*4");
    if (int st = set_device(f)) return st;
    IQPT_HIP(hipMemcpyAsync(dst_device, bgra_device, bytes, hipMemcpyDeviceToDevice, f.stream));
    IQPT_HIP(hipStreamSynchronize(f.stream));
    return IQPT_OK;
}

}  // namespace iqp
