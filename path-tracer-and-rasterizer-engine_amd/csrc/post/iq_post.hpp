// iq_post.hpp — what the runtimes of the frame-sized post-process objects (denoise/, temporal/, svgf/) share: the
// one HIP error path of the library, the fields, creation and destruction every such object has, the copies in
// and out they all make, and the event timer behind their *_time entry points. The definitions are iq_post.cpp
// (and iqpt_runtime.cpp for hip_fail); the shared kernel is iq_post_kernels.hip.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <vector>

#include "iqpt_internal.hpp"

struct iqpt_camera;
struct iqpt_raster;

namespace iqpt {

// IQPT_ERR_HIP with "what: name (description)" as the last error (iqpt_runtime.cpp)
int hip_fail(hipError_t e, const char* what);

}  // namespace iqpt

#define IQPT_HIP(call)                                                  \
    do {                                                                \
        hipError_t e_ = (call);                                         \
        if (e_ != hipSuccess) return iqpt::hip_fail(e_, #call);         \
    } while (0)

namespace iqp {

// The BGRA8 encoding of a float4 plane alone (iq_post_kernels.hip): what a filter with levels = 0 runs. Enqueues
// on `s` and returns the launch status.
hipError_t launch_encode(hipStream_t s, uint32_t width, uint32_t height, const void* in, uint32_t* bgra);

// What every frame-sized object starts with: its device, its own stream, the frame size and every device buffer it
// owns.
struct frame {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t width = 0, height = 0;
    std::vector<void*> buffers;        // every allocation of frame_alloc, for frame_close
    size_t npix() const { return (size_t)width * height; }
};

// The events around the consecutive stages of one run on one stream: event k before stage k, event k + 1 after
// it. A run collects the one before it, records ev[0 .. n] in order on the stream and, once all are in, sets
// recorded = n + 1; collect waits for the last of them (wait = false: the caller knows it has passed, having
// waited for a later event of the same stream) and adds the run up.
struct event_timer {
    static constexpr int kMaxEvents = 10;
    hipEvent_t ev[kMaxEvents] = {};
    int recorded = 0;                  // events of the last run, not added up yet (0: nothing pending)
    double ms[kMaxEvents - 1] = {};    // ms[k]: from event k to event k + 1, summed over the runs since reset
    double total_ms = 0.0;             // from event 0 to the last one, where a run has more than one stage
    uint64_t runs = 0;
    int create(int events);            // once, on the object's device
    void destroy();
    int collect(bool wait = true);
    void reset();                      // the sums, after a *_time call has reported them
};

struct buffer_spec {
    void** p;
    size_t bytes;
    const char* what;                  // "hipMalloc(name)": the error detail if it fails
};

// The argument checks of every *_create (frame size 1..8192, a visible device of that index), before anything is
// made; then the object's fields, hipSetDevice and the stream.
int frame_check(int device, uint32_t width, uint32_t height);
int frame_open(frame& f, int device, uint32_t width, uint32_t height);
// All of `specs` in order; stops at the first failure (frame_close frees what was allocated before it).
int frame_alloc(frame& f, std::initializer_list<buffer_spec> specs);
// Waits for the stream, frees the buffers, the timers' events and the stream. Safe on a half-made object.
void frame_close(frame& f, std::initializer_list<event_timer*> timers);

// *_create whole: the checks, a new T (a frame), `init(t)` for its events, buffers and parts, and on failure
// `destroy(t)` with the failure's status and last error kept (destroying the parts must not lose it).
template <class T, class Init>
int frame_create(int device, uint32_t width, uint32_t height, T** out, int (*destroy)(T*), Init init) {
    if (!out) return iqpt::fail(IQPT_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (int st = frame_check(device, width, height)) return st;
    T* t = new T();
    int st = frame_open(*t, device, width, height);
    if (!st) st = init(t);
    if (st) {
        const std::string detail = iqpt_last_error();
        destroy(t);
        return iqpt::fail(st, detail);
    }
    *out = t;
    return IQPT_OK;
}

int set_device(const frame& f);
int check_camera(const frame& f, const iqpt_camera* cam);
// Both guide planes into the object's own on its stream, waited for: the caller's may go away or change.
int copy_guides(const frame& f, void* normal_z_dst, uint32_t* id_dst, const void* normal_z, const void* id,
                hipMemcpyKind kind);
// The rasterizer's view for an object of f's size: its G-buffer pass, the two plane pointers (device) and, where
// cam != NULL, its current camera (IQPT_ERR_NOT_READY without one). `whose`: the size mismatch's message names it.
int raster_view(const frame& f, iqpt_raster* r, const char* whose, const iqpt_camera** cam, const void** normal_z,
                const void** id);
// Either or both of a result's planes to the host (a NULL destination is skipped), waited for.
int read_planes(const frame& f, float* lin_rgba, const void* lin_device, uint8_t* bgra, const uint32_t* bgra_device);
// The BGRA8 frame to another device buffer of exactly width*height*4 bytes, waited for.
int copy_bgra(const frame& f, const uint32_t* bgra_device, void* dst_device, size_t bytes);

}  // namespace iqp
