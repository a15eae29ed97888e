/*
 * iqpt_temporal.h — C ABI of temporal reprojection (libiqpt.so): a history buffer that follows the camera, so
 * that the samples taken before a camera move are kept instead of thrown away by iqpt_reset. Every view's
 * history is gathered from the previous view's result through the rasterizer's G-buffer (iqpt_raster_gbuffer)
 * and both cameras' matrices; a resolve blends it with the path tracer's accumulator. The definition is
 * normative and written out in DESIGN.md §11; tests/temporal_ref.py restates it in numpy and the GPU result
 * equals it bit for bit.
 *
 * The reference has no temporal reuse. These entry points are additions: IQPT_ABI_VERSION (iqpt.h) is
 * unchanged. Conventions are iqpt.h's: every function returns IQPT_OK or an iqpt_status, iqpt_last_error() has
 * the detail, pointers are host pointers unless a name says "device".
 */
#ifndef IQPT_TEMPORAL_H
#define IQPT_TEMPORAL_H

#include "iqpt.h"
#include "raster/iqpt_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IQPT_TEMPORAL_MAX_HISTORY 16777216u   /* 2^24: what a float counts exactly */

typedef struct iqpt_temporal iqpt_temporal;

typedef struct iqpt_temporal_params {
    float normal_min;        /* finite: a history tap needs n_p . n_q >= normal_min */
    float plane_tolerance;   /* >= 0: and |n_p . (P_prev(q) - P(p))| <= plane_tolerance * c.w (c.w: the depth in the previous view) */
    uint32_t max_history;    /* 1..2^24: the cap on the history length carried into a view */
} iqpt_temporal_params;

/* The parameters a new object starts with. */
int iqpt_temporal_default_params(iqpt_temporal_params* out);

/* width, height: 1..8192. */
int iqpt_temporal_create(int device, uint32_t width, uint32_t height, iqpt_temporal** out);
int iqpt_temporal_destroy(iqpt_temporal* t);
int iqpt_temporal_set_params(iqpt_temporal* t, const iqpt_temporal_params* p);

/* A new view: cam (of the object's frame size) and its two guide planes, compact row-major: normal_z =
 * (n.x, n.y, n.z, z) per pixel, id = the draw index or IQPT_RASTER_NO_PRIM (the layout of
 * iqpt_raster_read_gbuffer / iqpt_raster_gbuffer_device). Computes every pixel's world position and gathers
 * its history from the previous view's last result (none: an empty history); the planes are copied into
 * buffers the object owns. The result is invalid until the next resolve. The device form copies on the
 * object's stream and synchronises that copy. */
int iqpt_temporal_begin_view(iqpt_temporal* t, const iqpt_camera* cam, const float* normal_z, const uint32_t* id);
int iqpt_temporal_begin_view_device(iqpt_temporal* t, const iqpt_camera* cam, const void* normal_z_device,
                                    const void* id_device);
/* The same from a rasterizer: its G-buffer (iqpt_raster_gbuffer, run here) and the camera it was last given.
 * IQPT_ERR_INVALID_ARG unless r has the object's frame size, IQPT_ERR_NOT_READY without a camera or scene. */
int iqpt_temporal_begin_view_raster(iqpt_temporal* t, iqpt_raster* r);
/* Forgets the view and the result. Call it on a scene change: ids are not comparable across scenes. */
int iqpt_temporal_clear(iqpt_temporal* t);

/* Blends the view's history with width*height float4 colours (xyz used) that hold the mean of n samples
 * (clamped to 2^24; 0: the reprojected history alone) and encodes the BGRA8 frame, on the object's own
 * stream, not waited for. The history is not modified: resolving a view again as the accumulator grows never
 * counts a sample twice. resolve_device reads its input in place, so it must stay valid and unchanged until
 * the object is synchronised. IQPT_ERR_NOT_READY without a view. */
int iqpt_temporal_resolve(iqpt_temporal* t, const float* colour, uint64_t n);
int iqpt_temporal_resolve_device(iqpt_temporal* t, const void* colour_device, uint64_t n);
/* The convenience call: ctx's accumulator through iqpt_copy_accum_device and its iqpt_frame_count as n.
 * IQPT_ERR_INVALID_ARG unless ctx owns exactly width*height pixels. */
int iqpt_temporal_resolve_ctx(iqpt_temporal* t, iqpt_ctx* ctx);

/* Synchronises and copies out the last result: lin_rgba = 4 floats per pixel (xyz the colour, w the number of
 * samples behind it), bgra = 4 bytes per pixel encoded as the path tracer's frame. Either pointer may be NULL.
 * IQPT_ERR_NOT_READY without a result. */
int iqpt_temporal_read(iqpt_temporal* t, float* lin_rgba, uint8_t* bgra);
/* The device buffer of the float4 result, to hand to iqpt_denoise_run_device. It stays the same buffer for the
 * object's lifetime; its contents are those of the last resolve once the object is synchronised. */
int iqpt_temporal_output_device(iqpt_temporal* t, const void** out_device);
/* Device-to-device copy of the BGRA8 result (width*height uint32) on the object's stream. Synchronises. */
int iqpt_temporal_copy_frame_device(iqpt_temporal* t, void* dst_device, size_t bytes);
int iqpt_temporal_sync(iqpt_temporal* t);
/* HIP-event durations since the last call (then cleared): the sum over the view kernels and their
 * number, the sum over the resolve kernels and their number. Synchronises. */
int iqpt_temporal_time(iqpt_temporal* t, double* view_ms, uint64_t* views, double* resolve_ms, uint64_t* resolves);
/* Of the last begin_view: the pixels with a guide (id != IQPT_RASTER_NO_PRIM) and those among them with a valid
 * history, counted by a reduction run by this call. Synchronises. IQPT_ERR_NOT_READY without a view. */
int iqpt_temporal_stats(iqpt_temporal* t, uint64_t* guided, uint64_t* valid);

#ifdef __cplusplus
}
#endif

#endif /* IQPT_TEMPORAL_H */
