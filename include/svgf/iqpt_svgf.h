/*
 * iqpt_svgf.h — C ABI of variance-guided filtering (libiqpt.so): two temporal histories (iqpt_temporal.h), one of
 * the colour and one of its first and second luminance moments, a per-pixel variance estimate from them (from the
 * pixel's 7x7 neighbourhood where the history is too short), and an à-trous filter whose colour weight that
 * variance normalises, so that a firefly accepts its neighbours and a converged pixel is left alone. The
 * definition is normative and written out in DESIGN.md §12; tests/svgf_ref.py restates it in numpy and the GPU
 * result equals it bit for bit.
 *
 * The reference has no counterpart. These entry points are additions: IQPT_ABI_VERSION (iqpt.h) is unchanged.
 * Conventions are iqpt.h's: every function returns IQPT_OK or an iqpt_status, iqpt_last_error() has the detail,
 * pointers are host pointers unless a name says "device". Every call keeps the argument rules of its
 * iqpt_temporal_* namesake.
 */
#ifndef IQPT_SVGF_H
#define IQPT_SVGF_H

#include "iqpt.h"
#include "raster/iqpt_raster.h"
#include "temporal/iqpt_temporal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IQPT_SVGF_MAX_LEVELS 8u
#define IQPT_SVGF_MAX_SQUARINGS 7u

typedef struct iqpt_svgf iqpt_svgf;

typedef struct iqpt_svgf_params {
    float normal_min;            /* the three parameters of both histories: iqpt_temporal_params */
    float plane_tolerance;
    uint32_t max_history;
    uint32_t min_history;        /* 1..2^24: the temporal estimate needs this many views' worth of samples behind a pixel */
    uint32_t levels;             /* L, 0..8: level i filters with step 2^i; 0 returns the variance estimate's plane */
    uint32_t normal_squarings;   /* q, 0..7: the normal weight is max(n_p . n_q, 0)^(2^q) */
    float depth_sharpness;       /* s_z, finite, >= 0: the depth weight is 1 / (1 + ((z_p - z_q) s_z)^2) */
    float colour_sigma;          /* sigma, finite, >= 0: the colour weight is 1 / (1 + |c_p - c_q|^2 / (sigma^2 var + floor)) */
    float variance_floor;        /* finite, > 0 */
} iqpt_svgf_params;

/* The parameters a new object starts with. */
int iqpt_svgf_default_params(iqpt_svgf_params* out);

/* width, height: 1..8192. */
int iqpt_svgf_create(int device, uint32_t width, uint32_t height, iqpt_svgf** out);
int iqpt_svgf_destroy(iqpt_svgf* s);
int iqpt_svgf_set_params(iqpt_svgf* s, const iqpt_svgf_params* p);

/* A new view of both histories (iqpt_temporal_begin_view*); the guide planes are also kept for the filter. */
int iqpt_svgf_begin_view(iqpt_svgf* s, const iqpt_camera* cam, const float* normal_z, const uint32_t* id);
int iqpt_svgf_begin_view_device(iqpt_svgf* s, const iqpt_camera* cam, const void* normal_z_device, const void* id_device);
int iqpt_svgf_begin_view_raster(iqpt_svgf* s, iqpt_raster* r);
/* Forgets the view, both histories and the result. Call it on a scene change. */
int iqpt_svgf_clear(iqpt_svgf* s);

/* The whole chain for width*height float4 colours (xyz used) that hold the mean of n samples (clamped to 2^24):
 * both histories' resolves, the variance estimate and the levels, the last part on the object's own stream and
 * not waited for. Neither history is modified. resolve_device reads its input in place. IQPT_ERR_NOT_READY
 * without a view. */
int iqpt_svgf_resolve(iqpt_svgf* s, const float* colour, uint64_t n);
int iqpt_svgf_resolve_device(iqpt_svgf* s, const void* colour_device, uint64_t n);
/* ctx's accumulator through iqpt_copy_accum_device and its iqpt_frame_count as n. IQPT_ERR_INVALID_ARG unless ctx
 * owns exactly width*height pixels. */
int iqpt_svgf_resolve_ctx(iqpt_svgf* s, iqpt_ctx* ctx);

/* Synchronises and copies out the last result: lin_rgba = 4 floats per pixel (xyz the filtered colour, w the
 * filtered variance), bgra = 4 bytes per pixel encoded as the path tracer's frame. Either pointer may be NULL.
 * IQPT_ERR_NOT_READY without a result. */
int iqpt_svgf_read(iqpt_svgf* s, float* lin_rgba, uint8_t* bgra);
/* The stages before the filter, 4 floats per pixel each: temporal_rgba = the colour history's result (w the
 * samples behind the pixel), variance_rgba = c_0 (xyz the same colour, w the variance estimate). Either pointer
 * may be NULL. Synchronises. IQPT_ERR_NOT_READY without a result. */
int iqpt_svgf_read_stages(iqpt_svgf* s, float* temporal_rgba, float* variance_rgba);
/* Device-to-device copy of the BGRA8 result (width*height uint32) on the object's stream. Synchronises. */
int iqpt_svgf_copy_frame_device(iqpt_svgf* s, void* dst_device, size_t bytes);
int iqpt_svgf_sync(iqpt_svgf* s);
/* HIP-event durations since the last call (then cleared), summed over `resolves` resolves: the moments kernel,
 * the variance kernel, each level (level_ms[8], levels not run stay 0; L = 0: the encode kernel counts as level
 * 0), and the two histories' own times passed through from iqpt_temporal_time, [0] the colour history and [1]
 * the moments history: view_ms[2] over their begin_views, history_resolve_ms[2] over their resolves. level_ms,
 * view_ms and history_resolve_ms may be NULL. Synchronises. */
int iqpt_svgf_time(iqpt_svgf* s, double* moments_ms, double* variance_ms, double* level_ms, uint64_t* resolves,
                   double* view_ms, double* history_resolve_ms);
/* Of the last begin_view: the pixels with a guide and those among them with a valid history
 * (iqpt_temporal_stats of the colour history); of the last resolve of that view: the pixels that took the spatial
 * estimate (0 before one). Synchronises. IQPT_ERR_NOT_READY without a view. */
int iqpt_svgf_stats(iqpt_svgf* s, uint64_t* guided, uint64_t* valid, uint64_t* spatial);

#ifdef __cplusplus
}
#endif

#endif /* IQPT_SVGF_H */
