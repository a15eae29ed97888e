/*
 * iqpt_upscale.h — C ABI of guided upsampling (libiqpt.so): the path tracer runs at 1/f of the frame in each
 * dimension and its colour is carried to the full frame by joint bilateral upsampling, steered by the
 * rasterizer's G-buffers of both sizes (iqpt_raster_gbuffer): a low-resolution colour reaches a full-resolution
 * pixel only across the same surface. The definition is normative and written out in DESIGN.md §14;
 * tests/upscale_ref.py restates it in numpy and the GPU result equals it bit for bit.
 *
 * The reference has no counterpart. These entry points are additions: IQPT_ABI_VERSION (iqpt.h) is unchanged.
 * Conventions are iqpt.h's: every function returns IQPT_OK or an iqpt_status, iqpt_last_error() has the detail,
 * pointers are host pointers unless a name says "device". "hi" is the full frame, width x height; "lo" is the
 * traced one, (width / factor) x (height / factor).
 */
#ifndef IQPT_UPSCALE_H
#define IQPT_UPSCALE_H

#include "iqpt.h"
#include "raster/iqpt_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IQPT_UPSCALE_MIN_FACTOR 2u
#define IQPT_UPSCALE_MAX_FACTOR 4u
#define IQPT_UPSCALE_MAX_SQUARINGS 7u

typedef struct iqpt_upscale iqpt_upscale;

typedef struct iqpt_upscale_params {
    uint32_t normal_squarings;   /* q, 0..7: the normal weight is max(n_P . n_q, 0)^(2^q) */
    float depth_sharpness;       /* s_z >= 0: the depth weight is 1 / (1 + ((z_P - z_q) s_z)^2); 0 switches it off */
} iqpt_upscale_params;

/* The defaults a new upscaler starts with: the denoiser's q and s_z, not measured for this
 * stage. */
int iqpt_upscale_default_params(iqpt_upscale_params* out);

/* width, height: the hi frame, 1..8192, each a multiple of factor; factor: 2, 3 or 4. */
int iqpt_upscale_create(int device, uint32_t width, uint32_t height, uint32_t factor, iqpt_upscale** out);
int iqpt_upscale_destroy(iqpt_upscale* u);
int iqpt_upscale_set_params(iqpt_upscale* u, const iqpt_upscale_params* p);

/* Both pairs of guide planes, compact row-major, the lo pair of the lo size and the hi pair of the hi size:
 * normal_z = (n.x, n.y, n.z, z) per pixel, id = the draw index or IQPT_RASTER_NO_PRIM (the layout of
 * iqpt_raster_read_gbuffer / iqpt_raster_gbuffer_device). Copied into buffers the upscaler owns; the device
 * form copies on the upscaler's stream and synchronises. */
int iqpt_upscale_set_guides(iqpt_upscale* u, const float* normal_z_lo, const uint32_t* id_lo, const float* normal_z_hi,
                            const uint32_t* id_hi);
int iqpt_upscale_set_guides_device(iqpt_upscale* u, const void* normal_z_lo_device, const void* id_lo_device,
                                   const void* normal_z_hi_device, const void* id_hi_device);

/* Upsample the lo frame's float4 colours (xyz used) under the current guides and parameters: one kernel launch
 * on the upscaler's own stream, not waited for. The input is never modified; run_device reads it in place, so
 * it must stay valid and unchanged until the upscaler is synchronised. */
int iqpt_upscale_run(iqpt_upscale* u, const float* colour_lo);
int iqpt_upscale_run_device(iqpt_upscale* u, const void* colour_lo_device);

/* The convenience call: takes ctx's accumulator through iqpt_copy_accum_device and both G-buffers through
 * iqpt_raster_gbuffer (all every call), then runs. IQPT_ERR_INVALID_ARG unless ctx owns exactly the lo frame's
 * pixels, r_lo and r_hi have the lo and the hi frame size, and their cameras' view and projection matrices are
 * bit-equal (IQPT_ERR_NOT_READY before either rasterizer has a camera). ctx's pixels are checked by their number
 * alone, as iqpt_denoise_frame checks them: a context that owns a pixel subset of another frame size which
 * happens to hold as many pixels passes, and its accumulator is then read as a compact lo frame; hand it a
 * context created for the whole lo frame. */
int iqpt_upscale_frame(iqpt_upscale* u, iqpt_ctx* ctx, iqpt_raster* r_lo, iqpt_raster* r_hi);

/* Synchronises and copies out the last result at the hi size: lin_rgba = 4 floats per pixel (w = the pixel's
 * class: +0 guided, 1 widened, 2 unguided), bgra = 4 bytes per pixel encoded as the path tracer's frame. Either
 * pointer may be NULL. */
int iqpt_upscale_read(iqpt_upscale* u, float* lin_rgba, uint8_t* bgra);
/* The float4 result on the device (width*height float4, owned by the upscaler, rewritten by the next run): what
 * iqpt_denoise_run_device or iqpt_temporal_resolve_device of the hi size then takes. Synchronises, so the plane
 * is complete on return. */
int iqpt_upscale_output_device(iqpt_upscale* u, const void** lin_device);
/* Device-to-device copy of the BGRA8 result (width*height uint32) on the upscaler's stream. Synchronises. */
int iqpt_upscale_copy_frame_device(iqpt_upscale* u, void* dst_device, size_t bytes);
int iqpt_upscale_sync(iqpt_upscale* u);
/* HIP-event duration of the kernel, summed over the runs since the last call (then cleared), and their number.
 * Synchronises. */
int iqpt_upscale_time(iqpt_upscale* u, double* total_ms, uint64_t* runs);
/* The hi pixels of each class in the last result (they add up to width*height), counted on request by a small
 * kernel of its own over the result's fourth component. Synchronises. Any of the three may be NULL. */
int iqpt_upscale_stats(iqpt_upscale* u, uint64_t* guided, uint64_t* widened, uint64_t* unguided);

#ifdef __cplusplus
}
#endif

#endif /* IQPT_UPSCALE_H */
