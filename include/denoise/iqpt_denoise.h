/*
 * iqpt_denoise.h — C ABI of the rasterizer-guided denoiser (libiqpt.so): an edge-avoiding à-trous wavelet
 * filter over the path tracer's accumulator, steered by the rasterizer's G-buffer (iqpt_raster_gbuffer). The
 * filter is normative and written out in DESIGN.md §10; tests/denoise_ref.py restates it in numpy and the GPU
 * result equals it bit for bit.
 *
 * The reference has no denoiser: this is the first feature in which its two engines cooperate. These entry
 * points are additions: IQPT_ABI_VERSION (iqpt.h) is unchanged. Conventions are iqpt.h's: every function
 * returns IQPT_OK or an iqpt_status, iqpt_last_error() has the detail, pointers are host pointers unless a
 * name says "device".
 */
#ifndef IQPT_DENOISE_H
#define IQPT_DENOISE_H

#include "iqpt.h"
#include "raster/iqpt_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IQPT_DENOISE_MAX_LEVELS 8u
#define IQPT_DENOISE_MAX_SQUARINGS 7u

typedef struct iqpt_denoise iqpt_denoise;

typedef struct iqpt_denoise_params {
    uint32_t levels;             /* L, 0..8: level i filters with step 2^i; 0 is the identity */
    uint32_t normal_squarings;   /* q, 0..7: the normal weight is max(n_p . n_q, 0)^(2^q) */
    float depth_sharpness;       /* s_z >= 0: the depth weight is 1 / (1 + ((z_p - z_q) s_z)^2); 0 switches it off */
    float colour_sharpness;      /* s_c >= 0: the colour weight is 1 / (1 + |c_p - c_q|^2 s_c^2 4^i); 0 switches it off */
} iqpt_denoise_params;

/* The defaults a new denoiser starts with. */
int iqpt_denoise_default_params(iqpt_denoise_params* out);

/* width, height: 1..8192. */
int iqpt_denoise_create(int device, uint32_t width, uint32_t height, iqpt_denoise** out);
int iqpt_denoise_destroy(iqpt_denoise* d);
int iqpt_denoise_set_params(iqpt_denoise* d, const iqpt_denoise_params* p);

/* The two guide planes, compact row-major: normal_z = (n.x, n.y, n.z, z) per pixel, id = the draw index or
 * IQPT_RASTER_NO_PRIM (the layout of iqpt_raster_read_gbuffer / iqpt_raster_gbuffer_device). Copied into
 * buffers the denoiser owns; the device form copies on the denoiser's stream and synchronises. */
int iqpt_denoise_set_guides(iqpt_denoise* d, const float* normal_z, const uint32_t* id);
int iqpt_denoise_set_guides_device(iqpt_denoise* d, const void* normal_z_device, const void* id_device);

/* Filter width*height float4 colours (xyz used) under the current guides and parameters: one kernel launch per
 * level on the denoiser's own stream, not waited for. The input is never modified; run_device reads it in
 * place during the first level, so it must stay valid and unchanged until the denoiser is synchronised. A
 * multi-GPU root may pass the buffer iqpt_gather_accum filled. */
int iqpt_denoise_run(iqpt_denoise* d, const float* colour);
int iqpt_denoise_run_device(iqpt_denoise* d, const void* colour_device);

/* The convenience call: takes ctx's accumulator through iqpt_copy_accum_device and r's G-buffer through
 * iqpt_raster_gbuffer (both every call), then runs. IQPT_ERR_INVALID_ARG unless ctx owns exactly
 * width*height pixels and r has the denoiser's frame size. */
int iqpt_denoise_frame(iqpt_denoise* d, iqpt_ctx* ctx, iqpt_raster* r);

/* Synchronises and copies out the last result: lin_rgba = 4 floats per pixel (w = +0 on filtered pixels),
 * bgra = 4 bytes per pixel encoded as the path tracer's frame. Either pointer may be NULL. */
int iqpt_denoise_read(iqpt_denoise* d, float* lin_rgba, uint8_t* bgra);
/* Device-to-device copy of the BGRA8 result (width*height uint32) on the denoiser's stream. Synchronises. */
int iqpt_denoise_copy_frame_device(iqpt_denoise* d, void* dst_device, size_t bytes);
int iqpt_denoise_sync(iqpt_denoise* d);
/* HIP-event durations of the runs since the last call (then cleared): the sum over runs, first level to last,
 * the sum per level (level_ms[8], levels not run stay 0; may be NULL), and the number of runs. Synchronises. */
int iqpt_denoise_time(iqpt_denoise* d, double* total_ms, double* level_ms, uint64_t* runs);

#ifdef __cplusplus
}
#endif

#endif /* IQPT_DENOISE_H */
