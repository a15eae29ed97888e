/*
 * iqpt_raster.h — C ABI of the headless HIP rasterizer (libiqpt.so), the engine's second renderer.
 *
 * The reference owns a rasterizer and a path tracer behind renderer_template (IoniqRE/renderer.cu:45-78,
 * renderer.h:34); its rasterizer is Direct3D 11 (rasterizer.cu, vertex_shader.hlsl, pixel_shader.hlsl). This
 * is that engine as a tile-based rasterizer in HIP, rendering into a headless BGRA8 frame. The pipeline
 * (clipping, snapping, top-left rule, depth, shading, resolve) is normative and written out in DESIGN.md §9;
 * tests/raster_ref.py restates it in numpy and the GPU frame equals it bit for bit.
 *
 *   reference                                                  this ABI
 *   --------------------------------------------------------  ----------------------------------------
 *   rasterizer::rasterizer (rasterizer.cu:25-104: MSAA target,
 *     D32 depth, CULL_BACK, m_samples) / rasterizer::shutdown  iqpt_raster_create / iqpt_raster_destroy
 *   shader::update_view_proj (shader.cu:55-60)                 iqpt_raster_set_camera
 *   mesh::setup_mesh vertex / index buffers (mesh.cu:37-64)
 *     + shader::update_transform per model (shader.cu:48-53)   iqpt_raster_upload_scene
 *   rasterizer::begin_frame clear + draw_scene's DrawIndexed
 *     loop + end_frame's ResolveSubresource (rasterizer.cu)    iqpt_raster_draw
 *   DrawIndexed on vertices the caller transformed itself      iqpt_raster_draw_clip
 *   Present (renderer_base) replaced by a readback             iqpt_raster_read / iqpt_raster_copy_frame_device
 *
 * These entry points are additions: IQPT_ABI_VERSION (iqpt.h) is unchanged. Conventions are iqpt.h's: every
 * function returns IQPT_OK or an iqpt_status, iqpt_last_error() has the detail, pointers are host pointers
 * unless a name says "device".
 */
#ifndef IQPT_RASTER_H
#define IQPT_RASTER_H

#include "iqpt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IQPT_RASTER_MAX_DIM 8192u            /* guard-band coordinates fit the 16.8 fixed-point range */
#define IQPT_RASTER_NO_PRIM 0xffffffffu      /* primitive index of a sample nothing covered */

typedef struct iqpt_raster iqpt_raster;

/* One draw of the scene in draw order (iqpt_scene_draw_list): what rasterizer::draw_scene binds per model. */
typedef struct iqpt_draw_item {
    float transform[16];           /* model::transform, row-vector, translation in row 3 */
    const iqpt_vertex* vertices;   /* owned by the scene; valid until it is modified or destroyed */
    const uint32_t* indices;       /* clockwise triples */
    uint32_t num_vertices;
    uint32_t num_indices;
    float albedo[3];               /* the pixel shader's (1, 0, 0), or the assigned material's albedo */
    int32_t mesh_type;             /* iqpt_mesh_type of the mesh (both are drawn with their mesh data) */
} iqpt_draw_item;

/* The models in the order iqpt_scene_build_packet walks them (mesh name, then insertion; scene.h:58-67), with
 * BOTH mesh types (the uv-spheres of IQPT_MESH_SPHERES included). `items` may be NULL to ask for the count;
 * otherwise up to `capacity` items are written. *count is always the number of models. */
int iqpt_scene_draw_list(const iqpt_scene* s, iqpt_draw_item* items, uint32_t capacity, uint32_t* count);

/* samples: 1 (pixel centre) or 4 (D3D11's standard pattern, the reference's m_samples). */
int iqpt_raster_create(int device, uint32_t width, uint32_t height, uint32_t samples, iqpt_raster** out);
int iqpt_raster_destroy(iqpt_raster* r);

/* Uses cam->view and cam->projection; cam->width / height must equal the frame's. */
int iqpt_raster_set_camera(iqpt_raster* r, const iqpt_camera* cam);

/* Copies every mesh and model of the scene to the device (the scene may be destroyed afterwards). */
int iqpt_raster_upload_scene(iqpt_raster* r, const iqpt_scene* scene);

/* Clear, draw the uploaded scene through the camera, resolve. Kernels run on the rasterizer's own stream and
 * the call does not wait for the frame; it waits once, mid-draw, for two counters (the number of set-up
 * triangles and of (tile, triangle) pairs) that size the bin lists. */
int iqpt_raster_draw(iqpt_raster* r);

/* The same frame from pre-transformed vertices, entering at the clipping stage: clip_xyzw 4 floats and normals
 * 3 floats per vertex (the world normals the pixel shader receives), indices clockwise triples; triangle k of
 * the index list has submission index k. Albedo is the shader's (1, 0, 0). */
int iqpt_raster_draw_clip(iqpt_raster* r, const float* clip_xyzw, const float* normals, uint32_t nverts,
                          const uint32_t* indices, uint32_t nindices);

/* Synchronises and copies out the last drawn frame: bgra = width*height*4 bytes (B, G, R, A; row-major).
 * depth_samples / prim_samples (either may be NULL): width*height*samples floats / uint32, sample-minor
 * ([y][x][s]): the D32 value and the submission index of the triangle that owns each sample
 * (IQPT_RASTER_NO_PRIM: cleared). Asking for them re-runs the tile kernel of the last draw with those outputs
 * on; a plain draw never writes them. */
int iqpt_raster_read(iqpt_raster* r, uint8_t* bgra, float* depth_samples, uint32_t* prim_samples);
/* Device-to-device copy of the BGRA8 frame (width*height uint32) on the rasterizer's stream. Synchronises. */
int iqpt_raster_copy_frame_device(iqpt_raster* r, void* dst_device, size_t bytes);
int iqpt_raster_sync(iqpt_raster* r);
/* Sum of the draws' durations (HIP events on the rasterizer's stream, first kernel to last) and their count
 * since the last call (then cleared). Synchronises. */
int iqpt_raster_time(iqpt_raster* r, double* total_ms, uint64_t* draws);
/* Per-stage split of the same draws, in ms: [0] vertex, [1] setup (incl. the counter readback), [2] bin,
 * [3] sort, [4] tile kernel. Cleared by iqpt_raster_time. */
int iqpt_raster_stage_time(iqpt_raster* r, double stage_ms[5]);
/* Work of the last draw: [0] triangles submitted, [1] set-up records, [2] (tile, triangle) pairs. */
int iqpt_raster_stats(iqpt_raster* r, uint64_t counts[3]);

/* ---------------------------------------------------------------- G-buffer
 * What a denoiser needs of the uploaded scene through the current camera, per pixel and noise-free: the pipeline
 * with ONE sample per pixel (whatever `samples` is) over an index list in which every triangle appears with both
 * windings, so that surfaces seen from behind have a guide too (the path tracer's triangle test is two-sided).
 * Per pixel, for the piece that owns the centre after the depth test:
 *   normal_z: 4 floats, the interpolated world normal normalised (not flipped towards the viewer; 0, 0, 0 where
 *             nothing was drawn) and the D32 depth (1.0 where nothing was drawn);
 *   id:       the draw index (the model's position in iqpt_scene_draw_list), IQPT_RASTER_NO_PRIM where nothing
 *             was drawn.
 * Both are compact row-major, width*height entries. A draw's frame does not depend on G-buffer passes before or
 * after it, and iqpt_raster_read keeps returning the last draw. */
/* Enqueues the pass on the rasterizer's stream (it waits once for two counters, as a draw does). The result is
 * kept until the camera or the scene changes: a second call in between does nothing. */
int iqpt_raster_gbuffer(iqpt_raster* r);
/* Synchronises and copies the G-buffer out. Either pointer may be NULL. IQPT_ERR_NOT_READY without a G-buffer
 * of the current camera and scene. */
int iqpt_raster_read_gbuffer(iqpt_raster* r, float* normal_z, uint32_t* id);
/* Synchronises and returns the device buffers; they stay valid until the next iqpt_raster_gbuffer,
 * iqpt_raster_upload_scene, iqpt_raster_set_camera or iqpt_raster_destroy. */
int iqpt_raster_gbuffer_device(iqpt_raster* r, const void** normal_z_device, const void** id_device);
/* Sum of the passes' durations (HIP events, vertex stage to tile kernel) and their count since the last call
 * (then cleared). Synchronises. */
int iqpt_raster_gbuffer_time(iqpt_raster* r, double* total_ms, uint64_t* passes);

#ifdef __cplusplus
}
#endif

#endif /* IQPT_RASTER_H */
