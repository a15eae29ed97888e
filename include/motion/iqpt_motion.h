/*
 * iqpt_motion.h — C ABI of moving-model reprojection (libiqpt_motion.so, which links libiqpt.so): a temporal
 * object (temporal/iqpt_temporal.h) whose history also follows the models. A model "moves" by
 * building the next scene with the same meshes and models and other transforms; iqpt_motion_table turns the two
 * scenes' draw lists into one entry per draw index, and begin_view sends every pixel of a moved model back
 * through its entry before it is projected into the previous view. The definition is normative and written out
 * in DESIGN.md §15; tests/motion_ref.py restates it in numpy and the GPU result equals it bit for bit.
 *
 * The reference has no temporal reuse. These entry points are additions in a library of their own:
 * IQPT_ABI_VERSION (iqpt.h) and libiqpt.so's exports are unchanged. Conventions are iqpt.h's: every function
 * returns IQPT_OK or an iqpt_status, iqpt_last_error() has the detail, pointers are host pointers unless a name
 * says "device".
 */
#ifndef IQPT_MOTION_H
#define IQPT_MOTION_H

#include "iqpt.h"
#include "raster/iqpt_raster.h"
#include "temporal/iqpt_temporal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IQPT_MOTION_MAX_ENTRIES 1048576u   /* 2^20 */

typedef struct iqpt_motion iqpt_motion;

/* One draw index's motion between the previous view's scene and the current one: 128 bytes. */
typedef struct iqpt_motion_entry {
    float back[16];       /* row-vector 4x4, row-major: a point of the current world -> where that point of the model
                             was in the previous view's world */
    float nback[12];      /* 3 rows of 4: the normal matrix of back; the fourth column is ignored */
    uint32_t moved;       /* 0 or 1 */
    uint32_t reserved[3]; /* 0 */
} iqpt_motion_entry;

/* The table of two iqpt_scene_draw_list results (host only). IQPT_ERR_INVALID_ARG unless the counts are equal
 * and each draw has the same num_vertices and num_indices in both. A draw whose 16 transform words are bit-equal
 * gets moved = 0 and identity matrices; any other gets moved = 1, back = inversed(cur) * prev and nback = the
 * first three rows of normal_matrix(back), in iq_host_math.hpp's arithmetic. A singular cur makes back all
 * infinity: that draw then has no history. `out` receives n_cur entries. */
int iqpt_motion_table(const iqpt_draw_item* prev_items, uint32_t n_prev, const iqpt_draw_item* cur_items,
                      uint32_t n_cur, iqpt_motion_entry* out);

/* iqpt_temporal_default_params' values. */
int iqpt_motion_default_params(iqpt_temporal_params* out);

/* width, height: 1..8192. */
int iqpt_motion_create(int device, uint32_t width, uint32_t height, iqpt_motion** out);
int iqpt_motion_destroy(iqpt_motion* m);
int iqpt_motion_set_params(iqpt_motion* m, const iqpt_temporal_params* p);

/* A new view, as iqpt_temporal_begin_view, with the motion table of the scene change that led to it: n entries
 * (0..2^20), one per draw index; table may be NULL only with n == 0, which is iqpt_temporal_begin_view itself. A
 * pixel whose id is >= n (n > 0) starts with an empty history. IQPT_ERR_INVALID_ARG for an entry whose moved is
 * neither 0 nor 1 or with a non-zero reserved word. The table is a host pointer in every form; it is copied to a
 * device buffer of the object's on its stream before the view kernel runs. */
int iqpt_motion_begin_view(iqpt_motion* m, const iqpt_camera* cam, const float* normal_z, const uint32_t* id,
                           const iqpt_motion_entry* table, uint32_t n);
int iqpt_motion_begin_view_device(iqpt_motion* m, const iqpt_camera* cam, const void* normal_z_device,
                                  const void* id_device, const iqpt_motion_entry* table, uint32_t n);
int iqpt_motion_begin_view_raster(iqpt_motion* m, iqpt_raster* r, const iqpt_motion_entry* table, uint32_t n);
/* Forgets the view and the result. Call it when the next scene has other meshes or models than the last. */
int iqpt_motion_clear(iqpt_motion* m);

/* As iqpt_temporal_resolve*, _read, _output_device, _copy_frame_device, _sync and _time. */
int iqpt_motion_resolve(iqpt_motion* m, const float* colour, uint64_t n);
int iqpt_motion_resolve_device(iqpt_motion* m, const void* colour_device, uint64_t n);
int iqpt_motion_resolve_ctx(iqpt_motion* m, iqpt_ctx* ctx);
int iqpt_motion_read(iqpt_motion* m, float* lin_rgba, uint8_t* bgra);
int iqpt_motion_output_device(iqpt_motion* m, const void** out_device);
int iqpt_motion_copy_frame_device(iqpt_motion* m, void* dst_device, size_t bytes);
int iqpt_motion_sync(iqpt_motion* m);
int iqpt_motion_time(iqpt_motion* m, double* view_ms, uint64_t* views, double* resolve_ms, uint64_t* resolves);
/* Of the last begin_view: the pixels with a guide, those among them with a valid history, the pixels whose
 * entry has moved == 1 and those among these with a valid history, counted by a reduction run by this call.
 * Synchronises. IQPT_ERR_NOT_READY without a view. */
int iqpt_motion_stats(iqpt_motion* m, uint64_t* guided, uint64_t* valid, uint64_t* moved, uint64_t* moved_valid);

#ifdef __cplusplus
}
#endif

#endif /* IQPT_MOTION_H */
