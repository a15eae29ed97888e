// iq_raster.hpp — types shared by the rasterizer's runtime (iq_raster.cpp) and its kernels
// (iq_raster_kernels.hip). The pipeline these implement is DESIGN.md §9.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

struct iqpt_raster;
struct iqpt_camera;

namespace iqr {

constexpr int kTile = 8;                       // 8 x 8 pixels: one wave64 per tile, lane = pixel
constexpr int kSubpixelBits = 8;               // 16.8 fixed point
constexpr int kMaxClipVerts = 9;               // a triangle against six planes
constexpr int kMaxPieces = kMaxClipVerts - 2;  // fan of the clipped polygon
constexpr int kPieceBits = 3;                  // sort key = submission index << 3 | piece
constexpr uint32_t kMaxTriangles = 1u << 28;   // the key fits 31 bits; (tile << key_bits | key) is the 64-bit sort key
constexpr uint32_t kNoPrim = 0xffffffffu;
constexpr uint32_t kClearBgra = 0xff9ed6ffu;   // (0.62, 0.84, 1.0, 1) -> B 255, G 214, R 158, A 255

// One draw: a slice of the vertex pool and of the index pool, its transform and normal matrix.
struct draw_rec {
    float model[16];        // row-vector transform, m[r][c]
    float normal[12];       // iq::normal_matrix(model), rows 0..2, 4 floats each (w column unused)
    float albedo[4];
    uint32_t vbase;         // first vertex of the draw in the transformed-vertex arrays
    uint32_t src_vbase;     // first vertex of its mesh in the mesh vertex pool
    uint32_t ibase;         // first index of its mesh in the index pool
    uint32_t tbase;         // submission index of its first triangle
    uint32_t item;          // the draw index: its model's position in iqpt_scene_draw_list (setup_rec.pad[0])
};

// Set-up triangle, 32 words, read wave-uniformly by the tile kernel.
struct setup_rec {
    int32_t x0, y0, x1, y1, x2, y2;   // snapped screen positions, 1/256 pixel
    float z0, dz1, dz2;               // z_s of vertex 0, z1 - z0, z2 - z0
    float rw0, rw1, rw2;              // 1 / w
    float n0[3], n1[3], n2[3];        // world normals
    float albedo[3];
    uint32_t key;                     // submission index << kPieceBits | piece
    uint32_t tile_x0y0, tile_x1y1;    // inclusive tile bounding box, x | y << 16
    uint32_t pair_base;               // first of its (tile, key) pairs
    uint32_t pad[4];                  // pad[0]: the draw index (draw_rec.item), what the G-buffer's id plane holds
};
static_assert(sizeof(setup_rec) == 128, "setup record is 32 words");

struct frame_params {
    uint32_t width, height, samples;
    uint32_t ntx, nty;
};

struct counters {
    unsigned long long nrec;     // set-up records wanted (may exceed the capacity: then the pass is redone)
    unsigned long long npairs;   // (tile, record) pairs
};

// launchers (iq_raster_kernels.hip); every one enqueues on `s` and returns the launch status
hipError_t launch_vertex(hipStream_t s, const draw_rec* draws, uint32_t ndraws, const uint32_t* draw_vend,
                         uint32_t nverts, const float* mesh_verts, const float* view, const float* proj,
                         float* clip, float* wn);
hipError_t launch_setup(hipStream_t s, const frame_params& fp, const draw_rec* draws, uint32_t ndraws,
                        const uint32_t* draw_tend, uint32_t ntris, const uint32_t* indices, const float* clip,
                        const float* wn, setup_rec* recs, uint32_t rec_cap, counters* cnt);
// The G-buffer's setup: the doubled index list, thread t = submission index t of 2 ntris: triangle
// t >> 1, its second and third index swapped when t is odd. fp.samples must be 1.
hipError_t launch_setup_guide(hipStream_t s, const frame_params& fp, const draw_rec* draws, uint32_t ndraws,
                              const uint32_t* draw_tend, uint32_t ntris, const uint32_t* indices, const float* clip,
                              const float* wn, setup_rec* recs, uint32_t rec_cap, counters* cnt);
hipError_t launch_bin(hipStream_t s, const frame_params& fp, const setup_rec* recs, uint32_t nrec, unsigned key_bits,
                      unsigned long long* keys, uint32_t* vals);
// range: two words per tile, the run [start, end) of the tile's pairs in the sorted arrays (0, 0: none)
hipError_t launch_ranges(hipStream_t s, const frame_params& fp, const unsigned long long* keys, uint32_t npairs,
                         unsigned key_bits, uint32_t* range);
hipError_t sort_pairs(hipStream_t s, void* temp, size_t& temp_bytes, const unsigned long long* keys_in,
                      unsigned long long* keys_out, const uint32_t* vals_in, uint32_t* vals_out, uint32_t n,
                      unsigned end_bit);
hipError_t launch_tiles(hipStream_t s, const frame_params& fp, const setup_rec* recs, const uint32_t* vals,
                        const uint32_t* range, uint32_t* frame, float* depth_samples, uint32_t* prim_samples);
// The G-buffer's tile kernel: normal_z = float4 (n, z) and id = the owning record's draw index per pixel.
hipError_t launch_guide_tiles(hipStream_t s, const frame_params& fp, const setup_rec* recs, const uint32_t* vals,
                              const uint32_t* range, void* normal_z, uint32_t* id);

// the frame size of a rasterizer, for the library's other parts (the denoiser checks it against its own)
void frame_size(const iqpt_raster* r, uint32_t* width, uint32_t* height);
// the camera of the last iqpt_raster_set_camera, whole (the temporal history needs its inverse matrices too);
// NULL before the first one
const iqpt_camera* current_camera(const iqpt_raster* r);

}  // namespace iqr
