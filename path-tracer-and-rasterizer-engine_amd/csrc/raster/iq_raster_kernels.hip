// iq_raster_kernels.hip — the rasterizer's kernels for gfx950 (wave64): vertex stage, triangle setup
// (clipping, snapping, culling), binning into 8x8 tiles, the (tile, submission index) sort and the tile
// kernel (coverage, depth, shading, resolve). DESIGN.md §9 is the pipeline these restate; every float
// operation below is written in that section's order and compiled with -ffp-contract=off.
#include <cstring>   // rocprim's headers use memset without including it

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "raster/iq_raster.hpp"

namespace iqr {

namespace {

constexpr int kBlock = 256;

// smallest d with i < ends[d] (ends ascending, i < ends[n - 1])
__device__ inline uint32_t find_draw(const uint32_t* __restrict__ ends, uint32_t n, uint32_t i) {
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (i < ends[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// iqvec::transformed (vector.h:371-383): a row vector times a row-major matrix, each component a
// left-to-right dot product over the column
__device__ inline void mul_row(const float v[4], const float* __restrict__ m, float out[4]) {
    for (int c = 0; c < 4; ++c) out[c] = v[0] * m[c] + v[1] * m[4 + c] + v[2] * m[8 + c] + v[3] * m[12 + c];
}

// ------------------------------------------------------------------------------------------ vertex stage
// vertex_shader.hlsl: world = (pos, 1) model, clip = world view projection, wn = normalize(n N) with N the
// path tracer's normal matrix (iq_host_math.hpp normal_matrix) and normalize in normalized3's order.
__global__ void __launch_bounds__(kBlock) iqr_vertex_kernel(const draw_rec* __restrict__ draws, uint32_t ndraws,
                                                           const uint32_t* __restrict__ draw_vend, uint32_t nverts,
                                                           const float* __restrict__ mesh_verts,
                                                           const float* __restrict__ view,
                                                           const float* __restrict__ proj, float* __restrict__ clip,
                                                           float* __restrict__ wn) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nverts) return;
    const draw_rec& d = draws[find_draw(draw_vend, ndraws, i)];
    const float* src = mesh_verts + 6 * (size_t)(d.src_vbase + (i - d.vbase));
    const float p[4] = {src[0], src[1], src[2], 1.0f};
    float world[4], eye[4], c[4];
    mul_row(p, d.model, world);
    mul_row(world, view, eye);
    mul_row(eye, proj, c);
    // the normal as a direction (w = 0) through N, whose fourth row is (0, 0, 0, 1)
    float n[3];
    for (int k = 0; k < 3; ++k)
        n[k] = src[3] * d.normal[k] + src[4] * d.normal[4 + k] + src[5] * d.normal[8 + k] + 0.0f * 0.0f;
    const float eps = 0.00001f;
    float o[3] = {0.0f, 0.0f, 0.0f};
    if (!(fabsf(n[0]) < eps && fabsf(n[1]) < eps && fabsf(n[2]) < eps)) {
        const float inv = 1.0f / sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        o[0] = n[0] * inv; o[1] = n[1] * inv; o[2] = n[2] * inv;
    }
    reinterpret_cast<float4*>(clip)[i] = make_float4(c[0], c[1], c[2], c[3]);
    reinterpret_cast<float4*>(wn)[i] = make_float4(o[0], o[1], o[2], 0.0f);
}

// ------------------------------------------------------------------------------------------ setup
struct cvert {
    float v[7];   // clip x, y, z, w, world normal x, y, z
};

__device__ inline float plane_dist(const cvert& a, int plane) {
    const float x = a.v[0], y = a.v[1], z = a.v[2], w = a.v[3];
    switch (plane) {
    case 0: return z;
    case 1: return w - z;
    case 2: return x + 4.0f * w;
    case 3: return 4.0f * w - x;
    case 4: return y + 4.0f * w;
    default: return 4.0f * w - y;
    }
}

// new vertex on the edge from the inside vertex a to the outside vertex b
__device__ inline cvert intersect(const cvert& a, float da, const cvert& b, float db) {
    const float t = da / (da - db);
    cvert r;
    for (int k = 0; k < 7; ++k) r.v[k] = a.v[k] + t * (b.v[k] - a.v[k]);
    return r;
}

constexpr float kMaxScreen = 32768.0f;   // pixels; the guard band of an 8192-wide frame ends at 20480

__device__ inline int imax(int a, int b) { return a > b ? a : b; }
__device__ inline int imin(int a, int b) { return a < b ? a : b; }

// kGuide: the G-buffer's doubled index list: thread t is submission index t of 2 ntris, triangle
// t >> 1 of the index list, with its second and third index swapped when t is odd, so that CULL_BACK keeps
// whichever of the two faces the camera.
template <bool kGuide>
__global__ void __launch_bounds__(kBlock) iqr_setup_kernel(frame_params fp, const draw_rec* __restrict__ draws,
                                                          uint32_t ndraws, const uint32_t* __restrict__ draw_tend,
                                                          uint32_t ntris, const uint32_t* __restrict__ indices,
                                                          const float* __restrict__ clip,
                                                          const float* __restrict__ wn, setup_rec* __restrict__ recs,
                                                          uint32_t rec_cap, counters* __restrict__ cnt) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;          // the submission index
    const uint32_t tri = kGuide ? t >> 1 : t;
    if (tri >= ntris) return;
    const draw_rec& d = draws[find_draw(draw_tend, ndraws, tri)];
    const uint32_t* idx = indices + d.ibase + 3 * (size_t)(tri - d.tbase);
    const bool swap = kGuide && (t & 1u);

    cvert poly[kMaxClipVerts], tmp[kMaxClipVerts];
    bool need_clip = false;
    unsigned all_out = 0x3fu;       // bit p: every vertex is outside plane p
    for (int k = 0; k < 3; ++k) {
        const uint32_t vi = d.vbase + idx[swap && k ? 3 - k : k];
        const float4 c = reinterpret_cast<const float4*>(clip)[vi];
        const float4 n = reinterpret_cast<const float4*>(wn)[vi];
        poly[k].v[0] = c.x; poly[k].v[1] = c.y; poly[k].v[2] = c.z; poly[k].v[3] = c.w;
        poly[k].v[4] = n.x; poly[k].v[5] = n.y; poly[k].v[6] = n.z;
        for (int p = 0; p < 6; ++p) {
            const bool in = plane_dist(poly[k], p) >= 0.0f;
            need_clip |= !in;
            if (in) all_out &= ~(1u << p);
        }
    }
    if (all_out) return;            // entirely outside one plane
    int n = 3;
    if (need_clip) {
        // Sutherland-Hodgman, planes in the order z >= 0, z <= w, x >= -4w, x <= 4w, y >= -4w, y <= 4w
        for (int p = 0; p < 6 && n > 0; ++p) {
            int m = 0;
            for (int i = 0; i < n; ++i) {
                const cvert& a = poly[i];
                const cvert& b = poly[i + 1 == n ? 0 : i + 1];
                const float da = plane_dist(a, p), db = plane_dist(b, p);
                const bool ia = da >= 0.0f, ib = db >= 0.0f;
                if (ia) {
                    if (m < kMaxClipVerts) tmp[m++] = a;
                    if (!ib && m < kMaxClipVerts) tmp[m++] = intersect(a, da, b, db);
                } else if (ib) {
                    if (m < kMaxClipVerts) tmp[m++] = intersect(b, db, a, da);
                }
            }
            for (int i = 0; i < m; ++i) poly[i] = tmp[i];
            n = m;
        }
    }
    if (n < 3) return;
    for (int i = 0; i < n; ++i)
        if (!(poly[i].v[3] > 0.0f)) return;     // w = 0 survives the planes only at the origin: no projection

    // viewport and snapping to 16.8, round to nearest even
    int32_t sx[kMaxClipVerts], sy[kMaxClipVerts];
    float sz[kMaxClipVerts], rw[kMaxClipVerts];
    const float fw = (float)fp.width, fh = (float)fp.height;
    for (int i = 0; i < n; ++i) {
        const float w = poly[i].v[3];
        const float xs = (poly[i].v[0] / w + 1.0f) * fw * 0.5f;
        const float ys = (1.0f - poly[i].v[1] / w) * fh * 0.5f;
        if (!(fabsf(xs) <= kMaxScreen) || !(fabsf(ys) <= kMaxScreen)) return;   // not finite, or beyond any guard band
        sx[i] = (int32_t)rintf(xs * 256.0f);
        sy[i] = (int32_t)rintf(ys * 256.0f);
        sz[i] = fminf(fmaxf(poly[i].v[2] / w, 0.0f), 1.0f);
        rw[i] = 1.0f / w;
    }

    for (int piece = 0; piece + 2 < n; ++piece) {
        const int a = 0, b = piece + 1, c = piece + 2;
        const long long area = (long long)(sx[b] - sx[a]) * (sy[c] - sy[a]) - (long long)(sx[c] - sx[a]) * (sy[b] - sy[a]);
        if (area <= 0) continue;                // CULL_BACK (clockwise front, y down) and zero area
        const int xmin = imin(sx[a], imin(sx[b], sx[c])), xmax = imax(sx[a], imax(sx[b], sx[c]));
        const int ymin = imin(sy[a], imin(sy[b], sy[c])), ymax = imax(sy[a], imax(sy[b], sy[c]));
        // pixels with a sample coordinate inside the box: the sample coordinates are the lattice 256 k + 128
        // (1 sample) or 64 k + 32 (the four-sample pattern), per axis
        int px0, px1, py0, py1;
        if (fp.samples == 1) {
            px0 = (xmin - 128 + 255) >> 8; px1 = (xmax - 128) >> 8;
            py0 = (ymin - 128 + 255) >> 8; py1 = (ymax - 128) >> 8;
        } else {
            const int kx0 = (xmin - 32 + 63) >> 6, kx1 = (xmax - 32) >> 6;
            const int ky0 = (ymin - 32 + 63) >> 6, ky1 = (ymax - 32) >> 6;
            if (kx0 > kx1 || ky0 > ky1) continue;
            px0 = kx0 >> 2; px1 = kx1 >> 2;
            py0 = ky0 >> 2; py1 = ky1 >> 2;
        }
        px0 = imax(px0, 0); py0 = imax(py0, 0);
        px1 = imin(px1, (int)fp.width - 1); py1 = imin(py1, (int)fp.height - 1);
        if (px0 > px1 || py0 > py1) continue;
        const uint32_t tx0 = (uint32_t)px0 / kTile, tx1 = (uint32_t)px1 / kTile;
        const uint32_t ty0 = (uint32_t)py0 / kTile, ty1 = (uint32_t)py1 / kTile;
        const uint32_t ntiles = (tx1 - tx0 + 1) * (ty1 - ty0 + 1);
        const unsigned long long slot = atomicAdd(&cnt->nrec, 1ull);
        const unsigned long long pair_base = atomicAdd(&cnt->npairs, (unsigned long long)ntiles);
        if (slot >= rec_cap || pair_base + ntiles > 0xffffffffull) continue;   // the host grows the buffer and redoes the pass
        setup_rec r;
        r.x0 = sx[a]; r.y0 = sy[a]; r.x1 = sx[b]; r.y1 = sy[b]; r.x2 = sx[c]; r.y2 = sy[c];
        r.z0 = sz[a]; r.dz1 = sz[b] - sz[a]; r.dz2 = sz[c] - sz[a];
        r.rw0 = rw[a]; r.rw1 = rw[b]; r.rw2 = rw[c];
        for (int k = 0; k < 3; ++k) {
            r.n0[k] = poly[a].v[4 + k]; r.n1[k] = poly[b].v[4 + k]; r.n2[k] = poly[c].v[4 + k];
            r.albedo[k] = d.albedo[k];
        }
        r.key = t << kPieceBits | (uint32_t)piece;
        r.tile_x0y0 = tx0 | ty0 << 16;
        r.tile_x1y1 = tx1 | ty1 << 16;
        r.pair_base = (uint32_t)pair_base;
        r.pad[0] = d.item;
        r.pad[1] = r.pad[2] = r.pad[3] = 0;
        recs[slot] = r;
    }
}

// ------------------------------------------------------------------------------------------ binning
// One (tile << key_bits | key, record) pair per tile of a record's bounding box, at the positions the setup pass
// reserved. Small boxes are written by the record's own lane, large ones by the whole wave.
__global__ void __launch_bounds__(kBlock) iqr_bin_kernel(frame_params fp, const setup_rec* __restrict__ recs,
                                                        uint32_t nrec, unsigned key_bits,
                                                        unsigned long long* __restrict__ keys,
                                                        uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool valid = i < nrec;
    uint32_t tx0 = 0, ty0 = 0, bw = 0, bh = 0, key = 0, base = 0;
    if (valid) {
        const setup_rec& r = recs[i];
        tx0 = r.tile_x0y0 & 0xffffu; ty0 = r.tile_x0y0 >> 16;
        bw = (r.tile_x1y1 & 0xffffu) - tx0 + 1; bh = (r.tile_x1y1 >> 16) - ty0 + 1;
        key = r.key; base = r.pair_base;
    }
    const uint32_t n = bw * bh;
    constexpr uint32_t kSmall = 32;
    if (valid && n <= kSmall) {
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t tile = (ty0 + j / bw) * fp.ntx + tx0 + j % bw;
            keys[base + j] = (unsigned long long)tile << key_bits | key;
            vals[base + j] = i;
        }
    }
    unsigned long long big = __ballot(valid && n > kSmall);
    while (big) {
        const int l = __ffsll((long long)big) - 1;
        big &= big - 1;
        const uint32_t btx0 = __shfl(tx0, l), bty0 = __shfl(ty0, l), bbw = __shfl(bw, l), bn = __shfl(n, l);
        const uint32_t bkey = __shfl(key, l), bbase = __shfl(base, l), bi = __shfl(i, l);
        for (uint32_t j = lane; j < bn; j += 64) {
            const uint32_t tile = (bty0 + j / bbw) * fp.ntx + btx0 + j % bbw;
            keys[bbase + j] = (unsigned long long)tile << key_bits | bkey;
            vals[bbase + j] = bi;
        }
    }
}

// ------------------------------------------------------------------------------------------ tile kernel
__device__ inline uint32_t unorm8(float c) {
    return (uint32_t)(fminf(fmaxf(c, 0.0f), 1.0f) * 255.0f + 0.5f);
}

// After the sort: the run of pairs [range[2t], range[2t + 1]) of every tile t that has any (range is zeroed first).
__global__ void __launch_bounds__(kBlock) iqr_range_kernel(const unsigned long long* __restrict__ keys, uint32_t npairs,
                                                          unsigned key_bits, uint32_t* __restrict__ range) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= npairs) return;
    const uint32_t t = (uint32_t)(keys[i] >> key_bits);
    if (i == 0 || (uint32_t)(keys[i - 1] >> key_bits) != t) range[2 * t] = i;
    if (i + 1 == npairs || (uint32_t)(keys[i + 1] >> key_bits) != t) range[2 * t + 1] = i + 1;
}

// sample offsets from the pixel centre in 1/256 pixel: the centre, or D3D11's standard 4x pattern
// (-2,-6), (6,-2), (-6,2), (2,6) sixteenths
template <int S> __device__ inline int sample_ox(int s) { return S == 1 ? 0 : (s == 0 ? -32 : s == 1 ? 96 : s == 2 ? -96 : 32); }
template <int S> __device__ inline int sample_oy(int s) { return S == 1 ? 0 : (s == 0 ? -96 : s == 1 ? -32 : s == 2 ? 32 : 96); }

// One record against one pixel's samples. Coordinates are relative to the tile's origin (differences are what the
// edge functions use); T is the integer the edge functions are evaluated in: int where the triangle is small
// enough for every product to fit (the caller decides, wave-uniformly), else long long. Both are exact.
template <int S, typename T>
__device__ inline void raster_record(const setup_rec& r, int tox, int toy, int pcx, int pcy, float (&depth)[S],
                                     uint32_t (&colour)[S], uint32_t (&prim)[S]) {
    const int x0 = r.x0 - tox, y0 = r.y0 - toy, x1 = r.x1 - tox, y1 = r.y1 - toy, x2 = r.x2 - tox, y2 = r.y2 - toy;
    // edge k is opposite vertex k: e0 = v1 -> v2, e1 = v2 -> v0, e2 = v0 -> v1
    const int dx0 = x2 - x1, dy0 = y2 - y1, dx1 = x0 - x2, dy1 = y0 - y2, dx2 = x1 - x0, dy2 = y1 - y0;
    // top-left rule: a zero edge function is inside on a top edge (dy == 0, dx > 0) or a left edge (dy < 0)
    const T bias0 = (dy0 < 0 || (dy0 == 0 && dx0 > 0)) ? 0 : 1;
    const T bias1 = (dy1 < 0 || (dy1 == 0 && dx1 > 0)) ? 0 : 1;
    const T bias2 = (dy2 < 0 || (dy2 == 0 && dx2 > 0)) ? 0 : 1;
    const T e0c = (T)dx0 * (T)(pcy - y1) - (T)dy0 * (T)(pcx - x1);
    const T e1c = (T)dx1 * (T)(pcy - y2) - (T)dy1 * (T)(pcx - x2);
    const T e2c = (T)dx2 * (T)(pcy - y0) - (T)dy2 * (T)(pcx - x0);
    bool cov[S];
    T e1s[S], e2s[S];
    bool any_cov = false;
    for (int s = 0; s < S; ++s) {
        const int ox = sample_ox<S>(s), oy = sample_oy<S>(s);
        const T e0 = e0c + ((T)dx0 * oy - (T)dy0 * ox);
        e1s[s] = e1c + ((T)dx1 * oy - (T)dy1 * ox);
        e2s[s] = e2c + ((T)dx2 * oy - (T)dy2 * ox);
        cov[s] = e0 >= bias0 && e1s[s] >= bias1 && e2s[s] >= bias2;
        any_cov |= cov[s];
    }
    if (!any_cov) return;
    const long long area = (long long)dx2 * (y2 - y0) - (long long)(x2 - x0) * dy2;
    const float farea = (float)area;
    bool pass[S];
    float zs[S];
    bool any = false;
    for (int s = 0; s < S; ++s) {
        pass[s] = false;
        if (cov[s]) {
            const float b1 = (float)e1s[s] / farea, b2 = (float)e2s[s] / farea;
            float z = r.z0 + b1 * r.dz1 + b2 * r.dz2;
            z = fminf(fmaxf(z, 0.0f), 1.0f);
            zs[s] = z;
            pass[s] = z < depth[s];                 // LESS; in-order walk: the earlier submission keeps ties
            any |= pass[s];
        }
    }
    if (!any) return;
    // pixel_shader.hlsl at the pixel centre (extrapolated when the centre is uncovered)
    const float amb_r = 0.2f * 0.62f, amb_g = 0.2f * 0.84f, amb_b = 0.2f * 1.0f;
    const float p0 = (float)e0c / farea * r.rw0, p1 = (float)e1c / farea * r.rw1, p2 = (float)e2c / farea * r.rw2;
    const float sum = p0 + p1 + p2;
    const float nx = (p0 * r.n0[0] + p1 * r.n1[0] + p2 * r.n2[0]) / sum;
    const float ny = (p0 * r.n0[1] + p1 * r.n1[1] + p2 * r.n2[1]) / sum;
    const float nz = (p0 * r.n0[2] + p1 * r.n1[2] + p2 * r.n2[2]) / sum;
    const float diffuse = fmaxf((-nx) * 0.0f + (-ny) * -1.0f + (-nz) * 0.0f, 0.0f);
    const float cr = (amb_r + diffuse) * r.albedo[0];
    const float cg = (amb_g + diffuse) * r.albedo[1];
    const float cb = (amb_b + diffuse) * r.albedo[2];
    const uint32_t c = unorm8(cb) | unorm8(cg) << 8 | unorm8(cr) << 16 | 0xff000000u;
    const uint32_t id = r.key >> kPieceBits;
    for (int s = 0; s < S; ++s)
        if (pass[s]) {
            depth[s] = zs[s];
            colour[s] = c;
            prim[s] = id;
        }
}

__device__ inline int iabs(int a) { return a < 0 ? -a : a; }

// One wave64 per 8x8 tile, lane = pixel. The tile's records are a contiguous, ascending run of the sorted
// pairs; they are walked in that order with wave-uniform loads, the samples' depth, colour and primitive
// index stay in registers and the resolved pixel is stored once.
template <int S>
__global__ void __launch_bounds__(64) iqr_tile_kernel(frame_params fp, const setup_rec* __restrict__ recs,
                                                     const uint32_t* __restrict__ vals,
                                                     const uint32_t* __restrict__ range,
                                                     uint32_t* __restrict__ frame, float* __restrict__ depth_out,
                                                     uint32_t* __restrict__ prim_out) {
    const uint32_t tile = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const int tox = (int)(tile % fp.ntx) * kTile * 256, toy = (int)(tile / fp.ntx) * kTile * 256;
    const uint32_t px = (tile % fp.ntx) * kTile + (lane & 7u);
    const uint32_t py = (tile / fp.ntx) * kTile + (lane >> 3);
    const int pcx = (int)(lane & 7u) * 256 + 128, pcy = (int)(lane >> 3) * 256 + 128;

    float depth[S];
    uint32_t colour[S], prim[S];
    for (int s = 0; s < S; ++s) {
        depth[s] = 1.0f;
        colour[s] = kClearBgra;
        prim[s] = kNoPrim;
    }

    uint32_t lo = 0, hi = 0;
    if (range) {
        lo = range[2 * tile];
        hi = range[2 * tile + 1];
    }
    lo = __builtin_amdgcn_readfirstlane(lo);
    hi = __builtin_amdgcn_readfirstlane(hi);

    for (uint32_t chunk = lo; chunk < hi; chunk += 64) {
        const uint32_t cn = hi - chunk < 64u ? hi - chunk : 64u;
        const uint32_t my = lane < cn ? vals[chunk + lane] : 0u;
        for (uint32_t j = 0; j < cn; ++j) {
            const uint32_t slot = __builtin_amdgcn_readlane(my, j);
            const setup_rec& r = recs[slot];
            // 32-bit edge functions where no product can overflow: extents up to 64 pixels, and the vertices
            // are then within 72 pixels of the tile's origin (the triangle's box meets the tile)
            const int ext = imax(imax(iabs(r.x1 - r.x0), iabs(r.x2 - r.x0)), iabs(r.x2 - r.x1)) |
                            imax(imax(iabs(r.y1 - r.y0), iabs(r.y2 - r.y0)), iabs(r.y2 - r.y1));
            if (ext < 16384) raster_record<S, int>(r, tox, toy, pcx, pcy, depth, colour, prim);
            else raster_record<S, long long>(r, tox, toy, pcx, pcy, depth, colour, prim);
        }
    }

    if (px >= fp.width || py >= fp.height) return;
    uint32_t out;
    if (S == 1) {
        out = colour[0];
    } else {
        out = 0;
        for (int ch = 0; ch < 4; ++ch) {
            uint32_t acc = 2;
            for (int s = 0; s < S; ++s) acc += colour[s] >> (8 * ch) & 0xffu;
            out |= (acc >> 2) << (8 * ch);
        }
    }
    const size_t pix = (size_t)py * fp.width + px;
    frame[pix] = out;
    if (depth_out)
        for (int s = 0; s < S; ++s) depth_out[pix * S + s] = depth[s];
    if (prim_out)
        for (int s = 0; s < S; ++s) prim_out[pix * S + s] = prim[s];
}

// ------------------------------------------------------------------------------------------ G-buffer tiles
// One record against one pixel centre: coverage and depth only; the lane that passes remembers the record.
template <typename T>
__device__ inline void guide_record(const setup_rec& r, uint32_t slot, int tox, int toy, int pcx, int pcy, float& depth,
                                    uint32_t& owner) {
    const int x0 = r.x0 - tox, y0 = r.y0 - toy, x1 = r.x1 - tox, y1 = r.y1 - toy, x2 = r.x2 - tox, y2 = r.y2 - toy;
    const int dx0 = x2 - x1, dy0 = y2 - y1, dx1 = x0 - x2, dy1 = y0 - y2, dx2 = x1 - x0, dy2 = y1 - y0;
    const T bias0 = (dy0 < 0 || (dy0 == 0 && dx0 > 0)) ? 0 : 1;
    const T bias1 = (dy1 < 0 || (dy1 == 0 && dx1 > 0)) ? 0 : 1;
    const T bias2 = (dy2 < 0 || (dy2 == 0 && dx2 > 0)) ? 0 : 1;
    const T e0 = (T)dx0 * (T)(pcy - y1) - (T)dy0 * (T)(pcx - x1);
    const T e1 = (T)dx1 * (T)(pcy - y2) - (T)dy1 * (T)(pcx - x2);
    const T e2 = (T)dx2 * (T)(pcy - y0) - (T)dy2 * (T)(pcx - x0);
    if (!(e0 >= bias0 && e1 >= bias1 && e2 >= bias2)) return;
    const long long area = (long long)dx2 * (y2 - y0) - (long long)(x2 - x0) * dy2;
    const float farea = (float)area;
    const float b1 = (float)e1 / farea, b2 = (float)e2 / farea;
    float z = r.z0 + b1 * r.dz1 + b2 * r.dz2;
    z = fminf(fmaxf(z, 0.0f), 1.0f);
    if (z < depth) {                                // LESS; in-order walk: the earlier submission keeps ties
        depth = z;
        owner = slot;
    }
}

// The tile kernel's G-buffer instantiation: the same walk with one sample at the pixel centre;
// each lane keeps the depth and the slot of the record that owns it and evaluates that record's interpolated
// normal once, after the walk (a per-lane load of 128 bytes instead of shading every record that passes).
__global__ void __launch_bounds__(64) iqr_guide_tile_kernel(frame_params fp, const setup_rec* __restrict__ recs,
                                                           const uint32_t* __restrict__ vals,
                                                           const uint32_t* __restrict__ range,
                                                           float4* __restrict__ normal_z, uint32_t* __restrict__ id) {
    const uint32_t tile = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const int tox = (int)(tile % fp.ntx) * kTile * 256, toy = (int)(tile / fp.ntx) * kTile * 256;
    const uint32_t px = (tile % fp.ntx) * kTile + (lane & 7u);
    const uint32_t py = (tile / fp.ntx) * kTile + (lane >> 3);
    const int pcx = (int)(lane & 7u) * 256 + 128, pcy = (int)(lane >> 3) * 256 + 128;

    float depth = 1.0f;
    uint32_t owner = kNoPrim;
    uint32_t lo = 0, hi = 0;
    if (range) {
        lo = range[2 * tile];
        hi = range[2 * tile + 1];
    }
    lo = __builtin_amdgcn_readfirstlane(lo);
    hi = __builtin_amdgcn_readfirstlane(hi);
    for (uint32_t chunk = lo; chunk < hi; chunk += 64) {
        const uint32_t cn = hi - chunk < 64u ? hi - chunk : 64u;
        const uint32_t my = lane < cn ? vals[chunk + lane] : 0u;
        for (uint32_t j = 0; j < cn; ++j) {
            const uint32_t slot = __builtin_amdgcn_readlane(my, j);
            const setup_rec& r = recs[slot];
            const int ext = imax(imax(iabs(r.x1 - r.x0), iabs(r.x2 - r.x0)), iabs(r.x2 - r.x1)) |
                            imax(imax(iabs(r.y1 - r.y0), iabs(r.y2 - r.y0)), iabs(r.y2 - r.y1));
            if (ext < 16384) guide_record<int>(r, slot, tox, toy, pcx, pcy, depth, owner);
            else guide_record<long long>(r, slot, tox, toy, pcx, pcy, depth, owner);
        }
    }

    if (px >= fp.width || py >= fp.height) return;
    const size_t pix = (size_t)py * fp.width + px;
    float4 out = make_float4(0.0f, 0.0f, 0.0f, depth);
    uint32_t draw = kNoPrim;
    if (owner != kNoPrim) {
        const setup_rec& r = recs[owner];
        const int x0 = r.x0 - tox, y0 = r.y0 - toy, x1 = r.x1 - tox, y1 = r.y1 - toy, x2 = r.x2 - tox, y2 = r.y2 - toy;
        const long long e0c = (long long)(x2 - x1) * (pcy - y1) - (long long)(y2 - y1) * (pcx - x1);
        const long long e1c = (long long)(x0 - x2) * (pcy - y2) - (long long)(y0 - y2) * (pcx - x2);
        const long long e2c = (long long)(x1 - x0) * (pcy - y0) - (long long)(y1 - y0) * (pcx - x0);
        const long long area = (long long)(x1 - x0) * (y2 - y0) - (long long)(x2 - x0) * (y1 - y0);
        const float farea = (float)area;
        // step 8's normal at the pixel centre, then iq::normalized3
        const float p0 = (float)e0c / farea * r.rw0, p1 = (float)e1c / farea * r.rw1, p2 = (float)e2c / farea * r.rw2;
        const float sum = p0 + p1 + p2;
        const float nx = (p0 * r.n0[0] + p1 * r.n1[0] + p2 * r.n2[0]) / sum;
        const float ny = (p0 * r.n0[1] + p1 * r.n1[1] + p2 * r.n2[1]) / sum;
        const float nz = (p0 * r.n0[2] + p1 * r.n1[2] + p2 * r.n2[2]) / sum;
        const float eps = 0.00001f;
        if (!(fabsf(nx) < eps && fabsf(ny) < eps && fabsf(nz) < eps)) {
            const float inv = 1.0f / sqrtf(nx * nx + ny * ny + nz * nz);
            out.x = nx * inv; out.y = ny * inv; out.z = nz * inv;
        }
        draw = r.pad[0];
    }
    normal_z[pix] = out;
    id[pix] = draw;
}

inline uint32_t blocks(uint32_t n) { return (n + kBlock - 1) / kBlock; }

}  // namespace

hipError_t launch_vertex(hipStream_t s, const draw_rec* draws, uint32_t ndraws, const uint32_t* draw_vend,
                         uint32_t nverts, const float* mesh_verts, const float* view, const float* proj,
                         float* clip, float* wn) {
    if (!nverts) return hipSuccess;
    iqr_vertex_kernel<<<blocks(nverts), kBlock, 0, s>>>(draws, ndraws, draw_vend, nverts, mesh_verts, view, proj, clip, wn);
    return hipGetLastError();
}

hipError_t launch_setup(hipStream_t s, const frame_params& fp, const draw_rec* draws, uint32_t ndraws,
                        const uint32_t* draw_tend, uint32_t ntris, const uint32_t* indices, const float* clip,
                        const float* wn, setup_rec* recs, uint32_t rec_cap, counters* cnt) {
    if (!ntris) return hipSuccess;
    iqr_setup_kernel<false><<<blocks(ntris), kBlock, 0, s>>>(fp, draws, ndraws, draw_tend, ntris, indices, clip, wn, recs,
                                                             rec_cap, cnt);
    return hipGetLastError();
}

hipError_t launch_setup_guide(hipStream_t s, const frame_params& fp, const draw_rec* draws, uint32_t ndraws,
                              const uint32_t* draw_tend, uint32_t ntris, const uint32_t* indices, const float* clip,
                              const float* wn, setup_rec* recs, uint32_t rec_cap, counters* cnt) {
    if (!ntris) return hipSuccess;
    iqr_setup_kernel<true><<<blocks(2 * ntris), kBlock, 0, s>>>(fp, draws, ndraws, draw_tend, ntris, indices, clip, wn,
                                                                recs, rec_cap, cnt);
    return hipGetLastError();
}

hipError_t launch_guide_tiles(hipStream_t s, const frame_params& fp, const setup_rec* recs, const uint32_t* vals,
                              const uint32_t* range, void* normal_z, uint32_t* id) {
    iqr_guide_tile_kernel<<<fp.ntx * fp.nty, 64, 0, s>>>(fp, recs, vals, range, static_cast<float4*>(normal_z), id);
    return hipGetLastError();
}

hipError_t launch_bin(hipStream_t s, const frame_params& fp, const setup_rec* recs, uint32_t nrec, unsigned key_bits,
                      unsigned long long* keys, uint32_t* vals) {
    if (!nrec) return hipSuccess;
    iqr_bin_kernel<<<blocks(nrec), kBlock, 0, s>>>(fp, recs, nrec, key_bits, keys, vals);
    return hipGetLastError();
}

hipError_t launch_ranges(hipStream_t s, const frame_params& fp, const unsigned long long* keys, uint32_t npairs,
                         unsigned key_bits, uint32_t* range) {
    const hipError_t e = hipMemsetAsync(range, 0, (size_t)fp.ntx * fp.nty * 2 * sizeof(uint32_t), s);
    if (e != hipSuccess || !npairs) return e;
    iqr_range_kernel<<<blocks(npairs), kBlock, 0, s>>>(keys, npairs, key_bits, range);
    return hipGetLastError();
}

hipError_t sort_pairs(hipStream_t s, void* temp, size_t& temp_bytes, const unsigned long long* keys_in,
                      unsigned long long* keys_out, const uint32_t* vals_in, uint32_t* vals_out, uint32_t n,
                      unsigned end_bit) {
    return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0u, end_bit, s);
}

hipError_t launch_tiles(hipStream_t s, const frame_params& fp, const setup_rec* recs, const uint32_t* vals,
                        const uint32_t* range, uint32_t* frame, float* depth_samples, uint32_t* prim_samples) {
    const uint32_t ntiles = fp.ntx * fp.nty;
    if (fp.samples == 1)
        iqr_tile_kernel<1><<<ntiles, 64, 0, s>>>(fp, recs, vals, range, frame, depth_samples, prim_samples);
    else
        iqr_tile_kernel<4><<<ntiles, 64, 0, s>>>(fp, recs, vals, range, frame, depth_samples, prim_samples);
    return hipGetLastError();
}

}  // namespace iqr
