// iq_ctx.hpp — private to the runtime sources (iqpt_runtime.cpp, runtime/*.cpp): the render context behind
// include/iqpt.h, the runtime's constants and the helpers more than one of those sources needs. Host only: no kernel
// includes it, so it is no part of the kernels' identity (_build.kernel_source_sha16).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "iqpt.h"
#include "iqpt_internal.hpp"
#include "post/iq_post.hpp"   // IQPT_HIP, hip_fail

namespace iqpt {

// LDS budget under which the whole scene stays resident per block (no barriers in the loop).
constexpr uint32_t kLdsResidentBytes = 32 * 1024;
// Batch sizes when the scene is streamed through LDS (pairs: 10 KB + 4 KB; with the table, mask
// slots and scatter stack a block stays under 32 KB, so 5 blocks fit a CU).
constexpr uint32_t kTriBatch = 256;   // primitives per LDS batch (128 pairs = 10 KB)
constexpr uint32_t kSphBatch = 256;
// kOptBvhPrimary launches leave the batch region unused and park 13 words of path state per thread there
static_assert((kTriBatch / 2) * kTriPairFloat4 * 16 + (kSphBatch / 2) * kSphPairFloat4 * 16 >= 13 * kRenderBlock * 4,
              "the BVH-primary path-state slots must fit the scene-batch region");
constexpr int kTuneLaunches = 4;     // timed launches before the camera-ray path is chosen (A, B, A, B)
// kOptSplit auto mode: split when the owned pixels are fewer than this many per resident lane
constexpr double kSplitAutoPixelsPerLane = 1.2;
// spec launches: AUTO takes them below this many owned pixels per resident lane of the
// plain kernel (C3 shares: N = 8 has 0.8, N = 4 1.6, N = 2 3.2; pipelined spec launches 0.27 / 0.47 / 0.87 ms
// per step through the gather against plain 0.95 / 1.0 / 0.91; N = 1, 6.3, stays plain; profiles/r03/
// split_share_run37.json, r03_share_v11.json, run49_share{2,4,8}_2.json)
constexpr double kSpecAutoPixelsPerLane = 4.0;
constexpr size_t kSplitResBudget = size_t(8) << 30;   // speculative results (bytes)
constexpr uint32_t kSplitRefillMin = 16;   // idle lanes before a refill in split launches
constexpr bool kSplitAllTiles = false;     // every tile in the split set (wall tiles: one slot per sample)
constexpr double kSpecPlanCap = 0.97;      // a spec plan's lanes: this fraction of the resident lanes

}  // namespace iqpt

using iqpt::float4_storage;

struct iqpt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t width = 0, height = 0;
    iqpt_pixel_set set{};
    uint32_t ncols = 0, npix = 0;
    uint64_t seed = 0;
    int max_depth = 0;
    uint64_t frame = 0;
    int num_cus = 0;
    int num_xcc = 0;              // XCDs of the device (overlapped launches bind tiles to the 8 XCDs)
    uint32_t lds_per_block = 0;   // the device's LDS limit per workgroup (bytes)
    int opt = iqpt::kOptDefault;
    bool have_camera = false, have_packet = false;
    iqpt_camera cam{};
    // pixel state (compact over the owned set)
    float4_storage* d_lin = nullptr;
    uint32_t* d_bgra = nullptr;
    uint32_t* d_rng = nullptr;
    unsigned long long* d_rays = nullptr;
    uint32_t* d_queue = nullptr;
    unsigned long long* d_stats = nullptr;   // kOptStats counters (diagnostic variants)
    // scene (world space)
    float4_storage* d_tris = nullptr;
    float4_storage* d_tri_pairs = nullptr;
    float4_storage* d_tri_shade = nullptr;
    float4_storage* d_sph = nullptr;
    float4_storage* d_sph_pairs = nullptr;
    uint32_t ntri = 0, nsph = 0;
    std::vector<float4_storage> h_sph;   // world-space spheres (host copy: per-pixel sphere bundles, build_split)
    // material table (§8f.3), null without one
    uint32_t* d_tri_mat = nullptr;
    uint32_t* d_sph_mat = nullptr;
    float4_storage* d_mats = nullptr;
    // exact BVH for secondary rays (iq_bvh.hpp), null when the packet has few triangles
    float4_storage* d_bvh_nodes = nullptr;
    float4_storage* d_bvh_pairs = nullptr;
    uint32_t* d_bvh_always = nullptr;
    uint32_t bvh_nnodes = 0, bvh_nalways = 0;
    float bvh_md = 0.0f, bvh_gulp = 0.0f;
    // exact sphere BVH (iq_bvh.hpp), null when the packet has few spheres
    float4_storage* d_sbvh_nodes = nullptr;
    float4_storage* d_sbvh_sph = nullptr;
    uint32_t* d_sbvh_idx = nullptr;
    uint32_t* d_sbvh_always = nullptr;
    uint32_t sbvh_nnodes = 0, sbvh_nalways = 0;
    float sbvh_gulp = 0.0f;
    bool fast_rcp_ok = true;   // packet within the range of the kOptFastDiv reciprocals (upload)
    // kOptCull tile masks (iq_interval.h), rebuilt on the stream after a camera or packet change
    uint32_t* d_cull = nullptr;
    uint32_t* d_certain = nullptr;      // per tile: 64-bit mask of pixels certain to end on an emissive triangle
    bool certain_valid = false;         // d_certain holds the current masks' flags (no material table)
    bool certain_on = true;             // iqpt_debug_set_certain (A/B: 0 renders certain tiles normally)
    // certain-miss pixels: the tiles holding some (d_certain + 2 ntiles has their masks), the
    // pixel count; plain launches hand them to iqpt_sky_kernel (iqpt_debug_set_sky: 0 traces them as before)
    uint32_t* d_sky_tiles = nullptr;
    uint32_t n_sky_tiles = 0, n_sky_pixels = 0;
    bool sky_on = true;
    bool sky_active = false;            // the masks' miss pixels are the sky kernel's: the fan lists exclude them
    std::vector<uint64_t> h_miss;       // per tile: the certain-miss mask (host copy, for the fan lists)
    hipEvent_t ev_sky = nullptr;        // after the last sky kernel (the next one, maybe on the other stream, waits)
    hipStream_t sky_last = nullptr;     // the stream of the last sky kernel since the streams were joined
    uint32_t* d_tile_order = nullptr;   // work-queue order over tiles, built with the masks
    uint32_t* d_list = nullptr;         // candidate lists of the masks, then their offsets (tri, sph)
    uint64_t list_total = 0;
    uint32_t* d_pmask = nullptr;        // per-tile word offsets (ntiles + 1), the per-pixel candidate masks (kparams::pmask),
                                        // then 2 words per tile of certain pixels (kparams::pmask_certain)
    int pmask_mode = 2;                 // iqpt_debug_set_pixel_masks: 0 none, 1 in the plain kernel, 2 + iqpt_anyhit_kernel
    uint32_t pmask_tiles = 0;           // tiles with masks (a triangle list of 1 .. kPixMaskMax entries)
    uint64_t pmask_words = 0;           // mask words after the offsets
    bool pmask_all = false;             // every list within kAnyMaxEntries and no tile with a sphere candidate
    uint32_t list_max = 0;              // the longest triangle list
    bool last_anyk = false;             // the last launch ran iqpt_anyhit_kernel
    size_t cull_cap = 0;       // words allocated
    bool cull_valid = false;
    uint32_t cull_ntx = 0, cull_nty = 0, cull_wt = 0, cull_stride = 0;
    // timing
    // e1b: the second stream's end (pipelined spec), or null (hidden, and so the templates instantiated over it)
    struct __attribute__((visibility("hidden"))) timed_launch { hipEvent_t e0, e1, e1b; };
    std::vector<timed_launch> timed;
    std::vector<hipEvent_t> event_pool;
    // camera rays of a streamed scene with a BVH: tile masks or the BVH (kOptBvhPrimary), whichever
    // the first two launches after a packet upload time faster per sample (results are identical);
    // tools/ab_kernel.py fixes the option set instead (opt_fixed)
    bool opt_fixed = false;
    // stages 0..kTuneLaunches-1 time masks (even) and the BVH (odd) alternately; stage kTuneLaunches
    // decides on the fastest launch of each; reset by a packet upload or a camera change
    int tune_stage = 0;
    bool tune_primary = false;
    hipEvent_t tune_ev[2 * 4] = {};
    int last_opt = -1;           // option set of the last render launch (iqpt_debug_last_options)
    // the kernels of the last render launch (iqpt_debug_last_launch): maxd, streamed, the plain or spec kernel's
    // option set, then the rows of the sky, fan, spec, any-hit and split-stitch tables it launched (-1: not
    // launched). cur_launch is the launch being enqueued (note_kernel); it becomes last_launch where last_opt is set
    int32_t last_launch[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    int32_t cur_launch[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    bool last_xcd_lists = false; // the last launch dealt its tiles to per-XCD lists (overlapped or streamed)
    // kOptSplit, sample-parallel chains: mode (IQPT_SPLIT_*), the split set built with
    // the masks (tiles whose camera rays may scatter), per-slot buffers sized for the launch
    int split_mode = IQPT_SPLIT_AUTO;
    bool split_last = false;     // the last launch ran split
    uint32_t n_split_tiles = 0, n_anchor = 0;
    uint32_t* d_split = nullptr;        // anchor_order[n_anchor], split_tiles[nst], sp_pix, sp_win, sp_rho,
                                        // left (ns_cap each)
    uint32_t* d_sp_st = nullptr;        // 6 x ns_cap
    uint32_t* d_run_st = nullptr;       // (g_max + 1) x 6 x ns_cap
    uint32_t* d_chunks = nullptr;       // 2 x g_max x split tiles: round-1 run chunks
    float4_storage* d_sp_acc = nullptr; // ns_cap
    float4_storage* d_res = nullptr;    // m_cap x ns_cap
    uint8_t* d_nres = nullptr;          // ns_cap x m_cap
    // idle lanes before a wave's refill (split launches: kSplitRefillMin)
    uint32_t stream_refill_min = 64;    // ... in streamed launches: whole waves (iqpt_debug_set_stream_refill)
    uint32_t resident_refill_min = 1;   // ... in resident plain launches (iqpt_debug_set_resident_refill)
    bool fan_last = false;              // the last launch ran the anchored tiles in iqpt_fan_kernel
    // spec launches with the fan kernel: the pixels of split tiles whose own camera-ray
    // bundle may reach a sphere (the spec kernel's pixel list, "chain pixels"), and the fan kernel's tiles with
    // the lanes it owns (anchored tiles whole; split tiles without their sphere pixels)
    uint32_t* d_chain_pix = nullptr;
    uint32_t n_chain_pix = 0;
    uint32_t* d_fan_tiles = nullptr;
    uint64_t* d_fan_lanes = nullptr;
    uint32_t n_fan_tiles = 0;
    // spec launches: per sphere pixel (d_chain_pix) the last window, the chain's slots per
    // sample (history, zeroed when the pixel list changes), the slot colours; sized for (spec_n, spec_mcap)
    uint32_t* d_spec = nullptr;         // m, rho (spec_n each), run_count (2)
    float4_storage* d_spec_res = nullptr;
    uint32_t spec_n = 0, spec_mcap = 0;
    bool spec_rho_valid = false;
    bool spec_last = false;
    uint32_t spec_rho0 = iqpt::kSpecRho0;   // window of a pixel without history (iqpt_debug_set_spec)
    uint32_t spec_parity_rho = iqpt::kSpecParityRho;   // parity pixels' threshold (iqpt_debug_set_spec_parity; 0 off)
    uint32_t spec_parity_hi = iqpt::kSpecParityHi;     // ... and upper bound
    bool anyhit_on = true;                  // any-hit queries in triangle-only scenes (iqpt_debug_set_anyhit)
    bool pipe_on = true;                    // two rays per lane in resident plain launches (kOptPipe, iqpt_debug_set_two_ray)
    uint32_t spec_margin_div = 16;          // window margin: 1/16 of the extra slots, at least 4 (iqpt_debug_set_spec;
                                            // against 1/4, 5 % of the chains take a second round instead of 0.6 %,
                                            // yet -4 % per launch at N = 2 / 4 / 8, profiles/r03/spec_margins.json)
    // spec launches (iqpt_debug_set_specfan): 0 the two kernels on two streams, pipelined (the default), 1 one
    // after the other on one stream (measurement)
    int specfan_mode = 0;
    // spec plan: the sphere pixels ordered by their last chain's work, heaviest first, the
    // heavy ones with 32 or 64 lanes; built on the host from an asynchronous read of the history (performance
    // only: every plan gives the same bits). iqpt_debug_spec_plan: 0 off, 1 asynchronous (default), 2..5
    // synchronous before every launch (tests; 3, 4: every pixel 32 / 64 lanes, 5: mixed)
    int spec_plan_mode = 1;
    uint32_t* h_spec_rho = nullptr;      // pinned: the history read back (spec_n)
    uint32_t* h_spec_plan = nullptr;     // pinned: staging of the plan (3 spec_n)
    hipEvent_t ev_spec_rho = nullptr, ev_spec_plan = nullptr;
    bool spec_rho_pending = false;       // a history read in flight
    bool spec_plan_up = false;           // a plan upload was enqueued (ev_spec_plan)
    uint32_t* d_spec_plan = nullptr;     // order (spec_n words), then 2 words per block
    uint32_t spec_plan_n = 0;            // pixels of the plan (0: none; must equal n_chain_pix to be used)
    uint32_t spec_plan_blocks = 0;
    uint32_t spec_plan_age = 0;          // launches since the plan was built
    // Pipelined spec and fan launches: the spec kernel (or, FAN, the plain kernel over the
    // split tiles) on `stream`, the fan kernel on `stream2`, and no join at the end of a launch — launch
    // k + 1's pixels on `stream` follow launch k's there, its fan pixels launch k's on `stream2` (the two sets
    // are disjoint and the same for launches of one kind), so the fan stream runs ahead into the other's tail. Every other entry point joins (join_streams). Frame copies (iqpt_copy_frame_device_async)
    // go on `stream3` behind both kernels; from the first such copy on, launches write the two frame buffers
    // in turn and a launch waits only for the copy that read its buffer two launches earlier.
    bool pipe = false;                   // the last launch was pipelined and nothing has joined since
    int pipe_kind = 0;                   // ... a spec launch (1)
    hipStream_t stream3 = nullptr;
    hipEvent_t ev_pipe_end = nullptr;    // on `stream`, recorded by a copy behind a pipelined launch
    // the events the last pipelined launch's kernels recorded at their ends on `stream` / `stream2` (timing
    // events bound to the dispatches), or null: a copy behind the launch waits for them instead of recording
    // markers of its own
    hipEvent_t end1 = nullptr, end2 = nullptr;
    // copies behind pipelined launches (iqpt_copy_frame_device_async, the gather's send copy): from the first
    // one on, pipelined launches write a ring of kPipeRing frame buffers in turn (d_bgra points at the one
    // the last launch wrote). Copy s (1-based, copy_seq counts them) records pev[s % kPipeRing] on stream3
    // after reading its launch's buffer; pseq[b] is the last copy that read ring buffer b. A launch about
    // to write buffer b that a copy newer than pwaited read makes both render streams wait for copy
    // copy_seq - 2 (three launches back when every launch is copied: a copy still in flight is not waited
    // for), which stream3's order makes cover every buffer copied up to it: one wait per kPipeRing - 2
    // launches instead of one per launch (each wait is a packet on both streams between two kernels:
    // r04 run 21, 0.015-0.02 ms per share-8 step)
    uint32_t* d_pring[iqpt::kPipeRing] = {};
    hipEvent_t pev[iqpt::kPipeRing] = {};
    uint64_t pseq[iqpt::kPipeRing] = {};
    uint64_t copy_seq = 0, pwaited = 0;
    int pidx = 0;
    bool pring_on = false;
    uint32_t* d_bgra_own = nullptr;     // the allocations behind d_bgra / d_bgra_alt (views that swap)
    uint32_t* d_alt_own = nullptr;
    unsigned long long* d_spec_tl = nullptr;   // iqpt_debug_spec_timeline: per spec block timestamps
    size_t spec_tl_blocks = 0;
    bool spec_tl_on = false;
    size_t res_slots = 0;               // m_cap x ns_cap allocated (res, nres)
    double tune_work[4] = {0.0, 0.0, 0.0, 0.0};
    // kOptOverlap: consecutive render launches alternate between `stream` and
    // `stream2`, so launch k + 1 fills the CUs that launch k's tail leaves idle; it takes a tile only
    // when launch k has finished it (tile_done). Every other entry point joins the streams first.
    int overlap_mode = IQPT_OVERLAP_AUTO;
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_pre = nullptr;        // on `stream`, before its last overlapped launch
    hipEvent_t ev_s2 = nullptr;         // on `stream2`, after its last launch (join)
    bool s2_pending = false;            // stream2 has work `stream` has not waited for
    bool next_on_main = true;           // the next overlapped launch goes to `stream`
    bool ovl_zero = true;               // tile_done must be zeroed before the next overlapped launch
    uint32_t ovl_epoch = 0;             // overlapped launches since tile_done was zeroed
    uint32_t* d_tile_done = nullptr;    // ntiles
    uint32_t* d_xcd_order = nullptr;    // ntiles: XCD x's tiles at [xcd_off[x], xcd_off[x + 1])
    uint32_t xcd_off[9] = {};
    // streamed scenes (iqpt_debug_set_stream_xcd): 0 one queue over the cost order; 1 the per-XCD lists above
    // (a queue word per XCD: C5 -9 % at 1 spp per launch, where tiles are short and the one queue word is
    // contended; +0.2..1.4 % at 16 spp and C4 +4 % at 256, where the fixed lists end unevenly, r05 runs 38-39);
    // 2 per-XCD bands of kXcdBandRows tile rows dealt round-robin (each XCD's L2 sees a band at a time: +17 % at
    // 16 spp, the bands are not in cost order); 3 (default) 1 up to kStreamXcdMaxSpp samples per launch, else 0
    int stream_xcd = 3;
    uint32_t* d_xcd_band = nullptr;     // ntiles: XCD x's bands at [xcd_band_off[x], xcd_band_off[x + 1])
    uint32_t xcd_band_off[9] = {};
    uint32_t* d_ovl_err = nullptr;
    // stream-ordered frame copies across overlapped launches (iqpt_copy_frame_device_async): once the
    // first such copy is asked for, each overlapped launch writes the BGRA frame into the buffer the
    // previous launch did not (d_bgra is always the last written, d_bgra_alt the other), so launch k's
    // copy, queued on launch k's stream, reads a frame launch k + 1 never touches, and launch k + 2
    // (the same stream) writes it only after that copy
    uint32_t* d_bgra_alt = nullptr;
    hipStream_t last_ls = nullptr;      // the stream of the last render launch
    bool last_ovl = false;              // ... which was overlapped, and no call has joined the streams since
    double last_span_ms = 0.0;          // iqpt_kernel_time: first start to last end of the timed launches
    // forward-progress bound of the kernels (iqpt_debug_set_limits lowers it in tests) and a bias added
    // to the per-tile wait targets of overlapped launches (tests: a wait that can never be satisfied)
    uint32_t spin_limit = iqpt::kOverlapSpinLimit, wait_bias = 0;
    // the kernels' error word, latched at the first synchronising call that sees it: after a wait that
    // gave up or a chain wave past its bound the pixel state is undefined, so every later call that
    // returns or persists pixel state fails until iqpt_checkpoint_load replaces the whole state
    uint32_t dev_err = 0;
    // multi-GPU frame delivery (iqpt_comm_init): an RCCL communicator over the ranks of one
    // frame's cyclic row split and its own stream. A gather copies the rank's pixels (compact order, padded
    // to comm_stride pixels) into one of kSendRing send buffers in turn — the copy of gather g waits only for
    // gather g - kSendRing — then ncclGather to the root, which assembles the frame from the rank blocks.
    void* comm = nullptr;                // ncclComm_t
    int comm_rank = 0, comm_world = 0;
    uint64_t comm_stride = 0;            // pixels per rank block: the most rows any rank owns x W
    hipStream_t cstream = nullptr;
    // send buffers in turn (the copy of gather g waits for gather g - kSendRing, long done: with two, a
    // gather slowed by the renders beside it held the next copies and, through them, the render streams)
    uint32_t* d_gsend[iqpt::kSendRing] = {};     // comm_stride x 4 words each
    hipEvent_t ev_gdone[iqpt::kSendRing] = {};   // on cstream, after the gather that read d_gsend[i]
    bool gdone_pend[iqpt::kSendRing] = {};
    uint32_t gpar = 0;                   // the send buffer of the next gather
    hipEvent_t ev_gcopy = nullptr;       // after the copy into the send buffer (cstream waits for it)
    hipEvent_t ev_gend = nullptr;        // on cstream, after the last gather (every other entry point joins it)
    bool comm_pend = false;
    uint32_t* d_grecv = nullptr;         // root: comm_world x comm_stride x 4 words
    uint32_t* d_gframe = nullptr;        // root: the assembled W x H x 4 words of iqpt_gather_read
    std::vector<std::pair<hipEvent_t, hipEvent_t>> gtimed;   // per gather: cstream events around it (iqpt_comm_time)
    // the gather's share of the CUs it runs beside (iqpt_debug_set_gather, before iqpt_comm_init): RCCL's
    // blocks per collective (ncclConfig_t::maxCTAs; 0: RCCL's choice) and cstream's priority (-1 lowest,
    // 0 the default, 1 highest)
    int gather_ctas = iqpt::kGatherCtas;
    int gather_prio = 0;
    int gather_skip = 0;                 // measurement only: 1 skips the collective, 2 the root's assembly,
                                         // 4 the render streams' waits for the frame copies
    bool timing_on = true;               // the launches' timing events (iqpt_debug_set_timing)
    bool sky_after = true;               // overlapped launches: the sky kernel behind the plain kernel (r04 run 35:
                                         // 0.988-0.992 -> 0.975-0.982 ms per C2 step)
};

// Helpers that more than one runtime source calls. Hidden: the library's dynamic symbol table is the C ABI and the
// kernels' launchers, not these.
#define IQPT_RT_LOCAL __attribute__((visibility("hidden")))

namespace iqpt::rt {
// hipFree / hipEventDestroy of what is there; the handle is null afterwards
template <typename T>
IQPT_RT_LOCAL inline void dev_free(T*& p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}
IQPT_RT_LOCAL inline void event_free(hipEvent_t& e) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
}

// iqpt_runtime.cpp
IQPT_RT_LOCAL int use_device(const iqpt_ctx* c);
IQPT_RT_LOCAL int join_streams(iqpt_ctx* c);
IQPT_RT_LOCAL int ensure_copy_stream(iqpt_ctx* c);
IQPT_RT_LOCAL int enter(iqpt_ctx* c);
IQPT_RT_LOCAL int fetch_compact(iqpt_ctx* c, const void* dev, uint32_t words, uint32_t planes, void* host);
IQPT_RT_LOCAL int store_compact(iqpt_ctx* c, const void* host, uint32_t words, uint32_t planes, void* dev);
IQPT_RT_LOCAL int read_rays(iqpt_ctx* c, unsigned long long* total);
IQPT_RT_LOCAL int check_dev_err(iqpt_ctx* c);
IQPT_RT_LOCAL hipEvent_t take_event(iqpt_ctx* c);
// runtime/iq_cull.cpp
IQPT_RT_LOCAL void free_split(iqpt_ctx* c);
IQPT_RT_LOCAL int build_cull(iqpt_ctx* c);
IQPT_RT_LOCAL void cam_constants(const iqpt_camera& cam, uint32_t* is_const, float* near_rw, float* far_rw);
IQPT_RT_LOCAL bool cam_axis_constants(const iqpt_camera& cam, float* k);
IQPT_RT_LOCAL void free_comm(iqpt_ctx* c);   // runtime/iq_comm.cpp
}  // namespace iqpt::rt

// iqpt_runtime.cpp, for the gather's send copy. Under plain names: functions of an unnamed namespace inside
// extern "C" kept theirs in the dynamic symbol table, which tests/test_exports.py pins (these, render_launch, fnv1a,
// comm_check, gather_*). Hiding them and dropping them from the fixture is a change of its own.
extern "C" {
int ensure_ring(iqpt_ctx* c);
int copy_frame_async(iqpt_ctx* c, uint32_t* dst, hipEvent_t wait, hipStream_t* used);
}
