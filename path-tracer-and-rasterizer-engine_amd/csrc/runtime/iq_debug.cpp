// iq_debug.cpp — the iqpt_debug_* entry points (tests and tools; not part of include/iqpt.h).
#include "iq_bvh.hpp"
#include "iq_interval.h"
#include "runtime/iq_ctx.hpp"

using namespace iqpt::rt;

extern "C" {

/* Internal (tools): the per-pixel split of the last camera / packet — sphere pixels (the chain and spec
 * kernels' list), fan tiles, anchored tiles, split tiles — and, after a spec launch, the sum of its
 * windows and of its chains' slots per sample, and since the last call (the call clears them) the chains
 * finished past their window (out8[7] low 32 bits) and the parity chains that needed the fix-up pass (out8[7]
 * high 32 bits). Synchronises. */
int iqpt_debug_spec_info(iqpt_ctx* c, unsigned long long* out8) {
    if (!c || !out8) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    int st = enter(c);
    if (st) return st;
    IQPT_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    out8[0] = c->n_chain_pix;
    out8[1] = c->n_fan_tiles;
    out8[2] = c->n_anchor;
    out8[3] = c->n_split_tiles;
    if (c->spec_last && c->d_spec && c->spec_n >= c->n_chain_pix) {
        const uint32_t n = c->n_chain_pix;
        std::vector<uint32_t> v(2 * (size_t)n + 2);
        IQPT_HIP(hipMemcpy(v.data(), c->d_spec, v.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        out8[4] = c->spec_plan_n == n && c->spec_plan_mode ? c->spec_plan_blocks : 0;   // plan blocks (0: none)
        out8[7] = (unsigned long long)v[2 * (size_t)n + 1] | ((unsigned long long)v[2 * (size_t)n] << 32);
        unsigned long long m = 0, rho = 0;
        for (uint32_t q = 0; q < n; ++q) {
            m += v[q];
            rho += v[n + q];
        }
        out8[5] = m;
        out8[6] = rho;
        IQPT_HIP(hipMemset(c->d_spec + 2 * (size_t)n, 0, 2 * sizeof(uint32_t)));
    }
    return IQPT_OK;
}

/* Internal (measurement): record per spec block s_memrealtime stamps (100 MHz) in later spec launches —
 * start, after round 0's slots, after round 0's walk, end | rounds << 48, then the slot-loop iterations of
 * its four waves (8 words per block) — and read the last launch's. */
int iqpt_debug_spec_timeline(iqpt_ctx* c, int on) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    c->spec_tl_on = on != 0;
    return IQPT_OK;
}

int iqpt_debug_read_spec_timeline(iqpt_ctx* c, unsigned long long* out, uint32_t cap_blocks, uint32_t* n) {
    if (!c || !out || !n) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    *n = 0;
    int st = enter(c);
    if (st) return st;
    IQPT_HIP(hipStreamSynchronize(c->stream));
    if (!c->d_spec_tl || !c->spec_last) return IQPT_OK;
    const size_t nspec = c->spec_plan_n == c->n_chain_pix && c->spec_plan_n && c->spec_plan_mode
                             ? c->spec_plan_blocks
                             : (c->n_chain_pix + iqpt::kSpecPixPerBlock - 1) / iqpt::kSpecPixPerBlock;
    const size_t nb = std::min<size_t>(nspec, std::min<size_t>(cap_blocks, c->spec_tl_blocks));
    if (nb) IQPT_HIP(hipMemcpy(out, c->d_spec_tl, nb * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    *n = (uint32_t)nb;
    return IQPT_OK;
}

/* Internal (measurement): the spec plan in use and the history behind it — order (n words), blocks (2 words
 * each, *nb of them) and the sphere pixels' slots per sample x 256 (n words); *n = sphere pixels (0: no plan).
 * Synchronises. */
int iqpt_debug_read_spec_plan(iqpt_ctx* c, uint32_t* order, uint32_t* blocks, uint32_t* rho, uint32_t cap,
                              uint32_t* n, uint32_t* nb) {
    if (!c || !order || !blocks || !rho || !n || !nb) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    *n = *nb = 0;
    int st = enter(c);
    if (st) return st;
    IQPT_HIP(hipStreamSynchronize(c->stream));
    const uint32_t np = c->n_chain_pix;
    if (!c->spec_plan_n || c->spec_plan_n != np || np > cap || !c->d_spec_plan) return IQPT_OK;
    IQPT_HIP(hipMemcpy(order, c->d_spec_plan, (size_t)np * sizeof(uint32_t), hipMemcpyDeviceToHost));
    IQPT_HIP(hipMemcpy(blocks, c->d_spec_plan + np, 2 * (size_t)c->spec_plan_blocks * sizeof(uint32_t),
                       hipMemcpyDeviceToHost));
    IQPT_HIP(hipMemcpy(rho, c->d_spec + np, (size_t)np * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *n = np;
    *nb = c->spec_plan_blocks;
    return IQPT_OK;
}

/* Internal (tests, A/B): the spec plan — 0 none (16 lanes per pixel, list order), 1 from an asynchronous
 * read of the history (the default), 2 rebuilt synchronously before every launch, 3 / 4 the same with
 * every pixel on 32 / 64 lanes, 5 the same with the lane count cycling over 8, 16, 24, 32, 48, 64. Drops the plan. */
int iqpt_debug_spec_plan(iqpt_ctx* c, int mode) {
    if (!c || mode < 0 || mode > 5) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL or mode not 0..5");
    c->spec_plan_mode = mode;
    c->spec_plan_n = 0;
    return IQPT_OK;
}

/* Internal (A/B, tests): certain tiles (kparams::certain) folded at once (1, the default) or rendered like
 * every other tile (0). Rebuilds the masks at the next launch. */
int iqpt_debug_set_certain(iqpt_ctx* c, int on) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    int st = enter(c);
    if (st) return st;
    c->certain_on = on != 0;
    c->cull_valid = false;
    return IQPT_OK;
}

/* Internal (A/B, tests): certain-miss pixels rendered by iqpt_sky_kernel beside plain launches (1, the default)
 * or traced by the plain kernel like every other pixel (0). Rebuilds the masks at the next launch. */
int iqpt_debug_set_sky(iqpt_ctx* c, int on) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    int st = enter(c);
    if (st) return st;
    c->sky_on = on != 0;
    c->cull_valid = false;
    return IQPT_OK;
}

/* Internal (A/B): the gather's footprint beside the render kernels, for the next iqpt_comm_init — RCCL's
 * blocks per collective (ncclConfig_t::maxCTAs; 0: RCCL's own choice) and the communicator stream's priority
 * (-1 the lowest; 0 HIP's default, the default; 1 the highest); skip (measurement only, wrong frames): 1 leaves
 * out the collective, 2 the root's assembly, 4 the render streams' waits for the copies of their frame buffers. */
int iqpt_debug_set_gather(iqpt_ctx* c, int ctas, int prio, int skip) {
    if (!c || ctas < 0 || ctas > 64 || prio < -1 || prio > 1 || skip < 0 || skip > 7)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL, ctas not 0..64, prio not -1..1 or skip not 0..7");
    c->gather_ctas = ctas;
    c->gather_prio = prio;
    c->gather_skip = skip;
    return IQPT_OK;
}

/* Internal (A/B): overlapped launches run the sky kernel ahead of the plain kernel on the launch's stream (0)
 * or behind it (1, the default). Same bits either way. */
int iqpt_debug_set_sky_order(iqpt_ctx* c, int after) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    c->sky_after = after != 0;
    return IQPT_OK;
}

/* Internal (A/B): the timing events around launches and gathers (iqpt_kernel_time, iqpt_comm_time) — 1 on (the
 * default), 0 off: those then report nothing. Each event is a packet on its stream between two kernels. */
int iqpt_debug_set_timing(iqpt_ctx* c, int on) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    c->timing_on = on != 0;
    return IQPT_OK;
}

/* Internal (tools): the certain-miss pixels of the current masks and the tiles holding them. */
int iqpt_debug_sky_info(iqpt_ctx* c, uint32_t* pixels, uint32_t* tiles) {
    if (!c || !pixels || !tiles) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    *pixels = c->certain_valid ? c->n_sky_pixels : 0u;
    *tiles = c->certain_valid ? c->n_sky_tiles : 0u;
    return IQPT_OK;
}

/* Internal (tools, tests): certain pixels of the current masks (*n; 0 without masks or flags), the tile
 * count and the tile grid's width in tiles (*ntx) and, if masks is not NULL, up to cap tiles' 64-bit
 * masks (two words per tile). Synchronises. */
int iqpt_debug_certain_tiles(iqpt_ctx* c, uint32_t* n, uint32_t* ntiles, uint32_t* ntx, uint32_t* masks, uint32_t cap) {
    if (!c || !n || !ntiles || !ntx) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    *ntx = c->cull_ntx;
    *n = *ntiles = 0;
    int st = enter(c);
    if (st) return st;
    if (!c->certain_valid || !c->d_certain) return IQPT_OK;
    const uint32_t nt = c->cull_ntx * c->cull_nty;
    std::vector<uint32_t> v(2 * (size_t)nt);
    // the folded hit masks: what the kernels fold (the tile rule's pixels and the beside-a-sphere ones)
    IQPT_HIP(hipMemcpy(v.data(), c->d_certain + 2 * (size_t)iqpt::kCertainFolded * nt, v.size() * sizeof(uint32_t),
                       hipMemcpyDeviceToHost));
    for (size_t i = 0; i < v.size(); ++i) *n += (uint32_t)__builtin_popcount(v[i]);
    *ntiles = nt;
    if (masks) std::memcpy(masks, v.data(), std::min<size_t>(v.size(), 2 * (size_t)cap) * sizeof(uint32_t));
    return IQPT_OK;
}

/* Internal (tests, A/B): any-hit queries for triangle-only scenes under the reference's materials (1, the
 * default) or the closest-hit search (0). Same bits either way. */
int iqpt_debug_set_anyhit(iqpt_ctx* c, int on) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    int st = enter(c);
    if (st) return st;
    c->anyhit_on = on != 0;
    c->cull_valid = false;               // the candidate lists' order follows the setting
    return IQPT_OK;
}

/* Internal (tests, A/B): per-pixel candidate masks over the streamed kernel's tile lists: 2 (the default) with
 * iqpt_anyhit_kernel for any-hit scenes whose every tile has them, 1 in the plain kernel only, 0 none (the whole
 * list for every lane). Same bits either way. */
int iqpt_debug_set_pixel_masks(iqpt_ctx* c, int on) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    int st = enter(c);
    if (st) return st;
    if (on < 0 || on > 2) return iqpt::fail(IQPT_ERR_INVALID_ARG, "pixel mask mode must be 0, 1 or 2");
    c->pmask_mode = on;
    c->cull_valid = false;
    return IQPT_OK;
}

/* Internal (tests, tools): tiles whose triangle lists have per-pixel masks (0: none built), whether every tile has
 * them and no tile has a sphere candidate (iqpt_anyhit_kernel's condition besides an any-hit scene), and the longest
 * triangle list (null: not wanted). */
int iqpt_debug_pixel_mask_info(iqpt_ctx* c, uint32_t* tiles, int* all, uint32_t* list_max) {
    if (!c || !tiles || !all) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    *tiles = c->pmask_tiles;
    *all = c->pmask_all ? 1 : 0;
    if (list_max) *list_max = c->list_max;
    return IQPT_OK;
}

/* Internal (tests, A/B): resident plain launches under the reference's materials trace the lane's path ray and
 * its pixel's next camera ray together (kOptPipe, 1, the default) or one ray per iteration (0). Same bits either
 * way. */
int iqpt_debug_set_two_ray(iqpt_ctx* c, int on) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    int st = enter(c);
    if (st) return st;
    c->pipe_on = on != 0;
    return IQPT_OK;
}

/* Internal (tests, A/B): idle lanes a wave of a streamed-scene launch waits for before it takes new pixels
 * (1..64; 1 = every iteration with an idle lane, round 4; 64, a whole tile at a time, by default). Same bits
 * either way. */
int iqpt_debug_set_stream_refill(iqpt_ctx* c, uint32_t lanes) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    if (lanes < 1u || lanes > 64u) return iqpt::fail(IQPT_ERR_INVALID_ARG, "lanes 1..64");
    c->stream_refill_min = lanes;
    return IQPT_OK;
}

/* Internal (tests, A/B): how streamed-scene launches deal tiles — 0 one queue over the cost order, 1 per-XCD
 * queues over the cost order dealt round-robin, 2 per-XCD queues over bands of tile rows dealt round-robin
 * (spatially coherent work per XCD L2), 3 (default) 1 for launches of up to 4 samples per pixel, else 0. Same
 * bits either way. */
int iqpt_debug_set_stream_xcd(iqpt_ctx* c, int mode) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    if (mode < 0 || mode > 3) return iqpt::fail(IQPT_ERR_INVALID_ARG, "mode 0..3");
    c->stream_xcd = mode;
    return IQPT_OK;
}

/* Internal (tests, A/B): the same for the plain kernel's launches over resident scenes (1 by default; split
 * launches keep their own, kSplitRefillMin). Same bits either way. */
int iqpt_debug_set_resident_refill(iqpt_ctx* c, uint32_t lanes) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    if (lanes < 1u || lanes > 64u) return iqpt::fail(IQPT_ERR_INVALID_ARG, "lanes 1..64");
    c->resident_refill_min = lanes;
    return IQPT_OK;
}

/* Internal (tests, A/B): the spec kernel's parity pixels — a pixel whose last chain took at least rho256 / 256
 * slots per sample traces the even slots of its window first and the odd ones only from where its chain lands on
 * one (pooled over the block's lanes); 0 traces every slot of every window (round 4). Same bits either way. */
int iqpt_debug_set_spec_parity(iqpt_ctx* c, uint32_t rho256) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    int st = enter(c);
    if (st) return st;
    c->spec_parity_rho = rho256;
    return IQPT_OK;
}

/* Internal (A/B, measurement): how spec launches run the fan tiles beside the sphere pixels — 0 two kernels on
 * two streams, pipelined across launches (the default), 1 two kernels one after the other on one stream. (Round
 * 4's mode 2, spec and fan blocks in one grid, measured slower and is archived: branch round4-ab-archive.)
 * `lead` is ignored. */
int iqpt_debug_set_specfan(iqpt_ctx* c, int mode, uint32_t lead) {
    (void)lead;
    if (!c || mode < 0 || mode > 1) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL or mode not 0..1");
    int st = enter(c);
    if (st) return st;
    c->specfan_mode = mode;
    return IQPT_OK;
}

/* Internal (tests, A/B): the slots per sample (x 256) a spec window assumes for a pixel without history (a
 * small value makes the chains of sphere pixels leave their first window: the walker then finishes them)
 * and the window margin divisor. 0 restores a default; the history is dropped. */
int iqpt_debug_set_spec(iqpt_ctx* c, uint32_t rho0, uint32_t margin_div) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    c->spec_margin_div = margin_div ? margin_div : 16u;
    c->spec_rho0 = rho0 ? rho0 : iqpt::kSpecRho0;
    c->spec_rho_valid = false;
    return IQPT_OK;
}

/* Internal (tests): after joining the context's streams, fills the LDS of every CU with non-zero garbage (blocks of
 * the largest per-block allocation, eight per CU) on the context's stream, ahead of the next launch, which then
 * starts joined behind it: a kernel that reads LDS before writing it gives other bits than the oracle. */
int iqpt_debug_poison_lds(iqpt_ctx* c, uint32_t pattern) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    int st = enter(c);
    if (st) return st;
    const uint32_t bytes = c->lds_per_block & ~3u;
    const int le = iqpt::launch_lds_poison(c->stream, pattern, bytes, (uint32_t)c->num_cus * 8u);
    if (le != 0) return iqpt::hip_fail((hipError_t)le, "LDS poison kernel");
    IQPT_HIP(hipStreamSynchronize(c->stream));
    return IQPT_OK;
}

/* Internal (tests): lower the kernels' forward-progress bound (0 keeps the default) and bias the per-tile wait targets
 * of overlapped launches, so that tests can force the error path. iter_limit bounded the archived chain kernel's loop: it is
 * kept in the signature and ignored. */
int iqpt_debug_set_limits(iqpt_ctx* c, uint32_t spin_limit, uint32_t /*iter_limit*/, uint32_t wait_bias) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    c->spin_limit = spin_limit ? spin_limit : iqpt::kOverlapSpinLimit;
    c->wait_bias = wait_bias;
    return IQPT_OK;
}

// kOptSplit statistics of the last launch (tools/split_share.py): split tiles, anchored tiles, split
// slots, leftovers of round 1, sum of the windows M, sum of the slots-per-sample estimates (x 256),
// split pixels, whether the last launch ran split. Synchronises.
int iqpt_debug_split_info(iqpt_ctx* c, unsigned long long* out8) {
    if (!c || !out8) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    int st = enter(c);
    if (st) return st;
    IQPT_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    out8[0] = c->n_split_tiles;
    out8[1] = c->n_anchor;
    const size_t ns = (size_t)c->n_split_tiles * iqpt::kQueueChunk;
    out8[2] = ns;
    // launch mode: 0 plain, 1 split, 5 split + fan, 6 spec (sphere pixels slot-parallel, the rest fan); 2-4 were the
    // chain and FAN launches (archived in round 6)
    out8[7] = c->spec_last ? 6 : (c->split_last ? (c->fan_last ? 5 : 1) : 0);
    if (!c->d_split || ns == 0) return IQPT_OK;
    uint32_t left = 0;
    IQPT_HIP(hipMemcpy(&left, c->d_queue + 2, sizeof left, hipMemcpyDeviceToHost));
    out8[3] = left;
    std::vector<uint32_t> v(3 * ns);
    IQPT_HIP(hipMemcpy(v.data(), c->d_split + c->n_anchor + c->n_split_tiles, v.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < ns; ++i) {
        if (v[i] == ~0u) continue;
        out8[4] += v[ns + i];
        out8[5] += v[2 * ns + i];
        out8[6] += 1;
    }
    return IQPT_OK;
}

// The production option mask (kOptDefault) for A/B tools and tests.
int iqpt_debug_default_options(void) { return iqpt::kOptDefault; }

int iqpt_debug_set_kernel_options(iqpt_ctx* c, int opt) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    // (resident launches add kOptPrio when only that form is built, as iqpt_render does)
    if (!iqpt::render_variant_exists(c->max_depth, false, opt) &&
        !iqpt::render_variant_exists(c->max_depth, false, opt | iqpt::kOptPrio) &&
        !iqpt::render_variant_exists(c->max_depth, true, opt))
        return iqpt::fail(IQPT_ERR_UNSUPPORTED, "kernel option set not compiled into this build");
    int st = enter(c);
    if (st) return st;
    if ((opt & iqpt::kOptStats) && !c->d_stats) {
        const size_t words = iqpt::kStatsHeader + 3 * (size_t)iqpt::kStatsWaveSlots + iqpt::kStatsQueueSlots +
                             iqpt::kStatsPhaseWords * (size_t)iqpt::kStatsWaveSlots;
        if (hipMalloc(&c->d_stats, words * sizeof(unsigned long long)) != hipSuccess)
            return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "stats");
        IQPT_HIP(hipMemset(c->d_stats, 0, words * sizeof(unsigned long long)));
        // the context's streams do not wait for the null stream: the counters must be clear before a launch adds to them
        IQPT_HIP(hipDeviceSynchronize());
    }
    c->opt = opt;
    c->opt_fixed = true;
    return IQPT_OK;
}

/* Internal (tests/test_cull.py): the host build of iq_interval.h for one tile of camera rays,
 * x in [xa, xb], y in [ya, yb]. tris: ntri x 9 floats (v0, e1, e2 world space); spheres: nsph x 4
 * (center, radius). Writes 1 per culled primitive; returns 0 with all flags 0 if the bundle is
 * unbounded (nothing can be culled). */
int iqpt_debug_cull_tile(const iqpt_camera* cam, uint32_t xa, uint32_t xb, uint32_t ya, uint32_t yb,
                         const float* tris, uint32_t ntri, const float* spheres, uint32_t nsph,
                         uint8_t* tri_culled, uint8_t* sph_culled) {
    if (!cam || (ntri && (!tris || !tri_culled)) || (nsph && (!spheres || !sph_culled)))
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    iqiv::camera_in ci;
    ci.width = cam->width;
    ci.height = cam->height;
    ci.rcp_width = 0.0f;
    ci.rcp_height = 0.0f;
    ci.inv_proj = cam->inv_proj;
    ci.inv_view = cam->inv_view;
    uint32_t cc = 0;
    cam_constants(*cam, &cc, &ci.near_rw, &ci.far_rw);
    ci.cam_const = (int)cc;
    const iqiv::bundle b = iqiv::camera_bundle(ci, xa, xb, ya, yb);
    for (uint32_t k = 0; k < ntri; ++k)
        tri_culled[k] = b.ok && iqiv::tri_culled(b, tris + 9 * k, tris + 9 * k + 3, tris + 9 * k + 6) ? 1 : 0;
    for (uint32_t k = 0; k < nsph; ++k) {
        const float* sp = spheres + 4 * k;
        sph_culled[k] = b.ok && iqiv::sphere_culled(b, sp, sp[3]) ? 1 : 0;
    }
    return b.ok ? 1 : 0;
}

/* Internal (tests/test_certain.py): the host build of iq_interval.h's tri_certain for one bundle of camera rays,
 * same conventions as iqpt_debug_cull_tile. Writes 1 per triangle that every ray of the bundle is proved to hit
 * as a first hit; returns 0 with all flags 0 if the bundle is unbounded (nothing is certain). */
int iqpt_debug_certain_tile(const iqpt_camera* cam, uint32_t xa, uint32_t xb, uint32_t ya, uint32_t yb,
                            const float* tris, uint32_t ntri, uint8_t* certain_out) {
    if (!cam || (ntri && (!tris || !certain_out))) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    iqiv::camera_in ci;
    ci.width = cam->width;
    ci.height = cam->height;
    ci.rcp_width = 0.0f;
    ci.rcp_height = 0.0f;
    ci.inv_proj = cam->inv_proj;
    ci.inv_view = cam->inv_view;
    uint32_t cc = 0;
    cam_constants(*cam, &cc, &ci.near_rw, &ci.far_rw);
    ci.cam_const = (int)cc;
    const iqiv::bundle b = iqiv::camera_bundle(ci, xa, xb, ya, yb);
    for (uint32_t k = 0; k < ntri; ++k)
        certain_out[k] = b.ok && iqiv::tri_certain(b, tris + 9 * k, tris + 9 * k + 3, tris + 9 * k + 6) ? 1 : 0;
    return b.ok ? 1 : 0;
}

/* Internal (tests/test_gpu_proofs.py): what the proof kernels wrote and read for the current masks, as 32-bit
 * words copied from the device after a synchronise. *n = the buffer's size in words (0 where it was not built);
 * copied into out if out is not NULL (cap words must hold it). IQPT_ERR_NOT_READY without valid masks (before the
 * first launch or iqpt_prepare, or after a change that invalidates them). what:
 *   0  12 words: cull_ntx, cull_nty, cull_wt, cull_stride, ntri, nsph, certain masks built, lists built,
 *      list entries, per-pixel masks built, per-pixel mask words, 0
 *   1  d_cull: ntiles x stride words (iqpt_bin_kernel)
 *   2  d_certain: 2 ntiles words of certain-hit masks, then 2 ntiles of certain-miss masks (iqpt_certain_kernel)
 *   3  d_list: the candidate lists, then the triangle offsets (ntiles + 1) and the sphere offsets (ntiles + 1)
 *   4  d_pmask: the per-tile word offsets (ntiles + 1), the per-pixel mask words, then iqpt_pixel_mask_kernel's
 *      2 ntiles certain words
 *   5  d_tris: ntri x 12 floats (v0, e1, e2 world space, three pad words)
 *   6  d_sph: nsph x 4 floats (centre, radius)
 *   7  d_certain's third plane: 2 ntiles words of beside-a-sphere hit masks (the pixels of tiles with a sphere
 *      candidate that iqpt_certain_kernel proves certain hits; the folded masks kparams::certain reads are the
 *      hit masks of 2 OR these, iqpt_debug_certain_tiles) */
int iqpt_debug_read_proofs(iqpt_ctx* c, int what, uint32_t* out, uint64_t cap, uint64_t* n) {
    if (!c || !n) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    *n = 0;
    if (!c->have_camera || !c->have_packet || !c->cull_valid) return iqpt::fail(IQPT_ERR_NOT_READY, "no valid masks");
    int st = enter(c);
    if (st) return st;
    IQPT_HIP(hipStreamSynchronize(c->stream));
    const uint64_t nt = (uint64_t)c->cull_ntx * c->cull_nty;
    const bool masks = nt * c->cull_stride > 0 && c->d_cull;
    const bool lists = masks && c->d_list;
    const bool pm = lists && c->d_pmask;
    const uint32_t grid[12] = {c->cull_ntx, c->cull_nty, c->cull_wt, c->cull_stride, c->ntri, c->nsph,
                               masks && c->certain_valid && c->d_certain ? 1u : 0u, lists ? 1u : 0u,
                               lists ? (uint32_t)c->list_total : 0u, pm ? 1u : 0u, pm ? (uint32_t)c->pmask_words : 0u, 0u};
    const void* src = nullptr;
    uint64_t words = 0;
    switch (what) {
    case 0: words = 12; break;
    case 1: if (masks) { src = c->d_cull; words = nt * c->cull_stride; } break;
    case 2: if (grid[6]) { src = c->d_certain; words = 4 * nt; } break;
    case 3: if (lists) { src = c->d_list; words = c->list_total + 2 * (nt + 1); } break;
    case 4: if (pm) { src = c->d_pmask; words = nt + 1 + c->pmask_words + 2 * nt; } break;
    case 5: if (c->d_tris) { src = c->d_tris; words = (uint64_t)c->ntri * iqpt::kTriFloat4 * 4; } break;
    case 6: if (c->d_sph) { src = c->d_sph; words = (uint64_t)c->nsph * 4; } break;
    case 7: if (grid[6]) { src = c->d_certain + 2 * iqpt::kCertainBeside * nt; words = 2 * nt; } break;
    default: return iqpt::fail(IQPT_ERR_INVALID_ARG, "unknown buffer selector");
    }
    *n = words;
    if (!out || words == 0) return IQPT_OK;
    if (cap < words) return iqpt::fail(IQPT_ERR_INVALID_ARG, "buffer too small");
    if (what == 0) std::memcpy(out, grid, sizeof grid);
    else IQPT_HIP(hipMemcpy(out, src, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return IQPT_OK;
}

/* Internal (tests/test_gpu_bvh.py): the BVH of the uploaded packet — node count and the number of
 * triangles left on the always-tested list (both 0 without a BVH). */
int iqpt_debug_bvh_info(iqpt_ctx* c, uint32_t* nnodes, uint32_t* nalways) {
    if (!c || !nnodes || !nalways) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    *nnodes = c->d_bvh_nodes ? c->bvh_nnodes : 0u;
    *nalways = c->d_bvh_nodes ? c->bvh_nalways : 0u;
    return IQPT_OK;
}

/* Internal (tests/test_gpu_sphere_bvh.py): the sphere BVH of the uploaded packet — node count and the
 * number of spheres on the always-tested list (both 0 without one). */
int iqpt_debug_sbvh_info(iqpt_ctx* c, uint32_t* nnodes, uint32_t* nalways) {
    if (!c || !nnodes || !nalways) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    *nnodes = c->d_sbvh_nodes ? c->sbvh_nnodes : 0u;
    *nalways = c->d_sbvh_nodes ? c->sbvh_nalways : 0u;
    return IQPT_OK;
}

/* Internal (tests/test_sphere_bvh.py): the sphere bound of iq_bvh.hpp, growth(S) for radii r_min,
 * r_max at origin distance S. */
double iqpt_debug_sphere_growth(double rmin, double rmax, double S) { return iqbvh::sphere_growth(rmin, rmax, S); }

/* Internal (tests/test_bvh.py): the error bound of iq_bvh.hpp for one triangle's edges, evaluated
 * at S = max_i |o_i - v0_i| and a lower bound D of the accepted determinant (D <= 1e-6: the reject
 * threshold). out: box growth, dt_a, dt_b (|t^ - t| <= dt_a + dt_b |t|), safety x E_det. Returns 1 if
 * the triangle is BVH-eligible, 0 if not. */
int iqpt_debug_bvh_bound(const float* e1, const float* e2, double S, double Md, double D, double* out4) {
    if (!e1 || !e2 || !out4) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    const iqbvh::tri_coeffs b = iqbvh::triangle_coeffs(e1, e2, Md);
    const double lambda = D > iqbvh::kDetMin ? iqbvh::kDetMin / D : 1.0;
    out4[0] = lambda * (b.gR + b.gB * S) + b.gC;
    out4[1] = lambda * b.tA * S;
    out4[2] = b.tB;
    out4[3] = b.edet;
    return b.eligible ? 1 : 0;
}

/* Internal (tests/test_gpu_libm.py): evaluate the device build of the shared math on n inputs on
 * the current device (synchronous). */
int iqpt_debug_libm(int fn, const float* a, const float* b, float* out, uint64_t n) {
    if (!a || !b || !out) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (n == 0) return IQPT_OK;
    if (n > (1ull << 28)) return iqpt::fail(IQPT_ERR_INVALID_ARG, "n too large");
    float *da = nullptr, *db = nullptr, *dout = nullptr;
    const size_t bytes = (size_t)n * sizeof(float);
    int st = IQPT_OK;
    if (hipMalloc(&da, bytes) != hipSuccess || hipMalloc(&db, bytes) != hipSuccess ||
        hipMalloc(&dout, bytes) != hipSuccess) {
        st = iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "libm probe buffers");
    } else {
        hipError_t e = hipMemcpy(da, a, bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(db, b, bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = (hipError_t)iqpt::launch_libm(nullptr, fn, da, db, dout, (uint32_t)n);
        if (e == hipSuccess) e = hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) st = iqpt::hip_fail(e, "libm probe");
    }
    (void)hipFree(da);
    (void)hipFree(db);
    (void)hipFree(dout);
    return st;
}

/* Internal (tests/test_gpu_scatter_probe.py): n Oren-Nayar scatters on the current device (synchronous), one per
 * case, by the form `form` of or_scatter_core (0-4, iqpt_internal.hpp launch_scatter_probe); sphere != 0 runs
 * sphere_hit and oren_nayar_scatter instead (forms 0-3; A, B and albedo unused). in: 12 floats per case, states: 6
 * words, active: 1 byte (layouts at iqpt_scatter_probe_kernel). ray (6 floats), vals (3 floats), states_out (6 words)
 * and fell_back (1 byte) per case go to the device as the caller filled them and come back: what an inactive case
 * holds afterwards is what the caller put there. */
int iqpt_debug_scatter(int form, int sphere, float A, float B, float albedo, const float* in, const uint32_t* states,
                       const uint8_t* active, uint64_t n, float* ray, float* vals, uint32_t* states_out,
                       uint8_t* fell_back) {
    if (!in || !states || !active || !ray || !vals || !states_out || !fell_back)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (form < 0 || form > 4 || (form == 4 && sphere)) return iqpt::fail(IQPT_ERR_INVALID_ARG, "no such scatter form");
    if (n == 0) return IQPT_OK;
    if (n > (1ull << 24)) return iqpt::fail(IQPT_ERR_INVALID_ARG, "n too large");
    const size_t sizes[7] = {n * 12 * sizeof(float), n * 6 * sizeof(uint32_t), n, n * 6 * sizeof(float),
                             n * 3 * sizeof(float), n * 6 * sizeof(uint32_t), n};
    const void* src[7] = {in, states, active, ray, vals, states_out, fell_back};
    void* back[7] = {nullptr, nullptr, nullptr, ray, vals, states_out, fell_back};
    void* dev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int st = IQPT_OK;
    for (int i = 0; i < 7 && st == IQPT_OK; ++i)
        if (hipMalloc(&dev[i], sizes[i]) != hipSuccess) st = iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "scatter probe buffers");
    if (st == IQPT_OK) {
        hipError_t e = hipSuccess;
        for (int i = 0; i < 7 && e == hipSuccess; ++i) e = hipMemcpy(dev[i], src[i], sizes[i], hipMemcpyHostToDevice);
        iqpt::kscatter_probe k;
        k.in = (const float*)dev[0];
        k.st_in = (const uint32_t*)dev[1];
        k.active = (const uint8_t*)dev[2];
        k.ray = (float*)dev[3];
        k.vals = (float*)dev[4];
        k.st_out = (uint32_t*)dev[5];
        k.fell_back = (uint8_t*)dev[6];
        k.n = (uint32_t)n;
        k.A = A;
        k.B = B;
        k.albedo = albedo;
        if (e == hipSuccess) e = (hipError_t)iqpt::launch_scatter_probe(nullptr, form, sphere != 0, k);
        for (int i = 3; i < 7 && e == hipSuccess; ++i) e = hipMemcpy(back[i], dev[i], sizes[i], hipMemcpyDeviceToHost);
        if (e != hipSuccess) st = iqpt::hip_fail(e, "scatter probe");
    }
    for (int i = 0; i < 7; ++i) (void)hipFree(dev[i]);
    return st;
}

/* Internal (tests/test_camera_axis.py): 1 if the camera qualifies for the short pitch-only transform
 * (kOptCamAxis), its 16 launch constants in k16; 0 otherwise. Host only. */
int iqpt_debug_cam_axis(const iqpt_camera* cam, float* k16) {
    if (!cam || !k16) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    std::memset(k16, 0, 16 * sizeof(float));
    return cam_axis_constants(*cam, k16) ? 1 : 0;
}

/* Internal (tests/test_gpu_camera.py): the general camera transform and, if the camera qualifies,
 * the kOptCamAxis one, on the GPU for n (x_ndc, y_ndc) pairs; 6 floats (origin, direction) per ray
 * into gen / axis. Returns 1 if the axis form ran, 0 if not (synchronous). */
int iqpt_debug_camera_rays(const iqpt_camera* cam, const float* ndc, uint64_t n, float* gen, float* axis) {
    if (!cam || !ndc || !gen || !axis) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (n > (1ull << 24)) return iqpt::fail(IQPT_ERR_INVALID_ARG, "n too large");
    iqpt::kparams p;
    std::memset(&p, 0, sizeof p);
    p.width = cam->width;
    p.height = cam->height;
    std::memcpy(p.inv_proj, cam->inv_proj, sizeof p.inv_proj);
    std::memcpy(p.inv_view, cam->inv_view, sizeof p.inv_view);
    cam_constants(*cam, &p.cam_const, &p.cam_near_rw, &p.cam_far_rw);
    const bool ax = cam_axis_constants(*cam, p.cam_ax);
    if (n == 0) return ax ? 1 : 0;
    float *dn = nullptr, *dg = nullptr, *da = nullptr;
    int st = IQPT_OK;
    if (hipMalloc(&dn, n * 2 * sizeof(float)) != hipSuccess || hipMalloc(&dg, n * 6 * sizeof(float)) != hipSuccess ||
        hipMalloc(&da, n * 6 * sizeof(float)) != hipSuccess) {
        st = iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "camera probe buffers");
    } else {
        hipError_t e = hipMemcpy(dn, ndc, n * 2 * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(da, 0, n * 6 * sizeof(float));
        if (e == hipSuccess) e = (hipError_t)iqpt::launch_camera_probe(nullptr, p, dn, dg, da, (uint32_t)n, ax);
        if (e == hipSuccess) e = hipMemcpy(gen, dg, n * 6 * sizeof(float), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(axis, da, n * 6 * sizeof(float), hipMemcpyDeviceToHost);
        if (e != hipSuccess) st = iqpt::hip_fail(e, "camera probe");
    }
    (void)hipFree(dn);
    (void)hipFree(dg);
    (void)hipFree(da);
    return st ? st : (ax ? 1 : 0);
}

/* Internal (tests/test_gpu_materials.py): set the frame counter (frames accumulated so far), e.g.
 * beyond 2^32 to exercise the running mean's large-n forms. */
int iqpt_debug_set_frame(iqpt_ctx* c, uint64_t frame) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    c->frame = frame;
    return IQPT_OK;
}

/* Internal (tests): the kernel option set of the context's last render launch (-1 before any), with bit 30 set when
 * that launch dealt its tiles to per-XCD lists and queue words (overlapped launches; streamed launches,
 * iqpt_debug_set_stream_xcd): the kernels fall back to one queue silently otherwise; bit 29 when it ran
 * iqpt_anyhit_kernel instead of the plain kernel (any-hit scenes with per-pixel masks on every tile). */
int iqpt_debug_last_options(iqpt_ctx* c, int* opt) {
    if (!c || !opt) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    *opt = c->last_opt < 0 ? c->last_opt
                           : (c->last_opt | (c->last_xcd_lists ? (1 << 30) : 0) | (c->last_anyk ? (1 << 29) : 0));
    return IQPT_OK;
}

/* Internal (tests/test_variant_cases.py, tests/test_gpu_variant_census.py): the kernel variant tables of
 * iqpt_kernels.hip as data, three int32 per row: maxd (8 or 16), streamed (0 or 1), opt (the instantiated kOpt* set);
 * -1 for a field the table does not have. table: 0 iqpt_render_kernel, 1 iqpt_fan_kernel, 2 iqpt_sky_kernel,
 * 3 iqpt_anyhit_kernel, 4 iqpt_spec_kernel, 5 iqpt_split_stitch_kernel. *nrows = the table's rows; up to cap_rows of
 * them are written to out (which may be NULL with cap_rows 0). Reads the arrays the launchers search. Host only: no
 * context, no device. */
int iqpt_debug_variant_table(int table, int32_t* out, uint32_t cap_rows, uint32_t* nrows) {
    if (!nrows || (cap_rows && !out)) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    *nrows = 0;
    if (table < iqpt::kTableRender || table > iqpt::kTableStitch) return iqpt::fail(IQPT_ERR_INVALID_ARG, "table not 0..5");
    int r3[3];
    uint32_t n = 0;
    for (; iqpt::variant_table_row(table, n, r3); ++n)
        if (n < cap_rows)
            for (int k = 0; k < 3; ++k) out[3 * (size_t)n + k] = r3[k];
    *nrows = n;
    return IQPT_OK;
}

/* Internal (tests/test_gpu_variant_census.py): the kernels of the context's last render launch (of the last launch
 * of an iqpt_render call that the running-mean table splits in several). out8: 0 maxd, 1 streamed, 2 the option set of
 * the plain kernel (iqpt_debug_last_options without its bits 29 and 30) or of the spec kernel's row, -1 if neither
 * ran; 3..7 the rows of iqpt_debug_variant_table's tables 2 (sky), 1 (fan), 4 (spec), 3 (any-hit) and 5 (split-stitch)
 * the launch ran, -1 for a kernel it did not launch. All -1 before the first launch. */
int iqpt_debug_last_launch(iqpt_ctx* c, int32_t* out8) {
    if (!c || !out8) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    std::memcpy(out8, c->last_launch, sizeof c->last_launch);
    return IQPT_OK;
}

/* Internal (tools/wave_timeline.py): per wave slot of the last kOptStats launch, the shader-clock cycles spent in the
 * closest hits, the shading, the next rays and the rest of the loop (kStatsPhaseWords each, same slots as
 * iqpt_debug_read_wave_times). Call before iqpt_debug_read_stats. */
int iqpt_debug_read_wave_phases(iqpt_ctx* c, unsigned long long* out, uint32_t cap) {
    if (!c || !out) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    int st = enter(c);
    if (st) return st;
    IQPT_HIP(hipStreamSynchronize(c->stream));
    if (!c->d_stats) return iqpt::fail(IQPT_ERR_INVALID_ARG, "no stats buffer (kOptStats not set)");
    const size_t m = std::min<size_t>(cap, iqpt::kStatsWaveSlots);
    IQPT_HIP(hipMemcpy(out, c->d_stats + iqpt::kStatsHeader + 3 * (size_t)iqpt::kStatsWaveSlots + iqpt::kStatsQueueSlots,
                       iqpt::kStatsPhaseWords * m * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return IQPT_OK;
}

int iqpt_debug_read_wave_times(iqpt_ctx* c, unsigned long long* out, uint32_t cap, uint32_t* n) {
    if (!c || !out || !n) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    *n = 0;
    int st = enter(c);
    if (st) return st;
    IQPT_HIP(hipStreamSynchronize(c->stream));
    if (!c->d_stats) return IQPT_OK;
    unsigned long long cnt = 0;
    IQPT_HIP(hipMemcpy(&cnt, c->d_stats + 11, sizeof cnt, hipMemcpyDeviceToHost));
    const uint32_t m = (uint32_t)std::min<unsigned long long>({cnt, (unsigned long long)cap,
                                                               (unsigned long long)iqpt::kStatsWaveSlots});
    if (m) IQPT_HIP(hipMemcpy(out, c->d_stats + iqpt::kStatsHeader, 3 * (size_t)m * sizeof(unsigned long long),
                              hipMemcpyDeviceToHost));
    *n = m;
    return IQPT_OK;
}

/* Internal (tools/wave_timeline.py, tests/test_gpu_scatter_lean.py): the counter words after the 24 that
 * iqpt_debug_read_stats returns (word 24 first), at most cap of them; *n = how many. Does not clear: call before
 * iqpt_debug_read_stats, which clears every counter word. */
int iqpt_debug_read_stats_ext(iqpt_ctx* c, unsigned long long* out, uint32_t cap, uint32_t* n) {
    if (!c || !out || !n) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    *n = 0;
    int st = enter(c);
    if (st) return st;
    IQPT_HIP(hipStreamSynchronize(c->stream));
    const uint32_t m = std::min<uint32_t>(cap, iqpt::kStatsHeader - iqpt::kStatsLegacyWords);
    if (!c->d_stats) std::memset(out, 0, m * sizeof(unsigned long long));
    else IQPT_HIP(hipMemcpy(out, c->d_stats + iqpt::kStatsLegacyWords, m * sizeof(unsigned long long),
                            hipMemcpyDeviceToHost));
    *n = m;
    return IQPT_OK;
}

int iqpt_debug_read_stats(iqpt_ctx* c, unsigned long long* out16) {
    unsigned long long* out8 = out16;   // the first kStatsLegacyWords (24) counters (tools/ab_kernel.py)
    if (!c || !out8) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    int st = enter(c);
    if (st) return st;
    IQPT_HIP(hipStreamSynchronize(c->stream));
    if (!c->d_stats) {
        std::memset(out8, 0, iqpt::kStatsLegacyWords * sizeof(unsigned long long));
        return IQPT_OK;
    }
    IQPT_HIP(hipMemcpy(out8, c->d_stats, iqpt::kStatsLegacyWords * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    IQPT_HIP(hipMemset(c->d_stats, 0, iqpt::kStatsHeader * sizeof(unsigned long long)));   // counters, wave slot index
    IQPT_HIP(hipDeviceSynchronize());   // before the next launch on the context's (non-blocking) streams adds to them
    return IQPT_OK;
}

}  // extern "C"
