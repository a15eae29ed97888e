// iq_launch.cpp — iqpt_render: one launch (render_launch) and the named steps it is made of.
#include "runtime/iq_ctx.hpp"

using namespace iqpt::rt;

namespace {
// The spec plan from the history rho (n sphere pixels) into h: the order (n words: pixel q
// at each position), then 2 words per block (first position, count | log2(lanes / 8) << 8); returns the
// block count. Work of pixel q: the slots of its window (spec_window of its last chain's slots per sample)
// times their mean length (those slots per sample again). Lanes per pixel (8, 16, 32 or 64) come from one
// per-lane work target E, the smallest whose lanes all fit the resident blocks (one block-wave; if even 8
// lanes each do not fit, E = total work / resident lanes): pixel q takes the fewest lanes with w_q / lanes
// <= E. Each block holds one lane class (256 lanes), pixels sorted by work per lane, and the blocks run
// heaviest per lane first, so the launch's longest block starts first and light blocks fill the tail.
uint32_t spec_build_plan(iqpt_ctx* c, const iqpt::kparams& p, const iqpt::kspec& ks, int opt, const uint32_t* rho,
                         uint32_t* h) {
    const uint32_t n = ks.n;
    std::vector<double> w(n);
    double total = 0.0, wmax = 0.0;
    for (uint32_t q = 0; q < n; ++q) {
        const uint32_t r = rho[q] ? rho[q] : ks.rho0;
        const uint32_t m = iqpt::spec_window(r, p.spp, ks.m_cap, ks.margin_div);
        // slots traced (the window's; a parity pixel's even ones and, expected, a quarter of the window's odd
        // ones in the pooled fix-up pass) times their mean length
        const bool parity = ks.parity_rho != 0u && r >= ks.parity_rho && r <= ks.parity_hi;
        w[q] = (double)m * (parity ? 0.625 : 1.0) * (double)std::max<uint32_t>(r, 256u) / 256.0;
        total += w[q];
        wmax = std::max(wmax, w[q]);
    }
    int occ = 0;
    if (iqpt::spec_occupancy(p, ks, opt, &occ) != 0 || occ < 1) occ = 1;
    const double cap = iqpt::kSpecPlanCap * (double)c->num_cus * occ * 256.0;     // resident lanes, a little slack
    // lane classes: 256 / lanes pixels per block (a class that does not divide 256 leaves lanes idle); the
    // in-between classes let a plan use resident lanes that the next power of two would overfill (most
    // sphere pixels have the same work: r04 run 27)
    static constexpr uint32_t kLanes[iqpt::kSpecLaneClasses] = {8u, 16u, 32u, 64u};   // dividing 64: a pixel's
                                                                                           // lanes are one wave's
    constexpr uint8_t kTop = iqpt::kSpecLaneClasses - 1;
    auto cls_of = [&](uint32_t q, double e) -> uint8_t {
        uint8_t k = 0;
        while (k < kTop && w[q] > e * (double)kLanes[k]) ++k;
        return k;
    };
    auto lanes_at = [&](double e) {
        double sum = 0.0;
        for (uint32_t q = 0; q < n; ++q) sum += (double)kLanes[cls_of(q, e)];
        return sum;
    };
    double e = total / cap;                      // several block-waves: balanced work per lane
    if (lanes_at(wmax / 8.0) <= cap) {
        double lo = 0.0, hi = wmax / 8.0;        // lanes_at(hi) fits; find the smallest E that fits
        for (int it = 0; it < 40; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (lanes_at(mid) <= cap) hi = mid;
            else lo = mid;
        }
        e = hi;
    }
    std::vector<uint8_t> cls(n);
    double emax = 0.0;
    for (uint32_t q = 0; q < n; ++q) {
        uint8_t k = cls_of(q, e);
        if (c->spec_plan_mode == 3) k = 3;                                // 32 lanes
        if (c->spec_plan_mode == 4) k = kTop;                             // 64 lanes
        if (c->spec_plan_mode == 5) k = (uint8_t)(q % iqpt::kSpecLaneClasses);   // every class
        cls[q] = k;
        emax = std::max(emax, w[q] / (double)kLanes[k]);
    }
    // counting sort by (lane class, work per lane) descending
    constexpr uint32_t kB = 1024;
    constexpr uint32_t kC = iqpt::kSpecLaneClasses;
    std::vector<uint32_t> key(n), cnt((kC + 1) * kB + 2, 0);
    for (uint32_t q = 0; q < n; ++q) {
        const double pe = w[q] / (double)kLanes[cls[q]];
        const uint32_t b = emax > 0.0 ? std::min<uint32_t>(kB - 1, (uint32_t)(pe / emax * (kB - 1))) : 0u;
        key[q] = (kTop - cls[q]) * kB + (kB - 1 - b);   // ascending key: most lanes first, heaviest first
        cnt[key[q] + 1]++;
    }
    for (uint32_t k = 0; k < kC * kB + 1; ++k) cnt[k + 1] += cnt[k];
    for (uint32_t q = 0; q < n; ++q) h[cnt[key[q]]++] = q;
    // blocks of one class, then ordered by their first (heaviest) pixel's work per lane
    struct blk { double e; uint32_t first, word; };
    std::vector<blk> blocks;
    for (uint32_t i = 0; i < n;) {
        const uint32_t k = cls[h[i]], per = (uint32_t)iqpt::kSpecBlockLanes / kLanes[k];
        uint32_t m = 0;
        while (m < per && i + m < n && cls[h[i + m]] == k) ++m;
        blocks.push_back({w[h[i]] / (double)kLanes[k], i, m | (kLanes[k] << 8)});
        i += m;
    }
    std::stable_sort(blocks.begin(), blocks.end(), [](const blk& a, const blk& b) { return a.e > b.e; });
    for (size_t b = 0; b < blocks.size(); ++b) {
        h[n + 2 * b] = blocks[b].first;
        h[n + 2 * b + 1] = blocks[b].word;
    }
    return (uint32_t)blocks.size();
}

// The launch parameters that are plain reads of the context: frame, camera, limits, scene, pixel state. (The
// last eight, ntx to stats, were read after join_streams / build_cull before this was a function; neither writes
// what they read. kparams::iter_limit stays 0: no kernel reads it.)
void fill_scene_params(const iqpt_ctx* c, uint32_t spp, iqpt::kparams& p) {
    std::memset(&p, 0, sizeof p);
    p.width = c->width;
    p.height = c->height;
    p.x0 = c->set.x0;
    p.ncols = c->ncols;
    p.y0 = c->set.y0;
    p.ystep = c->set.ystep;
    p.nrows = c->set.nrows;
    p.npix = c->npix;
    p.frame0 = c->frame;
    p.spp = spp;
    p.max_depth = c->max_depth;
    std::memcpy(p.inv_proj, c->cam.inv_proj, sizeof p.inv_proj);
    std::memcpy(p.inv_view, c->cam.inv_view, sizeof p.inv_view);
    cam_constants(c->cam, &p.cam_const, &p.cam_near_rw, &p.cam_far_rw);
    p.acc_tab = spp <= iqpt::kAccTableMax ? 1u : 0u;
    p.spin_limit = c->spin_limit;
    p.frames32 = (c->frame + (uint64_t)spp) < (1ull << 32) ? 1u : 0u;
    // running mean under kOptFastDiv: c / n by Markstein's correction is exact while the quotient is
    // normal, c >= 2^-125 n; with n <= frame0 + spp the threshold 2^-124 (frame0 + spp) (rounded up,
    // at least 2^-100 for the operand range) routes the rest to the IEEE division (mean_terms)
    {
        const double nmax = (double)(c->frame + (uint64_t)spp);
        p.mean_tiny = (float)std::max(std::ldexp(nmax, -124) * 2.0, std::ldexp(1.0, -99));
    }
    p.tris = c->d_tris;
    p.tri_pairs = c->d_tri_pairs;
    p.ntri = c->ntri;
    p.ntri_pairs = (c->ntri + 1) / 2;
    p.spheres = c->d_sph;
    p.sph_pairs = c->d_sph_pairs;
    p.nsph = c->nsph;
    p.nsph_pairs = (c->nsph + 1) / 2;
    p.tri_mat = c->d_tri_mat;
    p.sph_mat = c->d_sph_mat;
    if (c->d_bvh_nodes && c->bvh_nnodes) {
        p.bvh_nodes = c->d_bvh_nodes;
        p.bvh_pairs = c->d_bvh_pairs;
        p.bvh_always = c->d_bvh_always;
        p.bvh_nnodes = c->bvh_nnodes;
        p.bvh_nalways = c->bvh_nalways;
        p.bvh_md = c->bvh_md;
        p.bvh_gulp = c->bvh_gulp;
    }
    if (c->d_sbvh_nodes && c->sbvh_nnodes) {
        p.sbvh_nodes = c->d_sbvh_nodes;
        p.sbvh_sph = c->d_sbvh_sph;
        p.sbvh_idx = c->d_sbvh_idx;
        p.sbvh_always = c->d_sbvh_always;
        p.sbvh_nnodes = c->sbvh_nnodes;
        p.sbvh_nalways = c->sbvh_nalways;
        p.sbvh_gulp = c->sbvh_gulp;
        p.bvh_md = 1.001f;          // bvh_ray_ok: |d_i| bound shared with the triangle BVH
    }
    p.mats = c->d_mats;
    p.tri_shade = c->d_tri_shade;
    // no sphere, no material table: every triangle emissive, a ray decided by its first accepted triangle
    p.anyhit = (c->nsph == 0 && !c->d_mats && c->anyhit_on) ? 1u : 0u;
    p.rcp_width = 1.0f / (float)c->width;
    p.rcp_height = 1.0f / (float)c->height;
    p.ntx = (c->ncols + iqpt::kCullTile - 1) / iqpt::kCullTile;
    p.ntiles = p.ntx * ((c->set.nrows + iqpt::kCullTile - 1) / iqpt::kCullTile);
    p.lin = c->d_lin;
    p.bgra = c->d_bgra;
    p.rng = c->d_rng;
    p.rays = c->d_rays;
    p.queue = c->d_queue;
    p.stats = c->d_stats;
}

// ... and the tile masks, candidate lists and per-pixel masks of the current camera and packet (build_cull)
void fill_mask_params(const iqpt_ctx* c, iqpt::kparams& p) {
    p.cull = c->d_cull;
    // (the folded hit masks of iqpt_certain_kernel's planes: the tile rule's and the beside-a-sphere pixels)
    p.certain = c->certain_valid && c->certain_on
                    ? c->d_certain + 2 * (size_t)iqpt::kCertainFolded * c->cull_ntx * c->cull_nty
                    : nullptr;
    p.tile_order = c->d_tile_order;
    p.cull_ntx = c->cull_ntx;
    p.cull_wt = c->cull_wt;
    p.cull_stride = c->cull_stride;
    if (c->d_list) {
        p.list = c->d_list;
        p.list_off_tri = c->d_list + c->list_total;
        p.list_off_sph = p.list_off_tri + (c->cull_ntx * c->cull_nty + 1);
        if (c->d_pmask) {
            const uint32_t nt = c->cull_ntx * c->cull_nty;
            p.pmask_off = c->d_pmask;
            p.pmask = c->d_pmask + (nt + 1);
            p.pmask_certain = c->d_pmask + (nt + 1) + c->pmask_words;
        }
    }
}

// kOptBvhPrimary by timing (iqpt_ctx::tune_stage), for a launch that may take either camera-ray path: decides
// once the timed launches are in, else makes this launch the next timed one. Returns the timing slot (-1: not
// a timed launch) and switches opt to prim_opt where this launch takes the BVH.
int tune_camera_rays(iqpt_ctx* c, int prim_opt, uint32_t lds, int& opt) {
    int tune_slot = -1;
    if (c->tune_stage == iqpt::kTuneLaunches) {
        // per variant the fastest of its timed launches, per sample-pixel of work
        double best[2] = {1e300, 1e300};
        bool ok = hipEventSynchronize(c->tune_ev[2 * iqpt::kTuneLaunches - 1]) == hipSuccess;
        for (int s = 0; ok && s < iqpt::kTuneLaunches; ++s) {
            float ms = 0.0f;
            ok = hipEventElapsedTime(&ms, c->tune_ev[2 * s], c->tune_ev[2 * s + 1]) == hipSuccess;
            if (ok) best[s & 1] = std::min(best[s & 1], (double)ms / std::max(1.0, c->tune_work[s]));
        }
        c->tune_primary = ok && best[1] < best[0];
        c->tune_stage = iqpt::kTuneLaunches + 1;
    }
    if (c->tune_stage < iqpt::kTuneLaunches) {
        tune_slot = c->tune_stage;
        for (int k = 0; k < 2; ++k) {
            hipEvent_t& ev = c->tune_ev[2 * tune_slot + k];
            if (!ev && hipEventCreate(&ev) != hipSuccess) ev = nullptr;
            if (!ev) tune_slot = -1;
        }
        if (tune_slot == 0) {   // load both code objects before either is timed
            int o2 = 0;
            (void)iqpt::render_occupancy(c->max_depth, true, prim_opt, lds, &o2);
        }
    }
    if ((tune_slot >= 0 && (tune_slot & 1)) || (tune_slot < 0 && c->tune_primary)) opt = prim_opt;
    return tune_slot;
}

// kOptSplit: the per-slot result buffers, grown for this launch; over the budget the launch is not split
int grow_split_results(iqpt_ctx* c, size_t ns_cap, uint32_t m_cap, uint32_t g_max, bool& split) {
    if (c->d_res || c->d_nres || c->d_run_st || c->d_chunks) {
        IQPT_HIP(hipStreamSynchronize(c->stream));
        dev_free(c->d_res);
        dev_free(c->d_nres);
        dev_free(c->d_run_st);
        dev_free(c->d_chunks);
        c->res_slots = 0;
    }
    const size_t slots = (size_t)m_cap * ns_cap;
    const size_t st_words = (size_t)(g_max + 1) * 6 * ns_cap;
    const size_t chunk_words = 2 * (size_t)g_max * c->n_split_tiles;
    if (slots * (sizeof(float4_storage) + 1) + (st_words + chunk_words) * 4 <= iqpt::kSplitResBudget &&
        hipMalloc(&c->d_res, slots * sizeof(float4_storage)) == hipSuccess &&
        hipMalloc(&c->d_nres, slots) == hipSuccess &&
        hipMalloc(&c->d_run_st, st_words * sizeof(uint32_t)) == hipSuccess &&
        hipMalloc(&c->d_chunks, chunk_words * sizeof(uint32_t)) == hipSuccess) {
        c->res_slots = slots;
    } else {
        (void)hipGetLastError();
        split = false;     // over the budget: the plain kernel (same bits)
    }
    return IQPT_OK;
}

// kOptSplit: the split set in the plain kernel's parameters and in those of the prep and stitch kernels
int fill_split_params(const iqpt_ctx* c, uint32_t spp, size_t ns_cap, uint32_t m_cap, uint32_t g_max,
                      iqpt::kparams& p, iqpt::ksplit& ks) {
    uint32_t* base = c->d_split;
    uint32_t* sp_pix = base + c->n_anchor + c->n_split_tiles;
    p.anchor_order = base;
    p.n_anchor = c->n_anchor;
    p.n_split_tiles = c->n_split_tiles;
    p.split_tiles = base + c->n_anchor;
    p.chunks = c->d_chunks;
    p.chunk_count = c->d_queue + 3;
    p.split_len = iqpt::kSplitRunLen;
    p.run_st = c->d_run_st;
    static_assert(iqpt::kSplitRefillMin >= 1u && iqpt::kSplitRefillMin <= 64u, "idle lanes of one wave");
    p.refill_min = iqpt::kSplitRefillMin;
    p.ns_cap = (uint32_t)ns_cap;
    p.m_cap = m_cap;
    p.sp_pix = sp_pix;
    p.sp_win = sp_pix + ns_cap;
    p.sp_rho = sp_pix + 2 * ns_cap;
    p.left = sp_pix + 3 * ns_cap;
    p.left_count = c->d_queue + 2;
    p.res = c->d_res;
    p.nres = c->d_nres;
    p.sp_st = c->d_sp_st;
    p.sp_acc = c->d_sp_acc;
    ks.ns_cap = (uint32_t)ns_cap;
    ks.spp = spp;
    ks.m_cap = m_cap;
    ks.g_max = g_max;
    ks.run_len = iqpt::kSplitRunLen;
    ks.heavy_rho = iqpt::kSplitHeavyRho;
    ks.run_st = c->d_run_st;
    ks.split_tiles = base + c->n_anchor;
    ks.chunks = c->d_chunks;
    ks.chunk_count = c->d_queue + 3;
    ks.max_depth = c->max_depth;
    ks.frame0 = c->frame;
    ks.mean_tiny = p.mean_tiny;
    ks.npix = c->npix;
    ks.ncols = c->ncols;
    ks.nrows = c->set.nrows;
    ks.sp_pix = sp_pix;
    ks.sp_win = sp_pix + ns_cap;
    ks.sp_rho = sp_pix + 2 * ns_cap;
    ks.left = sp_pix + 3 * ns_cap;
    ks.left_count = c->d_queue + 2;
    ks.res = c->d_res;
    ks.nres = c->d_nres;
    ks.sp_st = c->d_sp_st;
    ks.sp_acc = c->d_sp_acc;
    ks.lin = c->d_lin;
    ks.bgra = c->d_bgra;
    ks.rng = c->d_rng;
    ks.rays = c->d_rays;
    if (!c->split_last) {
        // no chain history from the previous launch (new split set or the plain kernel ran)
        IQPT_HIP(hipMemsetAsync(sp_pix + 2 * ns_cap, 0, ns_cap * sizeof(uint32_t), c->stream));
    }
    return IQPT_OK;
}

// kOptOverlap: the launch's stream (ls: `stream` and `stream2` in turn), its queue words and tile counts, the
// frame buffer it writes, and the waits that order it behind what it must not overtake
int begin_overlapped(iqpt_ctx* c, iqpt::kparams& p, hipStream_t& ls) {
    int st = IQPT_OK;
    if (c->ovl_zero || c->ovl_epoch >= (1u << 24)) {
        if ((st = join_streams(c)) != IQPT_OK) return st;
        IQPT_HIP(hipMemsetAsync(c->d_tile_done, 0, (size_t)p.ntiles * sizeof(uint32_t), c->stream));
        c->ovl_zero = false;
        c->ovl_epoch = 0;
    }
    if (!c->next_on_main) {
        // after everything `stream` held before its last launch, that launch's list resets included
        ls = c->stream2;
        IQPT_HIP(hipStreamWaitEvent(c->stream2, c->ev_pre, 0));
        c->s2_pending = true;
    }
    const uint32_t parity = c->ovl_epoch & 1u;
    p.queue = c->d_queue + 4 + parity * (iqpt::kOverlapQueueWords / 2);
    p.tile_done = c->d_tile_done;
    p.done_target = c->ovl_epoch ? c->ovl_epoch + c->wait_bias : 0u;
    p.xcd_order = c->d_xcd_order;
    std::memcpy(p.xcd_off, c->xcd_off, sizeof p.xcd_off);
    p.ovl_err = c->d_ovl_err;
    if (c->copy_seq > c->pwaited) {    // copies behind earlier pipelined launches may still read d_bgra
        IQPT_HIP(hipStreamWaitEvent(ls, c->pev[c->copy_seq % iqpt::kPipeRing], 0));
        c->pwaited = c->copy_seq;
    }
    if (c->d_bgra_alt) {
        std::swap(c->d_bgra, c->d_bgra_alt);
        p.bgra = c->d_bgra;
    }
    IQPT_HIP(hipMemsetAsync(p.queue, 0, (iqpt::kOverlapQueueWords / 2) * sizeof(uint32_t), ls));
    // the next launch (stream2) starts after all of this but not after this launch
    if (ls == c->stream) IQPT_HIP(hipEventRecord(c->ev_pre, c->stream));
    return IQPT_OK;
}

// pipelined launches (spec, FAN): the frame buffer this launch writes (the other one once copies are
// asynchronous), after the copy that read it two launches ago; the second stream after everything
// `stream` held unless the launch continues a pipeline
int pipe_begin(iqpt_ctx* c, bool pipe_next, iqpt::kparams& p) {
    if (c->pring_on) {
        c->pidx = (c->pidx + 1) % iqpt::kPipeRing;
        c->d_bgra = c->d_pring[c->pidx];
        p.bgra = c->d_bgra;
        if (c->pseq[c->pidx] > c->pwaited) {
            const uint64_t tgt = std::max<uint64_t>(c->pseq[c->pidx], c->copy_seq > 2u ? c->copy_seq - 2u : 0u);
            if (!(c->gather_skip & 4)) {
                IQPT_HIP(hipStreamWaitEvent(c->stream, c->pev[tgt % iqpt::kPipeRing], 0));
                IQPT_HIP(hipStreamWaitEvent(c->stream2, c->pev[tgt % iqpt::kPipeRing], 0));
            }
            c->pwaited = tgt;
        }
    }
    if (!pipe_next) {
        IQPT_HIP(hipEventRecord(c->ev_pre, c->stream));
        IQPT_HIP(hipStreamWaitEvent(c->stream2, c->ev_pre, 0));
    }
    return IQPT_OK;
}

// ... and its end: no join; the copy stream and every other entry point wait for both streams
int pipe_end(iqpt_ctx* c, int kind, hipEvent_t e1, bool e1_bound, hipEvent_t& e1b, int le) {
    if (!c->ev_pipe_end && hipEventCreateWithFlags(&c->ev_pipe_end, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        return iqpt::fail(IQPT_ERR_HIP, "pipelined launch events");
    }
    if (int s = ensure_copy_stream(c)) return s;
    // the kernels' own end events (bound timing events) where there are some; otherwise a copy records
    // markers on both streams when it is asked for
    c->end1 = e1_bound ? e1 : nullptr;
    c->end2 = e1b;
    if (!e1b) {
        e1b = take_event(c);
        if (e1b) (void)hipEventRecord(e1b, c->stream2);
    }
    c->s2_pending = true;
    c->pipe = le == 0;
    c->pipe_kind = kind;
    return IQPT_OK;
}

// ---- the spec kernel's buffers, parameters, plan and history (pipelined spec launches on `stream`):
// every enqueue of these on the spec kernel's stream `ss`
int spec_buffers(iqpt_ctx* c, uint32_t spp, hipStream_t ss, iqpt::kparams& p, iqpt::kspec& ks2) {
    std::memset(&ks2, 0, sizeof ks2);
    const uint32_t n = c->n_chain_pix;
    const uint32_t m_cap = iqpt::split_m_cap(spp);
    if (n > 0 && n <= c->spec_n && m_cap > c->spec_mcap) {
        // a longer launch on the same pixel list: only the slot results grow (the history and the plan stay)
        IQPT_HIP(hipStreamSynchronize(c->stream));
        dev_free(c->d_spec_res);
        c->spec_mcap = 0;
        const size_t slots = (size_t)c->spec_n * m_cap;
        if (slots * 16 > iqpt::kSplitResBudget ||
            hipMalloc(&c->d_spec_res, slots * sizeof(float4_storage)) != hipSuccess) {
            (void)hipGetLastError();
            c->d_spec_res = nullptr;
            return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "spec slot results");
        }
        c->spec_mcap = m_cap;
    }
    if (n > 0 && n > c->spec_n) {
        IQPT_HIP(hipStreamSynchronize(c->stream));
        dev_free(c->d_spec);
        dev_free(c->d_spec_res);
        dev_free(c->d_spec_plan);
        for (uint32_t** b : {&c->h_spec_rho, &c->h_spec_plan}) {
            if (*b) (void)hipHostFree(*b);
            *b = nullptr;
        }
        c->spec_n = c->spec_mcap = 0;
        c->spec_plan_n = 0;
        c->spec_rho_pending = c->spec_plan_up = false;
        const size_t slots = (size_t)n * m_cap;
        if ((!c->ev_spec_rho && hipEventCreateWithFlags(&c->ev_spec_rho, hipEventDisableTiming) != hipSuccess) ||
            (!c->ev_spec_plan && hipEventCreateWithFlags(&c->ev_spec_plan, hipEventDisableTiming) != hipSuccess) ||
            slots * 16 > iqpt::kSplitResBudget ||
            hipMalloc(&c->d_spec, (2 * (size_t)n + 2) * sizeof(uint32_t)) != hipSuccess ||
            hipMalloc(&c->d_spec_res, slots * sizeof(float4_storage)) != hipSuccess ||
            hipMalloc(&c->d_spec_plan, 3 * (size_t)n * sizeof(uint32_t)) != hipSuccess ||
            hipHostMalloc(&c->h_spec_rho, (size_t)n * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc(&c->h_spec_plan, 3 * (size_t)n * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "spec buffers");
        }
        // the statistics counters run from here (iqpt_debug_spec_info reads and clears them)
        IQPT_HIP(hipMemsetAsync(c->d_spec + 2 * (size_t)n, 0, 2 * sizeof(uint32_t), ss));
        c->spec_n = n;
        c->spec_mcap = m_cap;
        c->spec_rho_valid = false;
    }
    p.ovl_err = c->d_ovl_err;
    ks2.n = n;
    ks2.m_cap = m_cap;
    ks2.rho0 = c->spec_rho0;
    ks2.margin_div = c->spec_margin_div;
    ks2.parity_rho = c->spec_parity_rho;
    ks2.parity_hi = c->spec_parity_hi;
    ks2.pix = c->d_chain_pix;
    ks2.m = c->d_spec;
    ks2.rho = c->d_spec + n;
    ks2.run_count = c->d_spec + 2 * (size_t)n;
    ks2.res = c->d_spec_res;
    // a new pixel list: no history, and the statistics counters behind it (d_spec + 2 n) restart too
    // (after a list that shrank n they pointed into the old history)
    if (n > 0 && !c->spec_rho_valid) IQPT_HIP(hipMemsetAsync(ks2.rho, 0, ((size_t)n + 2) * sizeof(uint32_t), ss));
    c->spec_rho_valid = c->spec_rho_valid || n > 0;
    return IQPT_OK;
}

int spec_plan(iqpt_ctx* c, const iqpt::kparams& p, int opt, hipStream_t ss, iqpt::kspec& ks2) {
    const uint32_t n = ks2.n;
    // the plan: built from the history read after an earlier launch (asynchronous), or, for tests,
    // synchronously from the current history
    if (n > 0 && c->spec_plan_mode >= 2) {
        IQPT_HIP(hipStreamSynchronize(ss));
        IQPT_HIP(hipMemcpy(c->h_spec_rho, ks2.rho, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        const uint32_t nb = spec_build_plan(c, p, ks2, opt, c->h_spec_rho, c->h_spec_plan);
        IQPT_HIP(hipMemcpy(c->d_spec_plan, c->h_spec_plan, ((size_t)n + 2 * (size_t)nb) * sizeof(uint32_t),
                           hipMemcpyHostToDevice));
        c->spec_plan_n = n;
        c->spec_plan_blocks = nb;
    } else if (n > 0 && c->spec_plan_mode == 1 && c->spec_rho_pending &&
               hipEventQuery(c->ev_spec_rho) == hipSuccess &&
               (!c->spec_plan_up || hipEventQuery(c->ev_spec_plan) == hipSuccess)) {
        const uint32_t nb = spec_build_plan(c, p, ks2, opt, c->h_spec_rho, c->h_spec_plan);
        IQPT_HIP(hipMemcpyAsync(c->d_spec_plan, c->h_spec_plan, ((size_t)n + 2 * (size_t)nb) * sizeof(uint32_t),
                                hipMemcpyHostToDevice, ss));
        IQPT_HIP(hipEventRecord(c->ev_spec_plan, ss));
        c->spec_plan_up = true;
        c->spec_rho_pending = false;
        c->spec_plan_n = n;
        c->spec_plan_blocks = nb;
        c->spec_plan_age = 0;
    }
    if (n > 0 && c->spec_plan_mode >= 1 && c->spec_plan_n == n) {
        ks2.order = c->d_spec_plan;
        ks2.blocks = c->d_spec_plan + n;
        ks2.nblocks = c->spec_plan_blocks;
    }
    if (c->spec_tl_on && n > 0) {
        const size_t nb = ks2.blocks ? ks2.nblocks : (n + iqpt::kSpecPixPerBlock - 1) / iqpt::kSpecPixPerBlock;
        if (nb > c->spec_tl_blocks) {
            IQPT_HIP(hipStreamSynchronize(ss));
            dev_free(c->d_spec_tl);
            c->spec_tl_blocks = 0;
            if (hipMalloc(&c->d_spec_tl, nb * 8 * sizeof(unsigned long long)) != hipSuccess) {
                (void)hipGetLastError();
                return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "spec timeline");
            }
            c->spec_tl_blocks = nb;
        }
        IQPT_HIP(hipMemsetAsync(c->d_spec_tl, 0, nb * 8 * sizeof(unsigned long long), ss));
        ks2.tl = c->d_spec_tl;
    }
    return IQPT_OK;
}

// read this launch's history for the next plan: before the first plan, then every kSpecReplan launches
int spec_history(iqpt_ctx* c, hipStream_t ss, const iqpt::kspec& ks2) {
    const uint32_t n = ks2.n;
    if (n > 0 && c->spec_plan_mode == 1 && !c->spec_rho_pending &&
        (c->spec_plan_n != n || ++c->spec_plan_age >= iqpt::kSpecReplan)) {
        IQPT_HIP(hipMemcpyAsync(c->h_spec_rho, ks2.rho, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, ss));
        IQPT_HIP(hipEventRecord(c->ev_spec_rho, ss));
        c->spec_rho_pending = true;
    }
    return IQPT_OK;
}

// ---- iqpt_debug_last_launch's bookkeeping, beside each kernel's enqueue: the plain kernel's option set, and the
// row of its table an auxiliary kernel's launcher takes for `opt` (iqpt::variant_row, the launchers' own lookups)
void note_plain(iqpt_ctx* c, int opt) { c->cur_launch[2] = opt; }
void note_kernel(iqpt_ctx* c, int table, int opt) {
    const int row = iqpt::variant_row(table, c->max_depth, false, opt);
    switch (table) {
    case iqpt::kTableSky: c->cur_launch[3] = row; break;
    case iqpt::kTableFan: c->cur_launch[4] = row; break;
    case iqpt::kTableSpec: {
        int r3[3];
        c->cur_launch[5] = row;
        c->cur_launch[2] = row >= 0 && iqpt::variant_table_row(table, (uint32_t)row, r3) ? r3[2] : -1;
        break;
    }
    case iqpt::kTableAnyHit: c->cur_launch[6] = row; break;
    case iqpt::kTableStitch: c->cur_launch[7] = row; break;
    default: break;
    }
}

// ---- the enqueue of overlapped, spec and split launches; le: the kernels' launch status (reported after the
// bookkeeping). Overlapped: the plain kernel on ls, the sky kernel behind it where it was deferred
int enqueue_overlapped(iqpt_ctx* c, const iqpt::kparams& p, hipStream_t ls, uint32_t grid, uint32_t lds, int opt,
                       bool bind_ovl, bool sky_deferred, hipEvent_t e0, hipEvent_t e1, bool& e0_bound,
                       bool& e1_bound, int& le) {
    if (bind_ovl) iqpt::bind_launch_events(e0_bound ? nullptr : e0, sky_deferred ? nullptr : e1);
    le = iqpt::launch_render(ls, p, grid, lds, false, opt);
    note_plain(c, opt);
    iqpt::bind_launch_events(nullptr, nullptr);
    if (bind_ovl) {
        if (le != 0 && e0 && !e0_bound) (void)hipEventRecord(e0, ls);   // (not read: the launch failed)
        e0_bound = true;
        e1_bound = le == 0 && e1 != nullptr && !sky_deferred;
    }
    if (sky_deferred && le == 0) {
        if (c->sky_last && c->sky_last != ls) IQPT_HIP(hipStreamWaitEvent(ls, c->ev_sky, 0));
        iqpt::bind_launch_events(nullptr, e1);
        le = iqpt::launch_sky(ls, p, c->d_sky_tiles, c->n_sky_tiles, opt);
        note_kernel(c, iqpt::kTableSky, opt);
        iqpt::bind_launch_events(nullptr, nullptr);
        e1_bound = le == 0 && e1 != nullptr;
        if (le != 0) return iqpt::hip_fail((hipError_t)le, "sky kernel launch");
        IQPT_HIP(hipEventRecord(c->ev_sky, ls));
        c->sky_last = ls;
    }
    c->ovl_epoch += 1;
    c->next_on_main = !c->next_on_main;
    if (le != 0) c->ovl_zero = true;     // a failed launch breaks the chain's counts: restart it
    return IQPT_OK;
}

// Spec
int enqueue_spec(iqpt_ctx* c, iqpt::kparams& p, uint32_t spp, int opt, bool pipe_next, hipEvent_t e0, hipEvent_t e1,
                 hipEvent_t& e1b, bool& e1_bound, int& le) {
    int st = IQPT_OK;
    // every pixel without a sphere in reach in the fan kernel on stream2; the sphere pixels in
    // iqpt_spec_kernel on stream (slots, then the walk)
    iqpt::kspec ks2;
    if ((st = spec_buffers(c, spp, c->stream, p, ks2)) != IQPT_OK) return st;
    if (c->specfan_mode == 0 && (st = pipe_begin(c, pipe_next, p)) != IQPT_OK) return st;
    iqpt::kparams pf = p;
    pf.tile_order = c->d_fan_tiles;
    pf.fan_lanes = c->d_fan_lanes;
    // the certain-miss pixels the fan lists left out: the sky kernel, ahead of the fan
    // kernel on its stream (consecutive launches' sky kernels are ordered there)
    if (c->sky_active) {
        iqpt::kparams pm = pf;
        pm.miss = c->d_certain + 2 * (size_t)c->cull_ntx * c->cull_nty;
        le = iqpt::launch_sky(c->specfan_mode == 0 ? c->stream2 : c->stream, pm, c->d_sky_tiles, c->n_sky_tiles, opt);
        if (c->n_sky_tiles > 0) note_kernel(c, iqpt::kTableSky, opt);
        if (le != 0) return iqpt::hip_fail((hipError_t)le, "sky kernel launch");
    }
    if ((st = spec_plan(c, p, opt, c->stream, ks2)) != IQPT_OK) return st;
    const uint32_t n = ks2.n;
    auto run_spec = [&]() -> int {
        note_kernel(c, iqpt::kTableSpec, opt);
        return iqpt::launch_spec(c->stream, p, ks2, opt);
    };
    if (le == 0 && c->n_fan_tiles > 0) note_kernel(c, iqpt::kTableFan, opt);   // (either branch launches it)
    if (c->specfan_mode == 1) {
        if (n > 0) le = run_spec();
        if (le == 0 && c->n_fan_tiles > 0) le = iqpt::launch_fan(c->stream, pf, c->n_fan_tiles, opt);
    } else {
        if (n > 0) {
            iqpt::bind_launch_events(e0, e1);
            le = run_spec();
            iqpt::bind_launch_events(nullptr, nullptr);
            e1_bound = le == 0 && e1 != nullptr;
            if (le != 0 && e0) (void)hipEventRecord(e0, c->stream);   // (unrecorded events are not read)
        }
        if (le == 0 && c->n_fan_tiles > 0) {
            e1b = take_event(c);
            iqpt::bind_launch_events(nullptr, e1b);
            le = iqpt::launch_fan(c->stream2, pf, c->n_fan_tiles, opt);
            iqpt::bind_launch_events(nullptr, nullptr);
            if (le != 0 && e1b) {
                c->event_pool.push_back(e1b);
                e1b = nullptr;
            }
        }
        if ((st = pipe_end(c, 1, e1, e1_bound, e1b, le)) != IQPT_OK) return st;
    }
    if (le == 0 && (st = spec_history(c, c->stream, ks2)) != IQPT_OK) return st;
    return IQPT_OK;
}

// Split (resident scenes only)
int enqueue_split(iqpt_ctx* c, iqpt::kparams& p, const iqpt::ksplit& ks, uint32_t grid, uint32_t lds, int opt,
                  bool fan_split, int& le) {
    // prep -> round 1 (runs, anchored tiles, light split pixels) -> stitch -> round 2 (leftovers); with
    // the fan kernel the anchored tiles leave round 1 for iqpt_fan_kernel on stream2
    if (fan_split) {
        iqpt::kparams pf = p;
        pf.tile_order = c->d_split;
        IQPT_HIP(hipEventRecord(c->ev_pre, c->stream));
        IQPT_HIP(hipStreamWaitEvent(c->stream2, c->ev_pre, 0));
        le = iqpt::launch_fan(c->stream2, pf, c->n_anchor, opt);
        if (c->n_anchor > 0) note_kernel(c, iqpt::kTableFan, opt);
        p.n_anchor = 0;
    }
    if (le == 0) le = iqpt::launch_split_prep(c->stream, ks);
    p.split_round = 1;
    p.queue = c->d_queue;
    if (le == 0) le = iqpt::launch_render(c->stream, p, grid, lds, false, opt);
    note_plain(c, opt);
    if (le == 0) le = iqpt::launch_split_stitch(c->stream, ks, (opt & iqpt::kOptFastDiv) != 0);
    if (ks.ns_cap > 0) note_kernel(c, iqpt::kTableStitch, opt);
    p.split_round = 2;
    p.queue = c->d_queue + 1;
    if (le == 0) le = iqpt::launch_render(c->stream, p, grid, lds, false, opt);
    if (fan_split) {
        IQPT_HIP(hipEventRecord(c->ev_s2, c->stream2));
        IQPT_HIP(hipStreamWaitEvent(c->stream, c->ev_s2, 0));
    }
    return IQPT_OK;
}

}  // namespace

extern "C" {

// (an unnamed namespace inside extern "C": plain names in the symbol table, kept so; see iq_ctx.hpp)
namespace {
int render_launch(iqpt_ctx* c, uint32_t spp) {
    int st = IQPT_OK;
    iqpt::kparams p;
    fill_scene_params(c, spp, p);
    // kOptFastDiv only for packets inside its range (upload) and frames up to 2^24 wide / high
    // (camera_ray divides by W and H with the pre-rounded reciprocals p.rcp_width, p.rcp_height)
    int opt = c->opt;
    if (!c->fast_rcp_ok || c->width > (1u << 24) || c->height > (1u << 24)) opt &= ~iqpt::kOptFastDiv;
    if (!(opt & iqpt::kOptPair)) opt &= ~iqpt::kOptCull;       // masks are per primitive pair
    if (c->d_mats) opt |= iqpt::kOptMaterials;                  // the packet carries a material table
    const bool cam_axis = (opt & iqpt::kOptCamConst) && cam_axis_constants(c->cam, p.cam_ax);
    const bool pair = (opt & iqpt::kOptPair) != 0;
    const uint32_t tri_rec = pair ? iqpt::kTriPairFloat4 * 16 : iqpt::kTriFloat4 * 16;   // bytes per LDS record
    const uint32_t sph_rec = pair ? iqpt::kSphPairFloat4 * 16 : 16;
    const uint32_t tri_recs = pair ? p.ntri_pairs : p.ntri;
    const uint32_t sph_recs = pair ? p.nsph_pairs : p.nsph;
    const uint64_t resident = (uint64_t)tri_recs * tri_rec + (uint64_t)sph_recs * sph_rec;
    const bool stream_batches = resident > iqpt::kLdsResidentBytes;
    // production streamed variants are built without the 5-wave bound (registers for the BVH)
    if (stream_batches && !iqpt::render_variant_exists(c->max_depth, true, opt) &&
        iqpt::render_variant_exists(c->max_depth, true, opt & ~iqpt::kOptLB5))
        opt &= ~iqpt::kOptLB5;
    // streamed any-hit scenes take the variants with the first-hit exits (kOptAnyHit), where one exists
    if (stream_batches && p.anyhit && iqpt::render_variant_exists(c->max_depth, true, opt | iqpt::kOptAnyHit))
        opt |= iqpt::kOptAnyHit;
    // kOptCamAxis: the short camera transform, kept only where the camera qualifies (a caller's option
    // mask may ask for it; production launches add it below, where a variant exists: DESIGN.md §3.8)
    if (!cam_axis) opt &= ~iqpt::kOptCamAxis;
    // resident production variants carry kOptPrio (VALU priority for scatter-heavy waves; same bits)
    if (!stream_batches && !iqpt::render_variant_exists(c->max_depth, false, opt) &&
        iqpt::render_variant_exists(c->max_depth, false, opt | iqpt::kOptPrio))
        opt |= iqpt::kOptPrio;
    if (stream_batches) {
        p.tri_batch = pair ? iqpt::kTriBatch / 2 : iqpt::kTriBatch;   // records
        p.sph_batch = pair ? iqpt::kSphBatch / 2 : iqpt::kSphBatch;
        // a wave takes new pixels once this many of its lanes are idle (64: a whole tile at a time, its rays
        // coherent through the BVHs)
        p.refill_min = std::min<uint32_t>(64u, std::max<uint32_t>(1u, c->stream_refill_min));
    } else {
        p.refill_min = std::min<uint32_t>(64u, std::max<uint32_t>(1u, c->resident_refill_min));
        p.tri_batch = tri_recs;
        p.sph_batch = sph_recs;
    }
    // scene batch + running-mean table (padded to 16 B) + (kOptCull) one uint4 slot per thread +
    // the scatter-record stack (max_depth - 1 records per thread; one float each)
    uint32_t lds = p.tri_batch * tri_rec + p.sph_batch * sph_rec +
                         (p.acc_tab ? iqpt::acc_table_lds_bytes(spp) : 0u) +
                         ((opt & iqpt::kOptCull) ? iqpt::kRenderBlock * 16u : 0u) +
                         (uint32_t)std::max(c->max_depth, 1) * iqpt::kRenderBlock * 4u *
                             ((opt & iqpt::kOptMaterials) ? 3u : 1u);
    if ((opt & iqpt::kOptCull) && (c->ntri + c->nsph) > 0) {
        if (!c->cull_valid) {
            if ((st = join_streams(c)) != IQPT_OK) return st;   // new masks and tile lists: the chain restarts
            if ((st = build_cull(c)) != IQPT_OK) return st;
        }
        fill_mask_params(c, p);
    }
    // any-hit scenes whose every tile list has per-pixel masks: iqpt_anyhit_kernel renders the launch (one camera
    // ray per sample, the lane's own candidates; no BVH-primary tuning, no queue)
    const bool anyk = c->pmask_mode == 2 && !c->opt_fixed && stream_batches && p.anyhit && (opt & iqpt::kOptAnyHit) &&
                      p.pmask != nullptr && c->pmask_all && p.list != nullptr && spp > 0 && spp <= iqpt::kAccTableMax &&
                      iqpt::anyhit_variant_exists(opt);
    // kOptBvhPrimary: decided by timing (see iqpt_ctx::tune_stage). Its batch-free variants keep the 5-wave bound
    // the batched streamed variants drop for launches of up to kPrimaryLB5MaxSpp samples, and run at 4 waves
    // per SIMD (no spills) above that where that variant is built: C5 16 spp 54.0-54.3 -> 51.5 ms, 1 spp 3.17 ->
    // 3.39 ms (r06 run 36)
    constexpr uint32_t kPrimaryLB5MaxSpp = 4;
    const bool prim_lb5 = spp <= kPrimaryLB5MaxSpp ||
                          !iqpt::render_variant_exists(c->max_depth, true, (opt | iqpt::kOptBvhPrimary) & ~iqpt::kOptLB5);
    const int prim_opt = ((opt | iqpt::kOptBvhPrimary) & ~iqpt::kOptLB5) |
                         (prim_lb5 && iqpt::render_variant_exists(c->max_depth, true,
                                                                  opt | iqpt::kOptBvhPrimary | iqpt::kOptLB5)
                              ? iqpt::kOptLB5 : 0);
    int tune_slot = -1;
    if (!c->opt_fixed && !anyk && stream_batches && p.bvh_nodes && p.cull && (opt & iqpt::kOptBvh) &&
        iqpt::render_variant_exists(c->max_depth, true, prim_opt))
        tune_slot = tune_camera_rays(c, prim_opt, lds, opt);
    // kOptSplit: resident scenes with a split set, when the mode asks for it (auto:
    // fewer owned pixels than kSplitAutoPixelsPerLane per resident lane, i.e. too few pixel chains to
    // fill and drain the chip evenly)
    // (round 6: the chain kernel, DESIGN.md §3.9, and FAN launches, §3.10, left the library for the branch
    // round6-ab-archive; AUTO never chose FAN, and chain launches only where spec launches did not fit)
    bool auto_spec = false;             // AUTO: the share is small enough for spec launches (if they apply)
    if (c->split_mode == IQPT_SPLIT_AUTO && !stream_batches && p.cull && c->n_split_tiles > 0 && tune_slot < 0 &&
        !(opt & iqpt::kOptMaterials) && spp <= iqpt::kAccTableMax) {
        int occ_p = 0;
        if (iqpt::render_occupancy(c->max_depth, false, opt, lds, &occ_p) != 0) occ_p = 0;
        const double lanes = (double)c->num_cus * std::max(occ_p, 1) * iqpt::kRenderBlock;
        auto_spec = (double)c->npix < iqpt::kSpecAutoPixelsPerLane * lanes;
    }
    // the fan kernel: the anchored tiles (no sphere candidate) of spec and split launches
    const bool fan_ok = !stream_batches && p.cull && (c->n_anchor > 0 || c->n_fan_tiles > 0) && tune_slot < 0 &&
                        !(opt & iqpt::kOptMaterials) && spp <= iqpt::kAccTableMax && c->cull_wt <= 16 &&
                        iqpt::fan_variant_exists(opt);
    // spec launches: sphere pixels slot-parallel, every other pixel in the fan kernel
    bool spec = fan_ok && (c->split_mode == IQPT_SPLIT_SPEC || auto_spec) && c->n_split_tiles > 0 &&
                iqpt::spec_variant_exists(c->max_depth, opt) &&
                (size_t)c->n_chain_pix * iqpt::split_m_cap(spp) * 16u <= iqpt::kSplitResBudget;
    if (spec) {
        // the block's LDS (scene, tables, slot marks: 32 pixels x the window cap) must fit the device's per-block
        // limit with at least one resident block, else the plain path (same bits; ADVICE r3: a 1,024-spp launch
        // with a scene near the resident limit needs ~170 KB)
        iqpt::kspec probe;
        std::memset(&probe, 0, sizeof probe);
        probe.m_cap = iqpt::split_m_cap(spp);
        int occ_s = 0;
        spec = iqpt::spec_lds(p, probe) <= c->lds_per_block && probe.m_cap <= 65535u &&
               iqpt::spec_occupancy(p, probe, opt, &occ_s) == 0 && occ_s >= 1;
        (void)hipGetLastError();
    }
    uint32_t lds_split = lds + iqpt::kRenderBlock * (16u + 24u);   // + lds_sp and the base states
    bool split = false;
    if (!spec && c->split_mode != IQPT_SPLIT_OFF && c->split_mode != IQPT_SPLIT_SPEC && !stream_batches && p.cull &&
        c->n_split_tiles > 0 &&
        tune_slot < 0 && iqpt::render_variant_exists(c->max_depth, false, opt | iqpt::kOptSplit)) {
        int occ_s = 0;
        if (iqpt::render_occupancy(c->max_depth, false, opt | iqpt::kOptSplit, lds_split, &occ_s) != 0) occ_s = 0;
        const double lanes = (double)c->num_cus * std::max(occ_s, 1) * iqpt::kRenderBlock;
        split = occ_s > 0 && (c->split_mode == IQPT_SPLIT_ON || (double)c->npix < iqpt::kSplitAutoPixelsPerLane * lanes);
    }
    // pipelined spec launches continue without a join (the launch below orders itself); the others never overlap
    const bool pipe_next = c->pipe && spec && c->specfan_mode == 0 && c->pipe_kind == 1;
    if ((split || spec) && !pipe_next && (st = join_streams(c)) != IQPT_OK) return st;
    // split launches with the anchored tiles in the fan kernel beside the four split passes
    const bool fan_split = split && fan_ok;
    const size_t ns_cap = (size_t)c->n_split_tiles * iqpt::kQueueChunk;
    const uint32_t m_cap = iqpt::split_m_cap(spp);
    const uint32_t g_max = (m_cap + iqpt::kSplitRunLen - 1) / iqpt::kSplitRunLen;
    if (split && (size_t)m_cap * ns_cap > c->res_slots &&
        (st = grow_split_results(c, ns_cap, m_cap, g_max, split)) != IQPT_OK)
        return st;
    iqpt::ksplit ks;
    std::memset(&ks, 0, sizeof ks);
    if (split) {
        opt |= iqpt::kOptSplit;
        lds = lds_split;
        if ((st = fill_split_params(c, spp, ns_cap, m_cap, g_max, p, ks)) != IQPT_OK) return st;
    }
    // kOptOverlap: resident, culled, not split, not a tuning launch
    // Tiles are bound to the 8 XCDs (HW_REG_XCC_ID): only on a device that exposes 8 (not a partition
    // mode) and with at least 64 blocks, so that the observed round-robin dispatch puts blocks on every
    // XCD (HIP promises no placement; the kernel's last block checks it and raises an error bit if not)
    // kOptPipe: plain launches over resident scenes under the reference's materials take the
    // two-rays-per-lane variants where they are built (a caller's fixed option set keeps its own bits)
    if (!c->opt_fixed && c->pipe_on && !stream_batches && !split && !spec && tune_slot < 0 &&
        p.cull != nullptr && p.acc_tab && !(opt & iqpt::kOptMaterials) &&
        iqpt::render_variant_exists(c->max_depth, false, opt | iqpt::kOptPipe))
        opt |= iqpt::kOptPipe;
    bool ovl = c->overlap_mode != IQPT_OVERLAP_OFF && !stream_batches && !split && !spec &&
               p.cull != nullptr &&
               tune_slot < 0 && c->d_tile_done && c->d_xcd_order && c->num_xcc == 8 && c->num_cus >= 64 &&
               (uint64_t)c->npix >= 64ull * iqpt::kRenderBlock &&
               iqpt::render_variant_exists(c->max_depth, false, opt | iqpt::kOptOverlap);
    int occ = 0;
    if (iqpt::render_occupancy(c->max_depth, stream_batches, ovl ? (opt | iqpt::kOptOverlap) : opt, lds, &occ) != 0 ||
        occ < 1)
        occ = 1;
    // two launches in flight: each keeps one block slot per CU free for the other (occ - 1 per CU), so the
    // earlier launch, which the later one waits for, can always run
    if (ovl && occ < 2) ovl = false;
    if ((ovl || fan_split || spec) && !c->stream2) {
        if (hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_pre, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_s2, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            if (fan_split || spec) return iqpt::fail(IQPT_ERR_HIP, "second stream for the spec / fan kernel");
            ovl = false;
            c->overlap_mode = IQPT_OVERLAP_OFF;
        }
    }
    if (!ovl && !pipe_next && (st = join_streams(c)) != IQPT_OK) return st;
    hipStream_t ls = c->stream;                       // the launch's stream
    if (ovl) {
        opt |= iqpt::kOptOverlap;
        if ((st = begin_overlapped(c, p, ls)) != IQPT_OK) return st;
        occ -= 1;
    }
    // pitch-only cameras take the short camera transform (exact, kOptCamAxis) wherever that variant is
    // built: resident plain, overlapped and spec launches (C2 -14 % overlapped, C3 shares -3..-12 %,
    // profiles/r02/ab_camaxis_overlap.json, split_share_v17_camaxis.json)
    if (!c->opt_fixed && cam_axis && !stream_batches && !split &&
        iqpt::render_variant_exists(c->max_depth, false, opt | iqpt::kOptCamAxis) &&
        (!spec || iqpt::spec_variant_exists(c->max_depth, opt | iqpt::kOptCamAxis)))
        opt |= iqpt::kOptCamAxis;
    const uint64_t want = ((uint64_t)c->npix + iqpt::kRenderBlock - 1) / iqpt::kRenderBlock;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)c->num_cus * occ));
    // streamed scenes: per-XCD tile lists and queue words (iqpt_debug_set_stream_xcd), where the overlapped
    // launches could bind tiles to XCDs (8 XCDs, enough blocks; the kernel's last block checks the placement)
    constexpr uint32_t kStreamXcdMaxSpp = 4;
    const int xmode = c->stream_xcd == 3 ? (spp <= kStreamXcdMaxSpp ? 1 : 0) : c->stream_xcd;
    const bool xcdq = stream_batches && xmode != 0 && p.cull && c->d_xcd_order && c->d_xcd_band &&
                      !split && !spec && c->num_xcc == 8 && c->num_cus >= 64 && grid >= 64;
    if (xcdq) {
        p.xcd_order = xmode == 1 ? c->d_xcd_order : c->d_xcd_band;
        std::memcpy(p.xcd_off, xmode == 1 ? c->xcd_off : c->xcd_band_off, sizeof p.xcd_off);
        p.ovl_err = c->d_ovl_err;
    }
    if (!ovl && !spec)
        IQPT_HIP(hipMemsetAsync(c->d_queue, 0, (xcdq ? 16u * 8u + 1u : 4u) * sizeof(uint32_t), c->stream));
    hipEvent_t e0 = take_event(c), e1 = take_event(c), e1b = nullptr;
    // pipelined spec launches: the timing events are recorded by the spec and fan kernels' dispatches (no
    // marker packets between consecutive kernels on the two streams: -0.012 ms per step at N = 8, -0.04 with
    // a copy and gather every step, r04 run 12)
    const bool bind_spec = spec && c->specfan_mode == 0 && c->n_chain_pix > 0;
    // overlapped launches: recorded by the launch's first kernel on `ls` (the sky kernel or the plain kernel)
    // and its last (the plain kernel)
    const bool bind_ovl = ovl && tune_slot < 0;
    bool e0_bound = false, e1_bound = false;
    if (e0 && !bind_spec && !bind_ovl) (void)hipEventRecord(e0, ls);
    if (tune_slot >= 0) (void)hipEventRecord(c->tune_ev[2 * tune_slot], c->stream);
    int le = 0;
    for (int32_t& v : c->cur_launch) v = -1;
    c->cur_launch[0] = c->max_depth <= 8 ? 8 : 16;
    c->cur_launch[1] = stream_batches ? 1 : 0;
    // certain-miss pixels: plain launches hand them to iqpt_sky_kernel, ahead of the plain
    // kernel on the launch's stream; the plain kernel skips them. Consecutive sky kernels order themselves
    // through ev_sky (overlapped launches alternate streams); their pixels are disjoint from the plain kernel's.
    const bool sky = c->sky_on && c->certain_on && c->certain_valid && c->n_sky_tiles > 0 && p.certain != nullptr &&
                     !stream_batches && !split && !spec && tune_slot < 0 &&
                     !(opt & iqpt::kOptMaterials) && spp <= iqpt::kAccTableMax && iqpt::sky_variant_exists(opt);
    // overlapped launches may put the sky kernel behind the plain kernel on the launch's stream
    // (iqpt_debug_set_sky_order), so the plain kernel, whose sphere tiles carry the launch's longest chains,
    // is not queued behind it
    const bool sky_deferred = sky && ovl && bind_ovl && c->sky_after;
    if (sky) {
        p.miss = c->d_certain + 2 * (size_t)c->cull_ntx * c->cull_nty;
        if (!c->ev_sky && hipEventCreateWithFlags(&c->ev_sky, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            return iqpt::fail(IQPT_ERR_HIP, "sky kernel event");
        }
        if (!sky_deferred) {
            const hipStream_t ss = ovl ? ls : c->stream;
            if (c->sky_last && c->sky_last != ss) IQPT_HIP(hipStreamWaitEvent(ss, c->ev_sky, 0));
            const bool b0 = bind_ovl && e0 && p.spp > 0;
            if (b0) iqpt::bind_launch_events(e0, nullptr);
            le = iqpt::launch_sky(ss, p, c->d_sky_tiles, c->n_sky_tiles, opt);
            note_kernel(c, iqpt::kTableSky, opt);
            iqpt::bind_launch_events(nullptr, nullptr);
            e0_bound = b0 && le == 0;
            if (le != 0) return iqpt::hip_fail((hipError_t)le, "sky kernel launch");
            IQPT_HIP(hipEventRecord(c->ev_sky, ss));
            c->sky_last = ss;
        }
    }
    if (ovl) {
        st = enqueue_overlapped(c, p, ls, grid, lds, opt, bind_ovl, sky_deferred, e0, e1, e0_bound, e1_bound, le);
        if (st != IQPT_OK) return st;
    } else if (spec) {
        if ((st = enqueue_spec(c, p, spp, opt, pipe_next, e0, e1, e1b, e1_bound, le)) != IQPT_OK) return st;
    } else if (split) {
        if ((st = enqueue_split(c, p, ks, grid, lds, opt, fan_split, le)) != IQPT_OK) return st;
    } else if (anyk) {
        le = iqpt::launch_anyhit(c->stream, p, opt);
        note_kernel(c, iqpt::kTableAnyHit, opt);
    } else {
        le = iqpt::launch_render(c->stream, p, grid, lds, stream_batches, opt);
        note_plain(c, opt);
    }
    c->last_anyk = anyk;
    c->split_last = split;
    c->fan_last = fan_split || spec;
    c->spec_last = spec;
    c->last_ls = ls;
    c->last_ovl = ovl;
    c->last_xcd_lists = (ovl || xcdq) && !spec && !split && !anyk;
    if (tune_slot >= 0) (void)hipEventRecord(c->tune_ev[2 * tune_slot + 1], c->stream);
    if (e1 && !e1_bound) (void)hipEventRecord(e1, ls);
    if (e0 && e1) c->timed.push_back({e0, e1, e1b});
    if (le != 0) return iqpt::hip_fail((hipError_t)le, "render kernel launch");
    c->last_opt = opt;
    std::memcpy(c->last_launch, c->cur_launch, sizeof c->last_launch);
    if (tune_slot >= 0) {
        c->tune_work[tune_slot] = (double)spp * (double)c->npix;
        c->tune_stage = tune_slot + 1;
    }
    c->frame += spp;
    return IQPT_OK;
}
}  // namespace

int iqpt_render(iqpt_ctx* c, uint32_t spp) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    if (!c->have_camera || !c->have_packet) return iqpt::fail(IQPT_ERR_NOT_READY, "camera and packet must be set");
    if (spp == 0) return IQPT_OK;
    int st = use_device(c);
    if (st) return st;
    // launches of at most kAccTableMax samples, so the running-mean table always covers the launch
    // (a pixel's samples are sequential either way: same bits as one launch)
    while (spp > 0) {
        const uint32_t n = std::min(spp, iqpt::kAccTableMax);
        if ((st = render_launch(c, n)) != IQPT_OK) return st;
        spp -= n;
    }
    return IQPT_OK;
}

}  // extern "C"
