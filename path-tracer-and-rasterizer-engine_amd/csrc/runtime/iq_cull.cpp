// iq_cull.cpp — what is rebuilt after a camera or packet change: the kOptCull tile masks, lists and
// tile orders, the split set and its per-pixel split, and the camera launch constants.
#include "iq_interval.h"
#include "runtime/iq_ctx.hpp"

using namespace iqpt::rt;

namespace iqpt::rt {
void free_split(iqpt_ctx* c) {
    for (uint32_t** b : {&c->d_split, &c->d_sp_st, &c->d_run_st, &c->d_chunks}) dev_free(*b);
    for (float4_storage** b : {&c->d_sp_acc, &c->d_res}) dev_free(*b);
    dev_free(c->d_nres);
    for (uint32_t** b : {&c->d_chain_pix, &c->d_fan_tiles}) dev_free(*b);
    dev_free(c->d_fan_lanes);
    c->n_chain_pix = c->n_fan_tiles = 0;
    c->spec_rho_valid = false;           // a new pixel list: no chain history, no plan
    c->spec_plan_n = 0;
    c->spec_rho_pending = false;
    c->n_split_tiles = c->n_anchor = 0;
    c->res_slots = 0;
}
}  // namespace iqpt::rt

namespace {
// Chain launches with the fan kernel: which pixels of the split tiles can reach a sphere at all. The
// interval bundle of iq_interval.h (the same RN operation chain as the kernel's camera ray and sphere
// test, compiled for the host with contraction off) is evaluated per pixel over its jitter square: a
// pixel whose bundle rejects every sphere ends every sample on its first ray (every triangle is emissive
// under the reference's materials) and goes to the fan kernel with its tile's triangle mask; the rest
// are the chain kernel's. Without a material table and with at most 64 spheres (otherwise every pixel
// of a split tile stays with the chain kernel).
int build_pixel_split(iqpt_ctx* c, const std::vector<uint32_t>& anchor, const std::vector<uint32_t>& split,
                      const uint32_t* sp_pix) {
    // with the sky kernel on (sky_active), certain-miss pixels are its own: the fan kernel's lanes exclude them,
    // and tiles left with no lane leave its list
    std::vector<uint32_t> chain_pix, fan_tiles;
    std::vector<uint64_t> fan_lanes;
    const bool sky = c->sky_active && c->h_miss.size() == (size_t)c->cull_ntx * c->cull_nty;
    for (uint32_t t : anchor) {
        const uint64_t own = sky ? ~c->h_miss[t] : ~0ull;
        const uint32_t tx = t % c->cull_ntx, ty = t / c->cull_ntx;
        const uint32_t npt = std::min(iqpt::kCullTile, c->ncols - tx * iqpt::kCullTile) *
                             std::min(iqpt::kCullTile, c->set.nrows - ty * iqpt::kCullTile);
        if (own & (npt == 64u ? ~0ull : ((1ull << npt) - 1ull))) {
            fan_tiles.push_back(t);
            fan_lanes.push_back(own);
        }
    }
    const bool per_pixel = !c->d_mats && c->h_sph.size() == c->nsph && c->nsph <= 64;
    iqiv::camera_in ci;
    ci.width = c->width;
    ci.height = c->height;
    ci.rcp_width = 0.0f;
    ci.rcp_height = 0.0f;
    ci.inv_proj = c->cam.inv_proj;
    ci.inv_view = c->cam.inv_view;
    uint32_t cc = 0;
    cam_constants(c->cam, &cc, &ci.near_rw, &ci.far_rw);
    ci.cam_const = (int)cc;
    for (size_t st = 0; st < split.size(); ++st) {
        uint64_t lanes = 0;
        for (uint32_t i = 0; i < iqpt::kQueueChunk; ++i) {
            const uint32_t pix = sp_pix[st * iqpt::kQueueChunk + i];
            if (pix == ~0u) continue;
            // a certain miss is the sky kernel's whenever it runs (also without the per-pixel test below:
            // ADVICE r4, a resident scene of more than 64 spheres put them in the spec / chain list as well)
            if (sky && ((c->h_miss[split[st]] >> i) & 1ull)) continue;
            bool sphere = !per_pixel;
            if (per_pixel) {
                uint32_t col, row;
                iqpt::tile_decode(pix, c->ncols, c->set.nrows, &col, &row);
                const uint32_t x = c->set.x0 + col, y = c->set.y0 + row * c->set.ystep;
                const iqiv::bundle b = iqiv::camera_bundle(ci, x, x, y, y);
                for (uint32_t k = 0; k < c->nsph && !sphere; ++k) {
                    const float ctr[3] = {c->h_sph[k].x, c->h_sph[k].y, c->h_sph[k].z};
                    sphere = !(b.ok && iqiv::sphere_culled(b, ctr, c->h_sph[k].w));
                }
            }
            if (sphere) {
                chain_pix.push_back(pix);
            } else {
                lanes |= 1ull << i;
            }
        }
        if (sky) lanes &= ~c->h_miss[split[st]];
        if (lanes) {
            fan_tiles.push_back(split[st]);
            fan_lanes.push_back(lanes);
        }
    }
    if (!chain_pix.empty()) {
        if (hipMalloc(&c->d_chain_pix, chain_pix.size() * sizeof(uint32_t)) != hipSuccess)
            return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "chain pixel list");
        IQPT_HIP(hipMemcpy(c->d_chain_pix, chain_pix.data(), chain_pix.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (!fan_tiles.empty()) {
        if (hipMalloc(&c->d_fan_tiles, fan_tiles.size() * sizeof(uint32_t)) != hipSuccess ||
            hipMalloc(&c->d_fan_lanes, fan_lanes.size() * sizeof(uint64_t)) != hipSuccess)
            return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "fan tile list");
        IQPT_HIP(hipMemcpy(c->d_fan_tiles, fan_tiles.data(), fan_tiles.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        IQPT_HIP(hipMemcpy(c->d_fan_lanes, fan_lanes.data(), fan_lanes.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    c->n_chain_pix = (uint32_t)chain_pix.size();
    c->n_fan_tiles = (uint32_t)fan_tiles.size();
    return IQPT_OK;
}

// The split set of kOptSplit: the tiles whose camera rays may scatter — a sphere
// candidate in the masks under the reference's materials (every triangle is emissive), any candidate
// with a material table — in queue order, and the other tiles' queue order. Slot sp of the split set
// is pixel sp % 64 of split tile sp / 64 (tile-major storage index, ~0u past a partial tile's end).
int build_split(iqpt_ctx* c, const std::vector<uint32_t>& order, const std::vector<uint32_t>& cnt) {
    free_split(c);
    const uint32_t ntiles = (uint32_t)order.size();
    std::vector<uint32_t> anchor, split;
    for (uint32_t t : order) {
        const bool scatters = iqpt::kSplitAllTiles ||
                              (c->d_mats ? (cnt[t] + cnt[ntiles + t]) > 0 : cnt[ntiles + t] > 0);
        (scatters ? split : anchor).push_back(t);
    }
    if (anchor.empty() && split.empty()) return IQPT_OK;
    // (no split tile: the anchored list alone, for fan launches; every split launch needs split tiles)
    const size_t ns = split.size() * (size_t)iqpt::kQueueChunk;
    if (ns >= (1ull << 31)) return IQPT_OK;
    std::vector<uint32_t> host(anchor.size() + split.size() + 5 * ns, 0u);
    std::copy(anchor.begin(), anchor.end(), host.begin());
    std::copy(split.begin(), split.end(), host.begin() + anchor.size());
    uint32_t* sp_pix = host.data() + anchor.size() + split.size();
    for (size_t st = 0; st < split.size(); ++st) {
        const uint32_t t = split[st];
        const uint32_t tx = t % c->cull_ntx, ty = t / c->cull_ntx;
        const uint32_t th = std::min(iqpt::kCullTile, c->set.nrows - ty * iqpt::kCullTile);
        const uint32_t tw = std::min(iqpt::kCullTile, c->ncols - tx * iqpt::kCullTile);
        const uint32_t first = ty * iqpt::kCullTile * c->ncols + tx * iqpt::kCullTile * th;
        for (uint32_t i = 0; i < iqpt::kQueueChunk; ++i)
            sp_pix[st * iqpt::kQueueChunk + i] = i < tw * th ? first + i : ~0u;
    }
    if (hipMalloc(&c->d_split, host.size() * sizeof(uint32_t)) != hipSuccess ||
        (ns && hipMalloc(&c->d_sp_st, 6 * ns * sizeof(uint32_t)) != hipSuccess) ||
        (ns && hipMalloc(&c->d_sp_acc, ns * sizeof(float4_storage)) != hipSuccess)) {
        free_split(c);
        return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "split buffers");
    }
    IQPT_HIP(hipMemcpy(c->d_split, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->n_anchor = (uint32_t)anchor.size();
    c->n_split_tiles = (uint32_t)split.size();
    return build_pixel_split(c, anchor, split, sp_pix);
}
}  // namespace

namespace iqpt::rt {
// (Re)build the kOptCull tile masks of the current camera and packet on the context's stream.
constexpr uint64_t kListBudget = 1ull << 26;   // candidate-list entries (256 MB)

int build_cull(iqpt_ctx* c) {
    const uint32_t ntp = (c->ntri + 1) / 2, nsp = (c->nsph + 1) / 2;
    c->cull_ntx = (c->ncols + iqpt::kCullTile - 1) / iqpt::kCullTile;
    c->cull_nty = (c->set.nrows + iqpt::kCullTile - 1) / iqpt::kCullTile;
    c->cull_wt = (ntp + 31) / 32;
    c->cull_stride = c->cull_wt + (nsp + 31) / 32;
    const size_t words = (size_t)c->cull_ntx * c->cull_nty * c->cull_stride;
    if (words == 0) {
        c->cull_valid = true;
        return IQPT_OK;
    }
    if (words > c->cull_cap) {
        if (c->d_cull) {
            IQPT_HIP(hipStreamSynchronize(c->stream));
            (void)hipFree(c->d_cull);
            c->d_cull = nullptr;
            c->cull_cap = 0;
        }
        if (hipMalloc(&c->d_cull, words * sizeof(uint32_t)) != hipSuccess)
            return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "cull masks");
        c->cull_cap = words;
    }
    iqpt::kbin b;
    std::memset(&b, 0, sizeof b);
    b.width = c->width;
    b.height = c->height;
    b.x0 = c->set.x0;
    b.ncols = c->ncols;
    b.y0 = c->set.y0;
    b.ystep = c->set.ystep;
    b.nrows = c->set.nrows;
    std::memcpy(b.inv_proj, c->cam.inv_proj, sizeof b.inv_proj);
    std::memcpy(b.inv_view, c->cam.inv_view, sizeof b.inv_view);
    cam_constants(c->cam, &b.cam_const, &b.cam_near_rw, &b.cam_far_rw);
    b.tris = c->d_tris;
    b.spheres = c->d_sph;
    b.ntri = c->ntri;
    b.nsph = c->nsph;
    b.ntx = c->cull_ntx;
    b.nty = c->cull_nty;
    b.wt = c->cull_wt;
    b.stride = c->cull_stride;
    b.cull = c->d_cull;
    const int le = iqpt::launch_bin(c->stream, b);
    if (le != 0) return iqpt::hip_fail((hipError_t)le, "cull binning kernel");
    const uint32_t ntiles = c->cull_ntx * c->cull_nty;
    // certain pixels (iq_interval.h tri_certain): only under the reference's materials (every triangle
    // emissive) and for scenes resident in LDS. In a streamed scene a lane that leaves a certain pixel takes
    // a pixel of the next tile, so waves hold two tiles and their LDS batches test the union of both tiles'
    // candidates: C4 +66 % per launch whether the pixels are folded in the refill or by a kernel of their own
    // (profiles/r03/ab_certain.json, ab_streamed_certain_fold_rejected.json)
    // per tile: candidate triangle pairs and sphere pairs (the queue order's cost and the lists' sizes), read
    // back at once: the device buffer is freed before any later step can return early
    std::vector<uint32_t> cnt(2 * (size_t)ntiles);
    {
        uint32_t* d_cnt = nullptr;
        IQPT_HIP(hipMalloc(&d_cnt, 2 * (size_t)ntiles * sizeof(uint32_t)));
        const int lcnt = iqpt::launch_tile_count(c->stream, c->d_cull, ntiles, c->cull_wt, c->cull_stride, d_cnt,
                                                 d_cnt + ntiles);
        hipError_t e = lcnt ? (hipError_t)lcnt : hipMemcpyAsync(cnt.data(), d_cnt, cnt.size() * sizeof(uint32_t),
                                                                hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        (void)hipFree(d_cnt);
        if (e != hipSuccess) return iqpt::hip_fail(e, "tile counts");
    }
    c->certain_valid = false;
    c->sky_active = false;
    c->h_miss.clear();
    dev_free(c->d_certain);
    std::vector<uint32_t> certain;
    const uint64_t resident_bytes = (uint64_t)ntp * iqpt::kTriPairFloat4 * 16u + (uint64_t)nsp * iqpt::kSphPairFloat4 * 16u;
    dev_free(c->d_sky_tiles);
    c->n_sky_tiles = 0;
    c->n_sky_pixels = 0;
    // (resident scenes: streamed ones with certain pixels and the sky kernel — their BVH-primary variants, which
    // have no LDS batches — measured slower on C4 in round 5, 135 -> 161 ms)
    if (!c->d_mats && ntiles > 0 && resident_bytes <= iqpt::kLdsResidentBytes) {
        // per tile: the certain-hit mask by the tile rule (2 words), then after all tiles the certain-miss masks,
        // the beside-a-sphere hit masks and the folded hit masks (2 words each: iqpt::kCertainPlanes planes)
        const size_t ncw = 2 * (size_t)iqpt::kCertainPlanes * ntiles;
        if (hipMalloc(&c->d_certain, ncw * sizeof(uint32_t)) != hipSuccess)
            return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "certain pixel masks");
        const int lc = iqpt::launch_certain(c->stream, b, c->d_certain);
        if (lc != 0) return iqpt::hip_fail((hipError_t)lc, "certain pixel kernel");
        certain.resize(ncw);
        IQPT_HIP(hipMemcpyAsync(certain.data(), c->d_certain, ncw * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        IQPT_HIP(hipStreamSynchronize(c->stream));
        c->certain_valid = true;
        // the tiles holding certain-miss pixels: iqpt_sky_kernel's work list (one wave each)
        std::vector<uint32_t> sky;
        c->h_miss.assign(ntiles, 0ull);
        for (uint32_t t = 0; t < ntiles; ++t) {
            const uint64_t m = (uint64_t)certain[2 * (size_t)ntiles + 2 * (size_t)t] |
                               ((uint64_t)certain[2 * (size_t)ntiles + 2 * (size_t)t + 1] << 32);
            c->h_miss[t] = m;
            if (m) {
                sky.push_back(t);
                c->n_sky_pixels += (uint32_t)__builtin_popcountll(m);
            }
        }
        if (!sky.empty()) {
            if (hipMalloc(&c->d_sky_tiles, sky.size() * sizeof(uint32_t)) != hipSuccess)
                return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "sky tile list");
            IQPT_HIP(hipMemcpy(c->d_sky_tiles, sky.data(), sky.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            c->n_sky_tiles = (uint32_t)sky.size();
        }
    }
    c->sky_active = c->sky_on && c->certain_on && c->certain_valid && c->n_sky_tiles > 0;
    if (!c->sky_active) c->h_miss.clear();
    // queue order over tiles (a queue chunk is one tile): most expensive first, so the pixels that set
    // the end of the launch are cheap ones. Cost = candidate triangle pairs + 8 x candidate sphere pairs
    // (a camera ray that can hit a sphere starts an Oren-Nayar path: more rays and the scatter shading).
    std::vector<uint32_t> cost(ntiles);
    for (uint32_t t = 0; t < ntiles; ++t) cost[t] = cnt[t] + 8u * cnt[ntiles + t];
    // a certain pixel costs a fold of its samples: a tile's cost scales with its uncertain pixels (fully
    // certain tiles last in the order)
    if (c->certain_valid && c->certain_on)
        for (uint32_t t = 0; t < ntiles; ++t) {
            const uint32_t tx = t % c->cull_ntx, ty = t / c->cull_ntx;
            const uint32_t npt = std::min(iqpt::kCullTile, c->ncols - tx * iqpt::kCullTile) *
                                 std::min(iqpt::kCullTile, c->set.nrows - ty * iqpt::kCullTile);
            // (the folded hit mask: what the kernels fold)
            const uint32_t* hit = certain.data() + 2 * (size_t)iqpt::kCertainFolded * ntiles;
            uint32_t nc = (uint32_t)__builtin_popcountll((uint64_t)hit[2 * (size_t)t] | ((uint64_t)hit[2 * (size_t)t + 1] << 32));
            // certain misses leave the plain kernel's work too when the sky kernel takes them
            if (c->sky_on)
                nc += (uint32_t)__builtin_popcountll((uint64_t)certain[2 * (size_t)ntiles + 2 * (size_t)t] |
                                                     ((uint64_t)certain[2 * (size_t)ntiles + 2 * (size_t)t + 1] << 32));
            cost[t] = (uint32_t)(((uint64_t)cost[t] * (npt - std::min(nc, npt)) + npt - 1) / npt);
        }
    // candidate lists for the streamed kernel (pairs of a tile without scanning its mask words): only
    // worth building where the masks are long; skipped when they would exceed the list budget
    dev_free(c->d_list);
    dev_free(c->d_pmask);
    c->pmask_tiles = 0;
    c->pmask_all = false;
    c->list_max = 0;
    const bool want_lists = c->cull_stride > 8;
    uint64_t total = 0;
    std::vector<uint32_t> off(2 * ((size_t)ntiles + 1));
    for (uint32_t t = 0; t < ntiles; ++t) {
        off[t] = (uint32_t)std::min<uint64_t>(total, 0xffffffffull);
        total += cnt[t];
    }
    off[ntiles] = (uint32_t)std::min<uint64_t>(total, 0xffffffffull);
    for (uint32_t t = 0; t < ntiles; ++t) {
        off[ntiles + 1 + t] = (uint32_t)std::min<uint64_t>(total, 0xffffffffull);
        total += cnt[ntiles + t];
    }
    off[2 * (size_t)ntiles + 1] = (uint32_t)std::min<uint64_t>(total, 0xffffffffull);
    if (want_lists && total > 0 && total <= kListBudget) {
        uint32_t* d_off = nullptr;
        bool ok = hipMalloc(&c->d_list, (total + off.size()) * sizeof(uint32_t)) == hipSuccess;
        if (ok) {
            d_off = c->d_list + total;
            ok = hipMemcpyAsync(d_off, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                                c->stream) == hipSuccess &&
                 iqpt::launch_tile_list(c->stream, c->d_cull, ntiles, c->cull_wt, c->cull_stride, d_off,
                                        d_off + ntiles + 1, c->d_list) == 0 &&
                 // any-hit scenes: the lists most-hit pairs first (the launch's loop leaves at the wave's last hit)
                 (!(c->nsph == 0 && !c->d_mats && c->anyhit_on) ||
                  iqpt::launch_tile_list_order(c->stream, b, d_off, c->d_list) == 0) &&
                 hipStreamSynchronize(c->stream) == hipSuccess;
        }
        if (!ok) {
            dev_free(c->d_list);
        } else {
            c->list_total = total;
            // per-pixel masks over the triangle lists (a miss ray near a silhouette walks only the entries its
            // own pixel may meet); without them (allocation or launch failure) the kernel walks whole lists
            // compact: 64 words per 32 entries of each tile with at most kPixMaskMax entries, after the offsets
            std::vector<uint32_t> pm_off((size_t)ntiles + 1);
            uint64_t pm_words = 0;
            for (uint32_t t = 0; t < ntiles; ++t) {
                pm_off[t] = (uint32_t)pm_words;          // (used only when every offset fits: `fits` below)
                if (cnt[t] <= iqpt::kPixMaskMax) pm_words += 64u * (((uint64_t)cnt[t] + 31u) / 32u);
            }
            pm_off[ntiles] = (uint32_t)pm_words;
            const bool fits = (uint64_t)ntiles + 1 + pm_words < 0xffffffffull;
            if (c->pmask_mode != 0 && fits &&
                hipMalloc(&c->d_pmask, ((size_t)ntiles + 1 + pm_words + 2 * (size_t)ntiles) * sizeof(uint32_t)) ==
                    hipSuccess &&
                !(hipMemcpyAsync(c->d_pmask, pm_off.data(), pm_off.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                                 c->stream) == hipSuccess &&
                  iqpt::launch_pixel_mask(c->stream, b, d_off, c->d_list, c->d_pmask, c->d_pmask + ntiles + 1,
                                          c->d_pmask + ntiles + 1 + pm_words) == 0 &&
                  hipStreamSynchronize(c->stream) == hipSuccess)) {
                (void)hipFree(c->d_pmask);
                c->d_pmask = nullptr;
            }
            if (c->d_pmask) {
                c->pmask_words = pm_words;
                c->pmask_all = true;
                for (uint32_t t = 0; t < ntiles; ++t) {
                    c->list_max = std::max(c->list_max, cnt[t]);
                    c->pmask_tiles += (cnt[t] > 0 && cnt[t] <= iqpt::kPixMaskMax) ? 1u : 0u;
                    c->pmask_all = c->pmask_all && cnt[t] <= iqpt::kAnyMaxEntries && cnt[ntiles + t] == 0;
                }
            }
        }
    }
    std::vector<uint32_t> order(ntiles);
    for (uint32_t t = 0; t < ntiles; ++t) order[t] = t;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
    if (!c->d_tile_order && hipMalloc(&c->d_tile_order, (size_t)ntiles * sizeof(uint32_t)) != hipSuccess)
        return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "tile order");
    IQPT_HIP(hipMemcpy(c->d_tile_order, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    // kOptOverlap: the cost order dealt round-robin to the 8 XCDs (each list in cost order)
    {
        std::vector<uint32_t> xo;
        xo.reserve(ntiles);
        for (uint32_t x = 0; x < 8; ++x) {
            c->xcd_off[x] = (uint32_t)xo.size();
            for (uint32_t r = x; r < ntiles; r += 8) xo.push_back(order[r]);
        }
        c->xcd_off[8] = (uint32_t)xo.size();
        if (!c->d_xcd_order && hipMalloc(&c->d_xcd_order, (size_t)ntiles * sizeof(uint32_t)) != hipSuccess)
            return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "XCD tile order");
        if (!c->d_tile_done && hipMalloc(&c->d_tile_done, (size_t)ntiles * sizeof(uint32_t)) != hipSuccess)
            return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "tile completion counts");

        IQPT_HIP(hipMemcpy(c->d_xcd_order, xo.data(), xo.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        c->ovl_zero = true;
        // streamed scenes' bands: rows of tiles in bands of kXcdBandRows, band b to XCD b mod 8, in tile order
        constexpr uint32_t kXcdBandRows = 4;
        const uint32_t ntx = c->cull_ntx, nty = (ntiles + ntx - 1) / ntx;
        std::vector<uint32_t> xb;
        xb.reserve(ntiles);
        for (uint32_t x = 0; x < 8; ++x) {
            c->xcd_band_off[x] = (uint32_t)xb.size();
            for (uint32_t b = x; b * kXcdBandRows < nty; b += 8)
                for (uint32_t ty = b * kXcdBandRows; ty < std::min(nty, (b + 1) * kXcdBandRows); ++ty)
                    for (uint32_t tx = 0; tx < ntx; ++tx)
                        if (ty * ntx + tx < ntiles) xb.push_back(ty * ntx + tx);
        }
        c->xcd_band_off[8] = (uint32_t)xb.size();
        if (!c->d_xcd_band && hipMalloc(&c->d_xcd_band, (size_t)ntiles * sizeof(uint32_t)) != hipSuccess)
            return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "XCD tile bands");
        IQPT_HIP(hipMemcpy(c->d_xcd_band, xb.data(), xb.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    c->split_last = false;
    int st = build_split(c, order, cnt);
    if (st != IQPT_OK) return st;
    c->cull_valid = true;
    return IQPT_OK;
}

// w of the unprojected near/far points is a launch constant when the perspective row of the
// inverse projection is (0, 0, m23, m33) with finite non-zero m23, m33 (camera_ray).
void cam_constants(const iqpt_camera& cam, uint32_t* is_const, float* near_rw, float* far_rw) {
    const float* P = cam.inv_proj;
    const float wf = P[11] + P[15];
    const bool fin = std::isfinite(P[11]) && std::isfinite(P[15]) && std::isfinite(wf);
    *is_const = 0;
    *near_rw = 0.0f;
    *far_rw = 0.0f;
    if (P[3] == 0.0f && P[7] == 0.0f && fin && P[11] != 0.0f && P[15] != 0.0f && wf != 0.0f) {
        *is_const = 1;
        *near_rw = 1.0f / P[15];
        *far_rw = 1.0f / wf;
    }
}

// kOptCamAxis (camera_ray_axis in iqpt_kernels.hip): the zero pattern of a pitch-only camera under a
// standard perspective inverse, no -0 among the chains' last addends, every entry finite,
// kOptCamConst's constant w, and — from the interval bundle of every camera ray of the frame
// (iq_interval.h) — normalize3's zero branch never taken and |far - near| < 2^100. Fills the 16
// launch constants; false when the camera does not qualify.
bool cam_axis_constants(const iqpt_camera& cam, float* k) {
    const float* P = cam.inv_proj;
    const float* V = cam.inv_view;
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(P[i]) || !std::isfinite(V[i])) return false;
    uint32_t cc = 0;
    float nrw = 0.0f, frw = 0.0f;
    cam_constants(cam, &cc, &nrw, &frw);
    if (!cc || !std::isfinite(nrw) || !std::isfinite(frw)) return false;
    for (int i : {1, 2, 4, 6, 8, 9})
        if (P[i] != 0.0f) return false;
    for (int i : {1, 2, 4, 8})
        if (V[i] != 0.0f) return false;
    for (float last : {P[12], P[13], P[14], V[12], V[13], V[14]})
        if (last == 0.0f && std::signbit(last)) return false;
    if (cam.width == 0 || cam.height == 0) return false;
    iqiv::camera_in ci;
    ci.width = cam.width;
    ci.height = cam.height;
    ci.rcp_width = 0.0f;
    ci.rcp_height = 0.0f;
    ci.inv_proj = P;
    ci.inv_view = V;
    ci.cam_const = 1;
    ci.near_rw = nrw;
    ci.far_rw = frw;
    const iqiv::bundle b = iqiv::camera_bundle(ci, 0, cam.width - 1, 0, cam.height - 1);
    if (!b.ok || !(b.len.hi < 0x1p100f)) return false;
    // unprojected z of the near / far point (camera_ndc's chain; its zero terms only change the
    // sign of a zero inner sum, which the last addend P[14] (not -0) absorbs), divided by w
    const float zn = (((0.0f + 0.0f) + 0.0f * P[10]) + P[14]) * nrw;
    const float zf = (((0.0f + 0.0f) + 1.0f * P[10]) + P[14]) * frw;
    const float vals[16] = {P[0], P[5], P[12], P[13], nrw, frw, V[0], V[12], V[5], V[6], V[13], V[14],
                            zn * V[9], zf * V[9], zn * V[10], zf * V[10]};
    for (int i = 0; i < 16; ++i) {
        if (!std::isfinite(vals[i])) return false;
        k[i] = vals[i];
    }
    return true;
}
}  // namespace iqpt::rt
