// iq_checkpoint.cpp — iqpt_checkpoint_save / _load: the whole pixel state in one file.
#include <cstdio>

#include "runtime/iq_ctx.hpp"

using namespace iqpt::rt;

extern "C" {

// (an unnamed namespace inside extern "C": plain names in the symbol table, kept so; see iq_ctx.hpp)
namespace {
// Checkpoint file: header, then accumulator (npix float4), BGRA (npix u32), RNG (6 planes of npix u32).
struct ckpt_header {
    char magic[8];            // "IQPTCKP1"
    uint32_t version;         // 1
    uint32_t width, height;
    uint32_t x0, x1, y0, ystep, nrows;
    int32_t max_depth;
    uint64_t seed;
    uint64_t frame;
    uint64_t rays;
    uint64_t npix;
    uint64_t checksum;        // FNV-1a 64 over the payload
};
constexpr char kCkptMagic[8] = {'I', 'Q', 'P', 'T', 'C', 'K', 'P', '1'};

uint64_t fnv1a(const void* data, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char* b = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < n; ++i) {
        h ^= b[i];
        h *= 1099511628211ull;
    }
    return h;
}
}  // namespace

int iqpt_checkpoint_save(iqpt_ctx* c, const char* path) {
    if (!c || !path) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    int st = enter(c);
    if (st) return st;
    IQPT_HIP(hipStreamSynchronize(c->stream));
    const size_t n = c->npix;
    std::vector<float4_storage> lin(n);
    std::vector<uint32_t> bgra(n), rng(n * 6);
    unsigned long long rays = 0;
    // the file holds the compact row-major order (independent of the device layout)
    if ((st = check_dev_err(c)) != IQPT_OK) return st;     // never persist undefined state
    if ((st = fetch_compact(c, c->d_lin, 4, 1, lin.data())) != IQPT_OK ||
        (st = fetch_compact(c, c->d_rng, 1, 6, rng.data())) != IQPT_OK)
        return st;
    IQPT_HIP(hipMemcpy(bgra.data(), c->d_bgra, n * sizeof(uint32_t), hipMemcpyDeviceToHost));   // compact already
    if ((st = read_rays(c, &rays)) != IQPT_OK) return st;
    ckpt_header h;
    std::memset(&h, 0, sizeof h);
    std::memcpy(h.magic, kCkptMagic, 8);
    h.version = 1;
    h.width = c->width;
    h.height = c->height;
    h.x0 = c->set.x0;
    h.x1 = c->set.x1;
    h.y0 = c->set.y0;
    h.ystep = c->set.ystep;
    h.nrows = c->set.nrows;
    h.max_depth = c->max_depth;
    h.seed = c->seed;
    h.frame = c->frame;
    h.rays = rays;
    h.npix = n;
    uint64_t sum = fnv1a(lin.data(), n * sizeof(float4_storage));
    sum = fnv1a(bgra.data(), n * sizeof(uint32_t), sum);
    h.checksum = fnv1a(rng.data(), n * 6 * sizeof(uint32_t), sum);
    const std::string tmp = std::string(path) + ".tmp";
    FILE* f = std::fopen(tmp.c_str(), "wb");
    if (!f) return iqpt::fail(IQPT_ERR_INVALID_ARG, "cannot open " + tmp);
    bool ok = std::fwrite(&h, sizeof h, 1, f) == 1 &&
              std::fwrite(lin.data(), sizeof(float4_storage), n, f) == n &&
              std::fwrite(bgra.data(), sizeof(uint32_t), n, f) == n &&
              std::fwrite(rng.data(), sizeof(uint32_t), n * 6, f) == n * 6;
    ok = (std::fclose(f) == 0) && ok;
    if (!ok || std::rename(tmp.c_str(), path) != 0) {
        std::remove(tmp.c_str());
        return iqpt::fail(IQPT_ERR_INVALID_ARG, std::string("cannot write ") + path);
    }
    return IQPT_OK;
}

int iqpt_checkpoint_load(iqpt_ctx* c, const char* path) {
    if (!c || !path) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    FILE* f = std::fopen(path, "rb");
    if (!f) return iqpt::fail(IQPT_ERR_INVALID_ARG, std::string("cannot open ") + path);
    ckpt_header h;
    const size_t n = c->npix;
    std::vector<float4_storage> lin(n);
    std::vector<uint32_t> bgra(n), rng(n * 6);
    bool ok = std::fread(&h, sizeof h, 1, f) == 1;
    std::string why;
    if (!ok || std::memcmp(h.magic, kCkptMagic, 8) != 0 || h.version != 1) why = "not an iqpt checkpoint (v1)";
    else if (h.width != c->width || h.height != c->height || h.x0 != c->set.x0 || h.x1 != c->set.x1 ||
             h.y0 != c->set.y0 || h.ystep != c->set.ystep || h.nrows != c->set.nrows || h.npix != n)
        why = "frame size / pixel set differ from the context";
    else if (h.seed != c->seed || h.max_depth != c->max_depth) why = "seed / max_depth differ from the context";
    if (why.empty()) {
        ok = std::fread(lin.data(), sizeof(float4_storage), n, f) == n &&
             std::fread(bgra.data(), sizeof(uint32_t), n, f) == n &&
             std::fread(rng.data(), sizeof(uint32_t), n * 6, f) == n * 6;
        unsigned char extra;
        if (!ok || std::fread(&extra, 1, 1, f) != 0) why = "truncated or oversized checkpoint";
    }
    std::fclose(f);
    if (why.empty()) {
        uint64_t sum = fnv1a(lin.data(), n * sizeof(float4_storage));
        sum = fnv1a(bgra.data(), n * sizeof(uint32_t), sum);
        if (fnv1a(rng.data(), n * 6 * sizeof(uint32_t), sum) != h.checksum) why = "checksum mismatch";
    }
    // the accumulator's w is 0 from iqpt_create on and the kernel stores it as 0 (a whole float4 per
    // pixel): a checkpoint with another w did not come from a context
    if (why.empty())
        for (size_t i = 0; i < n; ++i)
            if (lin[i].w != 0.0f || std::signbit(lin[i].w)) {
                why = "accumulator w is not +0 (the kernel never produces another)";
                break;
            }
    if (!why.empty()) return iqpt::fail(IQPT_ERR_INVALID_ARG, std::string(path) + ": " + why);
    int st = enter(c);
    if (st) return st;
    IQPT_HIP(hipStreamSynchronize(c->stream));
    const unsigned long long rays = h.rays;
    if ((st = store_compact(c, lin.data(), 4, 1, c->d_lin)) != IQPT_OK ||
        (st = store_compact(c, rng.data(), 1, 6, c->d_rng)) != IQPT_OK)
        return st;
    IQPT_HIP(hipMemcpy(c->d_bgra, bgra.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));   // compact order
    {
        std::vector<unsigned long long> slots((size_t)iqpt::kRaySlots * iqpt::kRaySlotStride, 0ull);
        slots[0] = rays;
        IQPT_HIP(hipMemcpy(c->d_rays, slots.data(), slots.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    }
    c->frame = h.frame;
    // the whole pixel state is replaced: a latched kernel error no longer applies
    IQPT_HIP(hipMemset(c->d_ovl_err, 0, sizeof(uint32_t)));
    c->dev_err = 0;
    return IQPT_OK;
}

}  // extern "C"
