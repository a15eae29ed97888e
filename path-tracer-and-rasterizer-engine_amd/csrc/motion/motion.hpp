// motion.hpp — C++ facade of moving-model reprojection: iqpt::motion over the iqpt_motion_* C ABI
// (include/motion/iqpt_motion.h), header-only; a program that uses it links libiqpt_motion.so and
// libiqpt.so. iqpt::renderer does not own one (§15.6); the reference has no counterpart.
#pragma once

#include <string>
#include <vector>

#include "motion/iqpt_motion.h"
#include "path_tracer.hpp"

namespace iqpt {

class motion {
public:
    struct counts {
        uint64_t guided = 0, valid = 0, moved = 0, moved_valid = 0;
    };

    motion(uint32_t width, uint32_t height, int device = 0) : m_width(width), m_height(height) {
        IQPT_THROW_FAILED(iqpt_motion_create(device, width, height, &m_m));
        m_host_pixels.assign((size_t)width * height, path_tracer::pixel{0, 0, 0, 0});
    }
    ~motion() { iqpt_motion_destroy(m_m); }
    motion(const motion&) = delete;
    motion& operator=(const motion&) = delete;

    static iqpt_temporal_params default_params() {
        iqpt_temporal_params p{};
        IQPT_THROW_FAILED(iqpt_motion_default_params(&p));
        return p;
    }
    void set_params(const iqpt_temporal_params& p) { IQPT_THROW_FAILED(iqpt_motion_set_params(m_m, &p)); }

    // the motion table of a scene change: both scenes have the same meshes and models, in the same order
    static std::vector<iqpt_motion_entry> table(const scene& prev_scene, const scene& cur_scene) {
        const std::vector<iqpt_draw_item> prev = draw_list(prev_scene), cur = draw_list(cur_scene);
        std::vector<iqpt_motion_entry> t(cur.size());
        IQPT_THROW_FAILED(iqpt_motion_table(prev.data(), (uint32_t)prev.size(), cur.data(), (uint32_t)cur.size(), t.data()));
        return t;
    }
    // a new view from the rasterizer's G-buffer (it holds cur_scene and the view's camera), the models having moved
    // from where prev_scene had them
    void begin_view(iqpt_raster* raster, const scene& prev_scene, const scene& cur_scene) {
        const std::vector<iqpt_motion_entry> t = table(prev_scene, cur_scene);
        IQPT_THROW_FAILED(iqpt_motion_begin_view_raster(m_m, raster, t.data(), (uint32_t)t.size()));
        m_views += 1;
    }
    // the same with no model moved: temporal reprojection's begin_view
    void begin_view(iqpt_raster* raster) {
        IQPT_THROW_FAILED(iqpt_motion_begin_view_raster(m_m, raster, nullptr, 0));
        m_views += 1;
    }
    void clear() { IQPT_THROW_FAILED(iqpt_motion_clear(m_m)); }
    // the path tracer's accumulator blended with the view's history, read back into host_pixels()
    void resolve(iqpt_ctx* ctx) {
        IQPT_THROW_FAILED(iqpt_motion_resolve_ctx(m_m, ctx));
        IQPT_THROW_FAILED(iqpt_motion_read(m_m, nullptr, reinterpret_cast<uint8_t*>(m_host_pixels.data())));
        m_resolves += 1;
    }
    counts stats() const {
        counts c;
        IQPT_THROW_FAILED(iqpt_motion_stats(m_m, &c.guided, &c.valid, &c.moved, &c.moved_valid));
        return c;
    }
    const void* output_device() const {
        const void* p = nullptr;
        IQPT_THROW_FAILED(iqpt_motion_output_device(m_m, &p));
        return p;
    }
    void read_linear(std::vector<float>& rgba) const {
        rgba.resize((size_t)m_width * m_height * 4);
        IQPT_THROW_FAILED(iqpt_motion_read(m_m, rgba.data(), nullptr));
    }
    void write_ppm(const std::string& path) const {
        IQPT_THROW_FAILED(iqpt_write_ppm(path.c_str(), m_width, m_height, reinterpret_cast<const uint8_t*>(m_host_pixels.data())));
    }

    const std::vector<path_tracer::pixel>& host_pixels() const { return m_host_pixels; }
    uint64_t views() const { return m_views; }
    uint64_t resolves() const { return m_resolves; }
    iqpt_motion* context() const { return m_m; }

private:
    static std::vector<iqpt_draw_item> draw_list(const scene& s) {
        uint32_t n = 0;
        IQPT_THROW_FAILED(iqpt_scene_draw_list(s.handle(), nullptr, 0, &n));
        std::vector<iqpt_draw_item> items(n);
        if (n) IQPT_THROW_FAILED(iqpt_scene_draw_list(s.handle(), items.data(), n, &n));
        return items;
    }

    iqpt_motion* m_m = nullptr;
    uint32_t m_width, m_height;
    std::vector<path_tracer::pixel> m_host_pixels;
    uint64_t m_views = 0, m_resolves = 0;
};

}  // namespace iqpt
