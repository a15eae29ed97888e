// svgf.hpp — C++ facade of variance-guided filtering: iqpt::svgf over the iqpt_svgf_* C ABI
// (include/svgf/iqpt_svgf.h). iqpt::renderer owns one when renderer_options::svgf is on
// (raster/rasterizer.hpp); the reference has no counterpart.
#pragma once

#include <cstring>
#include <string>
#include <vector>

#include "path_tracer.hpp"
#include "svgf/iqpt_svgf.h"

namespace iqpt {

struct svgf_options {
    bool enabled = false;
    iqpt_svgf_params params = default_params();
    std::string ppm_path;                        // where the filtered frame goes ("" = none)

    static iqpt_svgf_params default_params() {
        iqpt_svgf_params p{};
        IQPT_THROW_FAILED(iqpt_svgf_default_params(&p));
        return p;
    }
};

class svgf {
public:
    svgf(uint32_t width, uint32_t height, int device = 0) : m_width(width), m_height(height) {
        IQPT_THROW_FAILED(iqpt_svgf_create(device, width, height, &m_s));
        m_host_pixels.assign((size_t)width * height, path_tracer::pixel{0, 0, 0, 0});
    }
    ~svgf() { iqpt_svgf_destroy(m_s); }
    svgf(const svgf&) = delete;
    svgf& operator=(const svgf&) = delete;

    void set_params(const iqpt_svgf_params& p) { IQPT_THROW_FAILED(iqpt_svgf_set_params(m_s, &p)); }
    // a new view from the rasterizer's G-buffer; cam is the camera the rasterizer has (the plain one: the path
    // tracer's is its aligned form), kept for same_view()
    void begin_view(iqpt_raster* raster, const iqpt_camera& cam) {
        IQPT_THROW_FAILED(iqpt_svgf_begin_view_raster(m_s, raster));
        m_camera = cam;
        m_have_view = true;
        m_views += 1;
    }
    bool have_view() const { return m_have_view; }
    // whether cam has the matrices of the view begun last
    bool same_view(const iqpt_camera& cam) const {
        return m_have_view && std::memcmp(cam.view, m_camera.view, sizeof cam.view) == 0 &&
               std::memcmp(cam.projection, m_camera.projection, sizeof cam.projection) == 0 &&
               std::memcmp(cam.inv_view, m_camera.inv_view, sizeof cam.inv_view) == 0 &&
               std::memcmp(cam.inv_proj, m_camera.inv_proj, sizeof cam.inv_proj) == 0;
    }
    void clear() {
        IQPT_THROW_FAILED(iqpt_svgf_clear(m_s));
        m_have_view = false;
    }
    // the path tracer's accumulator through both histories, the variance estimate and the filter, read back into
    // host_pixels()
    void resolve(iqpt_ctx* ctx) {
        IQPT_THROW_FAILED(iqpt_svgf_resolve_ctx(m_s, ctx));
        IQPT_THROW_FAILED(iqpt_svgf_read(m_s, nullptr, reinterpret_cast<uint8_t*>(m_host_pixels.data())));
        m_resolves += 1;
    }
    void read_linear(std::vector<float>& rgba) const {
        rgba.resize((size_t)m_width * m_height * 4);
        IQPT_THROW_FAILED(iqpt_svgf_read(m_s, rgba.data(), nullptr));
    }
    // the colour history's result and c_0, whose w is the variance estimate
    void read_stages(std::vector<float>& temporal_rgba, std::vector<float>& variance_rgba) const {
        temporal_rgba.resize((size_t)m_width * m_height * 4);
        variance_rgba.resize((size_t)m_width * m_height * 4);
        IQPT_THROW_FAILED(iqpt_svgf_read_stages(m_s, temporal_rgba.data(), variance_rgba.data()));
    }
    void write_ppm(const std::string& path) const {
        IQPT_THROW_FAILED(iqpt_write_ppm(path.c_str(), m_width, m_height, reinterpret_cast<const uint8_t*>(m_host_pixels.data())));
    }

    const std::vector<path_tracer::pixel>& host_pixels() const { return m_host_pixels; }
    uint64_t views() const { return m_views; }
    uint64_t resolves() const { return m_resolves; }
    iqpt_svgf* context() const { return m_s; }

private:
    iqpt_svgf* m_s = nullptr;
    uint32_t m_width, m_height;
    std::vector<path_tracer::pixel> m_host_pixels;
    iqpt_camera m_camera{};
    bool m_have_view = false;
    uint64_t m_views = 0, m_resolves = 0;
};

}  // namespace iqpt
