// temporal.hpp — C++ facade of temporal reprojection: iqpt::temporal over the iqpt_temporal_* C ABI
// (include/temporal/iqpt_temporal.h). iqpt::renderer owns one when renderer_options::temporal is
// on (raster/rasterizer.hpp); the reference has no counterpart.
#pragma once

#include <cstring>
#include <string>
#include <vector>

#include "path_tracer.hpp"
#include "temporal/iqpt_temporal.h"

namespace iqpt {

struct temporal_options {
    bool enabled = false;
    iqpt_temporal_params params = default_params();
    std::string ppm_path;                        // where the resolved frame goes ("" = none)

    static iqpt_temporal_params default_params() {
        iqpt_temporal_params p{};
        IQPT_THROW_FAILED(iqpt_temporal_default_params(&p));
        return p;
    }
};

class temporal {
public:
    temporal(uint32_t width, uint32_t height, int device = 0) : m_width(width), m_height(height) {
        IQPT_THROW_FAILED(iqpt_temporal_create(device, width, height, &m_t));
        m_host_pixels.assign((size_t)width * height, path_tracer::pixel{0, 0, 0, 0});
    }
    ~temporal() { iqpt_temporal_destroy(m_t); }
    temporal(const temporal&) = delete;
    temporal& operator=(const temporal&) = delete;

    void set_params(const iqpt_temporal_params& p) { IQPT_THROW_FAILED(iqpt_temporal_set_params(m_t, &p)); }
    // a new view from the rasterizer's G-buffer; cam is the camera the rasterizer has (the plain one: the path
    // tracer's is its aligned form), kept for same_view()
    void begin_view(iqpt_raster* raster, const iqpt_camera& cam) {
        IQPT_THROW_FAILED(iqpt_temporal_begin_view_raster(m_t, raster));
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
        IQPT_THROW_FAILED(iqpt_temporal_clear(m_t));
        m_have_view = false;
    }
    // the path tracer's accumulator blended with the view's history, read back into host_pixels()
    void resolve(iqpt_ctx* ctx) {
        IQPT_THROW_FAILED(iqpt_temporal_resolve_ctx(m_t, ctx));
        IQPT_THROW_FAILED(iqpt_temporal_read(m_t, nullptr, reinterpret_cast<uint8_t*>(m_host_pixels.data())));
        m_resolves += 1;
    }
    const void* output_device() const {
        const void* p = nullptr;
        IQPT_THROW_FAILED(iqpt_temporal_output_device(m_t, &p));
        return p;
    }
    void read_linear(std::vector<float>& rgba) const {
        rgba.resize((size_t)m_width * m_height * 4);
        IQPT_THROW_FAILED(iqpt_temporal_read(m_t, rgba.data(), nullptr));
    }
    void write_ppm(const std::string& path) const {
        IQPT_THROW_FAILED(iqpt_write_ppm(path.c_str(), m_width, m_height, reinterpret_cast<const uint8_t*>(m_host_pixels.data())));
    }

    const std::vector<path_tracer::pixel>& host_pixels() const { return m_host_pixels; }
    uint64_t views() const { return m_views; }
    uint64_t resolves() const { return m_resolves; }
    iqpt_temporal* context() const { return m_t; }

private:
    iqpt_temporal* m_t = nullptr;
    uint32_t m_width, m_height;
    std::vector<path_tracer::pixel> m_host_pixels;
    iqpt_camera m_camera{};
    bool m_have_view = false;
    uint64_t m_views = 0, m_resolves = 0;
};

}  // namespace iqpt
