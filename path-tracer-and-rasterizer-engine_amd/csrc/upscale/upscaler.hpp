// upscaler.hpp — C++ facade of guided upsampling: iqpt::upscaler over the iqpt_upscale_* C ABI
// (include/upscale/iqpt_upscale.h). iqpt::renderer does not own one: its two engines share one
// camera size (§14 "Not done"); the reference has no counterpart.
#pragma once

#include <string>
#include <vector>

#include "path_tracer.hpp"
#include "upscale/iqpt_upscale.h"

namespace iqpt {

class upscaler {
public:
    struct counts {
        uint64_t guided = 0, widened = 0, unguided = 0;
    };

    // width x height is the full frame; the path tracer's is (width / factor) x (height / factor)
    upscaler(uint32_t width, uint32_t height, uint32_t factor, int device = 0) : m_width(width), m_height(height), m_factor(factor) {
        IQPT_THROW_FAILED(iqpt_upscale_create(device, width, height, factor, &m_u));
        m_host_pixels.assign((size_t)width * height, path_tracer::pixel{0, 0, 0, 0});
    }
    ~upscaler() { iqpt_upscale_destroy(m_u); }
    upscaler(const upscaler&) = delete;
    upscaler& operator=(const upscaler&) = delete;

    static iqpt_upscale_params default_params() {
        iqpt_upscale_params p{};
        IQPT_THROW_FAILED(iqpt_upscale_default_params(&p));
        return p;
    }

    void set_params(const iqpt_upscale_params& p) { IQPT_THROW_FAILED(iqpt_upscale_set_params(m_u, &p)); }
    // the lo path tracer's accumulator under the two rasterizers' G-buffers, upsampled and read back into
    // host_pixels(); the context's camera is the aligned one of the lo rasterizer's (camera::aligned(), DESIGN.md
    // §9.7), the two rasterizers' are plain
    void frame(iqpt_ctx* ctx, iqpt_raster* raster_lo, iqpt_raster* raster_hi) {
        IQPT_THROW_FAILED(iqpt_upscale_frame(m_u, ctx, raster_lo, raster_hi));
        IQPT_THROW_FAILED(iqpt_upscale_read(m_u, nullptr, reinterpret_cast<uint8_t*>(m_host_pixels.data())));
        m_frames += 1;
    }
    void read_linear(std::vector<float>& rgba) const {
        rgba.resize((size_t)m_width * m_height * 4);
        IQPT_THROW_FAILED(iqpt_upscale_read(m_u, rgba.data(), nullptr));
    }
    // the float4 result on the device, complete: what a denoiser's frame_device of the full size takes
    const void* output_device() const {
        const void* p = nullptr;
        IQPT_THROW_FAILED(iqpt_upscale_output_device(m_u, &p));
        return p;
    }
    counts stats() const {
        counts c;
        IQPT_THROW_FAILED(iqpt_upscale_stats(m_u, &c.guided, &c.widened, &c.unguided));
        return c;
    }
    void write_ppm(const std::string& path) const {
        IQPT_THROW_FAILED(iqpt_write_ppm(path.c_str(), m_width, m_height, reinterpret_cast<const uint8_t*>(m_host_pixels.data())));
    }

    const std::vector<path_tracer::pixel>& host_pixels() const { return m_host_pixels; }
    uint32_t width() const { return m_width; }
    uint32_t height() const { return m_height; }
    uint32_t factor() const { return m_factor; }
    uint64_t frames() const { return m_frames; }
    iqpt_upscale* context() const { return m_u; }

private:
    iqpt_upscale* m_u = nullptr;
    uint32_t m_width, m_height, m_factor;
    std::vector<path_tracer::pixel> m_host_pixels;
    uint64_t m_frames = 0;
};

}  // namespace iqpt
