// denoiser.hpp — C++ facade of the rasterizer-guided denoiser: iqpt::denoiser over the iqpt_denoise_* C ABI
// (include/denoise/iqpt_denoise.h). iqpt::renderer owns one when renderer_options::denoise is on
// (raster/rasterizer.hpp); the reference has no counterpart.
#pragma once

#include <string>
#include <vector>

#include "denoise/iqpt_denoise.h"
#include "path_tracer.hpp"

namespace iqpt {

struct denoise_options {
    bool enabled = false;
    iqpt_denoise_params params = default_params();
    std::string ppm_path;                        // where the denoised frame goes ("" = none)

    static iqpt_denoise_params default_params() {
        iqpt_denoise_params p{};
        IQPT_THROW_FAILED(iqpt_denoise_default_params(&p));
        return p;
    }
};

class denoiser {
public:
    denoiser(uint32_t width, uint32_t height, int device = 0) : m_width(width), m_height(height) {
        IQPT_THROW_FAILED(iqpt_denoise_create(device, width, height, &m_d));
        m_host_pixels.assign((size_t)width * height, path_tracer::pixel{0, 0, 0, 0});
    }
    ~denoiser() { iqpt_denoise_destroy(m_d); }
    denoiser(const denoiser&) = delete;
    denoiser& operator=(const denoiser&) = delete;

    void set_params(const iqpt_denoise_params& p) { IQPT_THROW_FAILED(iqpt_denoise_set_params(m_d, &p)); }
    // the path tracer's accumulator under the rasterizer's G-buffer, filtered and read back into host_pixels(); the
    // context's camera is the aligned one of the rasterizer's (camera::aligned())
    void frame(iqpt_ctx* ctx, iqpt_raster* raster) {
        IQPT_THROW_FAILED(iqpt_denoise_frame(m_d, ctx, raster));
        IQPT_THROW_FAILED(iqpt_denoise_read(m_d, nullptr, reinterpret_cast<uint8_t*>(m_host_pixels.data())));
        m_frames += 1;
    }
    // the same for a float4 frame already on the device and complete (the temporal result)
    void frame_device(const void* colour_device, iqpt_raster* raster) {
        IQPT_THROW_FAILED(iqpt_raster_gbuffer(raster));
        const void *nz = nullptr, *id = nullptr;
        IQPT_THROW_FAILED(iqpt_raster_gbuffer_device(raster, &nz, &id));
        IQPT_THROW_FAILED(iqpt_denoise_set_guides_device(m_d, nz, id));
        IQPT_THROW_FAILED(iqpt_denoise_run_device(m_d, colour_device));
        IQPT_THROW_FAILED(iqpt_denoise_read(m_d, nullptr, reinterpret_cast<uint8_t*>(m_host_pixels.data())));
        m_frames += 1;
    }
    void read_linear(std::vector<float>& rgba) const {
        rgba.resize((size_t)m_width * m_height * 4);
        IQPT_THROW_FAILED(iqpt_denoise_read(m_d, rgba.data(), nullptr));
    }
    void write_ppm(const std::string& path) const {
        IQPT_THROW_FAILED(iqpt_write_ppm(path.c_str(), m_width, m_height, reinterpret_cast<const uint8_t*>(m_host_pixels.data())));
    }

    const std::vector<path_tracer::pixel>& host_pixels() const { return m_host_pixels; }
    uint64_t frames() const { return m_frames; }
    iqpt_denoise* context() const { return m_d; }

private:
    iqpt_denoise* m_d = nullptr;
    uint32_t m_width, m_height;
    std::vector<path_tracer::pixel> m_host_pixels;
    uint64_t m_frames = 0;
};

}  // namespace iqpt
