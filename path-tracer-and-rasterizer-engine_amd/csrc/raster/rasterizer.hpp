// rasterizer.hpp — C++ facade of the second engine: iqpt::rasterizer (IoniqRE/rasterizer.h) over the
// iqpt_raster_* C ABI and iqpt::renderer (IoniqRE/renderer.h:14-49, renderer.cu:18-78), which owns both
// engines behind renderer_template and switches between them at begin_frame.
#pragma once

#include <string>
#include <vector>

#include "path_tracer.hpp"
#include "raster/iqpt_raster.h"

namespace iqpt {

struct rasterizer_options {
    int device = 0;
    uint32_t samples = 4;                        // rasterizer.cu: m_samples
    std::string ppm_path;                        // headless present target ("" = none)
};

class rasterizer : public renderer_template {
public:
    static void init(camera* cam, const rasterizer_options& opt = rasterizer_options());
    static void shutdown();
    static rasterizer* get();

    void begin_frame() override;                 // the clear is part of the draw (rasterizer.cu:128-135)
    void end_frame() override;                   // resolve happened in the draw; reads back, writes the PPM
    void draw_scene(const scene& scene, std::vector<shader>& shaders, float dt) override;

    const std::vector<path_tracer::pixel>& host_pixels() const { return m_host_pixels; }
    uint64_t frames_drawn() const { return m_frames; }
    iqpt_raster* context() const { return m_r; }

private:
    rasterizer(camera* cam, const rasterizer_options& opt);
    ~rasterizer() override;

    iqpt_raster* m_r = nullptr;
    camera* m_camera;
    rasterizer_options m_opt;
    std::vector<path_tracer::pixel> m_host_pixels;
    bool m_have_scene = false, m_drawn = false;
    uint64_t m_frames = 0, m_scene_revision = 0;
};

struct renderer_options {
    path_tracer_options path_tracer;
    rasterizer_options rasterizer;
};

class renderer : public renderer_template {
public:
    enum class engine { INVALID = -1, RASTERIZER, PATHTRACER, NUMENGINES };   // renderer.h:17-23

    static void init(camera* cam, const renderer_options& opt = renderer_options());
    static void shutdown();
    static renderer* get();

    void begin_frame() override;                 // the engine changes here, never mid-frame (renderer.cu:45-53)
    void end_frame() override;
    void draw_scene(const scene& scene, std::vector<shader>& shaders, float dt) override;
    void toggle_engine() { m_new_engine = (engine)(((int)m_new_engine + 1) % 2); }   // renderer.h:36
    void reset();                                // the path tracer's deferred reset (renderer.cu:65-68)
    engine current_engine() const { return m_engine_idx; }

private:
    renderer();
    ~renderer() override = default;

    engine m_new_engine, m_engine_idx;
    renderer_template* m_engines[2];
};

}  // namespace iqpt
