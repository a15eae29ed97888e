// rasterizer.hpp — C++ facade of the second engine: iqpt::rasterizer (IoniqRE/rasterizer.h) over the
// iqpt_raster_* C ABI and iqpt::renderer (IoniqRE/renderer.h:14-49, renderer.cu:18-78), which owns both
// engines behind renderer_template and switches between them at begin_frame.
#pragma once

#include <string>
#include <vector>

#include "denoise/denoiser.hpp"
#include "path_tracer.hpp"
#include "raster/iqpt_raster.h"
#include "svgf/svgf.hpp"
#include "temporal/temporal.hpp"

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
    // the camera and the scene of draw_scene without the draw: what a G-buffer pass (iqpt_raster_gbuffer) needs
    // while the path tracer is the engine. A camera equal to the one already set is not set again, so the
    // G-buffer of an unchanged view is kept.
    void prepare(const scene& scene, std::vector<shader>& shaders);

    const std::vector<path_tracer::pixel>& host_pixels() const { return m_host_pixels; }
    uint64_t frames_drawn() const { return m_frames; }
    iqpt_raster* context() const { return m_r; }
    // the camera the context has (what prepare() set last); NULL before the first one
    const iqpt_camera* current_camera() const { return m_have_camera ? &m_set_camera : nullptr; }

private:
    rasterizer(camera* cam, const rasterizer_options& opt);
    ~rasterizer() override;

    iqpt_raster* m_r = nullptr;
    camera* m_camera;
    rasterizer_options m_opt;
    std::vector<path_tracer::pixel> m_host_pixels;
    bool m_have_scene = false, m_drawn = false, m_have_camera = false;
    uint64_t m_frames = 0, m_scene_revision = 0;
    iqpt_camera m_set_camera{};                  // the camera the context has
};

struct renderer_options {
    // with denoise, temporal or svgf enabled the path tracer runs under camera::aligned() (align_camera is forced
    // on), the rasterizer and the blocks under camera::raw(): DESIGN.md §9.7
    path_tracer_options path_tracer;
    rasterizer_options rasterizer;
    // enabled: end_frame under the path-tracing engine also filters the accumulator under the rasterizer's
    // G-buffer and writes the result to denoise.ppm_path. The path tracer's own frame, PPM and
    // accumulation are untouched. Single-GPU path tracer only (path_tracer.world == 1).
    denoise_options denoise;
    // enabled: end_frame under the path-tracing engine also keeps a history that follows the camera (DESIGN.md
    // §11): it begins a view when the rasterizer's camera differs from the temporal view's (or none exists),
    // clears first when the scene's revision changed, blends the accumulator with the view's history and
    // writes the result to temporal.ppm_path. With denoise on as well, the denoiser filters that result
    // instead of the accumulator. The path tracer's own frame, PPM and accumulation are untouched. Single-GPU
    // path tracer only. World positions come from the camera's inverse matrices, so a view and projection set
    // through shader::update_view_proj must be the camera's own.
    temporal_options temporal;
    // enabled: end_frame under the path-tracing engine also runs variance-guided filtering, as the
    // temporal block runs its history: it begins a view when the rasterizer's camera differs from the object's
    // (or none exists), clears first when the scene's revision changed, resolves the accumulator and writes the
    // filtered frame to svgf.ppm_path. Independent of the temporal and denoise blocks (it owns its two histories).
    // The path tracer's own frame, PPM and accumulation are untouched. Single-GPU path tracer only.
    svgf_options svgf;
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
    denoiser* get_denoiser() const { return m_denoiser; }                      // NULL unless the denoise block is on
    temporal* get_temporal() const { return m_temporal; }                      // NULL unless the temporal block is on
    svgf* get_svgf() const { return m_svgf; }                                  // NULL unless the svgf block is on

private:
    renderer(camera* cam, const renderer_options& opt);
    ~renderer() override;

    engine m_new_engine, m_engine_idx;
    renderer_template* m_engines[2];
    denoise_options m_denoise;
    denoiser* m_denoiser = nullptr;
    bool m_denoise_due = false;                  // the path tracer drew this frame
    temporal_options m_temporal_opt;
    temporal* m_temporal = nullptr;
    uint64_t m_temporal_revision = 0;            // the scene revision of the temporal view
    uint64_t m_scene_revision = 0;               // of the scene drawn last
    svgf_options m_svgf_opt;
    svgf* m_svgf = nullptr;
    uint64_t m_svgf_revision = 0;                // the scene revision of the svgf view
};

}  // namespace iqpt
