// rasterizer.cpp — the facade of raster/rasterizer.hpp (IoniqRE/rasterizer.cu:8-23, 128-175; renderer.cu:18-78;
// shader.cu:48-60).
#include "raster/rasterizer.hpp"

#include <cstring>

#include "iq_host_math.hpp"

namespace iqpt {

namespace {
rasterizer* g_rasterizer = nullptr;
renderer* g_renderer = nullptr;
}  // namespace

void shader::update_view_proj(const float view[16], const float proj[16]) {      // shader.cu:55-60
    std::memcpy(m_view, view, sizeof m_view);
    std::memcpy(m_proj, proj, sizeof m_proj);
    m_has_view_proj = true;
}

void shader::update_transform(const float tr[16]) {                              // shader.cu:48-53
    std::memcpy(m_model, tr, sizeof m_model);
    const iq::mat4 n = iq::normal_matrix(iq::mat4::from(tr));
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 4; ++b) m_normal[a * 4 + b] = n.m[a][b];
}

void rasterizer::init(camera* cam, const rasterizer_options& opt) {
    if (!g_rasterizer) g_rasterizer = new rasterizer(cam, opt);
}
void rasterizer::shutdown() {
    delete g_rasterizer;
    g_rasterizer = nullptr;
}
rasterizer* rasterizer::get() { return g_rasterizer; }

rasterizer::rasterizer(camera* cam, const rasterizer_options& opt) : m_camera(cam), m_opt(opt) {
    const uint32_t w = cam->get_width(), h = cam->get_height();
    IQPT_THROW_FAILED(iqpt_raster_create(opt.device, w, h, opt.samples, &m_r));
    m_host_pixels.assign((size_t)w * h, path_tracer::pixel{0, 0, 0, 0});
}

rasterizer::~rasterizer() { iqpt_raster_destroy(m_r); }

void rasterizer::begin_frame() {}

void rasterizer::end_frame() {
    if (!m_drawn) return;
    IQPT_THROW_FAILED(iqpt_raster_read(m_r, reinterpret_cast<uint8_t*>(m_host_pixels.data()), nullptr, nullptr));
    if (!m_opt.ppm_path.empty())
        IQPT_THROW_FAILED(iqpt_write_ppm(m_opt.ppm_path.c_str(), m_camera->get_width(), m_camera->get_height(),
                                         reinterpret_cast<const uint8_t*>(m_host_pixels.data())));
    m_drawn = false;
}

void rasterizer::prepare(const scene& scn, std::vector<shader>& shaders) {
    // the view and projection are the shader's once the application set them (shader.cu:55-60), else the camera's
    iqpt_camera cam = m_camera->raw();
    if (!shaders.empty() && shaders[0].has_view_proj()) {
        std::memcpy(cam.view, shaders[0].view(), sizeof cam.view);
        std::memcpy(cam.projection, shaders[0].projection(), sizeof cam.projection);
    }
    if (!m_have_camera || std::memcmp(cam.view, m_set_camera.view, sizeof cam.view) != 0 ||
        std::memcmp(cam.projection, m_set_camera.projection, sizeof cam.projection) != 0) {
        IQPT_THROW_FAILED(iqpt_raster_set_camera(m_r, &cam));
        m_set_camera = cam;
        m_have_camera = true;
    }
    if (!m_have_scene || scn.revision() != m_scene_revision) {
        // mesh::setup_mesh's buffers and every model's transform, once per scene change; scene::modified() is
        // left for the path tracer, whose own packet is built from it when that engine draws next
        IQPT_THROW_FAILED(iqpt_raster_upload_scene(m_r, scn.handle()));
        m_have_scene = true;
        m_scene_revision = scn.revision();
    }
}

void rasterizer::draw_scene(const scene& scn, std::vector<shader>& shaders, float /*dt*/) {   // rasterizer.cu:160-175
    prepare(scn, shaders);
    IQPT_THROW_FAILED(iqpt_raster_draw(m_r));
    m_drawn = true;
    m_frames += 1;
}

void renderer::init(camera* cam, const renderer_options& opt) {                  // renderer.cu:18-26
    if (!g_renderer) {
        rasterizer::init(cam, opt.rasterizer);
        // a block joins the path tracer's pixels with the rasterizer's planes: the aligned camera
        path_tracer_options pto = opt.path_tracer;
        if (opt.denoise.enabled || opt.temporal.enabled || opt.svgf.enabled) pto.align_camera = true;
        path_tracer::init(cam, pto);
        g_renderer = new renderer(cam, opt);
    }
}

void renderer::shutdown() {                                                      // renderer.cu:28-37
    if (g_renderer) {
        path_tracer::shutdown();
        rasterizer::shutdown();
        delete g_renderer;
        g_renderer = nullptr;
    }
}

renderer* renderer::get() { return g_renderer; }

renderer::renderer(camera* cam, const renderer_options& opt)                     // renderer.cu:70-78
    : m_engine_idx(engine::PATHTRACER), m_denoise(opt.denoise), m_temporal_opt(opt.temporal), m_svgf_opt(opt.svgf) {
    m_new_engine = m_engine_idx;
    m_engines[0] = rasterizer::get();
    m_engines[1] = path_tracer::get();
    if (m_denoise.enabled) {
        if (opt.path_tracer.world != 1)
            throw iqpt_exception(__LINE__, __FILE__, IQPT_ERR_UNSUPPORTED, "the denoise block needs a single-GPU path tracer");
        m_denoiser = new denoiser(cam->get_width(), cam->get_height(), opt.path_tracer.device);
        m_denoiser->set_params(m_denoise.params);
    }
    if (m_temporal_opt.enabled) {
        if (opt.path_tracer.world != 1)
            throw iqpt_exception(__LINE__, __FILE__, IQPT_ERR_UNSUPPORTED, "the temporal block needs a single-GPU path tracer");
        m_temporal = new temporal(cam->get_width(), cam->get_height(), opt.path_tracer.device);
        m_temporal->set_params(m_temporal_opt.params);
    }
    if (m_svgf_opt.enabled) {
        if (opt.path_tracer.world != 1)
            throw iqpt_exception(__LINE__, __FILE__, IQPT_ERR_UNSUPPORTED, "the svgf block needs a single-GPU path tracer");
        m_svgf = new svgf(cam->get_width(), cam->get_height(), opt.path_tracer.device);
        m_svgf->set_params(m_svgf_opt.params);
    }
}

renderer::~renderer() {
    delete m_svgf;
    delete m_temporal;
    delete m_denoiser;
}

void renderer::begin_frame() {                                                   // renderer.cu:45-53
    if (m_new_engine != m_engine_idx) m_engine_idx = m_new_engine;
    m_engines[(size_t)m_engine_idx]->begin_frame();
}

void renderer::end_frame() {
    m_engines[(size_t)m_engine_idx]->end_frame();
    // the denoised frame next to the path tracer's own: the accumulator as it stands after every launch issued
    // so far (the path tracer presents the frame before its last launch, path_tracer.cu:382-386), copied out of
    // the context, never written
    const bool due = m_denoise_due && m_engine_idx == engine::PATHTRACER;
    // the temporal frame first: a view of the rasterizer's camera when it moved, then the accumulator (of
    // frames() samples; none right after a reset: the reprojected history alone) blended with that view's history
    if (m_temporal && due) {
        rasterizer* rs = rasterizer::get();
        if (m_temporal->have_view() && m_scene_revision != m_temporal_revision) m_temporal->clear();
        if (!m_temporal->same_view(*rs->current_camera())) {
            m_temporal->begin_view(rs->context(), *rs->current_camera());
            m_temporal_revision = m_scene_revision;
        }
        m_temporal->resolve(path_tracer::get()->context());
        if (!m_temporal_opt.ppm_path.empty()) m_temporal->write_ppm(m_temporal_opt.ppm_path);
    }
    if (m_denoiser && due && (m_temporal || path_tracer::get()->frames() > 0)) {
        if (m_temporal) m_denoiser->frame_device(m_temporal->output_device(), rasterizer::get()->context());
        else m_denoiser->frame(path_tracer::get()->context(), rasterizer::get()->context());
        if (!m_denoise.ppm_path.empty()) m_denoiser->write_ppm(m_denoise.ppm_path);
    }
    // variance-guided filtering, on its own two histories: the same view logic as the temporal block
    if (m_svgf && due) {
        rasterizer* rs = rasterizer::get();
        if (m_svgf->have_view() && m_scene_revision != m_svgf_revision) m_svgf->clear();
        if (!m_svgf->same_view(*rs->current_camera())) {
            m_svgf->begin_view(rs->context(), *rs->current_camera());
            m_svgf_revision = m_scene_revision;
        }
        m_svgf->resolve(path_tracer::get()->context());
        if (!m_svgf_opt.ppm_path.empty()) m_svgf->write_ppm(m_svgf_opt.ppm_path);
    }
    m_denoise_due = false;
}

void renderer::draw_scene(const scene& scn, std::vector<shader>& shaders, float dt) {
    m_engines[(size_t)m_engine_idx]->draw_scene(scn, shaders, dt);
    if ((m_denoiser || m_temporal || m_svgf) && m_engine_idx == engine::PATHTRACER) {
        rasterizer::get()->prepare(scn, shaders);
        m_scene_revision = scn.revision();
        m_denoise_due = true;
    }
}

void renderer::reset() { static_cast<path_tracer*>(m_engines[1])->reset(); }    // renderer.cu:65-68

}  // namespace iqpt
