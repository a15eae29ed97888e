// iqpt_cli — headless stand-in for IoniqRE's application loop (application.cu:66-99) over the
// path_tracer facade: builds a preset scene, runs begin_frame / draw_scene / end_frame with a
// fixed dt, and dumps the frame as PPM (the D3D11 present path, path_tracer.cu:171-210, is out of
// scope). Usage:
//   iqpt_cli --preset cornell --width 1920 --height 1080 --spp 64 --max-depth 8 --out cornell.ppm
//   iqpt_cli --engine raster --preset cornell --samples 4 --out preview.ppm     (the rasterized preview)
//   iqpt_cli --preset cornell_lit --spp 4 --denoise [--denoise-levels 3] --out noisy.ppm --out-denoised clean.ppm
//     (the path tracer through iqpt::renderer with the denoise block on: both frames are written)
//   iqpt_cli --preset cornell_lit --spp 1 --temporal --views 8 --step-x 0.05 --out last.ppm --out-temporal kept.ppm
//     (K views, the camera moved by D along x per view and reset between them, --spp samples per view; the last
//     view's own frame and its temporal frame, which keeps the earlier views' samples, are written)
//   iqpt_cli --preset cornell_lit --spp 1 --svgf --views 8 --step-x 0.05 --out last.ppm --out-svgf filtered.ppm
//     (the same sequence through variance-guided filtering; may be combined with --temporal)
//   iqpt_cli --preset cornell_lit --width 1920 --height 1080 --spp 4 --upscale 2 --out lo.ppm --out-upscaled full.ppm
//     (guided upsampling, DESIGN.md §14: the path tracer runs at width/F x height/F, --out is that frame and
//     --out-upscaled the full-size one; alone, not with --denoise, --temporal or --svgf)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "path_tracer.hpp"
#include "raster/rasterizer.hpp"
#include "upscale/upscaler.hpp"

int main(int argc, char** argv) {
    std::string preset = "cornell", out = "iqpt.ppm", engine = "pt", out_denoised, out_temporal, out_svgf, out_upscaled;
    int width = 640, height = 360, spp = 16, launches = 1, max_depth = 8, device = 0, samples = 4, denoise_levels = -1;
    int views = -1, upscale = 0;
    bool have_upscale = false;
    float step_x = 0.0f;
    bool denoise = false, temporal = false, svgf = false, have_step = false;
    for (int i = 1; i < argc; i += 2) {
        const std::string k = argv[i];
        if (k == "--denoise" || k == "--temporal" || k == "--svgf") {   // the options without a value
            (k == "--denoise" ? denoise : k == "--temporal" ? temporal : svgf) = true;
            i -= 1;
            continue;
        }
        if (i + 1 >= argc) break;                // a trailing option without its value is ignored, as before
        const char* v = argv[i + 1];
        if (k == "--preset") preset = v;
        else if (k == "--out-denoised") out_denoised = v;
        else if (k == "--denoise-levels") denoise_levels = std::atoi(v);
        else if (k == "--out-temporal") out_temporal = v;
        else if (k == "--out-svgf") out_svgf = v;
        else if (k == "--out-upscaled") out_upscaled = v;
        else if (k == "--upscale") {
            upscale = std::atoi(v);
            have_upscale = true;
        }
        else if (k == "--views") views = std::atoi(v);
        else if (k == "--step-x") {
            step_x = (float)std::atof(v);
            have_step = true;
        }
        else if (k == "--out") out = v;
        else if (k == "--width") width = std::atoi(v);
        else if (k == "--height") height = std::atoi(v);
        else if (k == "--spp") spp = std::atoi(v);
        else if (k == "--launches") launches = std::atoi(v);
        else if (k == "--max-depth") max_depth = std::atoi(v);
        else if (k == "--device") device = std::atoi(v);
        else if (k == "--engine") engine = v;
        else if (k == "--samples") samples = std::atoi(v);
        else {
            std::fprintf(stderr, "unknown option %s\n", k.c_str());
            return 2;
        }
    }
    if (engine != "pt" && engine != "raster") {
        std::fprintf(stderr, "--engine must be pt or raster\n");
        return 2;
    }
    if (denoise && (engine != "pt" || out_denoised.empty())) {
        std::fprintf(stderr, "--denoise goes with the path tracer and needs --out-denoised PATH\n");
        return 2;
    }
    if (!denoise && (denoise_levels >= 0 || !out_denoised.empty())) {
        std::fprintf(stderr, "--denoise-levels and --out-denoised need --denoise\n");
        return 2;
    }
    if (temporal && (engine != "pt" || denoise || out_temporal.empty() || views == 0 || views < -1)) {
        std::fprintf(stderr, "--temporal goes with the path tracer alone, needs --out-temporal PATH and --views >= 1\n");
        return 2;
    }
    if (svgf && (engine != "pt" || denoise || out_svgf.empty() || views == 0 || views < -1)) {
        std::fprintf(stderr, "--svgf goes with the path tracer (and --temporal), needs --out-svgf PATH and --views >= 1\n");
        return 2;
    }
    if (!temporal && !out_temporal.empty()) {
        std::fprintf(stderr, "--out-temporal needs --temporal\n");
        return 2;
    }
    if (!svgf && !out_svgf.empty()) {
        std::fprintf(stderr, "--out-svgf needs --svgf\n");
        return 2;
    }
    if (!temporal && !svgf && (views != -1 || have_step)) {
        std::fprintf(stderr, "--views and --step-x need --temporal or --svgf\n");
        return 2;
    }
    if (have_upscale && (engine != "pt" || denoise || temporal || svgf || out_upscaled.empty())) {
        std::fprintf(stderr, "--upscale goes with the path tracer alone and needs --out-upscaled PATH\n");
        return 2;
    }
    if (!have_upscale && !out_upscaled.empty()) {
        std::fprintf(stderr, "--out-upscaled needs --upscale\n");
        return 2;
    }
    if (have_upscale && (upscale < (int)IQPT_UPSCALE_MIN_FACTOR || upscale > (int)IQPT_UPSCALE_MAX_FACTOR || width <= 0 ||
                         height <= 0 || width % upscale != 0 || height % upscale != 0)) {
        std::fprintf(stderr, "--upscale must be 2, 3 or 4 and divide --width and --height\n");
        return 2;
    }
    try {
        iqpt::camera cam((uint16_t)width, (uint16_t)height);
        iqpt::scene scn;
        scn.add_preset(preset);
        if (have_upscale) {
            // the contexts themselves: the path tracer and one rasterizer at the lo size, another rasterizer at the
            // full size, all under one camera (its matrices do not depend on the frame size)
            const uint32_t W = (uint32_t)width, H = (uint32_t)height, w = W / (uint32_t)upscale, h = H / (uint32_t)upscale;
            iqpt::camera cam_lo((uint16_t)w, (uint16_t)h);
            struct handles {                     // destroyed on every way out, after the upscaler declared below
                iqpt_ctx* ctx = nullptr;
                iqpt_raster *r_lo = nullptr, *r_hi = nullptr;
                ~handles() {
                    iqpt_raster_destroy(r_hi);
                    iqpt_raster_destroy(r_lo);
                    iqpt_destroy(ctx);
                }
            } own;
            IQPT_THROW_FAILED(iqpt_create(device, w, h, nullptr, IQPT_DEFAULT_SEED, max_depth, &own.ctx));
            IQPT_THROW_FAILED(iqpt_raster_create(device, w, h, 1, &own.r_lo));
            IQPT_THROW_FAILED(iqpt_raster_create(device, W, H, 1, &own.r_hi));
            iqpt_ctx* const ctx = own.ctx;
            iqpt_raster *const r_lo = own.r_lo, *const r_hi = own.r_hi;
            {
                iqpt::upscaler up(W, H, (uint32_t)upscale, device);
                const iqpt_packet_desc pk = scn.build_packet();
                const iqpt_camera pt_cam = cam_lo.aligned();
                IQPT_THROW_FAILED(iqpt_set_camera(ctx, &pt_cam));
                IQPT_THROW_FAILED(iqpt_upload_packet(ctx, &pk));
                IQPT_THROW_FAILED(iqpt_raster_upload_scene(r_lo, scn.handle()));
                IQPT_THROW_FAILED(iqpt_raster_upload_scene(r_hi, scn.handle()));
                IQPT_THROW_FAILED(iqpt_raster_set_camera(r_lo, &cam_lo.raw()));
                IQPT_THROW_FAILED(iqpt_raster_set_camera(r_hi, &cam.raw()));
                for (int l = 0; l < launches; ++l) IQPT_THROW_FAILED(iqpt_render(ctx, (uint32_t)spp));
                up.frame(ctx, r_lo, r_hi);
                up.write_ppm(out_upscaled);
                std::vector<uint8_t> bgra((size_t)w * h * 4);
                IQPT_THROW_FAILED(iqpt_read(ctx, nullptr, bgra.data()));
                IQPT_THROW_FAILED(iqpt_write_ppm(out.c_str(), w, h, bgra.data()));
                const iqpt::upscaler::counts n = up.stats();
                uint64_t frames = 0, runs = 0;
                double ms = 0.0;
                IQPT_THROW_FAILED(iqpt_frame_count(ctx, &frames));
                IQPT_THROW_FAILED(iqpt_upscale_time(up.context(), &ms, &runs));
                std::printf("{\"preset\": \"%s\", \"upscale\": %d, \"lo_width\": %u, \"lo_height\": %u, \"frames\": %llu, "
                            "\"out\": \"%s\", \"out_upscaled\": \"%s\", \"guided\": %llu, \"widened\": %llu, "
                            "\"unguided\": %llu, \"upscale_ms\": %.4f}\n",
                            preset.c_str(), upscale, w, h, (unsigned long long)frames, out.c_str(), out_upscaled.c_str(),
                            (unsigned long long)n.guided, (unsigned long long)n.widened, (unsigned long long)n.unguided, ms);
            }
            return 0;
        }
        if (temporal || svgf) {
            // the contexts themselves (the facade's camera never moves): every view sets the moved camera on the
            // path tracer and the rasterizer, resets the accumulation, begins a temporal view (an svgf view, or both)
            // from the G-buffer and resolves the view's samples into it
            if (views < 0) views = 1;
            iqpt_ctx* ctx = nullptr;
            iqpt_raster* rs = nullptr;
            IQPT_THROW_FAILED(iqpt_create(device, (uint32_t)width, (uint32_t)height, nullptr, IQPT_DEFAULT_SEED, max_depth, &ctx));
            IQPT_THROW_FAILED(iqpt_raster_create(device, (uint32_t)width, (uint32_t)height, 1, &rs));
            {
                std::unique_ptr<iqpt::temporal> tmp;
                std::unique_ptr<iqpt::svgf> vgf;
                if (temporal) tmp.reset(new iqpt::temporal((uint32_t)width, (uint32_t)height, device));
                if (svgf) vgf.reset(new iqpt::svgf((uint32_t)width, (uint32_t)height, device));
                const iqpt_packet_desc pk = scn.build_packet();
                IQPT_THROW_FAILED(iqpt_upload_packet(ctx, &pk));
                IQPT_THROW_FAILED(iqpt_raster_upload_scene(rs, scn.handle()));
                for (int k = 0; k < views; ++k) {
                    iqpt_camera moved;
                    float pos[4];
                    std::memcpy(pos, cam.raw().position, sizeof pos);
                    pos[0] = pos[0] + step_x * (float)k;
                    IQPT_THROW_FAILED(iqpt_camera_init(&moved, (uint16_t)width, (uint16_t)height, cam.raw().fovh, 0.01f, 100.0f,
                                                       pos, cam.raw().forward));
                    iqpt_camera pt_cam;
                    IQPT_THROW_FAILED(iqpt_camera_align(&moved, &pt_cam));
                    IQPT_THROW_FAILED(iqpt_set_camera(ctx, &pt_cam));
                    IQPT_THROW_FAILED(iqpt_reset(ctx));
                    IQPT_THROW_FAILED(iqpt_raster_set_camera(rs, &moved));
                    if (tmp) tmp->begin_view(rs, moved);
                    if (vgf) vgf->begin_view(rs, moved);
                    for (int l = 0; l < launches; ++l) IQPT_THROW_FAILED(iqpt_render(ctx, (uint32_t)spp));
                    if (tmp) tmp->resolve(ctx);
                    if (vgf) vgf->resolve(ctx);
                }
                std::vector<uint8_t> bgra((size_t)width * height * 4);
                IQPT_THROW_FAILED(iqpt_read(ctx, nullptr, bgra.data()));
                IQPT_THROW_FAILED(iqpt_write_ppm(out.c_str(), (uint32_t)width, (uint32_t)height, bgra.data()));
                uint64_t frames = 0, guided = 0, valid = 0, nviews = 0, nresolves = 0;
                double view_ms = 0.0, resolve_ms = 0.0;
                IQPT_THROW_FAILED(iqpt_frame_count(ctx, &frames));
                if (vgf) {
                    vgf->write_ppm(out_svgf);
                    uint64_t spatial = 0;
                    double moments_ms = 0.0, variance_ms = 0.0, level_ms[IQPT_SVGF_MAX_LEVELS] = {}, filter_ms = 0.0;
                    IQPT_THROW_FAILED(iqpt_svgf_stats(vgf->context(), &guided, &valid, &spatial));
                    IQPT_THROW_FAILED(iqpt_svgf_time(vgf->context(), &moments_ms, &variance_ms, level_ms, &nresolves, nullptr, nullptr));
                    for (double ms : level_ms) filter_ms += ms;
                    std::printf("{\"preset\": \"%s\", \"views\": %d, \"step_x\": %g, \"frames\": %llu, \"out\": \"%s\", "
                                "\"out_svgf\": \"%s\", \"guided\": %llu, \"valid\": %llu, \"spatial\": %llu, "
                                "\"moments_ms\": %.4f, \"variance_ms\": %.4f, \"levels_ms\": %.4f}\n",
                                preset.c_str(), views, (double)step_x, (unsigned long long)frames, out.c_str(), out_svgf.c_str(),
                                (unsigned long long)guided, (unsigned long long)valid, (unsigned long long)spatial, moments_ms,
                                variance_ms, filter_ms);
                }
                if (tmp) {      // the last line of the output, as before
                    tmp->write_ppm(out_temporal);
                    IQPT_THROW_FAILED(iqpt_temporal_stats(tmp->context(), &guided, &valid));
                    IQPT_THROW_FAILED(iqpt_temporal_time(tmp->context(), &view_ms, &nviews, &resolve_ms, &nresolves));
                    std::printf("{\"preset\": \"%s\", \"views\": %d, \"step_x\": %g, \"frames\": %llu, \"out\": \"%s\", "
                                "\"out_temporal\": \"%s\", \"guided\": %llu, \"valid\": %llu, \"view_ms\": %.4f, "
                                "\"resolve_ms\": %.4f}\n",
                                preset.c_str(), views, (double)step_x, (unsigned long long)frames, out.c_str(),
                                out_temporal.c_str(), (unsigned long long)guided, (unsigned long long)valid, view_ms, resolve_ms);
                }
            }
            iqpt_raster_destroy(rs);
            iqpt_destroy(ctx);
            return 0;
        }
        if (engine == "raster") {
            // the other engine (rasterizer.cu): one rasterized frame, presented as PPM by end_frame
            iqpt::rasterizer_options ro;
            ro.device = device;
            ro.samples = (uint32_t)samples;
            ro.ppm_path = out;
            iqpt::rasterizer::init(&cam, ro);
            iqpt::rasterizer* rs = iqpt::rasterizer::get();
            std::vector<iqpt::shader> sh(1);
            rs->begin_frame();
            rs->draw_scene(scn, sh, 0.0f);
            rs->end_frame();
            double ms = 0.0;
            uint64_t draws = 0, counts[3] = {};
            IQPT_THROW_FAILED(iqpt_raster_time(rs->context(), &ms, &draws));
            IQPT_THROW_FAILED(iqpt_raster_stats(rs->context(), counts));
            std::printf("{\"preset\": \"%s\", \"engine\": \"raster\", \"samples\": %d, \"draws\": %llu, "
                        "\"triangles\": %llu, \"draw_ms\": %.4f, \"out\": \"%s\"}\n",
                        preset.c_str(), samples, (unsigned long long)draws, (unsigned long long)counts[0], ms, out.c_str());
            iqpt::rasterizer::shutdown();
            return 0;
        }
        iqpt::path_tracer_options opt;
        opt.device = device;
        opt.max_depth = max_depth;
        opt.spp_per_launch = (uint32_t)spp;
        opt.launch_interval = 0.0f;
        opt.ppm_path = out;
        if (denoise) {
            // the same loop through the two-engine renderer, whose end_frame also filters the accumulator under
            // the rasterizer's G-buffer and writes it next to the path tracer's own frame
            iqpt::renderer_options ro;
            ro.path_tracer = opt;
            ro.rasterizer.device = device;
            ro.denoise.enabled = true;
            ro.denoise.ppm_path = out_denoised;
            if (denoise_levels >= 0) ro.denoise.params.levels = (uint32_t)denoise_levels;
            iqpt::renderer::init(&cam, ro);
            iqpt::renderer* rn = iqpt::renderer::get();
            iqpt::path_tracer* pt = iqpt::path_tracer::get();
            std::vector<iqpt::shader> shaders;
            for (int f = 0; f <= launches; ++f) {
                rn->begin_frame();
                rn->draw_scene(scn, shaders, f < launches ? 1.0f : 0.0f);
                rn->end_frame();
            }
            std::vector<uint8_t> bgra((size_t)width * height * 4);
            IQPT_THROW_FAILED(iqpt_read(pt->context(), nullptr, bgra.data()));
            IQPT_THROW_FAILED(iqpt_write_ppm(out.c_str(), (uint32_t)width, (uint32_t)height, bgra.data()));
            double ms = 0.0, level_ms[IQPT_DENOISE_MAX_LEVELS] = {};
            uint64_t runs = 0;
            IQPT_THROW_FAILED(iqpt_denoise_time(rn->get_denoiser()->context(), &ms, level_ms, &runs));
            std::printf("{\"preset\": \"%s\", \"frames\": %llu, \"rays\": %llu, \"out\": \"%s\", \"denoise_levels\": %u, "
                        "\"denoise_runs\": %llu, \"denoise_ms\": %.4f, \"out_denoised\": \"%s\"}\n",
                        preset.c_str(), (unsigned long long)pt->frames(), (unsigned long long)pt->rays_traced(), out.c_str(),
                        ro.denoise.params.levels, (unsigned long long)runs, ms, out_denoised.c_str());
            iqpt::renderer::shutdown();
            return 0;
        }
        iqpt::path_tracer::init(&cam, opt);
        iqpt::path_tracer* pt = iqpt::path_tracer::get();
        std::vector<iqpt::shader> shaders;
        // each frame: the launch of frame k is read back at frame k+1 (path_tracer.cu:382-386)
        for (int f = 0; f <= launches; ++f) {
            pt->begin_frame();
            if (f < launches) {
                pt->draw_scene(scn, shaders, 1.0f);
            } else {
                std::vector<float> lin;
                pt->read_linear(lin);   // sync
                pt->draw_scene(scn, shaders, 0.0f);
            }
            pt->end_frame();
        }
        // final readback + dump of the last launch
        iqpt::path_tracer_options o2 = opt;
        (void)o2;
        std::vector<uint8_t> bgra((size_t)width * height * 4);
        IQPT_THROW_FAILED(iqpt_read(pt->context(), nullptr, bgra.data()));
        IQPT_THROW_FAILED(iqpt_write_ppm(out.c_str(), (uint32_t)width, (uint32_t)height, bgra.data()));
        std::printf("{\"preset\": \"%s\", \"frames\": %llu, \"rays\": %llu, \"out\": \"%s\"}\n", preset.c_str(),
                    (unsigned long long)pt->frames(), (unsigned long long)pt->rays_traced(), out.c_str());
        iqpt::path_tracer::shutdown();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
