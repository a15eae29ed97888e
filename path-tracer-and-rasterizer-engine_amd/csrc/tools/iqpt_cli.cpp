// iqpt_cli — headless stand-in for IoniqRE's application loop (application.cu:66-99) over the
// path_tracer facade: builds a preset scene, runs begin_frame / draw_scene / end_frame with a
// fixed dt, and dumps the frame as PPM (the D3D11 present path, path_tracer.cu:171-210, is out of
// scope). Usage:
//   iqpt_cli --preset cornell --width 1920 --height 1080 --spp 64 --max-depth 8 --out cornell.ppm
//   iqpt_cli --engine raster --preset cornell --samples 4 --out preview.ppm     (the rasterized preview)
//   iqpt_cli --preset cornell_lit --spp 4 --denoise [--denoise-levels 3] --out noisy.ppm --out-denoised clean.ppm
//     (the path tracer through iqpt::renderer with the denoise block on: both frames are written)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "path_tracer.hpp"
#include "raster/rasterizer.hpp"

int main(int argc, char** argv) {
    std::string preset = "cornell", out = "iqpt.ppm", engine = "pt", out_denoised;
    int width = 640, height = 360, spp = 16, launches = 1, max_depth = 8, device = 0, samples = 4, denoise_levels = -1;
    bool denoise = false;
    for (int i = 1; i < argc; i += 2) {
        const std::string k = argv[i];
        if (k == "--denoise") {                  // the only option without a value
            denoise = true;
            i -= 1;
            continue;
        }
        if (i + 1 >= argc) break;                // a trailing option without its value is ignored, as before
        const char* v = argv[i + 1];
        if (k == "--preset") preset = v;
        else if (k == "--out-denoised") out_denoised = v;
        else if (k == "--denoise-levels") denoise_levels = std::atoi(v);
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
    try {
        iqpt::camera cam((uint16_t)width, (uint16_t)height);
        iqpt::scene scn;
        scn.add_preset(preset);
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
