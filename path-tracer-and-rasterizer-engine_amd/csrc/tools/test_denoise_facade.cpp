// test_denoise_facade — drives iqpt::renderer with the denoise block of renderer_options off and on: the path
// tracer's own PPM and accumulator must be the same either way, and the denoised PPM must be what a denoiser of
// its own makes of the same context and rasterizer through the C ABI. Prints one JSON line for
// tests/test_gpu_denoise_facade.py. Usage: test_denoise_facade PLAIN.ppm DENOISED.ppm
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "raster/rasterizer.hpp"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #c); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

namespace {

constexpr int kLaunches = 4;

// the CLI's loop: launch k is presented at frame k + 1, the last frame launches nothing
void run(iqpt::renderer* r, const iqpt::scene& s, std::vector<iqpt::shader>& sh) {
    for (int f = 0; f <= kLaunches; ++f) {
        r->begin_frame();
        r->draw_scene(s, sh, f < kLaunches ? 1.0f : 0.0f);
        r->end_frame();
    }
}

std::vector<char> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<char>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

}  // namespace

int main(int argc, char** argv) {
    const std::string plain = argc > 1 ? argv[1] : "denoise_facade_plain.ppm";
    const std::string denoised = argc > 2 ? argv[2] : "denoise_facade_denoised.ppm";
    const uint32_t w = 96, h = 54;
    try {
        iqpt::camera cam(w, h);
        iqpt::renderer_options opt;
        opt.path_tracer.max_depth = 8;
        opt.path_tracer.launch_interval = 0.0f;
        opt.path_tracer.ppm_path = plain;
        std::vector<iqpt::shader> shaders;

        // the block off
        std::vector<float> lin_off;
        {
            iqpt::scene scn;
            scn.add_preset("cornell_lit");
            // (under the aligned camera, which the renderer gives the path tracer by itself with a block on)
            iqpt::renderer_options off = opt;
            off.path_tracer.align_camera = true;
            iqpt::renderer::init(&cam, off);
            iqpt::renderer* r = iqpt::renderer::get();
            CHECK(r && !r->get_denoiser());
            run(r, scn, shaders);
            CHECK(iqpt::path_tracer::get()->frames() == (uint64_t)kLaunches);
            iqpt::path_tracer::get()->read_linear(lin_off);
            iqpt::renderer::shutdown();
        }
        const std::vector<char> ppm_off = slurp(plain);
        CHECK(!ppm_off.empty());
        CHECK(std::remove(plain.c_str()) == 0);

        // the block on
        iqpt::renderer_options on = opt;
        on.denoise.enabled = true;
        on.denoise.params = {3u, 5u, 1024.0f, 2.0f};
        on.denoise.ppm_path = denoised;
        std::vector<float> lin_on;
        unsigned long long changed = 0;
        {
            iqpt::scene scn;
            scn.add_preset("cornell_lit");
            iqpt::renderer::init(&cam, on);
            iqpt::renderer* r = iqpt::renderer::get();
            CHECK(r && r->get_denoiser());
            run(r, scn, shaders);
            iqpt::path_tracer* pt = iqpt::path_tracer::get();
            CHECK(pt->frames() == (uint64_t)kLaunches);
            CHECK(r->get_denoiser()->frames() == (uint64_t)kLaunches + 1);
            CHECK(iqpt::rasterizer::get()->frames_drawn() == 0);
            pt->read_linear(lin_on);

            // a denoiser of its own over the same context and rasterizer
            const auto& px = r->get_denoiser()->host_pixels();
            std::vector<uint8_t> own((size_t)w * h * 4), noisy((size_t)w * h * 4);
            iqpt_denoise* d = nullptr;
            IQPT_THROW_FAILED(iqpt_denoise_create(0, w, h, &d));
            IQPT_THROW_FAILED(iqpt_denoise_set_params(d, &on.denoise.params));
            IQPT_THROW_FAILED(iqpt_denoise_frame(d, pt->context(), iqpt::rasterizer::get()->context()));
            IQPT_THROW_FAILED(iqpt_denoise_read(d, nullptr, own.data()));
            IQPT_THROW_FAILED(iqpt_denoise_destroy(d));
            CHECK(px.size() * 4 == own.size() && std::memcmp(px.data(), own.data(), own.size()) == 0);
            IQPT_THROW_FAILED(iqpt_read(pt->context(), nullptr, noisy.data()));
            for (size_t i = 0; i < own.size(); i += 4) changed += std::memcmp(&own[i], &noisy[i], 4) != 0;
            CHECK(changed > (size_t)w * h / 4);

            // the engine toggled away: no denoised frame is made of a rasterized one
            r->toggle_engine();
            r->begin_frame();
            r->draw_scene(scn, shaders, 1.0f);
            r->end_frame();
            CHECK(r->get_denoiser()->frames() == (uint64_t)kLaunches + 1);
            iqpt::renderer::shutdown();
        }
        const std::vector<char> ppm_on = slurp(plain);
        CHECK(ppm_on == ppm_off);
        CHECK(lin_on.size() == lin_off.size() && !lin_on.empty());
        CHECK(std::memcmp(lin_on.data(), lin_off.data(), lin_on.size() * sizeof(float)) == 0);
        CHECK(!slurp(denoised).empty());
        std::printf("{\"ok\": true, \"plain_ppm_equal\": true, \"accumulator_equal\": true, \"launches\": %d, "
                    "\"pixels_changed\": %llu}\n", kLaunches, changed);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
