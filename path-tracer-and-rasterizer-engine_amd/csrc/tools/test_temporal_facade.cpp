// test_temporal_facade — drives iqpt::renderer with the temporal block of renderer_options off and on: the path
// tracer's own PPM and accumulator must be the same either way; a second camera begins a second view that carries
// the first one's samples; a scene revision clears the history; with the denoise block on as well the denoiser
// filters the temporal result. Prints one JSON line for tests/test_gpu_temporal_facade.py, which compares the PPMs
// with what the Python objects make of the same sequence.
// Usage: test_temporal_facade PLAIN.ppm TEMPORAL_A.ppm TEMPORAL_B.ppm DENOISED_B.ppm
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

constexpr int kLaunchesA = 3, kLaunchesB = 2;

// the CLI's loop: launch k is presented at frame k + 1, the last frame launches nothing
void run(iqpt::renderer* r, const iqpt::scene& s, std::vector<iqpt::shader>& sh, int launches) {
    for (int f = 0; f <= launches; ++f) {
        r->begin_frame();
        r->draw_scene(s, sh, f < launches ? 1.0f : 0.0f);
        r->end_frame();
    }
}

std::vector<char> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<char>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// pixels whose colour is the other frame's, bit for bit, and pixels whose w is `samples`
void compare(const std::vector<float>& temporal, const std::vector<float>& accum, float samples, size_t& same_colour,
             size_t& with_samples) {
    same_colour = with_samples = 0;
    for (size_t i = 0; i < temporal.size(); i += 4) {
        same_colour += std::memcmp(&temporal[i], &accum[i], 12) == 0;
        with_samples += temporal[i + 3] == samples;
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: test_temporal_facade PLAIN.ppm TEMPORAL_A.ppm TEMPORAL_B.ppm DENOISED_B.ppm\n");
        return 2;
    }
    const std::string plain = argv[1], temporal_a = argv[2], temporal_b = argv[3], denoised_b = argv[4];
    const uint32_t w = 96, h = 54;
    const size_t npix = (size_t)w * h;
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
            CHECK(r && !r->get_temporal() && !r->get_denoiser());
            run(r, scn, shaders, kLaunchesA);
            CHECK(iqpt::path_tracer::get()->frames() == (uint64_t)kLaunchesA);
            iqpt::path_tracer::get()->read_linear(lin_off);
            iqpt::renderer::shutdown();
        }
        const std::vector<char> ppm_off = slurp(plain);
        CHECK(!ppm_off.empty());
        CHECK(std::remove(plain.c_str()) == 0);

        // the block on, and the denoise block with it
        iqpt::renderer_options on = opt;
        on.temporal.enabled = true;
        on.temporal.params = {0.9f, 0.01f, 256u};
        on.temporal.ppm_path = temporal_b;
        on.denoise.enabled = true;
        on.denoise.params = {2u, 5u, 1024.0f, 1.0f};
        on.denoise.ppm_path = denoised_b;
        size_t carried = 0, same = 0, count = 0;
        {
            iqpt::scene scn;
            scn.add_preset("cornell_lit");
            iqpt::renderer::init(&cam, on);
            iqpt::renderer* r = iqpt::renderer::get();
            iqpt::temporal* t = r->get_temporal();
            iqpt::path_tracer* pt = iqpt::path_tracer::get();
            CHECK(r && t && r->get_denoiser());

            // camera A: one view, resolved at every end_frame; a first view is the accumulator itself
            run(r, scn, shaders, kLaunchesA);
            CHECK(pt->frames() == (uint64_t)kLaunchesA);
            CHECK(t->views() == 1 && t->resolves() == (uint64_t)kLaunchesA + 1);
            CHECK(r->get_denoiser()->frames() == (uint64_t)kLaunchesA + 1);
            CHECK(iqpt::rasterizer::get()->frames_drawn() == 0);
            std::vector<float> lin_on, lin_t;
            pt->read_linear(lin_on);
            CHECK(lin_on.size() == lin_off.size() && std::memcmp(lin_on.data(), lin_off.data(), lin_on.size() * sizeof(float)) == 0);
            CHECK(slurp(plain) == ppm_off);
            t->read_linear(lin_t);
            compare(lin_t, lin_on, (float)kLaunchesA, same, count);
            CHECK(same == npix && count == npix);
            CHECK(std::rename(temporal_b.c_str(), temporal_a.c_str()) == 0);

            // camera B (another field of view) and a reset: a second view that inherits A's samples
            cam = iqpt::camera(w, h, 50.0f);
            pt->update_camera();                 // the aligned form: the renderer turned align_camera on
            r->reset();
            run(r, scn, shaders, kLaunchesB);
            CHECK(pt->frames() == (uint64_t)kLaunchesB);
            CHECK(t->views() == 2 && t->resolves() == (uint64_t)(kLaunchesA + kLaunchesB) + 2);
            pt->read_linear(lin_on);
            t->read_linear(lin_t);
            compare(lin_t, lin_on, (float)(kLaunchesA + kLaunchesB), same, carried);
            CHECK(carried > npix / 4 && same < npix - carried + npix / 100);
            // the denoiser filtered the temporal result: a denoiser of its own over the same buffer and G-buffer
            {
                const auto& px = r->get_denoiser()->host_pixels();
                std::vector<uint8_t> own(npix * 4);
                iqpt_raster* rs = iqpt::rasterizer::get()->context();
                const void *nz = nullptr, *id = nullptr;
                iqpt_denoise* d = nullptr;
                IQPT_THROW_FAILED(iqpt_denoise_create(0, w, h, &d));
                IQPT_THROW_FAILED(iqpt_denoise_set_params(d, &on.denoise.params));
                IQPT_THROW_FAILED(iqpt_raster_gbuffer(rs));
                IQPT_THROW_FAILED(iqpt_raster_gbuffer_device(rs, &nz, &id));
                IQPT_THROW_FAILED(iqpt_denoise_set_guides_device(d, nz, id));
                IQPT_THROW_FAILED(iqpt_denoise_run_device(d, t->output_device()));
                IQPT_THROW_FAILED(iqpt_denoise_read(d, nullptr, own.data()));
                IQPT_THROW_FAILED(iqpt_denoise_destroy(d));
                CHECK(px.size() * 4 == own.size() && std::memcmp(px.data(), own.data(), own.size()) == 0);
            }
            const std::vector<char> ppm_b = slurp(temporal_b), den_b = slurp(denoised_b);
            CHECK(!ppm_b.empty() && !den_b.empty() && ppm_b != den_b);

            // a scene revision: the history is cleared, the next view starts from the accumulator alone
            const float one[4] = {0.2f, 0.2f, 0.2f, 0.0f}, none[4] = {0.0f, 0.0f, 0.0f, 0.0f}, at[4] = {0.0f, 0.3f, 0.0f, 0.0f};
            scn.add_model("temporal_facade_panel", "quad", one, none, at);    // one more model of the preset's quad
            r->reset();
            run(r, scn, shaders, 1);
            CHECK(t->views() == 3 && pt->frames() == 1);
            pt->read_linear(lin_on);
            t->read_linear(lin_t);
            compare(lin_t, lin_on, 1.0f, same, count);
            CHECK(same == npix && count == npix);
            // these frames overwrote the two PPMs: put B's back for the caller
            std::ofstream(temporal_b, std::ios::binary).write(ppm_b.data(), (std::streamsize)ppm_b.size());
            std::ofstream(denoised_b, std::ios::binary).write(den_b.data(), (std::streamsize)den_b.size());

            // the engine toggled away: no temporal frame is made of a rasterized one
            const uint64_t resolves = t->resolves();
            r->toggle_engine();
            r->begin_frame();
            r->draw_scene(scn, shaders, 1.0f);
            r->end_frame();
            CHECK(t->resolves() == resolves && t->views() == 3);
            iqpt::renderer::shutdown();
        }
        std::printf("{\"ok\": true, \"plain_ppm_equal\": true, \"accumulator_equal\": true, \"launches_a\": %d, "
                    "\"launches_b\": %d, \"pixels_carried\": %zu}\n", kLaunchesA, kLaunchesB, carried);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
