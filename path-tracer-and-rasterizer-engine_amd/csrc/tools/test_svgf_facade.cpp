// test_svgf_facade — drives iqpt::renderer with the svgf block of renderer_options off and on: the path tracer's
// own PPM and accumulator must be the same either way; a second camera begins a second view whose variance comes
// from the moments history where it is long enough; a scene revision clears both histories; the block runs
// without the temporal and denoise blocks. Prints one JSON line for tests/test_gpu_svgf_facade.py, which compares
// the PPMs with what the Python object makes of the same sequence.
// Usage: test_svgf_facade PLAIN.ppm SVGF_A.ppm SVGF_B.ppm
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

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: test_svgf_facade PLAIN.ppm SVGF_A.ppm SVGF_B.ppm\n");
        return 2;
    }
    const std::string plain = argv[1], svgf_a = argv[2], svgf_b = argv[3];
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
            CHECK(r && !r->get_svgf() && !r->get_temporal() && !r->get_denoiser());
            run(r, scn, shaders, kLaunchesA);
            CHECK(iqpt::path_tracer::get()->frames() == (uint64_t)kLaunchesA);
            iqpt::path_tracer::get()->read_linear(lin_off);
            iqpt::renderer::shutdown();
        }
        const std::vector<char> ppm_off = slurp(plain);
        CHECK(!ppm_off.empty());
        CHECK(std::remove(plain.c_str()) == 0);

        // the block on, alone
        iqpt::renderer_options on = opt;
        on.svgf.enabled = true;
        on.svgf.params = {0.9f, 0.01f, 256u, 2u, 3u, 5u, 1024.0f, 4.0f, 1e-6f};
        on.svgf.ppm_path = svgf_b;
        uint64_t guided = 0, valid = 0, spatial_a = 0, spatial_b = 0;
        {
            iqpt::scene scn;
            scn.add_preset("cornell_lit");
            iqpt::renderer::init(&cam, on);
            iqpt::renderer* r = iqpt::renderer::get();
            iqpt::svgf* s = r->get_svgf();
            iqpt::path_tracer* pt = iqpt::path_tracer::get();
            CHECK(r && s && !r->get_temporal() && !r->get_denoiser());

            // camera A: one view, resolved at every end_frame; a first view has no history, so every guided pixel
            // takes the spatial estimate and the colour stage is the accumulator itself
            run(r, scn, shaders, kLaunchesA);
            CHECK(pt->frames() == (uint64_t)kLaunchesA);
            CHECK(s->views() == 1 && s->resolves() == (uint64_t)kLaunchesA + 1);
            CHECK(iqpt::rasterizer::get()->frames_drawn() == 0);
            std::vector<float> lin_on, stage_t, stage_v, lin_s;
            pt->read_linear(lin_on);
            CHECK(lin_on.size() == lin_off.size() && std::memcmp(lin_on.data(), lin_off.data(), lin_on.size() * sizeof(float)) == 0);
            CHECK(slurp(plain) == ppm_off);
            s->read_stages(stage_t, stage_v);
            IQPT_THROW_FAILED(iqpt_svgf_stats(s->context(), &guided, &valid, &spatial_a));
            CHECK(guided > npix / 4 && valid == 0 && spatial_a == guided);
            for (size_t i = 0; i < npix; ++i) {
                CHECK(std::memcmp(&stage_t[4 * i], &lin_on[4 * i], 12) == 0 && stage_t[4 * i + 3] == (float)kLaunchesA);
                CHECK(std::memcmp(&stage_v[4 * i], &lin_on[4 * i], 12) == 0 && stage_v[4 * i + 3] >= 0.0f);
            }
            CHECK(std::rename(svgf_b.c_str(), svgf_a.c_str()) == 0);

            // camera B (another field of view) and a reset: a second view that inherits A's samples and moments
            cam = iqpt::camera(w, h, 50.0f);
            pt->update_camera();                 // the aligned form: the renderer turned align_camera on
            r->reset();
            run(r, scn, shaders, kLaunchesB);
            CHECK(pt->frames() == (uint64_t)kLaunchesB);
            CHECK(s->views() == 2 && s->resolves() == (uint64_t)(kLaunchesA + kLaunchesB) + 2);
            IQPT_THROW_FAILED(iqpt_svgf_stats(s->context(), &guided, &valid, &spatial_b));
            // min_history is 2 views of the current 2 samples: the 3 + 2 samples behind a pixel with a valid history
            // are enough for the temporal estimate, the 2 behind one without are not
            CHECK(valid > guided / 2 && spatial_b + valid == guided);
            s->read_linear(lin_s);
            size_t negative = 0;
            for (size_t i = 0; i < npix; ++i) negative += !(lin_s[4 * i + 3] >= 0.0f);
            CHECK(negative == 0);
            const std::vector<char> ppm_b = slurp(svgf_b);
            CHECK(!ppm_b.empty() && ppm_b != slurp(svgf_a));

            // a scene revision: both histories are cleared, the next view starts from the accumulator alone
            const float one[4] = {0.2f, 0.2f, 0.2f, 0.0f}, none[4] = {0.0f, 0.0f, 0.0f, 0.0f}, at[4] = {0.0f, 0.3f, 0.0f, 0.0f};
            scn.add_model("svgf_facade_panel", "quad", one, none, at);    // one more model of the preset's quad
            r->reset();
            run(r, scn, shaders, 1);
            CHECK(s->views() == 3 && pt->frames() == 1);
            pt->read_linear(lin_on);
            s->read_stages(stage_t, stage_v);
            for (size_t i = 0; i < npix; ++i)
                CHECK(std::memcmp(&stage_t[4 * i], &lin_on[4 * i], 12) == 0 && stage_t[4 * i + 3] == 1.0f);
            // this frame overwrote the PPM: put B's back for the caller
            std::ofstream(svgf_b, std::ios::binary).write(ppm_b.data(), (std::streamsize)ppm_b.size());

            // the engine toggled away: no filtered frame is made of a rasterized one
            const uint64_t resolves = s->resolves();
            r->toggle_engine();
            r->begin_frame();
            r->draw_scene(scn, shaders, 1.0f);
            r->end_frame();
            CHECK(s->resolves() == resolves && s->views() == 3);
            iqpt::renderer::shutdown();
        }
        std::printf("{\"ok\": true, \"plain_ppm_equal\": true, \"accumulator_equal\": true, \"launches_a\": %d, "
                    "\"launches_b\": %d, \"guided_b\": %llu, \"valid_b\": %llu, \"spatial_a\": %llu, \"spatial_b\": %llu}\n",
                    kLaunchesA, kLaunchesB, (unsigned long long)guided, (unsigned long long)valid,
                    (unsigned long long)spatial_a, (unsigned long long)spatial_b);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
