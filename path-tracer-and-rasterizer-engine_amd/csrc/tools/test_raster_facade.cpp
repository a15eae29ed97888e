// test_raster_facade — drives iqpt::renderer the way IoniqRE's application drives its two engines
// (application.cu:66-99, renderer.cu:45-78): toggles to the rasterizer, draws, toggles back, and checks that the
// path tracer's accumulation is untouched by the detour. Prints one JSON line for tests/test_gpu_raster_facade.py.
#include <cstdio>
#include <cstring>
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
void frame(iqpt::renderer* r, const iqpt::scene& s, std::vector<iqpt::shader>& sh) {
    r->begin_frame();
    r->draw_scene(s, sh, 0.2f);
    r->end_frame();
}
}  // namespace

int main(int argc, char** argv) {
    const std::string ppm = argc > 1 ? argv[1] : "raster_facade.ppm";
    using engine = iqpt::renderer::engine;
    try {
        iqpt::camera cam(96, 64);
        iqpt::renderer_options opt;
        opt.path_tracer.max_depth = 8;
        std::vector<iqpt::shader> shaders(1);
        shaders[0].update_view_proj(cam.raw().view, cam.raw().projection);       // application.cu: per frame
        const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        shaders[0].update_transform(identity);
        CHECK(shaders[0].normal_mat()[0] == 1.0f && shaders[0].normal_mat()[5] == 1.0f && shaders[0].model()[15] == 1.0f);

        // four launches without ever leaving the path tracer (the default engine)
        std::vector<float> lin_a;
        {
            iqpt::scene scn;
            scn.add_preset("cornell");
            iqpt::renderer::init(&cam, opt);
            iqpt::renderer* r = iqpt::renderer::get();
            CHECK(r && r->current_engine() == engine::PATHTRACER);
            for (int i = 0; i < 4; ++i) frame(r, scn, shaders);
            CHECK(iqpt::path_tracer::get()->frames() == 4);
            CHECK(iqpt::rasterizer::get()->frames_drawn() == 0);
            iqpt::path_tracer::get()->read_linear(lin_a);
            iqpt::renderer::shutdown();
            CHECK(!iqpt::renderer::get() && !iqpt::path_tracer::get() && !iqpt::rasterizer::get());
        }

        // two launches, two rasterized frames, two more launches
        std::vector<float> lin_b;
        size_t nonclear = 0;
        unsigned long long checksum = 1469598103934665603ull;
        {
            iqpt::scene scn;
            scn.add_preset("cornell");
            iqpt::renderer_options o = opt;
            o.rasterizer.ppm_path = ppm;
            iqpt::renderer::init(&cam, o);
            iqpt::renderer* r = iqpt::renderer::get();
            for (int i = 0; i < 2; ++i) frame(r, scn, shaders);
            r->toggle_engine();
            CHECK(r->current_engine() == engine::PATHTRACER);                    // the switch waits for begin_frame
            for (int i = 0; i < 2; ++i) frame(r, scn, shaders);
            CHECK(r->current_engine() == engine::RASTERIZER);
            CHECK(iqpt::rasterizer::get()->frames_drawn() == 2);
            CHECK(iqpt::path_tracer::get()->frames() == 2);
            const auto& px = iqpt::rasterizer::get()->host_pixels();
            CHECK(px.size() == 96u * 64u);
            for (const auto& p : px) {
                if (!(p.b == 255 && p.g == 214 && p.r == 158 && p.a == 255)) ++nonclear;
                for (uint8_t c : {p.b, p.g, p.r, p.a}) checksum = (checksum ^ c) * 1099511628211ull;   // FNV-1a
            }
            CHECK(nonclear > px.size() / 4);
            r->toggle_engine();
            for (int i = 0; i < 2; ++i) frame(r, scn, shaders);
            CHECK(r->current_engine() == engine::PATHTRACER);
            CHECK(iqpt::path_tracer::get()->frames() == 4);
            CHECK(iqpt::rasterizer::get()->frames_drawn() == 2);
            iqpt::path_tracer::get()->read_linear(lin_b);
            iqpt::renderer::shutdown();
        }
        CHECK(lin_a.size() == lin_b.size() && !lin_a.empty());
        const bool equal = std::memcmp(lin_a.data(), lin_b.data(), lin_a.size() * sizeof(float)) == 0;
        CHECK(equal);
        std::printf("{\"ok\": true, \"accumulator_equal\": true, \"raster_nonclear\": %zu, \"raster_fnv1a\": \"%016llx\"}\n",
                    nonclear, checksum);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
