// test_motion_facade — drives iqpt::motion (motion/motion.hpp) over libiqpt_motion.so and libiqpt.so: two views of a
// scene in which one cube moves (tests/motion_cases.py's movers without its material table, which iqpt::scene has no
// call for), through two rasterizer uploads and two packet uploads of one rasterizer and one path-tracing context.
// Prints one JSON line for tests/test_gpu_motion_facade.py: the four counts of the second view and the FNV-1a hashes
// of its float4 and BGRA8 results, which that test compares with tests/motion_ref.py's on the same planes.
// Usage: test_motion_facade
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "motion/motion.hpp"
#include "raster/iqpt_raster.h"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #c); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

namespace {

constexpr uint32_t kSpp = 2;

uint64_t fnv1a_64(const void* data, size_t bytes) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

// view k's scene: the moving cube at step k (a quarter of its width along x and 10 degrees about y per step)
void movers(iqpt::scene& s, int k) {
    const double pi = 3.14159265358979323846;
    s.add_mesh_quad("a_ground");
    s.add_mesh_cube("b_cube");
    s.add_mesh_cube("z_mover");
    const float gs[4] = {4.0f, 4.0f, 1.0f, 1.0f}, gr[4] = {(float)(pi / 2), 0.0f, 0.0f, 0.0f},
                gt[4] = {0.0f, -0.5f, 0.0f, 0.0f};
    const float bs[4] = {0.5f, 0.5f, 0.5f, 0.5f}, br[4] = {0.0f, 0.4f, 0.0f, 0.0f}, bt[4] = {-0.6f, -0.25f, 0.6f, 0.0f};
    const float ms[4] = {0.4f, 0.4f, 0.4f, 0.4f}, mr[4] = {0.0f, (float)(10.0 * (pi / 180.0) * k), 0.0f, 0.0f},
                mt[4] = {(float)(0.15 + 0.25 * 0.4 * k), -0.3f, -0.4f, 0.0f};
    s.add_model("ground", "a_ground", gs, gr, gt);
    s.add_model("box", "b_cube", bs, br, bt);
    s.add_model("mover", "z_mover", ms, mr, mt);
}

}  // namespace

int main() {
    const uint32_t w = 96, h = 54;
    const size_t npix = (size_t)w * h;
    iqpt_raster* raster = nullptr;
    iqpt_ctx* ctx = nullptr;
    int rc = 1;
    try {
        iqpt::camera cam(w, h);
        const iqpt_camera aligned = cam.aligned();
        iqpt::scene s0, s1;
        movers(s0, 0);
        movers(s1, 1);
        IQPT_THROW_FAILED(iqpt_raster_create(0, w, h, 1, &raster));
        IQPT_THROW_FAILED(iqpt_raster_set_camera(raster, &cam.raw()));
        IQPT_THROW_FAILED(iqpt_create(0, w, h, nullptr, IQPT_DEFAULT_SEED, 8, &ctx));
        IQPT_THROW_FAILED(iqpt_set_camera(ctx, &aligned));
        {
            iqpt::motion m(w, h);
            m.set_params({0.9f, 0.01f, 256u});

            // the table itself: ground and box stay, the cube moves
            const std::vector<iqpt_motion_entry> t = iqpt::motion::table(s0, s1);
            CHECK(t.size() == 3 && t[0].moved == 0 && t[1].moved == 0 && t[2].moved == 1);
            CHECK(t[0].back[0] == 1.0f && t[0].back[12] == 0.0f && std::isfinite(t[2].back[12]) && t[2].back[12] != 0.0f);
            const std::vector<iqpt_motion_entry> same = iqpt::motion::table(s1, s1);
            CHECK(same.size() == 3 && !same[0].moved && !same[1].moved && !same[2].moved);

            // view 0: no history yet
            iqpt_packet_desc pk = s0.build_packet();
            IQPT_THROW_FAILED(iqpt_upload_packet(ctx, &pk));
            IQPT_THROW_FAILED(iqpt_raster_upload_scene(raster, s0.handle()));
            m.begin_view(raster);
            iqpt::motion::counts c = m.stats();
            CHECK(c.guided > npix / 4 && c.valid == 0 && c.moved == 0 && c.moved_valid == 0);
            IQPT_THROW_FAILED(iqpt_render(ctx, kSpp));
            m.resolve(ctx);

            // view 1: the cube moved; the scene is uploaded again to both engines
            pk = s1.build_packet();
            IQPT_THROW_FAILED(iqpt_upload_packet(ctx, &pk));
            IQPT_THROW_FAILED(iqpt_reset(ctx));
            IQPT_THROW_FAILED(iqpt_raster_upload_scene(raster, s1.handle()));
            m.begin_view(raster, s0, s1);
            c = m.stats();
            CHECK(c.moved > 50 && c.moved_valid > c.moved / 2 && c.valid > c.guided / 2 && c.valid < c.guided);
            IQPT_THROW_FAILED(iqpt_render(ctx, kSpp));
            m.resolve(ctx);
            CHECK(m.views() == 2 && m.resolves() == 2);

            std::vector<float> lin;
            m.read_linear(lin);
            CHECK(lin.size() == npix * 4 && m.host_pixels().size() == npix);
            size_t carried = 0;
            for (size_t i = 0; i < npix; ++i) carried += lin[4 * i + 3] == (float)(2 * kSpp);
            CHECK(carried == c.valid);
            std::printf("{\"ok\": true, \"width\": %u, \"height\": %u, \"spp\": %u, \"guided\": %llu, \"valid\": %llu, "
                        "\"moved\": %llu, \"moved_valid\": %llu, \"lin_fnv1a\": \"%016llx\", \"bgra_fnv1a\": \"%016llx\"}\n",
                        w, h, kSpp, (unsigned long long)c.guided, (unsigned long long)c.valid, (unsigned long long)c.moved,
                        (unsigned long long)c.moved_valid, (unsigned long long)fnv1a_64(lin.data(), lin.size() * sizeof(float)),
                        (unsigned long long)fnv1a_64(m.host_pixels().data(), npix * 4));
        }
        rc = 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
    }
    if (ctx) iqpt_destroy(ctx);
    if (raster) iqpt_raster_destroy(raster);
    return rc;
}
