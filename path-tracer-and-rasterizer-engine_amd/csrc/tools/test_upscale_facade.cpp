// test_upscale_facade — drives iqpt::upscaler (upscale/upscaler.hpp): a path tracer of 48x27 and rasterizers of
// 48x27 and 96x54 over the same scene and camera, the accumulator upsampled to 96x54 by factor 2. The upscaler's
// frame must be what an iqpt_upscale of its own makes of the same objects through the C ABI, its counts must add
// up to the frame, its device output must be its read-back result, and the path tracer's accumulator must be the
// same before and after. Prints one JSON line for tests/test_gpu_upscale_facade.py.
// Usage: test_upscale_facade LO.ppm UPSCALED.ppm
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "denoise/iqpt_denoise.h"
#include "raster/rasterizer.hpp"
#include "upscale/upscaler.hpp"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #c); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

int main(int argc, char** argv) {
    const std::string lo_ppm = argc > 1 ? argv[1] : "upscale_facade_lo.ppm";
    const std::string hi_ppm = argc > 2 ? argv[2] : "upscale_facade_upscaled.ppm";
    const uint32_t W = 96, H = 54, f = 2, w = W / f, h = H / f, spp = 4;
    iqpt_ctx* ctx = nullptr;
    iqpt_raster *r_lo = nullptr, *r_hi = nullptr;
    int rc = 0;
    try {
        iqpt::camera cam_lo((uint16_t)w, (uint16_t)h), cam_hi((uint16_t)W, (uint16_t)H);
        CHECK(std::memcmp(cam_lo.raw().view, cam_hi.raw().view, sizeof cam_lo.raw().view) == 0);
        CHECK(std::memcmp(cam_lo.raw().projection, cam_hi.raw().projection, sizeof cam_lo.raw().projection) == 0);
        iqpt::scene scn;
        scn.add_preset("cornell_lit");
        IQPT_THROW_FAILED(iqpt_create(0, w, h, nullptr, IQPT_DEFAULT_SEED, 8, &ctx));
        IQPT_THROW_FAILED(iqpt_raster_create(0, w, h, 1, &r_lo));
        IQPT_THROW_FAILED(iqpt_raster_create(0, W, H, 1, &r_hi));
        const iqpt_packet_desc pk = scn.build_packet();
        const iqpt_camera pt_cam = cam_lo.aligned();
        IQPT_THROW_FAILED(iqpt_set_camera(ctx, &pt_cam));
        IQPT_THROW_FAILED(iqpt_upload_packet(ctx, &pk));
        IQPT_THROW_FAILED(iqpt_raster_upload_scene(r_lo, scn.handle()));
        IQPT_THROW_FAILED(iqpt_raster_upload_scene(r_hi, scn.handle()));
        IQPT_THROW_FAILED(iqpt_raster_set_camera(r_lo, &cam_lo.raw()));
        IQPT_THROW_FAILED(iqpt_raster_set_camera(r_hi, &cam_hi.raw()));
        IQPT_THROW_FAILED(iqpt_render(ctx, spp));
        std::vector<float> acc_before((size_t)w * h * 4), acc_after(acc_before.size());
        std::vector<uint8_t> lo_bgra((size_t)w * h * 4);
        IQPT_THROW_FAILED(iqpt_read(ctx, acc_before.data(), lo_bgra.data()));
        IQPT_THROW_FAILED(iqpt_write_ppm(lo_ppm.c_str(), w, h, lo_bgra.data()));

        iqpt::upscaler::counts n;
        {
            iqpt::upscaler up(W, H, f);
            const iqpt_upscale_params p = iqpt::upscaler::default_params();
            CHECK(p.normal_squarings == 5u && p.depth_sharpness == 1024.0f);
            up.set_params(p);
            CHECK(up.frames() == 0 && up.factor() == f);
            up.frame(ctx, r_lo, r_hi);
            CHECK(up.frames() == 1);
            up.write_ppm(hi_ppm);
            n = up.stats();
            CHECK(n.guided + n.widened + n.unguided == (uint64_t)W * H);
            CHECK(n.guided > (uint64_t)W * H / 2);

            // an iqpt_upscale of its own over the same context and rasterizers
            std::vector<uint8_t> own((size_t)W * H * 4);
            std::vector<float> own_lin((size_t)W * H * 4), lin, dev((size_t)W * H * 4);
            iqpt_upscale* u = nullptr;
            IQPT_THROW_FAILED(iqpt_upscale_create(0, W, H, f, &u));
            IQPT_THROW_FAILED(iqpt_upscale_frame(u, ctx, r_lo, r_hi));
            IQPT_THROW_FAILED(iqpt_upscale_read(u, own_lin.data(), own.data()));
            IQPT_THROW_FAILED(iqpt_upscale_destroy(u));
            const auto& px = up.host_pixels();
            CHECK(px.size() * 4 == own.size() && std::memcmp(px.data(), own.data(), own.size()) == 0);
            up.read_linear(lin);
            CHECK(lin.size() == own_lin.size() && std::memcmp(lin.data(), own_lin.data(), lin.size() * sizeof(float)) == 0);
            // the device plane is what a full-size stage takes: a denoiser of no levels hands it back as it is
            iqpt_denoise* d = nullptr;
            const iqpt_denoise_params none = {0u, 0u, 0.0f, 0.0f};
            IQPT_THROW_FAILED(iqpt_denoise_create(0, W, H, &d));
            IQPT_THROW_FAILED(iqpt_denoise_set_params(d, &none));
            IQPT_THROW_FAILED(iqpt_denoise_set_guides(d, lin.data(), reinterpret_cast<const uint32_t*>(own.data())));
            IQPT_THROW_FAILED(iqpt_denoise_run_device(d, up.output_device()));
            IQPT_THROW_FAILED(iqpt_denoise_read(d, dev.data(), nullptr));
            IQPT_THROW_FAILED(iqpt_denoise_destroy(d));
            CHECK(std::memcmp(dev.data(), lin.data(), lin.size() * sizeof(float)) == 0);

            // what the facade refuses: a factor outside 2..4, a size the factor does not divide, swapped rasterizers
            bool threw = false;
            try {
                iqpt::upscaler bad(W, H, 5);
            } catch (const std::exception&) {
                threw = true;
            }
            CHECK(threw);
            threw = false;
            try {
                iqpt::upscaler bad(W + 1, H, f);
            } catch (const std::exception&) {
                threw = true;
            }
            CHECK(threw);
            threw = false;
            try {
                up.frame(ctx, r_hi, r_lo);
            } catch (const std::exception&) {
                threw = true;
            }
            CHECK(threw && up.frames() == 1);
        }
        IQPT_THROW_FAILED(iqpt_read(ctx, acc_after.data(), nullptr));
        CHECK(std::memcmp(acc_before.data(), acc_after.data(), acc_before.size() * sizeof(float)) == 0);
        std::printf("{\"ok\": true, \"accumulator_equal\": true, \"width\": %u, \"height\": %u, \"factor\": %u, \"spp\": %u, "
                    "\"guided\": %llu, \"widened\": %llu, \"unguided\": %llu}\n", W, H, f, spp, (unsigned long long)n.guided,
                    (unsigned long long)n.widened, (unsigned long long)n.unguided);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 1;
    }
    iqpt_raster_destroy(r_hi);
    iqpt_raster_destroy(r_lo);
    iqpt_destroy(ctx);
    return rc;
}
