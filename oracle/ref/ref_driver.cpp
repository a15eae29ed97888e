// ref_driver.cpp — TEST INFRASTRUCTURE ONLY. Runs the reference engine's own hot-path source as a host loop.
//
// oracle/ref/build_ref.py compiles the reference's translation units verbatim (matrix, ray, random, onb, camera,
// material, shape, model, mesh, scene, ioniq_exception) behind the stand-in headers of oracle/ref/shim/, cuts
// the kernel ranges of path_tracer.cu into oracle/_ref/ at build time, and links them with this file into
// oracle/_ref/libref_<flavour>.so. Nothing of the reference is in this file: it only calls the reference's
// classes and lays their results out in flat arrays, next to the matching iqo_* hooks of oracle/iqpt_oracle.c.
//
// This file is compiled in two ways:
//   * with REF_KERNEL_DEPTH=<D> and REF_KERNEL_TEXT="<file>": the kernel part. It includes the extracted text of
//     path_tracer.cu (renderer_init_kernel, pixel_shader, ray_color, render_kernel) in which build_ref.py has set
//     `max_depth` to D, and registers a launcher for that depth. ray_color / pixel_shader are renamed per depth so
//     that several depths link into one library.
//   * without: the extern "C" surface (ref_*), the launch coordinates, and the few engine symbols the reference
//     sources need at link time (renderer_base::get and its exception classes).
//
// The random generator behind curandState is this project's restatement of cuRAND's XORWOW (csrc/iq_xorwow.h),
// the one part the reference does not contain (see shim/curand_kernel.h).
#include <cuda_runtime.h>
#include <curand_kernel.h>
#include <device_launch_parameters.h>

#ifdef REF_KERNEL_DEPTH
#define REF_CAT_(a, b) a##b
#define REF_CAT(a, b) REF_CAT_(a, b)
#define ray_color REF_CAT(ray_color_d, REF_KERNEL_DEPTH)
#define pixel_shader REF_CAT(pixel_shader_d, REF_KERNEL_DEPTH)
#include REF_KERNEL_TEXT
#else
#include "path_tracer.h"
#endif

#include "material.h"
#include "model.h"
#include "onb.h"
#include "random.h"

// ------------------------------------------------------------------ launches as host loops
struct ref_kernels {
    int depth;
    void (*init)(UINT width, UINT height, curandState* states);
    void (*render)(path_tracer::pixel* fb, iqvec* lin_fb, size_t num_frame, camera* cam, scene::gpu_packet packet,
                   curandState* states);
    ref_kernels* next;
};
extern ref_kernels* ref_kernel_list;

template <typename F>
static void ref_play(const dim3& grid, const dim3& block, F&& thread_body) {
    gridDim = grid;
    blockDim = block;
    for (unsigned by = 0; by < grid.y; ++by)
        for (unsigned bx = 0; bx < grid.x; ++bx)
            for (unsigned ty = 0; ty < block.y; ++ty)
                for (unsigned tx = 0; tx < block.x; ++tx) {
                    blockIdx = uint3{bx, by, 0};
                    threadIdx = uint3{tx, ty, 0};
                    thread_body();
                }
}

#ifdef REF_KERNEL_DEPTH
// ================================================================== kernel part (one per max_depth)
namespace {
// the launch shape of path_tracer.cu:50-51 (`threads` is the constant of the extracted text)
dim3 grid_for(UINT width, UINT height) { return dim3(width / threads + 1, height / threads + 1); }

void launch_init(UINT width, UINT height, curandState* states) {
    ref_play(grid_for(width, height), dim3(threads, threads),
             [&] { renderer_init_kernel(width, height, states); });
}
void launch_render(path_tracer::pixel* fb, iqvec* lin_fb, size_t num_frame, camera* cam, scene::gpu_packet packet,
                   curandState* states) {
    ref_play(grid_for(cam->get_width(), cam->get_height()), dim3(threads, threads),
             [&] { render_kernel(fb, lin_fb, num_frame, cam, packet, states); });
}
struct registrar {
    ref_kernels entry{REF_KERNEL_DEPTH, launch_init, launch_render, nullptr};
    registrar() {
        entry.next = ref_kernel_list;
        ref_kernel_list = &entry;
    }
} the_registrar;
}  // namespace

#else
// ================================================================== surface part
#include <new>
#include <string>
#include <vector>

thread_local uint3 threadIdx;
thread_local uint3 blockIdx;
thread_local dim3 blockDim;
thread_local dim3 gridDim;

ref_kernels* ref_kernel_list = nullptr;

// ---- engine symbols the reference's mesh / scene sources need at link time. The renderer is a zeroed object:
// its ComPtr members are empty, so every D3D call made through it lands on an inert stand-in (shim/wrl.h).
renderer_base* renderer_base::get() {
    alignas(renderer_base) static unsigned char zeroed[sizeof(renderer_base)] = {};
    return reinterpret_cast<renderer_base*>(zeroed);
}
renderer_base::hr_exception::hr_exception(int line, const std::string& file, HRESULT hr, const std::string& desc)
    : ioniq_exception(line, file), _hr(hr), _custom_desc(desc) {}
const char* renderer_base::hr_exception::what() const { return "ref_driver: D3D stand-in failed"; }
std::string renderer_base::hr_exception::get_description() const { return _custom_desc; }
renderer_base::cuda_exception::cuda_exception(int at_line, const std::string& in_file, cudaError code)
    : ioniq_exception(at_line, in_file), _err(code) {}
const char* renderer_base::cuda_exception::what() const { return "ref_driver: host allocation failed"; }

namespace {

iqvec v4(const float* p) { return iqvec(p[0], p[1], p[2], p[3]); }
void put(float* out, const iqvec& v) { out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w; }
iqmat m16(const float* p) {
    iqmat m;
    std::memcpy(m.m, p, sizeof m.m);
    return m;
}
void load_state(curandState* s, const uint32_t* st6) {
    for (int k = 0; k < 5; ++k) s->s.v[k] = st6[k];
    s->s.d = st6[5];
}
void store_state(uint32_t* st6, const curandState* s) {
    for (int k = 0; k < 5; ++k) st6[k] = s->s.v[k];
    st6[5] = s->s.d;
}
const ref_kernels* kernels_for(int depth) {
    for (const ref_kernels* k = ref_kernel_list; k; k = k->next)
        if (k->depth == depth) return k;
    return nullptr;
}

// the camera's private members by position (camera.h: two u16, the fov, two vectors, four matrices)
struct camera_fields {
    uint16_t width, height;
    float fovh;
    iqvec position, forward;
    iqmat view, projection, inv_view, inv_proj;
};
static_assert(sizeof(camera_fields) == sizeof(camera), "camera layout changed");

mesh* make_mesh(const char* generator, unsigned a, unsigned b, int flat, int type) {
    const std::string g(generator);
    if (g == "tri") return new tri();
    if (g == "quad") return new quad();
    if (g == "reg_polygon") return new reg_polygon(a);
    if (g == "cube") return new cube();
    if (g == "uv_sphere") return new uv_sphere(flat != 0, a, b, (mesh::type)type);
    return nullptr;
}

}  // namespace

struct ref_scene {
    scene scn;
    scene::gpu_packet pkt;
    bool built = false;
};

struct ref_frame {
    UINT width, height;
    const ref_kernels* kernels;
    camera* cam;
    path_tracer::pixel* fb;
    iqvec* lin_fb;
    curandState* states;
    size_t crt_frame = 0;
    bool pending_reset = false;
};

extern "C" {

// ------------------------------------------------------------------ what was built
int ref_flavour_b(void) {
#ifdef REF_FLAVOUR_B
    return 1;
#else
    return 0;
#endif
}
int ref_has_depth(int depth) { return kernels_for(depth) != nullptr; }

// ------------------------------------------------------------------ unit level (arrays of n cases)
// Outputs of a miss are left untouched, like the iqo_* hooks.
void ref_triangle_intersect(int64_t n, const float* v0, const float* v1, const float* v2, const float* n0,
                            const float* n1, const float* n2, const float* o, const float* d, const float* t_min,
                            const float* t_max, int32_t* hit, float* t, float* p, float* nrm, int32_t* front) {
    for (int64_t i = 0; i < n; ++i) {
        triangle tr(v4(v0 + 4 * i), v4(v1 + 4 * i), v4(v2 + 4 * i), v4(n0 + 4 * i), v4(n1 + 4 * i), v4(n2 + 4 * i));
        const ray r(v4(o + 4 * i), v4(d + 4 * i));
        hit_record hr;
        hit[i] = tr.intersect(r, t_min[i], t_max[i], &hr) ? 1 : 0;
        if (hit[i]) {
            t[i] = hr.t;
            put(p + 4 * i, hr.p);
            put(nrm + 4 * i, hr.n);
            front[i] = hr.front_face ? 1 : 0;
        }
    }
}

void ref_sphere_intersect(int64_t n, const float* c, const float* radius, const float* o, const float* d,
                          const float* t_min, const float* t_max, int32_t* hit, float* t, float* p, float* nrm,
                          int32_t* front) {
    for (int64_t i = 0; i < n; ++i) {
        sphere s(v4(c + 4 * i), radius[i]);
        const ray r(v4(o + 4 * i), v4(d + 4 * i));
        hit_record hr;
        hit[i] = s.intersect(r, t_min[i], t_max[i], &hr) ? 1 : 0;
        if (hit[i]) {
            t[i] = hr.t;
            put(p + 4 * i, hr.p);
            put(nrm + 4 * i, hr.n);
            front[i] = hr.front_face ? 1 : 0;
        }
    }
}

void ref_onb(int64_t n, const float* nrm, float* u, float* v, float* w) {
    for (int64_t i = 0; i < n; ++i) {
        const onb basis(v4(nrm + 4 * i));
        put(u + 4 * i, basis.u());
        put(v + 4 * i, basis.v());
        put(w + 4 * i, basis.w());
    }
}

void ref_real(int64_t n, uint32_t* states6, const float* lo, const float* hi, float* out) {
    for (int64_t i = 0; i < n; ++i) {
        curandState s;
        load_state(&s, states6 + 6 * i);
        out[i] = random::real(&s, lo[i], hi[i]);
        store_state(states6 + 6 * i, &s);
    }
}

void ref_cosine_weighted(int64_t n, uint32_t* states6, float* out) {
    for (int64_t i = 0; i < n; ++i) {
        curandState s;
        load_state(&s, states6 + 6 * i);
        put(out + 4 * i, random::cosine_weighted(&s));
        store_state(states6 + 6 * i, &s);
    }
}

void ref_oren_nayar(int64_t n, const float* albedo4, float sigma, const float* p, const float* nrm, const float* d_in,
                    uint32_t* states6, float* att, float* pdf, float* cosw, float* ro, float* rd, int32_t* ret) {
    const oren_nayar mat(v4(albedo4), sigma);
    for (int64_t i = 0; i < n; ++i) {
        curandState s;
        load_state(&s, states6 + 6 * i);
        hit_record hr;
        hr.p = v4(p + 4 * i);
        hr.n = v4(nrm + 4 * i);
        hr.t = 0.0f;
        hr.front_face = false;
        hr.mat = nullptr;
        const ray r_in(iqvec(0.0f), v4(d_in + 4 * i));
        scatter_record srec = {};
        ray r_out;
        ret[i] = mat.scatter(r_in, hr, &srec, &r_out, &s) ? 1 : 0;
        put(att + 4 * i, srec.attenuation);
        pdf[i] = srec.pdf_val;
        cosw[i] = srec.cos_law_weight;
        put(ro + 4 * i, r_out.origin());
        put(rd + 4 * i, r_out.direction());
        store_state(states6 + 6 * i, &s);
    }
}

void ref_emissive(int64_t n, const float* albedo4, float strength, const float* p, const float* nrm,
                  const float* d_in, uint32_t* states6, float* att, float* pdf, float* cosw, int32_t* ret) {
    const emissive light(v4(albedo4), strength);
    for (int64_t i = 0; i < n; ++i) {
        curandState s;
        load_state(&s, states6 + 6 * i);
        hit_record hr;
        hr.p = v4(p + 4 * i);
        hr.n = v4(nrm + 4 * i);
        hr.t = 0.0f;
        hr.front_face = false;
        hr.mat = nullptr;
        const ray r_in(iqvec(0.0f), v4(d_in + 4 * i));
        scatter_record srec = {};
        ray r_out;
        ret[i] = light.scatter(r_in, hr, &srec, &r_out, &s) ? 1 : 0;
        put(att + 4 * i, srec.attenuation);
        pdf[i] = srec.pdf_val;
        cosw[i] = srec.cos_law_weight;
        store_state(states6 + 6 * i, &s);
    }
}

// The normal matrix of the triangle loop (inverse of the transposed upper 3x3, reloaded as a 4x4).
void ref_normal_matrix(int64_t n, const float* transform16, float* out16) {
    for (int64_t i = 0; i < n; ++i) {
        mat3x3 upper = m16(transform16 + 16 * i).store3x3();
        upper.transpose();
        upper.inverse();
        const iqmat nm = iqmat::load3x3(upper);
        std::memcpy(out16 + 16 * i, nm.m, sizeof nm.m);
    }
}

// A vertex position as the triangle loop transforms it: loaded as a POINT, transformed with the default usage.
void ref_transform_point(int64_t n, const float* p3, const float* m16s, float* out4) {
    for (int64_t i = 0; i < n; ++i) {
        iqvec v = iqvec::load(vec3(p3[3 * i], p3[3 * i + 1], p3[3 * i + 2]), iqvec::usage::POINT);
        v.transform(m16(m16s + 16 * i));
        put(out4 + 4 * i, v);
    }
}

void ref_model_transform(const float* scale4, const float* rotation4, const float* translation4, float* out16) {
    model m("mesh");
    m.set_transforms(v4(scale4), v4(rotation4), v4(translation4));
    std::memcpy(out16, m.get_transform().m, 16 * sizeof(float));
}

// ------------------------------------------------------------------ camera
// position / forward NULL: the reference's camera as it is. Otherwise the constructor's two view lines are
// replayed with the given vectors through the reference's own look_at / inversed (the members are private and the
// reference has no setter).
void* ref_camera_create(uint16_t width, uint16_t height, float fovh, float znear, float zfar, const float* position4,
                        const float* forward4) {
    camera* cam = new camera(width, height, fovh, znear, zfar);
    if (position4 && forward4) {
        camera_fields f;
        std::memcpy(&f, cam, sizeof f);
        f.position = v4(position4);
        f.forward = v4(forward4);
        f.view = iqmat::look_at(f.position, f.position + f.forward);
        f.inv_view = f.view.inversed();
        std::memcpy((void*)cam, &f, sizeof f);
    }
    return cam;
}
void ref_camera_destroy(void* cam) { delete static_cast<camera*>(cam); }
void ref_camera_matrices(const void* cam, float* view16, float* proj16, float* inv_view16, float* inv_proj16) {
    camera_fields f;
    std::memcpy(&f, cam, sizeof f);
    std::memcpy(view16, f.view.m, 64);
    std::memcpy(proj16, f.projection.m, 64);
    std::memcpy(inv_view16, f.inv_view.m, 64);
    std::memcpy(inv_proj16, f.inv_proj.m, 64);
}
void ref_get_ray(void* cam, int64_t n, const uint32_t* x, const uint32_t* y, uint32_t* states6, float* o, float* d) {
    camera* c = static_cast<camera*>(cam);
    for (int64_t i = 0; i < n; ++i) {
        curandState s;
        load_state(&s, states6 + 6 * i);
        const ray r = c->get_ray((uint16_t)x[i], (uint16_t)y[i], &s);
        put(o + 4 * i, r.origin());
        put(d + 4 * i, r.direction());
        store_state(states6 + 6 * i, &s);
    }
}

// ------------------------------------------------------------------ meshes and scenes
// counts[3] = {vertices, indices, mesh type}; the arrays are filled when they are large enough (call twice).
int ref_mesh_generate(const char* generator, unsigned a, unsigned b, int flat, int type, float* vertices6,
                      uint32_t cap_vertices, uint32_t* indices, uint32_t cap_indices, uint32_t* counts) {
    mesh* m = make_mesh(generator, a, b, flat, type);
    if (!m) return 1;
    const std::vector<vertex>& v = m->get_vertices();
    const std::vector<UINT>& idx = m->get_indices();
    counts[0] = (uint32_t)v.size();
    counts[1] = (uint32_t)idx.size();
    counts[2] = (uint32_t)m->get_type();
    if (vertices6 && cap_vertices >= v.size()) std::memcpy(vertices6, v.data(), v.size() * sizeof(vertex));
    if (indices && cap_indices >= idx.size()) std::memcpy(indices, idx.data(), idx.size() * sizeof(UINT));
    delete m;
    return 0;
}

ref_scene* ref_scene_create(void) { return new ref_scene(); }
void ref_scene_destroy(ref_scene* s) {
    if (!s) return;
    if (s->built) s->scn.free_packet(&s->pkt);
    delete s;
}
int ref_scene_add_mesh(ref_scene* s, const char* name, const char* generator, unsigned a, unsigned b, int flat,
                       int type) {
    mesh* m = make_mesh(generator, a, b, flat, type);
    if (!m) return 1;
    s->scn.add_mesh(name, *m);
    delete m;
    return 0;
}
// the way the application adds a model: add it by mesh name, then set its transforms
int ref_scene_add_model(ref_scene* s, const char* name, const char* mesh_name, const float* scale4,
                        const float* rotation4, const float* translation4) {
    s->scn.add_model(name, model(mesh_name));
    s->scn.get_model(name).set_transforms(v4(scale4), v4(rotation4), v4(translation4));
    return 0;
}
int ref_scene_build(ref_scene* s) {
    if (s->built) s->scn.free_packet(&s->pkt);
    s->pkt = s->scn.build_packet();
    s->built = true;
    return 0;
}
// counts[3] = {triangle drawcalls, sphere drawcalls, triangle meshes}
void ref_packet_counts(const ref_scene* s, uint32_t* counts) {
    counts[0] = s->pkt.num_drawcalls[mesh::type::TRIANGLES];
    counts[1] = s->pkt.num_drawcalls[mesh::type::SPHERES];
    counts[2] = s->pkt.num_tri_meshes;
}
void ref_packet_mesh_counts(const ref_scene* s, uint32_t mesh_id, uint32_t* counts) {
    counts[0] = s->pkt.tri_meshes[mesh_id].num_vertices;
    counts[1] = s->pkt.tri_meshes[mesh_id].num_indices;
}
void ref_packet_mesh(const ref_scene* s, uint32_t mesh_id, float* vertices6, uint32_t* indices) {
    const scene::gpu_packet::tri_mesh& m = s->pkt.tri_meshes[mesh_id];
    std::memcpy(vertices6, m.vertices, m.num_vertices * sizeof(vertex));
    std::memcpy(indices, m.indices, m.num_indices * sizeof(UINT));
}
void ref_packet_tri_drawcall(const ref_scene* s, uint32_t i, float* transform16, uint32_t* mesh_id) {
    std::memcpy(transform16, s->pkt.tri_mesh_dcs[i].transform.m, 64);
    *mesh_id = s->pkt.tri_mesh_dcs[i].mesh_id;
}
void ref_packet_sphere_drawcall(const ref_scene* s, uint32_t i, float* center4, float* radius) {
    put(center4, s->pkt.sphere_dcs[i].center);
    *radius = s->pkt.sphere_dcs[i].radius;
}

// ------------------------------------------------------------------ frames: the path tracer's buffers and launches
// What path_tracer's constructor allocates and clears (BGRA frame, linear accumulator, one generator per pixel,
// frame counter 0) and what draw_scene does per launch, with the reference's camera for a width x height window.
ref_frame* ref_frame_create(uint16_t width, uint16_t height, int max_depth) {
    const ref_kernels* k = kernels_for(max_depth);
    if (!k) return nullptr;
    ref_frame* f = new ref_frame();
    f->width = width;
    f->height = height;
    f->kernels = k;
    f->cam = new camera(width, height);
    const size_t npix = (size_t)width * height;
    f->fb = static_cast<path_tracer::pixel*>(std::calloc(npix, sizeof(path_tracer::pixel)));
    f->lin_fb = static_cast<iqvec*>(std::calloc(npix, sizeof(iqvec)));
    f->states = static_cast<curandState*>(std::calloc(npix, sizeof(curandState)));
    k->init(width, height, f->states);
    return f;
}
void ref_frame_destroy(ref_frame* f) {
    if (!f) return;
    delete f->cam;
    std::free(f->fb);
    std::free(f->lin_fb);
    std::free(f->states);
    delete f;
}
void ref_frame_reset(ref_frame* f) { f->pending_reset = true; }
// `launches` kernel launches of one sample each. A pending reset clears the BGRA frame and the frame counter
// before the first of them; the counter is incremented before every launch.
int ref_frame_render(ref_frame* f, ref_scene* s, uint32_t launches) {
    if (!s->built) return 1;
    for (uint32_t i = 0; i < launches; ++i) {
        if (f->pending_reset) {
            std::memset(f->fb, 0, (size_t)f->width * f->height * sizeof(path_tracer::pixel));
            f->crt_frame = 0;
            f->pending_reset = false;
        }
        f->crt_frame++;
        f->kernels->render(f->fb, f->lin_fb, f->crt_frame, f->cam, s->pkt, f->states);
    }
    return 0;
}
void ref_frame_read(const ref_frame* f, float* lin4, uint8_t* bgra4, uint32_t* states6) {
    const size_t npix = (size_t)f->width * f->height;
    std::memcpy(lin4, f->lin_fb, npix * sizeof(iqvec));
    std::memcpy(bgra4, f->fb, npix * sizeof(path_tracer::pixel));
    for (size_t i = 0; i < npix; ++i) store_state(states6 + 6 * i, &f->states[i]);
}
void ref_frame_camera(const ref_frame* f, float* view16, float* proj16, float* inv_view16, float* inv_proj16) {
    ref_camera_matrices(f->cam, view16, proj16, inv_view16, inv_proj16);
}

}  // extern "C"
#endif
