// iq_motion.cpp — the iqpt_motion_* C ABI (include/motion/iqpt_motion.h) of libiqpt_motion.so: temporal
// reprojection's object (temporal/iq_temporal.cpp) with a motion table per view. Built on iqp::frame and the
// helpers libiqpt.so exports (post/iq_post.hpp); the resolve is iqt::launch_resolve. The kernels are
// iq_motion_kernels.hip; the definition is DESIGN.md §15.
#include <hip/hip_runtime.h>

#include <cstring>

#include "iq_host_math.hpp"
#include "motion/iq_motion.hpp"
#include "motion/iqpt_motion.h"
#include "post/iq_post.hpp"

static_assert(sizeof(iqpt_motion_entry) == 128, "DESIGN.md §15.1: an entry is 128 bytes");

struct iqpt_motion : iqp::frame {
    iqpt_temporal_params params{};
    iqt::view_planes planes[2] = {};   // planes[cur] is the current view's, the other one the previous view's
    int cur = 0;
    void* hist = nullptr;              // npix float4: the current view's history
    void* out = nullptr;               // npix float4: the last result
    uint32_t* bgra = nullptr;          // npix
    void* input = nullptr;             // npix float4: a host colour, or the accumulator resolve_ctx takes
    unsigned long long* counts = nullptr;   // 4, device
    iqpt_motion_entry* table = nullptr;     // device, table_capacity entries; grows on demand
    uint32_t table_capacity = 0;
    uint32_t table_n = 0;              // of the current view
    iqpt_camera camera{};              // the current view's
    bool have_view = false, have_result = false;
    iqp::event_timer view_t, resolve_t;     // each one stage: ev[0] before the kernel, ev[1] after it
};

namespace {

int check_table(const iqpt_motion_entry* table, uint32_t n) {
    if (n > IQPT_MOTION_MAX_ENTRIES) return iqpt::fail(IQPT_ERR_INVALID_ARG, "a motion table has at most 2^20 entries");
    if (n && !table) return iqpt::fail(IQPT_ERR_INVALID_ARG, "table is NULL with n > 0");
    for (uint32_t i = 0; i < n; ++i) {
        if (table[i].moved > 1u) return iqpt::fail(IQPT_ERR_INVALID_ARG, "a motion entry's moved must be 0 or 1");
        if (table[i].reserved[0] | table[i].reserved[1] | table[i].reserved[2])
            return iqpt::fail(IQPT_ERR_INVALID_ARG, "a motion entry's reserved words must be 0");
    }
    return IQPT_OK;
}

// the table into the object's device buffer on its stream (the caller waits for the stream before it returns)
int upload_table(iqpt_motion* m, const iqpt_motion_entry* table, uint32_t n) {
    if (n > m->table_capacity) {
        IQPT_HIP(hipStreamSynchronize(m->stream));          // a stats kernel in flight may still read the old one
        if (m->table) IQPT_HIP(hipFree(m->table));
        m->table = nullptr;
        m->table_capacity = 0;
        uint32_t cap = 64;
        while (cap < n) cap *= 2;
        IQPT_HIP(hipMalloc((void**)&m->table, (size_t)cap * sizeof(iqpt_motion_entry)));
        m->table_capacity = cap;
    }
    if (n) IQPT_HIP(hipMemcpyAsync(m->table, table, (size_t)n * sizeof(iqpt_motion_entry), hipMemcpyHostToDevice, m->stream));
    return IQPT_OK;
}

// the planes of the new view are in planes[1 - cur] already and the table in m->table: positions, history, swap
int begin(iqpt_motion* m, const iqpt_camera& cam, uint32_t n) {
    if (int st = m->view_t.collect()) return st;
    iqt::view_params p{};
    p.width = m->width;
    p.height = m->height;
    p.have_prev = m->have_view && m->have_result ? 1u : 0u;
    p.normal_min = m->params.normal_min;
    p.plane_tolerance = m->params.plane_tolerance;
    p.max_history = (float)m->params.max_history;
    std::memcpy(p.inv_proj, cam.inv_proj, sizeof p.inv_proj);
    std::memcpy(p.inv_view, cam.inv_view, sizeof p.inv_view);
    std::memcpy(p.view_prev, m->camera.view, sizeof p.view_prev);
    std::memcpy(p.proj_prev, m->camera.projection, sizeof p.proj_prev);
    const int next = 1 - m->cur;
    IQPT_HIP(hipEventRecord(m->view_t.ev[0], m->stream));
    IQPT_HIP(iqm::launch_view(m->stream, p, m->planes[next], m->planes[m->cur], m->out, m->hist, m->table, n));
    IQPT_HIP(hipEventRecord(m->view_t.ev[1], m->stream));
    m->view_t.recorded = 2;
    m->cur = next;
    m->camera = cam;
    m->table_n = n;
    m->have_view = true;
    m->have_result = false;
    return IQPT_OK;
}

int begin_planes(iqpt_motion* m, const iqpt_camera* cam, const void* normal_z, const void* id, hipMemcpyKind kind,
                 const iqpt_motion_entry* table, uint32_t n) {
    if (int st = iqp::check_camera(*m, cam)) return st;
    if (int st = check_table(table, n)) return st;
    if (int st = iqp::set_device(*m)) return st;
    if (int st = upload_table(m, table, n)) return st;
    const iqt::view_planes& v = m->planes[1 - m->cur];
    if (int st = iqp::copy_guides(*m, v.normal_z, v.id, normal_z, id, kind)) return st;      // waits for the table too
    return begin(m, *cam, n);
}

int resolve(iqpt_motion* m, const void* colour_device, uint64_t n) {
    if (!m->have_view) return iqpt::fail(IQPT_ERR_NOT_READY, "resolve before the first begin_view");
    if (int st = m->resolve_t.collect()) return st;
    const float nf = (float)(n > IQPT_TEMPORAL_MAX_HISTORY ? (uint64_t)IQPT_TEMPORAL_MAX_HISTORY : n);
    IQPT_HIP(hipEventRecord(m->resolve_t.ev[0], m->stream));
    IQPT_HIP(iqt::launch_resolve(m->stream, m->width, m->height, nf, m->hist, colour_device, m->out, m->bgra));
    IQPT_HIP(hipEventRecord(m->resolve_t.ev[1], m->stream));
    m->resolve_t.recorded = 2;
    m->have_result = true;
    return IQPT_OK;
}

void identity_entry(iqpt_motion_entry& e) {
    std::memset(&e, 0, sizeof e);
    e.back[0] = e.back[5] = e.back[10] = e.back[15] = 1.0f;
    e.nback[0] = e.nback[5] = e.nback[10] = 1.0f;
}

}  // namespace

extern "C" {

int iqpt_motion_table(const iqpt_draw_item* prev_items, uint32_t n_prev, const iqpt_draw_item* cur_items, uint32_t n_cur,
                      iqpt_motion_entry* out) {
    if (n_prev != n_cur) return iqpt::fail(IQPT_ERR_INVALID_ARG, "the two scenes have different numbers of draws");
    if (n_cur > IQPT_MOTION_MAX_ENTRIES) return iqpt::fail(IQPT_ERR_INVALID_ARG, "a motion table has at most 2^20 entries");
    if (n_cur && (!prev_items || !cur_items || !out)) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    for (uint32_t i = 0; i < n_cur; ++i)
        if (prev_items[i].num_vertices != cur_items[i].num_vertices || prev_items[i].num_indices != cur_items[i].num_indices)
            return iqpt::fail(IQPT_ERR_INVALID_ARG, "draw " + std::to_string(i) + " has another mesh in the two scenes");
    for (uint32_t i = 0; i < n_cur; ++i) {
        iqpt_motion_entry& e = out[i];
        identity_entry(e);
        if (std::memcmp(prev_items[i].transform, cur_items[i].transform, sizeof cur_items[i].transform) == 0) continue;
        e.moved = 1u;
        const iq::mat4 back = iq::inversed(iq::mat4::from(cur_items[i].transform)) * iq::mat4::from(prev_items[i].transform);
        const iq::mat4 nb = iq::normal_matrix(back);
        std::memcpy(e.back, back.m, sizeof e.back);
        std::memcpy(e.nback, nb.m, sizeof e.nback);
    }
    return IQPT_OK;
}

int iqpt_motion_default_params(iqpt_temporal_params* out) { return iqpt_temporal_default_params(out); }

int iqpt_motion_create(int device, uint32_t width, uint32_t height, iqpt_motion** out) {
    return iqp::frame_create(device, width, height, out, iqpt_motion_destroy, [](iqpt_motion* m) {
        if (int st = iqpt_temporal_default_params(&m->params)) return st;
        if (int st = m->view_t.create(2)) return st;
        if (int st = m->resolve_t.create(2)) return st;
        const size_t n = m->npix();
        iqt::view_planes *a = &m->planes[0], *b = &m->planes[1];
        return iqp::frame_alloc(*m, {{&a->normal_z, n * 16, "hipMalloc(normal_z)"},
                                     {(void**)&a->id, n * 4, "hipMalloc(id)"},
                                     {&a->pos, n * 16, "hipMalloc(pos)"},
                                     {&b->normal_z, n * 16, "hipMalloc(normal_z)"},
                                     {(void**)&b->id, n * 4, "hipMalloc(id)"},
                                     {&b->pos, n * 16, "hipMalloc(pos)"},
                                     {&m->hist, n * 16, "hipMalloc(hist)"},
                                     {&m->out, n * 16, "hipMalloc(out)"},
                                     {(void**)&m->bgra, n * 4, "hipMalloc(bgra)"},
                                     {&m->input, n * 16, "hipMalloc(input)"},
                                     {(void**)&m->counts, 4 * sizeof(unsigned long long), "hipMalloc(counts)"}});
    });
}

int iqpt_motion_destroy(iqpt_motion* m) {
    if (!m) return IQPT_OK;
    if (m->table) m->buffers.push_back(m->table);      // freed with the rest, after the stream was waited for
    m->table = nullptr;
    iqp::frame_close(*m, {&m->view_t, &m->resolve_t});
    delete m;
    return IQPT_OK;
}

int iqpt_motion_set_params(iqpt_motion* m, const iqpt_temporal_params* p) {
    if (!p) return iqpt::fail(IQPT_ERR_INVALID_ARG, "params is NULL");
    if (int st = iqt::check_params(*p)) return st;
    if (!m) return iqpt::fail(IQPT_ERR_INVALID_ARG, "motion object is NULL");
    m->params = *p;
    return IQPT_OK;
}

int iqpt_motion_begin_view(iqpt_motion* m, const iqpt_camera* cam, const float* normal_z, const uint32_t* id,
                           const iqpt_motion_entry* table, uint32_t n) {
    if (!m || !cam || !normal_z || !id) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    return begin_planes(m, cam, normal_z, id, hipMemcpyHostToDevice, table, n);
}

int iqpt_motion_begin_view_device(iqpt_motion* m, const iqpt_camera* cam, const void* normal_z_device, const void* id_device,
                                  const iqpt_motion_entry* table, uint32_t n) {
    if (!m || !cam || !normal_z_device || !id_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    return begin_planes(m, cam, normal_z_device, id_device, hipMemcpyDeviceToDevice, table, n);
}

int iqpt_motion_begin_view_raster(iqpt_motion* m, iqpt_raster* r, const iqpt_motion_entry* table, uint32_t n) {
    if (!m || !r) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = check_table(table, n)) return st;
    const iqpt_camera* cam = nullptr;
    const void *nz = nullptr, *id = nullptr;
    if (int st = iqp::raster_view(*m, r, "the object's", &cam, &nz, &id)) return st;
    return iqpt_motion_begin_view_device(m, cam, nz, id, table, n);
}

int iqpt_motion_clear(iqpt_motion* m) {
    if (!m) return iqpt::fail(IQPT_ERR_INVALID_ARG, "motion object is NULL");
    m->have_view = false;
    m->have_result = false;
    return IQPT_OK;
}

int iqpt_motion_resolve(iqpt_motion* m, const float* colour, uint64_t n) {
    if (!m || !colour) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (!m->have_view) return iqpt::fail(IQPT_ERR_NOT_READY, "resolve before the first begin_view");
    if (int st = iqp::set_device(*m)) return st;
    IQPT_HIP(hipMemcpyAsync(m->input, colour, m->npix() * 16, hipMemcpyHostToDevice, m->stream));
    IQPT_HIP(hipStreamSynchronize(m->stream));      // the caller's array may go away
    return resolve(m, m->input, n);
}

int iqpt_motion_resolve_device(iqpt_motion* m, const void* colour_device, uint64_t n) {
    if (!m || !colour_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = iqp::set_device(*m)) return st;
    return resolve(m, colour_device, n);
}

int iqpt_motion_resolve_ctx(iqpt_motion* m, iqpt_ctx* ctx) {
    if (!m || !ctx) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    uint64_t npix = 0, frames = 0;
    if (int st = iqpt_num_pixels(ctx, &npix)) return st;
    if (npix != m->npix()) return iqpt::fail(IQPT_ERR_INVALID_ARG, "the context does not own a whole frame of the object's size");
    if (!m->have_view) return iqpt::fail(IQPT_ERR_NOT_READY, "resolve before the first begin_view");
    if (int st = iqp::set_device(*m)) return st;
    IQPT_HIP(hipStreamSynchronize(m->stream));      // a resolve in flight may still read m->input
    if (int st = iqpt_copy_accum_device(ctx, m->input, m->npix() * 16)) return st;
    if (int st = iqpt_frame_count(ctx, &frames)) return st;
    return resolve(m, m->input, frames);
}

int iqpt_motion_read(iqpt_motion* m, float* lin_rgba, uint8_t* bgra) {
    if (!m) return iqpt::fail(IQPT_ERR_INVALID_ARG, "motion object is NULL");
    if (!m->have_result) return iqpt::fail(IQPT_ERR_NOT_READY, "read before a resolve of the current view");
    return iqp::read_planes(*m, lin_rgba, m->out, bgra, m->bgra);
}

int iqpt_motion_output_device(iqpt_motion* m, const void** out_device) {
    if (!m || !out_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    *out_device = m->out;
    return IQPT_OK;
}

int iqpt_motion_copy_frame_device(iqpt_motion* m, void* dst_device, size_t bytes) {
    if (!m || !dst_device) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (!m->have_result) return iqpt::fail(IQPT_ERR_NOT_READY, "copy before a resolve of the current view");
    return iqp::copy_bgra(*m, m->bgra, dst_device, bytes);
}

int iqpt_motion_sync(iqpt_motion* m) {
    if (!m) return iqpt::fail(IQPT_ERR_INVALID_ARG, "motion object is NULL");
    if (int st = iqp::set_device(*m)) return st;
    IQPT_HIP(hipStreamSynchronize(m->stream));
    return IQPT_OK;
}

int iqpt_motion_time(iqpt_motion* m, double* view_ms, uint64_t* views, double* resolve_ms, uint64_t* resolves) {
    if (!m || !view_ms || !views || !resolve_ms || !resolves) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (int st = iqp::set_device(*m)) return st;
    if (int st = m->view_t.collect()) return st;
    if (int st = m->resolve_t.collect()) return st;
    *view_ms = m->view_t.ms[0];
    *views = m->view_t.runs;
    *resolve_ms = m->resolve_t.ms[0];
    *resolves = m->resolve_t.runs;
    m->view_t.reset();
    m->resolve_t.reset();
    return IQPT_OK;
}

int iqpt_motion_stats(iqpt_motion* m, uint64_t* guided, uint64_t* valid, uint64_t* moved, uint64_t* moved_valid) {
    if (!m || !guided || !valid || !moved || !moved_valid) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (!m->have_view) return iqpt::fail(IQPT_ERR_NOT_READY, "stats before the first begin_view");
    if (int st = iqp::set_device(*m)) return st;
    unsigned long long host[4] = {0, 0, 0, 0};
    IQPT_HIP(hipMemsetAsync(m->counts, 0, sizeof host, m->stream));
    IQPT_HIP(iqm::launch_stats(m->stream, (uint32_t)m->npix(), m->planes[m->cur].id, m->hist, m->table, m->table_n, m->counts));
    IQPT_HIP(hipMemcpyAsync(host, m->counts, sizeof host, hipMemcpyDeviceToHost, m->stream));
    IQPT_HIP(hipStreamSynchronize(m->stream));
    *guided = host[0];
    *valid = host[1];
    *moved = host[2];
    *moved_valid = host[3];
    return IQPT_OK;
}

}  // extern "C"
