// iq_comm.cpp — multi-GPU frame delivery: the RCCL binding, iqpt_comm_* and iqpt_gather_*.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <mutex>

#include "runtime/iq_ctx.hpp"

using namespace iqpt::rt;

namespace {
// RCCL, bound at the first iqpt_comm_* call (dlopen by SONAME): a process that already holds an RCCL — the
// one PyTorch-ROCm ships, also librccl.so.1 — shares it instead of loading a second copy, and a single-GPU
// user of libiqpt never needs it. The entry points are RCCL's C API (/opt/rocm/include/rccl/rccl.h).
struct rccl_api {
    ncclResult_t (*get_unique_id)(ncclUniqueId*) = nullptr;
    ncclResult_t (*comm_init_rank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*comm_init_config)(ncclComm_t*, int, ncclUniqueId, int, ncclConfig_t*) = nullptr;   // optional
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    ncclResult_t (*gather)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*error_string)(ncclResult_t) = nullptr;
    std::string why;
};

const rccl_api& rccl() {
    static rccl_api api;
    static std::once_flag once;
    std::call_once(once, [] {
        void* h = nullptr;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
            if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) != nullptr) break;
        if (!h) {
            const char* e = dlerror();
            api.why = std::string("RCCL not loadable: ") + (e ? e : "librccl.so.1");
            return;
        }
        api.get_unique_id = reinterpret_cast<decltype(api.get_unique_id)>(dlsym(h, "ncclGetUniqueId"));
        api.comm_init_rank = reinterpret_cast<decltype(api.comm_init_rank)>(dlsym(h, "ncclCommInitRank"));
        api.comm_init_config = reinterpret_cast<decltype(api.comm_init_config)>(dlsym(h, "ncclCommInitRankConfig"));
        api.comm_destroy = reinterpret_cast<decltype(api.comm_destroy)>(dlsym(h, "ncclCommDestroy"));
        api.gather = reinterpret_cast<decltype(api.gather)>(dlsym(h, "ncclGather"));
        api.error_string = reinterpret_cast<decltype(api.error_string)>(dlsym(h, "ncclGetErrorString"));
        if (!api.get_unique_id || !api.comm_init_rank || !api.comm_destroy || !api.gather || !api.error_string) {
            api.get_unique_id = nullptr;
            api.why = "RCCL lacks ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclGather";
        }
    });
    return api;
}

int rccl_fail(ncclResult_t r, const char* what) {
    return iqpt::fail(IQPT_ERR_HIP, std::string(what) + ": " + (rccl().error_string ? rccl().error_string(r) : "?"));
}
}  // namespace

namespace iqpt::rt {
void free_comm(iqpt_ctx* c) {
    if (c->cstream) (void)hipStreamSynchronize(c->cstream);
    if (c->comm && rccl().comm_destroy) (void)rccl().comm_destroy(static_cast<ncclComm_t>(c->comm));
    c->comm = nullptr;
    for (int i = 0; i < iqpt::kSendRing; ++i) {
        dev_free(c->d_gsend[i]);
        event_free(c->ev_gdone[i]);
        c->gdone_pend[i] = false;
    }
    for (uint32_t** b : {&c->d_grecv, &c->d_gframe}) dev_free(*b);
    for (hipEvent_t* e : {&c->ev_gcopy, &c->ev_gend}) event_free(*e);
    for (auto& g : c->gtimed) {
        c->event_pool.push_back(g.first);
        c->event_pool.push_back(g.second);
    }
    c->gtimed.clear();
    if (c->cstream) (void)hipStreamDestroy(c->cstream);
    c->cstream = nullptr;
    c->comm_pend = false;
    c->comm_world = 0;
}
}  // namespace iqpt::rt

extern "C" {

// ---- multi-GPU frame delivery over RCCL ----------------------------------

int iqpt_comm_unique_id(void* id, size_t bytes) {
    if (!id || bytes < IQPT_COMM_ID_BYTES) return iqpt::fail(IQPT_ERR_INVALID_ARG, "id NULL or shorter than IQPT_COMM_ID_BYTES");
    if (!rccl().get_unique_id) return iqpt::fail(IQPT_ERR_UNSUPPORTED, rccl().why);
    static_assert(sizeof(ncclUniqueId) == IQPT_COMM_ID_BYTES, "RCCL's unique id size");
    ncclUniqueId u;
    const ncclResult_t r = rccl().get_unique_id(&u);
    if (r != ncclSuccess) return rccl_fail(r, "ncclGetUniqueId");
    std::memcpy(id, &u, sizeof u);
    return IQPT_OK;
}

int iqpt_comm_init(iqpt_ctx* c, int rank, int world, const void* id, size_t bytes) {
    if (!c || !id || bytes < IQPT_COMM_ID_BYTES) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument or short id");
    if (world < 1 || rank < 0 || rank >= world || (uint32_t)world > c->height)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "rank / world out of range");
    // the frame's cyclic row split (rank r owns rows r, r + S, ... of every column, S = the set's ystep), which
    // the root's assembly inverts: S = world on a node; S > world only for a one-GPU rehearsal of an S-way
    // share (the root then places the rows the communicator's ranks own)
    // (base = y0 - rank, the same on every rank: 0 on a node, rank 0's row offset in a rehearsal)
    const uint32_t split = c->set.ystep;
    const uint32_t nrows = (c->height - c->set.y0 + split - 1u) / split;
    if (c->set.x0 != 0 || c->set.x1 != c->width || c->set.y0 < (uint32_t)rank ||
        c->set.y0 - (uint32_t)rank + (uint32_t)world > split || c->set.nrows != nrows)
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "the context's pixel set is not rank's cyclic rows of a world-way split "
                                                "(iqpt_pixel_set {0, W, rank, world, ceil((H - rank) / world)})");
    if (!rccl().comm_init_rank) return iqpt::fail(IQPT_ERR_UNSUPPORTED, rccl().why);
    int st = enter(c);
    if (st) return st;
    IQPT_HIP(hipStreamSynchronize(c->stream));
    free_comm(c);
    const uint64_t stride = (uint64_t)((c->height + split - 1u) / split) * c->width;
    // the communicator's stream (its priority: iqpt_debug_set_gather; the lowest measured slower, r04 run 9:
    // the gather then finishes later and the double-buffered copies wait for it)
    int prio_least = 0, prio_greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) {
        (void)hipGetLastError();
        prio_least = prio_greatest = 0;
    }
    const int prio = c->gather_prio < 0 ? prio_least : (c->gather_prio > 0 ? prio_greatest : 0);
    if (hipStreamCreateWithPriority(&c->cstream, hipStreamNonBlocking, prio) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_gcopy, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_gend, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        free_comm(c);
        return iqpt::fail(IQPT_ERR_HIP, "communicator stream / events");
    }
    for (int i = 0; i < iqpt::kSendRing; ++i)
        if (hipMalloc(&c->d_gsend[i], stride * 16) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_gdone[i], hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            free_comm(c);
            return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "gather send buffers");
        }
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof u);
    ncclComm_t comm = nullptr;
    // collective over the ranks; a frame of a few MB per rank needs few of RCCL's blocks, and every block
    // it runs takes a CU slot from the render kernels beside it (ncclConfig_t::maxCTAs)
    ncclResult_t r;
    if (c->gather_ctas > 0 && rccl().comm_init_config) {
        ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
        cfg.minCTAs = 1;
        cfg.maxCTAs = c->gather_ctas;
        r = rccl().comm_init_config(&comm, world, u, rank, &cfg);
    } else {
        r = rccl().comm_init_rank(&comm, world, u, rank);
    }
    if (r != ncclSuccess) {
        free_comm(c);
        return rccl_fail(r, "ncclCommInitRank");
    }
    c->comm = comm;
    c->comm_rank = rank;
    c->comm_world = world;
    c->comm_stride = stride;
    c->gpar = 0;
    // the frame buffers pipelined launches write are the gather's send buffers as they are: pad every frame
    // buffer to the rank block. The last frame (d_bgra: the context's own buffer, the overlapped launches'
    // second one or a ring buffer) moves into the new own buffer; the second buffer, if there is one, is
    // re-made padded (the next overlapped launch overwrites it); a ring of the old size is dropped, rebuilt
    // at the next copy. (The views d_bgra / d_bgra_alt may point at any of these: none is kept.)
    if (stride > c->npix) {
        const size_t pbytes = (size_t)stride * sizeof(uint32_t);
        uint32_t* nb[2] = {};
        const int nbuf = c->d_alt_own ? 2 : 1;
        for (int k = 0; k < nbuf; ++k)
            if (hipMalloc(&nb[k], pbytes) != hipSuccess) {
                (void)hipGetLastError();
                for (uint32_t* b : nb)
                    if (b) (void)hipFree(b);
                free_comm(c);
                return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "padded frame buffer");
            }
        for (int k = 0; k < nbuf; ++k) IQPT_HIP(hipMemsetAsync(nb[k], 0, pbytes, c->stream));
        IQPT_HIP(hipMemcpyAsync(nb[0], c->d_bgra, (size_t)c->npix * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
        IQPT_HIP(hipStreamSynchronize(c->stream));
        (void)hipFree(c->d_bgra_own);
        c->d_bgra_own = c->d_bgra = nb[0];
        if (c->d_alt_own) {
            (void)hipFree(c->d_alt_own);
            c->d_alt_own = c->d_bgra_alt = nb[1];
        }
        for (int i = 0; i < iqpt::kPipeRing; ++i) {
            dev_free(c->d_pring[i]);
            c->pseq[i] = 0;
        }
        c->pring_on = false;
        c->copy_seq = c->pwaited = 0;
    }
    return IQPT_OK;
}

// (an unnamed namespace inside extern "C": plain names in the symbol table, kept so; see iq_ctx.hpp)
namespace {
// One gather of `words` words per pixel (comm_stride pixels) from src to the root, assembled there into dst
// (W x H pixels), on cstream behind whatever it already waits for.
int gather_from(iqpt_ctx* c, const uint32_t* src, int root, uint32_t* dst, uint32_t words) {
    // timing (iqpt_comm_time): from the moment the send buffer is complete to the end of the root's assembly —
    // the transfer plus any wait for slower ranks inside the collective
    hipEvent_t t0 = take_event(c), t1 = take_event(c);
    if (t0) (void)hipEventRecord(t0, c->cstream);
    const bool is_root = root == c->comm_rank;
    if (is_root && !c->d_grecv) {
        if (hipMalloc(&c->d_grecv, (size_t)c->comm_world * c->comm_stride * 16) != hipSuccess) {
            (void)hipGetLastError();
            c->d_grecv = nullptr;
            return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "gather receive buffer");
        }
    }
    if (!(c->gather_skip & 1)) {
        const ncclResult_t r = rccl().gather(src, is_root ? c->d_grecv : nullptr,
                                             (size_t)c->comm_stride * words, ncclUint32, root,
                                             static_cast<ncclComm_t>(c->comm), c->cstream);
        if (r != ncclSuccess) return rccl_fail(r, "ncclGather");
    }
    if (is_root && !(c->gather_skip & 2)) {
        const int le = iqpt::launch_assemble_rows(c->cstream, c->d_grecv, dst, c->width, c->height,
                                                  (uint32_t)c->comm_world, c->set.ystep,
                                                  c->set.y0 - (uint32_t)c->comm_rank, c->comm_stride, words);
        if (le != 0) return iqpt::hip_fail((hipError_t)le, "frame assembly");
    }
    if (t1) (void)hipEventRecord(t1, c->cstream);
    if (t0 && t1) c->gtimed.emplace_back(t0, t1);
    IQPT_HIP(hipEventRecord(c->ev_gend, c->cstream));
    c->comm_pend = true;
    return IQPT_OK;
}

// ... from send buffer d_gsend[b], filled on stream `from`: behind that copy and nothing else
int gather_enqueue(iqpt_ctx* c, uint32_t b, hipStream_t from, int root, uint32_t* dst, uint32_t words) {
    IQPT_HIP(hipEventRecord(c->ev_gcopy, from));
    IQPT_HIP(hipStreamWaitEvent(c->cstream, c->ev_gcopy, 0));
    int st = gather_from(c, c->d_gsend[b], root, dst, words);
    if (st) return st;
    IQPT_HIP(hipEventRecord(c->ev_gdone[b], c->cstream));
    c->gdone_pend[b] = true;
    c->gpar = (b + 1u) % (uint32_t)iqpt::kSendRing;
    return IQPT_OK;
}

int comm_check(iqpt_ctx* c, int root) {
    if (!c) return iqpt::fail(IQPT_ERR_INVALID_ARG, "ctx is NULL");
    if (!c->comm) return iqpt::fail(IQPT_ERR_NOT_READY, "no communicator: call iqpt_comm_init first");
    if (root < 0 || root >= c->comm_world) return iqpt::fail(IQPT_ERR_INVALID_ARG, "root out of range");
    return use_device(c);
}

// Synchronous gather of the accumulators (what & 1) and / or the BGRA8 frame (what & 2) into d_gframe on the
// root (W x H x 4 words, reused for each); `out_lin` / `out_bgra` (root, host) receive them.
int gather_sync(iqpt_ctx* c, int root, int what, float* out_lin, uint8_t* out_bgra) {
    int st = enter(c);
    if (st) return st;
    const bool is_root = root == c->comm_rank;
    const size_t frame_px = (size_t)c->width * c->height;
    if (is_root && !c->d_gframe && hipMalloc(&c->d_gframe, frame_px * 16) != hipSuccess) {
        (void)hipGetLastError();
        c->d_gframe = nullptr;
        return iqpt::fail(IQPT_ERR_OUT_OF_MEMORY, "assembled frame");
    }
    for (int k = 0; k < 2; ++k) {
        if (!(what & (1 << k))) continue;
        const uint32_t words = k == 0 ? 4u : 1u;
        const uint32_t b = c->gpar;
        if (c->gdone_pend[b]) IQPT_HIP(hipStreamWaitEvent(c->stream, c->ev_gdone[b], 0));
        if (k == 0) {
            const int le = iqpt::launch_relayout(c->stream, reinterpret_cast<const uint32_t*>(c->d_lin), c->d_gsend[b],
                                                 c->ncols, c->set.nrows, words, 1, true);
            if (le != 0) return iqpt::hip_fail((hipError_t)le, "gather copy");
        } else {
            IQPT_HIP(hipMemcpyAsync(c->d_gsend[b], c->d_bgra, (size_t)c->npix * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                                    c->stream));            // the BGRA8 frame is compact already
        }
        if ((st = gather_enqueue(c, b, c->stream, root, c->d_gframe, words)) != IQPT_OK) return st;
        IQPT_HIP(hipStreamSynchronize(c->cstream));
        c->comm_pend = false;
        if (is_root && (k == 0 ? (void*)out_lin : (void*)out_bgra))
            IQPT_HIP(hipMemcpy(k == 0 ? (void*)out_lin : (void*)out_bgra, c->d_gframe, frame_px * words * 4,
                               hipMemcpyDeviceToHost));
    }
    IQPT_HIP(hipStreamSynchronize(c->stream));
    return check_dev_err(c);
}
}  // namespace

int iqpt_gather_frame_async(iqpt_ctx* c, int root, void* dst_device, size_t bytes) {
    int st = comm_check(c, root);
    if (st) return st;
    if (root == c->comm_rank && (!dst_device || bytes < (size_t)c->width * c->height * 4))
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "root: destination NULL or smaller than W x H x 4 bytes");
    if (c->pipe && c->d_bgra && !c->dev_err) {
        // pipelined launches: the launch's frame buffer (compact order, padded to the rank block) is the send
        // buffer — no copy: the communicator stream waits for the launch's kernels' own end events, gathers, and
        // records the ring's reuse event (the next launches writing this buffer wait for it, pipe_begin)
        if ((st = ensure_ring(c)) != IQPT_OK) return st;
        if (!c->end1) IQPT_HIP(hipEventRecord(c->ev_pipe_end, c->stream));
        if (!c->end2) IQPT_HIP(hipEventRecord(c->ev_s2, c->stream2));
        IQPT_HIP(hipStreamWaitEvent(c->cstream, c->end1 ? c->end1 : c->ev_pipe_end, 0));
        IQPT_HIP(hipStreamWaitEvent(c->cstream, c->end2 ? c->end2 : c->ev_s2, 0));
        // the ring's reuse events stay in one order whatever mixes copies (stream3) and gathers (cstream)
        if (c->copy_seq > 0) IQPT_HIP(hipStreamWaitEvent(c->cstream, c->pev[c->copy_seq % iqpt::kPipeRing], 0));
        if ((st = gather_from(c, c->d_bgra, root, static_cast<uint32_t*>(dst_device), 1u)) != IQPT_OK) return st;
        c->copy_seq += 1;
        IQPT_HIP(hipEventRecord(c->pev[c->copy_seq % iqpt::kPipeRing], c->cstream));
        if (c->d_bgra == c->d_pring[c->pidx]) c->pseq[c->pidx] = c->copy_seq;
        return IQPT_OK;
    }
    const uint32_t b = c->gpar;
    hipStream_t used = nullptr;
    // the copy into send buffer b waits for the gather that read it two gathers ago (long done)
    if ((st = copy_frame_async(c, c->d_gsend[b], c->gdone_pend[b] ? c->ev_gdone[b] : nullptr, &used)) != IQPT_OK)
        return st;
    return gather_enqueue(c, b, used, root, static_cast<uint32_t*>(dst_device), 1u);
}

int iqpt_gather_accum(iqpt_ctx* c, int root, void* dst_device, size_t bytes) {
    int st = comm_check(c, root);
    if (st) return st;
    const size_t need = (size_t)c->width * c->height * 16;
    if (root == c->comm_rank && (!dst_device || bytes < need))
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "root: destination NULL or smaller than W x H x 16 bytes");
    if ((st = enter(c)) != IQPT_OK) return st;
    const uint32_t b = c->gpar;
    if (c->gdone_pend[b]) IQPT_HIP(hipStreamWaitEvent(c->stream, c->ev_gdone[b], 0));
    const int le = iqpt::launch_relayout(c->stream, reinterpret_cast<const uint32_t*>(c->d_lin), c->d_gsend[b], c->ncols,
                                         c->set.nrows, 4, 1, true);
    if (le != 0) return iqpt::hip_fail((hipError_t)le, "gather copy");
    if ((st = gather_enqueue(c, b, c->stream, root, static_cast<uint32_t*>(dst_device), 4u)) != IQPT_OK) return st;
    IQPT_HIP(hipStreamSynchronize(c->cstream));
    c->comm_pend = false;
    return check_dev_err(c);
}

int iqpt_gather_read(iqpt_ctx* c, int root, float* lin_rgba, uint8_t* bgra) {
    int st = comm_check(c, root);
    if (st) return st;
    // every rank takes part in the same two gathers (the accumulators, then the BGRA8 frame) whatever the
    // root's pointers are: which collectives run cannot depend on one rank's arguments; the root's pointers
    // only choose what is copied back to the host (NULL: not copied)
    return gather_sync(c, root, IQPT_GATHER_ACCUM | IQPT_GATHER_FRAME, lin_rgba, bgra);
}

int iqpt_gather_read_select(iqpt_ctx* c, int root, int what, float* lin_rgba, uint8_t* bgra) {
    int st = comm_check(c, root);
    if (st) return st;
    if (what < 1 || what > (IQPT_GATHER_ACCUM | IQPT_GATHER_FRAME))
        return iqpt::fail(IQPT_ERR_INVALID_ARG, "what must be IQPT_GATHER_ACCUM, IQPT_GATHER_FRAME or both");
    return gather_sync(c, root, what, lin_rgba, bgra);
}

int iqpt_comm_time(iqpt_ctx* c, double* total_ms, uint64_t* gathers) {
    if (!c || !total_ms || !gathers) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    *total_ms = 0.0;
    *gathers = 0;
    if (!c->comm) return IQPT_OK;
    int st = use_device(c);
    if (st) return st;
    IQPT_HIP(hipStreamSynchronize(c->cstream));
    double sum = 0.0;
    for (auto& g : c->gtimed) {
        float ms = 0.0f;
        IQPT_HIP(hipEventElapsedTime(&ms, g.first, g.second));
        sum += ms;
        c->event_pool.push_back(g.first);
        c->event_pool.push_back(g.second);
    }
    *total_ms = sum;
    *gathers = c->gtimed.size();
    c->gtimed.clear();
    return IQPT_OK;
}

int iqpt_comm_stream(iqpt_ctx* c, void** stream) {
    if (!c || !stream) return iqpt::fail(IQPT_ERR_INVALID_ARG, "NULL argument");
    if (!c->comm) return iqpt::fail(IQPT_ERR_NOT_READY, "no communicator: call iqpt_comm_init first");
    *stream = (void*)c->cstream;
    return IQPT_OK;
}

}  // extern "C"
