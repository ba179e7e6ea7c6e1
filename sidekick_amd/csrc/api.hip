// api.hip — device half of the quACK C ABI: context, scratch management,
// profiling events, batch encode entry points (device- and host-resident
// ids) and the synthetic id generators.  (Decode: decode.hip.)
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "ctx.h"
#include "field.h"

using namespace qk;

// teardown paths ignore the status of hipFree/hipEventDestroy/... by design
#pragma clang diagnostic ignored "-Wunused-value"
#pragma clang diagnostic ignored "-Wunused-result"

namespace qk {

QK_WARM_KERNEL(api)

// NULL is the HIP null (legacy default) stream, as in every HIP API: work
// enqueued there is ordered with the caller's default-stream work (torch's
// default stream has handle 0).
hipStream_t pick_stream(qk_ctx *ctx, void *stream) {
    (void)ctx;
    return (hipStream_t)stream;
}

int scratch_acquire(qk_ctx *ctx, hipStream_t s) {
    if (ctx->scratch_ev_valid) QK_HIP_TRY(hipStreamWaitEvent(s, ctx->scratch_ev, 0));
    return QK_OK;
}

int scratch_release(qk_ctx *ctx, hipStream_t s) {
    QK_HIP_TRY(hipEventRecord(ctx->scratch_ev, s));
    ctx->scratch_ev_valid = true;
    return QK_OK;
}

// Grow-only device buffers.  hipFree performs an implicit
// hipDeviceSynchronize, which would stall every stream of the device (the
// caller's unrelated work included) whenever a buffer grows, so a grown-out
// buffer is retired instead: it stays allocated until qk_ctx_trim or
// qk_ctx_destroy.  Growth is geometric (at least 2x), so the retired
// buffers together stay smaller than the live one.  A retired buffer may
// still be read by queued work (the encode scratch is handed between
// streams by ctx->scratch_ev; the flow arenas and the hit buffer are used
// only inside synchronous calls): nothing waits for that here.
static int regrow(qk_ctx *ctx, void **buf, size_t *have, size_t sz) {
    if (*buf) {
        ctx->retired.push_back(*buf);
        sz = std::max(sz, 2 * *have);
        *buf = nullptr;
        *have = 0;
    }
    if (hipMalloc(buf, sz) != hipSuccess) {
        (void)hipGetLastError();
        *buf = nullptr;
        return QK_E_NOMEM;
    }
    *have = sz;
    return QK_OK;
}

int ensure_scratch(qk_ctx *ctx, size_t bytes, hipStream_t s) {
    (void)s;
    if (bytes <= ctx->scratch_bytes) return QK_OK;
    return regrow(ctx, &ctx->d_scratch, &ctx->scratch_bytes, std::max(bytes, (size_t)1 << 20));
}

int ensure_flow(qk_ctx *ctx, int which, size_t bytes, hipStream_t s) {
    (void)s;
    if (bytes <= ctx->flow_bytes[which]) return QK_OK;
    // headroom for growing batches
    return regrow(ctx, &ctx->d_flow[which], &ctx->flow_bytes[which], std::max(bytes + bytes / 8, (size_t)1 << 20));
}

int ensure_hits(qk_ctx *ctx, size_t cap) {
    if (cap <= ctx->hits_cap) return QK_OK;
    size_t bytes = ctx->hits_cap * sizeof(uint64_t);
    const int rc = regrow(ctx, (void **)&ctx->d_hits, &bytes, std::max(cap, (size_t)1 << 16) * sizeof(uint64_t));
    ctx->hits_cap = rc ? 0 : bytes / sizeof(uint64_t);
    return rc;
}

int ensure_stage(qk_ctx *ctx, size_t bytes) {
    if (bytes <= ctx->stage_bytes) return QK_OK;
    for (int i = 0; i < 2; ++i) {
        if (ctx->h_stage[i]) hipHostFree(ctx->h_stage[i]);
        if (ctx->d_stage[i]) hipFree(ctx->d_stage[i]);
        ctx->h_stage[i] = ctx->d_stage[i] = nullptr;
    }
    ctx->stage_bytes = 0;
    for (int i = 0; i < 2; ++i) {
        if (hipHostMalloc(&ctx->h_stage[i], bytes, hipHostMallocDefault) != hipSuccess) return QK_E_NOMEM;
        if (hipMalloc(&ctx->d_stage[i], bytes) != hipSuccess) return QK_E_NOMEM;
    }
    ctx->stage_bytes = bytes;
    return QK_OK;
}

int ensure_items(qk_ctx *ctx, size_t bytes) {
    if (bytes <= ctx->h_items_bytes) return QK_OK;
    // the previous buffer is idle: every user synchronises before returning
    if (ctx->h_items) hipHostFree(ctx->h_items);
    ctx->h_items = ctx->h_items_dev = nullptr;
    ctx->h_items_bytes = 0;
    bytes = std::max(bytes, (size_t)1 << 20);
    if (hipHostMalloc(&ctx->h_items, bytes, hipHostMallocDefault) != hipSuccess ||
        hipHostGetDevicePointer(&ctx->h_items_dev, ctx->h_items, 0) != hipSuccess) {
        (void)hipGetLastError();
        if (ctx->h_items) hipHostFree(ctx->h_items);
        ctx->h_items = ctx->h_items_dev = nullptr;
        return QK_E_NOMEM;
    }
    ctx->h_items_bytes = bytes;
    return QK_OK;
}

bool is_device_ptr(const void *p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

int check_ctx_threshold(const qk_ctx *ctx, uint32_t threshold) {
    if (!ctx) return QK_E_INVAL;
    if (threshold == 0 || threshold > QK_MAX_THRESHOLD) return QK_E_THRESHOLD;
    return QK_OK;
}

static bool is_pinned_host_ptr(const void *p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return attr.type == hipMemoryTypeHost;
}

hipEvent_t prof_begin(qk_ctx *ctx, hipStream_t s) {
    if (!ctx->profiling) return nullptr;
    hipEvent_t e;
    if (!ctx->ev_pool.empty()) {
        e = ctx->ev_pool.back();
        ctx->ev_pool.pop_back();
    } else if (hipEventCreate(&e) != hipSuccess) {
        return nullptr;
    }
    (void)hipEventRecord(e, s);
    return e;
}

void prof_end(qk_ctx *ctx, hipStream_t s, hipEvent_t begin) {
    if (!ctx->profiling || !begin) return;
    hipEvent_t e;
    if (!ctx->ev_pool.empty()) {
        e = ctx->ev_pool.back();
        ctx->ev_pool.pop_back();
    } else if (hipEventCreate(&e) != hipSuccess) {
        ctx->ev_pool.push_back(begin);
        return;
    }
    (void)hipEventRecord(e, s);
    ctx->prof_pending.emplace_back(begin, e);
}

// ------------------------------------------------------------ fill kernels
template <typename T> __global__ void k_fill(T *out, uint64_t n, uint64_t seed, uint64_t start) {
    const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nthr)
        out[i] = (T)(splitmix_mix(seed + (start + i + 1) * GAMMA) >> (64 - 8 * sizeof(T)));
}

// Pageable -> pinned staging copy, split over a few host threads: one core's
// memcpy (~24 GB/s) is under half of the PCIe Gen5 rate the DMA can take.
static void staging_copy(void *dst, const void *src, size_t bytes) {
    static const unsigned nthr = [] {
        const unsigned hc = std::thread::hardware_concurrency();
        return hc >= 4 ? std::min(8u, hc / 2) : 1u;
    }();
    if (nthr <= 1 || bytes < ((size_t)8 << 20)) {
        memcpy(dst, src, bytes);
        return;
    }
    const size_t part = (bytes / nthr + 4095) & ~(size_t)4095;
    std::vector<std::thread> pool;
    pool.reserve(nthr - 1);
    size_t done = part;   // pieces below `done` are handed out (piece 0 to this thread)
    try {
        for (unsigned i = 1; i < nthr && done < bytes; ++i) {
            const size_t b = done, e = std::min(bytes, done + part);
            pool.emplace_back([=] { memcpy((char *)dst + b, (const char *)src + b, e - b); });
            done = e;
        }
    } catch (...) {   // no thread to spare: this thread copies the rest (no exception crosses the C ABI)
    }
    memcpy(dst, src, std::min(bytes, part));
    if (done < bytes) memcpy((char *)dst + done, (const char *)src + done, bytes - done);
    for (auto &th : pool) th.join();
}

// Host-resident ids: chunked H2D on copy_stream overlapped with the encode
// kernel on ctx->stream; two device slots.  Pinned input is DMA'd directly,
// pageable input is first copied into pinned staging (staging_copy).
template <typename IdT>
static int encode_host_impl(qk_ctx *ctx, const IdT *h_ids, size_t n, uint32_t t, uint64_t *partial_out) {
    const size_t words = Width<IdT>::partial_words(t);
    const size_t chunk_ids = (size_t)64 << 20 >> (sizeof(IdT) == 4 ? 2 : 3); // 64 MiB chunks
    const size_t chunk_bytes = chunk_ids * sizeof(IdT);
    int rc = ensure_stage(ctx, chunk_bytes);
    if (rc) return rc;
    const bool pinned = is_pinned_host_ptr(h_ids);
    hipStream_t cs = ctx->copy_stream, ks = ctx->stream;
    // destroyed on every exit; the streams are drained first so that no
    // queued wait or record still refers to them
    struct Events {
        hipEvent_t copied[2] = {nullptr, nullptr}, consumed[2] = {nullptr, nullptr};
        hipStream_t cs, ks;
        ~Events() {
            (void)hipStreamSynchronize(ks);
            (void)hipStreamSynchronize(cs);
            for (int i = 0; i < 2; ++i) {
                if (copied[i]) (void)hipEventDestroy(copied[i]);
                if (consumed[i]) (void)hipEventDestroy(consumed[i]);
            }
        }
    } ev;
    ev.cs = cs;
    ev.ks = ks;
    hipEvent_t *copied = ev.copied, *consumed = ev.consumed;
    for (int i = 0; i < 2; ++i) {
        if (hipEventCreateWithFlags(&copied[i], hipEventDisableTiming) != hipSuccess) return QK_E_HIP;
        if (hipEventCreateWithFlags(&consumed[i], hipEventDisableTiming) != hipSuccess) return QK_E_HIP;
    }
    // zero the accumulating partial
    QK_HIP_TRY(hipMemsetAsync(ctx->d_small, 0, words * 8, ks));
    bool used[2] = {false, false};
    for (size_t off = 0, c = 0; off < n; off += chunk_ids, ++c) {
        const int slot = (int)(c & 1);
        const size_t m = std::min(chunk_ids, n - off);
        if (used[slot]) {
            // the kernel that read d_stage[slot] (and the copy that read
            // h_stage[slot]) must be done before we overwrite them
            QK_HIP_TRY(hipStreamWaitEvent(cs, consumed[slot], 0));
            if (!pinned) QK_HIP_TRY(hipEventSynchronize(copied[slot]));
        }
        const void *src = h_ids + off;
        if (!pinned) {
            staging_copy(ctx->h_stage[slot], h_ids + off, m * sizeof(IdT));
            src = ctx->h_stage[slot];
        }
        QK_HIP_TRY(hipMemcpyAsync(ctx->d_stage[slot], src, m * sizeof(IdT), hipMemcpyHostToDevice, cs));
        QK_HIP_TRY(hipEventRecord(copied[slot], cs));
        QK_HIP_TRY(hipStreamWaitEvent(ks, copied[slot], 0));
        rc = Width<IdT>::launch_encode_acc(ctx, (const IdT *)ctx->d_stage[slot], m, t, ctx->d_small, ks);
        if (rc) return rc;
        QK_HIP_TRY(hipEventRecord(consumed[slot], ks));
        used[slot] = true;
    }
    QK_HIP_TRY(hipMemcpyAsync(partial_out, ctx->d_small, words * 8, hipMemcpyDeviceToHost, ks));
    QK_HIP_TRY(hipStreamSynchronize(ks));
    QK_HIP_TRY(hipStreamSynchronize(cs));
    return QK_OK;
}

// ----- typed entry points: one body for both id widths (ctx.h Width), named by the extern "C" wrappers below
template <typename T>
static int encode_device_async(qk_ctx *ctx, const T *d_ids, size_t n, uint32_t t, uint64_t *d_partial, void *stream) {
    if (!ctx || !d_partial || (n && !d_ids)) return QK_E_INVAL;
    if (t == 0 || t > QK_MAX_THRESHOLD) return QK_E_THRESHOLD;
    if ((n && !is_device_ptr(d_ids)) || !is_device_ptr(d_partial)) return QK_E_INVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    QK_HIP_TRY(hipSetDevice(ctx->device));
    return Width<T>::launch_encode(ctx, d_ids, n, t, d_partial, pick_stream(ctx, stream));
}

template <typename T>
static int encode_device(qk_ctx *ctx, const T *d_ids, size_t n, typename Width<T>::quack *q, void *stream) {
    if (!ctx || !q || (n && !d_ids)) return QK_E_INVAL;
    const uint32_t t = q->threshold;
    if (t == 0 || t > QK_MAX_THRESHOLD) return QK_E_THRESHOLD;
    if (n == 0) return QK_OK;
    if (!is_device_ptr(d_ids)) return QK_E_INVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    QK_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    if (int rc = Width<T>::launch_encode(ctx, d_ids, n, t, ctx->d_small, s)) return rc;
    QK_HIP_TRY(hipMemcpyAsync(ctx->h_small, ctx->d_small, Width<T>::partial_words(t) * 8, hipMemcpyDeviceToHost, s));
    QK_HIP_TRY(hipStreamSynchronize(s));
    return Width<T>::merge_partial(q, ctx->h_small, 1, (T)ctx->h_small[Width<T>::last_word(t)]);
}

template <typename T> static int encode_host(qk_ctx *ctx, const T *h_ids, size_t n, typename Width<T>::quack *q) {
    if (!ctx || !q || (n && !h_ids)) return QK_E_INVAL;
    const uint32_t t = q->threshold;
    if (t == 0 || t > QK_MAX_THRESHOLD) return QK_E_THRESHOLD;
    if (n == 0) return QK_OK;
    std::lock_guard<std::mutex> g(ctx->mu);
    QK_HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = encode_host_impl<T>(ctx, h_ids, n, t, ctx->h_small)) return rc;
    return Width<T>::merge_partial(q, ctx->h_small, 1, h_ids[n - 1]);
}

template <typename T>
static int fill_splitmix(qk_ctx *ctx, T *d_out, size_t n, uint64_t seed, uint64_t start, void *stream) {
    if (!ctx || (n && !d_out)) return QK_E_INVAL;
    if (n == 0) return QK_OK;
    if (!is_device_ptr(d_out)) return QK_E_INVAL;
    QK_HIP_TRY(hipSetDevice(ctx->device));
    const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, (uint64_t)ctx->num_cus * 16);
    hipLaunchKernelGGL(k_fill<T>, dim3((uint32_t)blocks), dim3(256), 0, pick_stream(ctx, stream), d_out, (uint64_t)n,
                       seed, start);
    QK_HIP_TRY(hipGetLastError());
    return QK_OK;
}

} // namespace qk

// =========================================================================
extern "C" {

int qk_device_count(int *n) {
    if (!n) return QK_E_INVAL;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) {
        (void)hipGetLastError();
        *n = 0;
        return QK_E_NO_DEVICE;
    }
    *n = c;
    return c > 0 ? QK_OK : QK_E_NO_DEVICE;
}

int qk_ctx_create(int device, qk_ctx **out) {
    if (!out) return QK_E_INVAL;
    *out = nullptr;
    int n = 0;
    if (qk_device_count(&n) != QK_OK || device < 0 || device >= n) return QK_E_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return QK_E_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return QK_E_NO_DEVICE; // code objects are gfx950-only
    if (hipSetDevice(device) != hipSuccess) return QK_E_HIP;
    qk_ctx *ctx = new (std::nothrow) qk_ctx();
    if (!ctx) return QK_E_NOMEM;
    ctx->device = device;
    ctx->num_cus = prop.multiProcessorCount;
    if (prop.maxThreadsPerMultiProcessor > 0) ctx->max_threads_per_cu = prop.maxThreadsPerMultiProcessor;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&ctx->d_small, SMALL_DEV_WORDS * sizeof(uint64_t)) != hipSuccess ||
        hipHostMalloc(&ctx->h_small, SMALL_WORDS * sizeof(uint64_t), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(&ctx->h_flow, 8 * sizeof(uint64_t), hipHostMallocDefault) != hipSuccess ||
        hipHostGetDevicePointer((void **)&ctx->h_small_dev, ctx->h_small, 0) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->stage_ev[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->stage_ev[1], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->scratch_ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->flow_ev[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->flow_ev[1], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->flow_ev[2], hipEventDisableTiming) != hipSuccess) {
        qk_ctx_destroy(ctx);
        return QK_E_HIP;
    }
    // every code object resident and the pageable-copy path set up now, not
    // inside the caller's first batch (ctx.h QK_WARM_KERNEL); the per-flow
    // work-item buffer (1 MiB) allocated
    uint64_t pageable[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ensure_items(ctx, (size_t)1 << 20) || warm_api(ctx->stream) || warm_encode(ctx->stream) || warm_decode(ctx->stream) ||
        warm_packets(ctx->stream) || warm_flows(ctx->stream) || warm_segments(ctx->stream) || warm_segdecode(ctx->stream) || warm_sender(ctx->stream) || warm_sendersteps(ctx->stream) || warm_senderlog(ctx->stream) || warm_snapshots(ctx->stream) || warm_pktsnap(ctx->stream) ||
        warm_flowtable(ctx->stream) || warm_wire(ctx->stream) || warm_comm(ctx->stream) ||
        hipMemsetAsync(ctx->d_small, 0, SMALL_DEV_WORDS * sizeof(uint64_t), ctx->stream) != hipSuccess ||
        hipMemcpyAsync(ctx->d_small, pageable, sizeof pageable, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(pageable, ctx->d_small, sizeof pageable, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) {
        qk_ctx_destroy(ctx);
        return QK_E_HIP;
    }
    *out = ctx;
    return QK_OK;
}

void qk_ctx_destroy(qk_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    for (auto &pr : ctx->prof_pending) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    for (auto e : ctx->ev_pool) hipEventDestroy(e);
    for (int i = 0; i < 2; ++i) {
        if (ctx->h_stage[i]) hipHostFree(ctx->h_stage[i]);
        if (ctx->d_stage[i]) hipFree(ctx->d_stage[i]);
        if (ctx->stage_ev[i]) hipEventDestroy(ctx->stage_ev[i]);
    }
    if (ctx->scratch_ev) hipEventDestroy(ctx->scratch_ev);
    for (hipEvent_t e : ctx->flow_ev)
        if (e) hipEventDestroy(e);
    if (ctx->d_scratch) hipFree(ctx->d_scratch);
    if (ctx->d_hits) hipFree(ctx->d_hits);
    for (void *f : ctx->d_flow)
        if (f) hipFree(f);
    for (void *r : ctx->retired) hipFree(r);
    if (ctx->d_seg_inv) hipFree(ctx->d_seg_inv);
    if (ctx->d_small) hipFree(ctx->d_small);
    if (ctx->h_small) hipHostFree(ctx->h_small);
    if (ctx->h_flow) hipHostFree(ctx->h_flow);
    if (ctx->h_items) hipHostFree(ctx->h_items);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    if (ctx->copy_stream) hipStreamDestroy(ctx->copy_stream);
    delete ctx;
}

int qk_ctx_synchronize(qk_ctx *ctx, void *stream) {
    if (!ctx) return QK_E_INVAL;
    QK_HIP_TRY(hipStreamSynchronize(pick_stream(ctx, stream)));
    return QK_OK;
}

int qk_ctx_set_profiling(qk_ctx *ctx, int on) {
    if (!ctx) return QK_E_INVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    ctx->profiling = on != 0;
    return QK_OK;
}

int qk_ctx_kernel_stats(qk_ctx *ctx, double *total_ms, uint64_t *launches) {
    if (!ctx || !total_ms || !launches) return QK_E_INVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    double tot = 0;
    uint64_t cnt = 0;
    int rc = QK_OK;
    for (auto &pr : ctx->prof_pending) {
        if (hipEventSynchronize(pr.second) != hipSuccess) rc = QK_E_HIP;
        float ms = 0;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { tot += ms; ++cnt; }
        ctx->ev_pool.push_back(pr.first);
        ctx->ev_pool.push_back(pr.second);
    }
    ctx->prof_pending.clear();
    *total_ms = tot;
    *launches = cnt;
    return rc;
}

int qk_ctx_trim(qk_ctx *ctx) {
    if (!ctx) return QK_E_INVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    if (ctx->retired.empty()) return QK_OK;
    QK_HIP_TRY(hipSetDevice(ctx->device));
    int rc = QK_OK;
    for (void *r : ctx->retired)
        if (hipFree(r) != hipSuccess) rc = QK_E_HIP;   // synchronises the device
    ctx->retired.clear();
    return rc;
}

int qk_ctx_set_grid(qk_ctx *ctx, uint32_t blocks) {
    if (!ctx) return QK_E_INVAL;
    ctx->grid_override = blocks;
    return QK_OK;
}

int qk_ctx_set_knob(qk_ctx *ctx, const char *name, int64_t value) {
    if (!ctx || !name) return QK_E_INVAL;
    struct K {
        const char *name;
        int qk_knobs::*field;
        int64_t lo, hi;
    };
    static const K table[] = {
        {"grid_mult", &qk_knobs::grid_mult, 1, 8},
        {"enc_dyn", &qk_knobs::enc_dyn, 0, 1},
        {"u32_basis", &qk_knobs::u32_basis, 0, 2},
        {"flow_hist", &qk_knobs::flow_hist, 0, 1 << 20},
        {"flow_byslot", &qk_knobs::flow_byslot, 0, 2},
        {"root_test", &qk_knobs::root_test, 0, 2},
        {"comm_fault", &qk_knobs::comm_fault, 0, 1 << 20},
        {"comm_delay_ms", &qk_knobs::comm_delay_ms, 0, 600000},
        {"rt_karg", &qk_knobs::rt_karg, 0, 1},
    };
    for (const K &k : table)
        if (strcmp(k.name, name) == 0) {
            if (value < k.lo || value > k.hi) return QK_E_INVAL;
            std::lock_guard<std::mutex> g(ctx->mu);
            ctx->knobs.*(k.field) = (int)value;
            return QK_OK;
        }
    return QK_E_INVAL;
}

// one wave: wall time from s_memrealtime (100 MHz), shader cycles from
// s_memtime; s_sleep between samples keeps the probe off the issue ports
__global__ void k_clock_probe(uint64_t *out, uint64_t ticks) {
    const uint64_t c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    uint64_t c1, r1;
    do {
        __builtin_amdgcn_s_sleep(32);
        c1 = __builtin_amdgcn_s_memtime();
        r1 = __builtin_amdgcn_s_memrealtime();
    } while (r1 - r0 < ticks);
    if (threadIdx.x == 0) {
        out[0] = c1 - c0;
        out[1] = r1 - r0;
    }
}

int qk_clock_probe(qk_ctx *ctx, uint32_t microseconds, uint64_t *d_out, void *stream) {
    if (!ctx || !d_out || !microseconds || microseconds > 10000000u) return QK_E_INVAL;
    if (!is_device_ptr(d_out)) return QK_E_INVAL;
    QK_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, (hipStream_t)stream, d_out, (uint64_t)microseconds * 100);
    QK_HIP_TRY(hipGetLastError());
    return QK_OK;
}

int qk_host_alloc(size_t bytes, void **out) {
    if (!out) return QK_E_INVAL;
    if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) { *out = nullptr; return QK_E_NOMEM; }
    return QK_OK;
}
int qk_host_free(void *p) {
    if (p && hipHostFree(p) != hipSuccess) return QK_E_HIP;
    return QK_OK;
}

// ------------------------------------------------------------ encode
int qk_u32_encode_device_async(qk_ctx *ctx, const uint32_t *d_ids, size_t n, uint32_t t, uint64_t *d_partial,
                               void *stream) {
    return encode_device_async<uint32_t>(ctx, d_ids, n, t, d_partial, stream);
}
int qk_u64_encode_device_async(qk_ctx *ctx, const uint64_t *d_ids, size_t n, uint32_t t, uint64_t *d_partial,
                               void *stream) {
    return encode_device_async<uint64_t>(ctx, d_ids, n, t, d_partial, stream);
}

int qk_u32_encode_device(qk_ctx *ctx, const uint32_t *d_ids, size_t n, qk_u32 *q, void *stream) {
    return encode_device<uint32_t>(ctx, d_ids, n, q, stream);
}
int qk_u64_encode_device(qk_ctx *ctx, const uint64_t *d_ids, size_t n, qk_u64 *q, void *stream) {
    return encode_device<uint64_t>(ctx, d_ids, n, q, stream);
}

int qk_u32_encode_host(qk_ctx *ctx, const uint32_t *h_ids, size_t n, qk_u32 *q) {
    return encode_host<uint32_t>(ctx, h_ids, n, q);
}
int qk_u64_encode_host(qk_ctx *ctx, const uint64_t *h_ids, size_t n, qk_u64 *q) {
    return encode_host<uint64_t>(ctx, h_ids, n, q);
}

// ------------------------------------------------------------ fills
int qk_fill_splitmix_u32(qk_ctx *ctx, uint32_t *d_out, size_t n, uint64_t seed, uint64_t start, void *stream) {
    return fill_splitmix<uint32_t>(ctx, d_out, n, seed, start, stream);
}
int qk_fill_splitmix_u64(qk_ctx *ctx, uint64_t *d_out, size_t n, uint64_t seed, uint64_t start, void *stream) {
    return fill_splitmix<uint64_t>(ctx, d_out, n, seed, start, stream);
}

} // extern "C"
