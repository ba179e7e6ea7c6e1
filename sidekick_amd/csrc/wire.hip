// wire.hip — the device wire leg: the message between the
// proxy's flow table and the sender's step, built and parsed in HBM.
//   emit     bincode::serialize(&quack) for the selected flows of a flow array
//            (sidekick_multi.rs:274-283), the images packed at the caller's stride
//   ingest   bincode::deserialize per received datagram (media_client.rs:
//            226-227), the newest accepted image of each flow placed in its row
//            of the peer record tensor the sender step takes
// Kernel boundaries are the only inter-workgroup ordering.
//
// Emit:
//   k_we_count     selected flows per tile of WE_TILE flows
//   k_we_scan      exclusive scan of the tile counts, the total to res[0]
//   (D2H, wait)    the total: QK_E_CAPACITY is decided before any output is written
//   k_we_compact   per tile: the ranks of its selected flows (a workgroup scan),
//                  then rows / lengths / keys of the output slots, and the
//                  threshold field of every selected record
//   k_we_emit      the m * stride output bytes cut into chunks of WE_CHUNK
//                  bytes on 16-byte boundaries of the address, whatever the
//                  stride and the base alignment: a thread forms one aligned
//                  16-byte vector from the aligned record words (wire.h
//                  wire_dword: two words funnelled; single bytes only around
//                  the tag) and stores it whole.  Single byte stores only in
//                  the first and last vector of the whole output.  The gap
//                  between an image's end and its slot's is written as zeros.
// Ingest:
//   k_wi_validate  a wave per datagram: wire.h wire_validate, the sums shared
//                  out over the lanes; the flow index tested; an accepted
//                  datagram publishes i + 1 into its flow's winner word by an
//                  atomic max (zeroed per call), so the result does not depend
//                  on the order of execution
//   (D2H, wait)    the flag of a flow index >= nseg: QK_E_INVAL is decided
//                  before d_peer or d_present is written
//   k_wi_place     a wave per datagram: the winner's image into its aligned
//                  record row, d_present, QK_WIRE_SUPERSEDED for the others
#include <algorithm>

#include "ctx.h"
#include "segments.h"
#include "wire.h"

namespace qk {

QK_WARM_KERNEL(wire)

constexpr uint32_t WR_BLOCK = 256;
constexpr uint32_t WE_IPT = 8;                       // flows per thread of a tile, consecutive
constexpr uint32_t WE_TILE = WR_BLOCK * WE_IPT;      // flows per tile
constexpr uint32_t WE_CHUNK = 16384;                 // output bytes per workgroup of k_we_emit: four vectors per thread
constexpr uint32_t WE_SCAN = 1024;
// res[] words (device, zeroed per call; read back through the pinned ctx->h_flow)
enum { WR_TOTAL = 0, WR_FLAGS = 1, WR_RES_WORDS = 4 };
enum : unsigned long long { WR_F_MISMATCH = 1, WR_F_FLOW = 2 };

__global__ __launch_bounds__(WR_BLOCK) void k_we_count(const uint8_t *__restrict__ select, uint64_t n,
                                                       uint32_t *__restrict__ tilecnt) {
    __shared__ uint32_t s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const uint64_t i0 = (uint64_t)blockIdx.x * WE_TILE + threadIdx.x * WE_IPT;
    uint32_t c = 0;
    for (uint32_t j = 0; j < WE_IPT; ++j)
        if (i0 + j < n) c += select[i0 + j] != 0;
    if (c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) tilecnt[blockIdx.x] = s_cnt;
}

// exclusive scan of the tile counts by one workgroup (each thread a contiguous
// run); res[WR_TOTAL] = the number of selected flows
__global__ __launch_bounds__(WE_SCAN) void k_we_scan(const uint32_t *__restrict__ tilecnt, uint32_t ntiles,
                                                     uint64_t *__restrict__ tilebase, unsigned long long *res) {
    __shared__ uint64_t part[WE_SCAN];
    const uint32_t per = (ntiles + WE_SCAN - 1) / WE_SCAN;
    const uint64_t b = std::min<uint64_t>((uint64_t)threadIdx.x * per, ntiles), e = std::min<uint64_t>(b + per, ntiles);
    uint64_t s = 0;
    for (uint64_t k = b; k < e; ++k) s += tilecnt[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t off = 1; off < WE_SCAN; off <<= 1) {
        const uint64_t v = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t run = part[threadIdx.x] - s;
    for (uint64_t k = b; k < e; ++k) {
        tilebase[k] = run;
        run += tilecnt[k];
    }
    if (threadIdx.x == WE_SCAN - 1) res[WR_TOTAL] = part[WE_SCAN - 1];
}

// select == null: every flow, slot = row (tilebase unused).  rows / keys_out
// may be null.  m: the total the scan reported; no slot at or past it is written.
__global__ __launch_bounds__(WR_BLOCK) void k_we_compact(const uint8_t *__restrict__ select, uint64_t n,
                                                         const uint64_t *__restrict__ tilebase,
                                                         const uint32_t *__restrict__ recs, uint32_t T,
                                                         const uint32_t *__restrict__ keys, uint32_t *__restrict__ rows,
                                                         uint32_t *__restrict__ lens, uint32_t *__restrict__ keys_out,
                                                         uint64_t m, unsigned long long *res) {
    __shared__ uint32_t s_scan[WR_BLOCK];
    const uint32_t tid = threadIdx.x, W = 4 + T;
    const uint64_t i0 = (uint64_t)blockIdx.x * WE_TILE + tid * WE_IPT;
    uint32_t mask = 0, c = 0;
    for (uint32_t j = 0; j < WE_IPT; ++j)
        if (i0 + j < n && (!select || select[i0 + j] != 0)) {
            mask |= 1u << j;
            ++c;
        }
    uint64_t slot;
    if (select) {
        s_scan[tid] = c;
        __syncthreads();
        for (uint32_t off = 1; off < WR_BLOCK; off <<= 1) {   // inclusive scan of the thread counts
            const uint32_t v = tid >= off ? s_scan[tid - off] : 0u;
            __syncthreads();
            s_scan[tid] += v;
            __syncthreads();
        }
        slot = tilebase[blockIdx.x] + s_scan[tid] - c;
    } else {
        slot = i0;
    }
    bool mismatch = false;
    for (uint32_t j = 0; j < WE_IPT; ++j) {
        if (!(mask >> j & 1) || slot >= m) continue;   // slot >= m: only when the selection changed under the call
        const uint64_t i = i0 + j;
        const uint32_t *rec = recs + i * W;
        mismatch |= rec[0] != T;
        lens[slot] = wire_len(rec, T);
        if (rows) rows[slot] = (uint32_t)i;
        if (keys_out)
            for (uint32_t k = 0; k < 3; ++k) keys_out[slot * 3 + k] = keys[i * 3 + k];
        ++slot;
    }
    if (mismatch) atomicOr(&res[WR_FLAGS], WR_F_MISMATCH);
}

// The output as (slot r, offset q < stride within it).
struct WeSrc {
    const uint32_t *recs, *rows;   // rows == null: slot r is row r
    uint32_t T;
    uint64_t stride, m, n;
    // a row index is clamped to the array (rows is the caller's memory when it asked for the rows)
    __device__ __forceinline__ const uint32_t *rec(uint64_t r) const {
        const uint64_t row = rows ? rows[r] : r;
        return recs + (row < n ? row : n - 1) * (4 + T);
    }
    // one byte; 0 past the image's end and past the last slot
    __device__ __forceinline__ uint32_t byte(uint64_t r, uint64_t q) const {
        return r < m && q < 4 * T + 17 ? wire_byte(rec(r), T, (uint32_t)q) : 0u;
    }
    // the four bytes from (r, q) on, running into slot r + 1 where the slot ends (stride > 4)
    __device__ __forceinline__ uint32_t dword(uint64_t r, uint64_t q) const {
        if (q + 4 <= stride) return r < m && q < 4 * T + 17 ? wire_dword(rec(r), T, (uint32_t)q) : 0u;
        uint32_t v = 0;
        for (uint32_t b = 0; b < 4; ++b) {
            const bool next = q + b >= stride;
            v |= byte(r + next, next ? q + b - stride : q + b) << (8 * b);
        }
        return v;
    }
};

// out: the first slot's address; its m * stride bytes are this kernel's to
// write.  Vector v of the grid is the 16 bytes at (out & ~15) + 16 v.
__global__ __launch_bounds__(WR_BLOCK) void k_we_emit(WeSrc src, uint8_t *__restrict__ out, uint64_t bytes) {
    const uint64_t mis = (uintptr_t)out & 15;
    uint8_t *const base = out - mis;                 // 16-byte aligned; bytes [mis, mis + bytes) are the output
    const uint64_t v0 = (uint64_t)blockIdx.x * (WE_CHUNK / 16);
    for (uint32_t k = threadIdx.x; k < WE_CHUNK / 16; k += WR_BLOCK) {
        const uint64_t a = (v0 + k) * 16;            // the vector's bytes: base + a .. base + a + 15
        if (a >= mis + bytes) return;
        // the slot and offset of its first output byte (of byte a, or of the output's first byte)
        const uint64_t o = a > mis ? a - mis : 0;
        uint64_t r = o / src.stride, q = o - r * src.stride;
        if (a >= mis && a + 16 <= mis + bytes) {
            uint32_t w[4];
            for (uint32_t d = 0; d < 4; ++d) {
                w[d] = src.dword(r, q);
                q += 4;
                if (q >= src.stride) {
                    q -= src.stride;
                    ++r;
                }
            }
            *reinterpret_cast<uint4 *>(base + a) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {   // the output's first or last vector: only its bytes inside the output
            const uint64_t lo = std::max<uint64_t>(a, mis), hi = std::min<uint64_t>(a + 16, mis + bytes);
            for (uint64_t x = lo; x < hi; ++x) {
                base[x] = (uint8_t)src.byte(r, q);
                if (++q >= src.stride) {
                    q = 0;
                    ++r;
                }
            }
        }
    }
}

// ------------------------------------------------------------------ ingest
constexpr uint32_t WR_WAVES = WR_BLOCK / 64;

__global__ __launch_bounds__(WR_BLOCK) void k_wi_validate(const uint8_t *__restrict__ wire, uint64_t stride,
                                                          const uint32_t *__restrict__ len,
                                                          const uint32_t *__restrict__ flow, uint32_t n, uint32_t T,
                                                          uint32_t nseg, uint32_t *__restrict__ winner,
                                                          int32_t *__restrict__ status, unsigned long long *res) {
    const uint64_t i = (uint64_t)blockIdx.x * WR_WAVES + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (i >= n) return;
    const int mine = wire_validate(wire + i * stride, len[i], stride, T, lane, 64);
    // every rule before the sums answers alike in all lanes; a sum >= p in any lane's share is QK_E_FORMAT
    const int st = __any(mine == QK_E_FORMAT) ? QK_E_FORMAT : mine;
    if (lane) return;
    status[i] = st;
    const uint32_t f = flow[i];
    if (f >= nseg) atomicOr(&res[WR_FLAGS], WR_F_FLOW);
    else if (st == QK_OK) atomicMax(&winner[f], (uint32_t)i + 1);
}

__global__ __launch_bounds__(WR_BLOCK) void k_wi_place(const uint8_t *__restrict__ wire, uint64_t stride,
                                                       const uint32_t *__restrict__ len,
                                                       const uint32_t *__restrict__ flow, uint32_t n, uint32_t T,
                                                       const uint32_t *__restrict__ winner, int32_t *__restrict__ status,
                                                       uint32_t *__restrict__ peer, uint8_t *__restrict__ present) {
    const uint64_t i = (uint64_t)blockIdx.x * WR_WAVES + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (i >= n || status[i] != QK_OK) return;
    const uint32_t f = flow[i];   // < nseg: k_wi_validate saw no other
    if (winner[f] != (uint32_t)i + 1) {
        if (lane == 0) status[i] = QK_WIRE_SUPERSEDED;
        return;
    }
    const uint8_t *buf = wire + i * stride;
    uint32_t *row = peer + (uint64_t)f * (4 + T);
    if (lane == 0) {
        uint32_t count, has_last, last;
        wire_header(buf, len[i], T, count, has_last, last);
        row[0] = T;
        row[1] = count;
        row[2] = has_last;
        row[3] = last;
        present[f] = 1;
    }
    for (uint32_t k = lane; k < T; k += 64) row[4 + k] = wire_get32(buf + 8 + 4 * (uint64_t)k);
}

// res[] into the pinned words, after everything enqueued on s
static int wr_read_res(qk_ctx *ctx, const unsigned long long *d_res, hipStream_t s, uint64_t *out) {
    QK_HIP_TRY(hipMemcpyAsync(ctx->h_flow, d_res, WR_RES_WORDS * 8, hipMemcpyDeviceToHost, s));
    QK_HIP_TRY(hipStreamSynchronize(s));
    std::copy(ctx->h_flow, ctx->h_flow + WR_RES_WORDS, out);
    return QK_OK;
}

} // namespace qk

using namespace qk;

extern "C" size_t qk_u32_wire_max(uint32_t threshold) { return 4 * (size_t)threshold + 17; }

extern "C" int qk_u32_flows_emit_device(qk_ctx *ctx, const qk_flow_key *d_keys, const uint8_t *d_sk, size_t n,
                                        uint32_t threshold, const uint8_t *d_select, size_t stride,
                                        qk_flow_key *d_keys_out, uint32_t *d_rows_out, uint8_t *d_wire_out,
                                        uint32_t *d_len_out, size_t cap, size_t *n_out, void *stream) {
    if (int e = check_ctx_threshold(ctx, threshold)) return e;
    if (!n_out || n > 0xFFFFFFFFull || stride < qk_u32_wire_max(threshold) || stride > 0xFFFFFFFFull) return QK_E_INVAL;
    *n_out = 0;
    const uint32_t T = threshold;
    const size_t rec = qk_u32_size(T);
    std::lock_guard<std::mutex> lk(ctx->mu);
    QK_HIP_TRY(hipSetDevice(ctx->device));
    if (n && (!dev_words(d_sk) || (d_select && !is_device_ptr(d_select)) || (d_keys_out && !dev_words(d_keys))))
        return QK_E_INVAL;
    if (cap && (!d_wire_out || !is_device_ptr(d_wire_out) || !dev_words(d_len_out) ||
                (d_rows_out && !dev_words(d_rows_out)) || (d_keys_out && !dev_words(d_keys_out))))
        return QK_E_INVAL;
    const void *in[3] = {d_keys_out ? d_keys : nullptr, d_sk, d_select};
    const size_t inb[3] = {n * 12, n * rec, n};
    const void *out[4] = {d_keys_out, d_rows_out, d_wire_out, d_len_out};
    const size_t outb[4] = {cap * 12, cap * 4, cap * stride, cap * 4};
    for (int o = 0; o < 4; ++o) {
        for (int i = 0; i < 3; ++i)
            if (ranges_overlap(out[o], outb[o], in[i], inb[i])) return QK_E_INVAL;
        for (int p = 0; p < o; ++p)
            if (ranges_overlap(out[o], outb[o], out[p], outb[p])) return QK_E_INVAL;
    }
    if (n == 0) return QK_OK;
    hipStream_t s = pick_stream(ctx, stream);
    const size_t ntiles = (n + WE_TILE - 1) / WE_TILE;
    unsigned long long *d_res = nullptr;
    uint32_t *tilecnt = nullptr, *rows = nullptr;
    uint64_t *tilebase = nullptr;
    if (int e = scratch_acquire(ctx, s)) return e;
    for (int pass = 0; pass < 2; ++pass) {
        Carve cv{pass ? (char *)ctx->d_scratch : nullptr};
        d_res = cv.take<unsigned long long>(WR_RES_WORDS);
        tilecnt = cv.take<uint32_t>(ntiles);
        tilebase = cv.take<uint64_t>(ntiles);
        rows = cv.take<uint32_t>(d_select && !d_rows_out ? n : 0);   // the emit kernel needs the rows of a selection
        if (!pass)
            if (int e = ensure_scratch(ctx, cv.off, s)) return e;
    }
    if (d_rows_out) rows = d_rows_out;
    int rc = QK_OK;
    uint64_t res[WR_RES_WORDS] = {0, 0, 0, 0};
    size_t m = n;
    if (hipMemsetAsync(d_res, 0, WR_RES_WORDS * 8, s) != hipSuccess) rc = QK_E_HIP;
    if (!rc && d_select) {
        hipLaunchKernelGGL(k_we_count, dim3((uint32_t)ntiles), dim3(WR_BLOCK), 0, s, d_select, (uint64_t)n, tilecnt);
        hipLaunchKernelGGL(k_we_scan, dim3(1), dim3(WE_SCAN), 0, s, tilecnt, (uint32_t)ntiles, tilebase, d_res);
        if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
        // the one place the number of selected flows is known: QK_E_CAPACITY
        // is decided here, before anything is written to the outputs
        if (!rc) rc = wr_read_res(ctx, d_res, s, res);
        if (!rc) m = (size_t)res[WR_TOTAL];
        if (!rc && m > n) rc = QK_E_HIP;
    }
    if (!rc) {
        *n_out = m;
        if (m > cap) rc = QK_E_CAPACITY;
    }
    const uint64_t bytes = (uint64_t)m * stride;
    const uint64_t nchunks = (((uintptr_t)d_wire_out & 15) + bytes + WE_CHUNK - 1) / WE_CHUNK;
    if (!rc && nchunks > 0x7FFFFFFFull) rc = QK_E_INVAL;
    if (!rc && m) {
        hipLaunchKernelGGL(k_we_compact, dim3((uint32_t)ntiles), dim3(WR_BLOCK), 0, s, d_select, (uint64_t)n, tilebase,
                           (const uint32_t *)d_sk, T, (const uint32_t *)d_keys, d_select || d_rows_out ? rows : nullptr,
                           d_len_out, (uint32_t *)d_keys_out, (uint64_t)m, d_res);
        const WeSrc src{(const uint32_t *)d_sk, d_select ? rows : nullptr, T, (uint64_t)stride, (uint64_t)m, (uint64_t)n};
        hipLaunchKernelGGL(k_we_emit, dim3((uint32_t)nchunks), dim3(WR_BLOCK), 0, s, src, d_wire_out, bytes);
        if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
        if (!rc) rc = wr_read_res(ctx, d_res, s, res);
        else (void)hipStreamSynchronize(s);
        if (!rc && (res[WR_FLAGS] & WR_F_MISMATCH)) rc = QK_E_MISMATCH;
    }
    if (int e = scratch_release(ctx, s))
        if (!rc) rc = e;
    return rc;
}

extern "C" int qk_u32_wire_ingest_device(qk_ctx *ctx, const uint8_t *d_wire, size_t stride, const uint32_t *d_len,
                                         const uint32_t *d_flow, size_t n, uint32_t threshold, size_t nseg,
                                         uint8_t *d_peer, uint8_t *d_present, int32_t *status, size_t *n_accepted,
                                         void *stream) {
    if (int e = check_ctx_threshold(ctx, threshold)) return e;
    if (!n_accepted || stride == 0 || n > 0xFFFFFFFFull || nseg > 0xFFFFFFFFull || (n && (nseg == 0 || !status)))
        return QK_E_INVAL;
    *n_accepted = 0;
    const uint32_t T = threshold;
    const size_t rec = qk_u32_size(T);
    std::lock_guard<std::mutex> lk(ctx->mu);
    QK_HIP_TRY(hipSetDevice(ctx->device));
    if (nseg && (!dev_words(d_peer) || !d_present || !is_device_ptr(d_present))) return QK_E_INVAL;
    if (n && (!d_wire || !is_device_ptr(d_wire) || !dev_words(d_len) || !dev_words(d_flow) || is_device_ptr(status)))
        return QK_E_INVAL;
    const void *in[3] = {d_wire, d_len, d_flow};
    const size_t inb[3] = {n * stride, n * 4, n * 4};
    const void *out[2] = {d_peer, d_present};
    const size_t outb[2] = {nseg * rec, nseg};
    for (int o = 0; o < 2; ++o)
        for (int i = 0; i < 3; ++i)
            if (ranges_overlap(out[o], outb[o], in[i], inb[i])) return QK_E_INVAL;
    if (ranges_overlap(d_peer, nseg * rec, d_present, nseg)) return QK_E_INVAL;
    if (nseg == 0) return QK_OK;
    hipStream_t s = pick_stream(ctx, stream);
    if (n == 0) {
        QK_HIP_TRY(hipMemsetAsync(d_present, 0, nseg, s));
        QK_HIP_TRY(hipStreamSynchronize(s));
        return QK_OK;
    }
    unsigned long long *d_res = nullptr;
    uint32_t *winner = nullptr;
    int32_t *d_status = nullptr;
    if (int e = scratch_acquire(ctx, s)) return e;
    for (int pass = 0; pass < 2; ++pass) {
        Carve cv{pass ? (char *)ctx->d_scratch : nullptr};
        d_res = cv.take<unsigned long long>(WR_RES_WORDS);
        winner = cv.take<uint32_t>(nseg);
        d_status = cv.take<int32_t>(n);
        if (!pass)
            if (int e = ensure_scratch(ctx, cv.off, s)) return e;
    }
    int rc = QK_OK;
    uint64_t res[WR_RES_WORDS] = {0, 0, 0, 0};
    const dim3 grid((uint32_t)((n + WR_WAVES - 1) / WR_WAVES));
    if (hipMemsetAsync(d_res, 0, WR_RES_WORDS * 8, s) != hipSuccess ||
        hipMemsetAsync(winner, 0, nseg * sizeof(uint32_t), s) != hipSuccess)
        rc = QK_E_HIP;
    if (!rc) {
        hipLaunchKernelGGL(k_wi_validate, grid, dim3(WR_BLOCK), 0, s, d_wire, (uint64_t)stride, d_len, d_flow,
                           (uint32_t)n, T, (uint32_t)nseg, winner, d_status, d_res);
        if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
    }
    // the call's one mid-way wait: a flow index out of range is decided here,
    // before d_peer or d_present is written
    if (!rc) rc = wr_read_res(ctx, d_res, s, res);
    else (void)hipStreamSynchronize(s);
    if (!rc && (res[WR_FLAGS] & WR_F_FLOW)) rc = QK_E_INVAL;
    if (!rc && hipMemsetAsync(d_present, 0, nseg, s) != hipSuccess) rc = QK_E_HIP;
    if (!rc) {
        hipLaunchKernelGGL(k_wi_place, grid, dim3(WR_BLOCK), 0, s, d_wire, (uint64_t)stride, d_len, d_flow, (uint32_t)n,
                           T, winner, d_status, (uint32_t *)d_peer, d_present);
        if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
        if (!rc && hipMemcpyAsync(status, d_status, n * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess)
            rc = QK_E_HIP;
        if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = QK_E_HIP;
    }
    if (!rc) {
        size_t acc = 0;
        for (size_t i = 0; i < n; ++i) acc += status[i] == QK_OK;
        *n_accepted = acc;
    }
    if (int e = scratch_release(ctx, s))
        if (!rc) rc = e;
    return rc;
}
