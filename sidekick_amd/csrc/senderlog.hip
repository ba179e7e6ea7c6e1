// senderlog.hip — the device-resident sender log takes new entries where it
// lives: seqno_ids.push((seqno, id)) for every packet sent (media_client.rs:
// 104-113) and every retransmission (:318-322), for a batch of packets over
// nseg flows, fused with the drain of :298,316 — the grouped log is read once
// and written once per round.
//
// The batch arrives ungrouped, in send order.  Per call:
//   k_sl_count      one pass over d_new_flow: a flag for an index >= nseg, the
//                   entry indices 0 .. n_new - 1 (the sort's values) and the
//                   chunk histograms of the sort's first digit
//   radix.h         stable LSD sort of (flow index, entry index) over
//                   bits(nseg - 1) bits: k_row_scan + k_rs_scatter per digit,
//                   k_rs_count8 between digits.  nseg == 1: no pass, the
//                   permutation is the identity
//   k_sl_starts     where each flow's run starts in the sorted indices: one
//                   plain store per flow with traffic, no atomic (a histogram
//                   by atomics on d_new_flow, pre-aggregated per wave, took
//                   1.98 ms for 5e7 shuffled entries over 1e5 flows, as long as
//                   the move itself: profiles/sender_log/)
//   (D2H, wait)     starts and flag into pinned memory: the call's one mid-way
//                   wait; validity and capacity are decided here, before any
//                   output array is written
//   (host)          counts from the starts; offsets_out and the copy items
//                   from offsets, drain and counts (senderlog.h)
//   k_log_update    a wave per item: kept entries by a straight copy
//                   (dr_copy), a flow's new entries as a gather through the
//                   permutation, out[dst + j] = new_ids[perm[src + j]] — the
//                   stores consecutive, only the batch's loads indirect (with
//                   aux: one 8-byte load of the (id, aux) pair k_sl_count laid
//                   side by side)
// No workgroup waits on another inside a kernel: kernel boundaries order them.
//
// The drain alone (qk_u32_log_drain_segments_device, at the end) is the same
// plan with an empty batch and the same kernel, with no sort and no wait.
#include <algorithm>

#include "ctx.h"
#include "radix.h"
#include "segments.h"
#include "senderlog.h"

namespace qk {

QK_WARM_KERNEL(senderlog)

constexpr uint32_t SL_BLOCK = 256;
constexpr uint32_t SL_WAVES = SL_BLOCK / 64;
constexpr uint32_t SL_WGPC = 4;   // sort workgroups per CU, as flows.hip's grouping sort

// *flag = 0 when an index >= nseg is seen (the host sets it to ~0 before).
// pairs (null without aux): (id, aux) of every entry side by side, so the
// move's gather takes one 8-byte load per entry where it would take two
// 4-byte loads from two random lines.
// cnt (null when the sort has no pass): the first digit's chunk histograms,
// digit-major as k_rs_count writes them.
__global__ __launch_bounds__(SL_BLOCK) void k_sl_count(const uint32_t *__restrict__ flow, uint64_t n, uint64_t chunk,
                                                       uint32_t nseg, uint32_t mask, uint32_t nwg,
                                                       uint32_t *__restrict__ flag, uint32_t *__restrict__ iota,
                                                       uint32_t *__restrict__ cnt, const uint32_t *__restrict__ ids,
                                                       const uint32_t *__restrict__ aux, uint2 *__restrict__ pairs) {
    __shared__ uint32_t h[rsort::R];
    for (uint32_t j = threadIdx.x; j < rsort::R; j += SL_BLOCK) h[j] = 0;
    __syncthreads();
    const uint64_t c0 = (uint64_t)blockIdx.x * chunk, c1 = c0 + chunk < n ? c0 + chunk : n;
    for (uint64_t i = c0 + threadIdx.x; i < c1; i += SL_BLOCK) {
        const uint32_t f = flow[i];
        iota[i] = (uint32_t)i;
        if (cnt) atomicAdd(&h[f & mask], 1u);
        if (f >= nseg) *flag = 0;
        if (pairs) pairs[i] = make_uint2(ids[i], aux[i]);
    }
    if (!cnt) return;
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < rsort::R; j += SL_BLOCK) cnt[(size_t)j * nwg + blockIdx.x] = h[j];
}

// keys: the flow indices in sorted order.  start[g] = the position of flow g's
// first entry; a flow without traffic keeps the ~0 the host put there.
__global__ __launch_bounds__(SL_BLOCK) void k_sl_starts(const uint32_t *__restrict__ keys, uint32_t n, uint32_t nseg,
                                                        uint32_t *__restrict__ start) {
    const uint32_t stride = gridDim.x * SL_BLOCK;
    for (uint64_t i = (uint64_t)blockIdx.x * SL_BLOCK + threadIdx.x; i < n; i += stride) {
        const uint32_t k = keys[i];
        if ((i == 0 || keys[i - 1] != k) && k < nseg) start[k] = (uint32_t)i;
    }
}

// perm == null: the identity (one flow)
__global__ __launch_bounds__(SL_BLOCK) void k_log_update(const DrItem *__restrict__ items, uint32_t nitems,
                                                         const uint32_t *__restrict__ log,
                                                         const uint32_t *__restrict__ aux,
                                                         const uint32_t *__restrict__ new_ids,
                                                         const uint32_t *__restrict__ new_aux,
                                                         const uint2 *__restrict__ pairs,
                                                         const uint32_t *__restrict__ perm, uint32_t *__restrict__ out,
                                                         uint32_t *__restrict__ aux_out) {
    const uint32_t w = blockIdx.x * SL_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w >= nitems) return;
    const DrItem it = items[w];
    if (it.kind == DR_KEPT) {
        dr_copy(log + it.src, out + it.dst, it.n, lane);
        if (aux_out) dr_copy(aux + it.src, aux_out + it.dst, it.n, lane);
    } else if (!perm) {
        dr_copy(new_ids + it.src, out + it.dst, it.n, lane);
        if (aux_out) dr_copy(new_aux + it.src, aux_out + it.dst, it.n, lane);
    } else {
        for (uint32_t j = lane; j < it.n; j += 64) {
            const uint32_t p = perm[it.src + j];
            if (pairs) {
                const uint2 v = pairs[p];
                out[it.dst + j] = v.x;
                aux_out[it.dst + j] = v.y;
            } else {
                out[it.dst + j] = new_ids[p];
            }
        }
    }
}

// ------------------------------------------------------------------- host
// the sort's buffers in the per-packet arena: X and Y each hold n_new (key,
// value) pairs, as two arrays (values after keys) or as one pair array
struct SlSort {
    uint32_t *x = nullptr, *y = nullptr;
    RsScratch sc{};
    uint2 *pairs = nullptr;   // aux mode: (id, aux) per entry for the gather
};
static void sl_carve(Carve &cv, SlSort &b, uint64_t n, uint32_t nwg, bool pairs) {
    if (pairs) b.pairs = cv.take<uint2>(n);
    b.x = cv.take<uint32_t>(2 * n);
    b.y = cv.take<uint32_t>(2 * n);
    b.sc.take(cv, nwg, n);
}

} // namespace qk

using namespace qk;

extern "C" int qk_u32_log_update_segments_device(qk_ctx *ctx, const uint32_t *d_log, const uint32_t *d_aux,
                                                 const uint64_t *offsets, const uint64_t *drain, size_t nseg,
                                                 const uint32_t *d_new_flow, const uint32_t *d_new_ids,
                                                 const uint32_t *d_new_aux, size_t n_new, uint32_t *d_log_out,
                                                 uint32_t *d_aux_out, size_t cap, uint64_t *offsets_out,
                                                 void *stream) {
    if (!ctx) return QK_E_INVAL;
    if (nseg == 0) {
        if (offsets_out) offsets_out[0] = 0;
        return n_new ? QK_E_INVAL : QK_OK;   // every flow index is >= 0 flows
    }
    if (!offsets || !offsets_out || nseg > 0xFFFFFFFFull || n_new > 0xFFFFFFFFull) return QK_E_INVAL;
    const bool auxm = d_aux_out != nullptr;
    if (!auxm && (d_aux || d_new_aux)) return QK_E_INVAL;
    uint64_t kept = 0;
    size_t kept_items = 0;
    if (!sl_check(offsets, drain, nseg, &kept, &kept_items)) return QK_E_INVAL;
    const uint64_t n_in = offsets[nseg] - offsets[0], total = kept + n_new;
    std::lock_guard<std::mutex> lk(ctx->mu);
    QK_HIP_TRY(hipSetDevice(ctx->device));
    if (is_device_ptr(offsets) || is_device_ptr(offsets_out) || (drain && is_device_ptr(drain))) return QK_E_INVAL;
    if (n_in && (!dev_words(d_log) || (auxm && !dev_words(d_aux)))) return QK_E_INVAL;
    if (n_new && (!dev_words(d_new_flow) || !dev_words(d_new_ids) || (auxm && !dev_words(d_new_aux)))) return QK_E_INVAL;
    const uint64_t wr = std::min<uint64_t>(cap, total);   // what a call of this cap can write
    if (wr && (!dev_words(d_log_out) || (auxm && !dev_words(d_aux_out)))) return QK_E_INVAL;
    const void *in[5] = {n_in ? d_log + offsets[0] : nullptr, n_in && d_aux ? d_aux + offsets[0] : nullptr, d_new_flow,
                         d_new_ids, d_new_aux};
    const size_t inb[5] = {(size_t)n_in * 4, (size_t)n_in * 4, n_new * 4, n_new * 4, n_new * 4};
    const void *out[2] = {d_log_out, d_aux_out};
    for (int o = 0; o < 2; ++o)
        for (int i = 0; i < 5; ++i)
            if (ranges_overlap(out[o], (size_t)wr * 4, in[i], inb[i])) return QK_E_INVAL;
    if (ranges_overlap(d_log_out, (size_t)wr * 4, d_aux_out, (size_t)wr * 4)) return QK_E_INVAL;
    hipStream_t s = pick_stream(ctx, stream);

    // pinned: the counts and the flag, then the items (their number bounded
    // before the counts are known, so the buffer never moves under the copy)
    const size_t cnt_bytes = (((nseg + 1) * sizeof(uint32_t)) + 15) & ~(size_t)15;
    const size_t bound = sl_items_bound(kept_items, nseg, n_new);
    if (bound > 0xFFFFFFFFull) return QK_E_INVAL;
    if (int e = ensure_items(ctx, cnt_bytes + bound * sizeof(DrItem))) return e;
    uint32_t *h_cnt = (uint32_t *)ctx->h_items;
    DrItem *items = (DrItem *)((char *)ctx->h_items + cnt_bytes);
    const DrItem *d_items = (const DrItem *)((const char *)ctx->h_items_dev + cnt_bytes);

    const uint32_t *perm = nullptr;
    const uint2 *pairs = nullptr;
    int rc = QK_OK;
    if (n_new) {
        const int bits = bit_width32((uint32_t)(nseg - 1));
        // 16-item chunks: k_rs_count8's loads of the digit bytes (rs_sort_k rounds its plan the same way)
        RsPlan pl = rs_plan(ctx, n_new, SL_WGPC);
        pl.chunk = (pl.chunk + 15) & ~(uint64_t)15;
        const uint32_t nwg = pl.nwg;
        SlSort b;
        uint32_t *fcnt = nullptr;
        for (int pass = 0; pass < 2; ++pass) {
            Carve cp{pass ? (char *)ctx->d_flow[0] : nullptr}, cf{pass ? (char *)ctx->d_flow[1] : nullptr};
            sl_carve(cp, b, n_new, nwg, auxm && bits > 0);
            fcnt = cf.take<uint32_t>(nseg + 1);
            if (!pass) {
                if (int e = ensure_flow(ctx, 0, cp.off, s)) return e;
                if (int e = ensure_flow(ctx, 1, cf.off, s)) return e;
            }
        }
        const int passes = (bits + rsort::DBITS - 1) / rsort::DBITS;
        const uint32_t mask0 = passes ? (1u << ((bits + passes - 1) / passes)) - 1 : 0u;
        // fcnt: every start and the flag ~0
        if (hipMemsetAsync(fcnt, 0xFF, (nseg + 1) * sizeof(uint32_t), s) != hipSuccess) rc = QK_E_HIP;
        if (!rc) {
            hipLaunchKernelGGL(k_sl_count, dim3(nwg), dim3(SL_BLOCK), 0, s, d_new_flow, (uint64_t)n_new, pl.chunk,
                               (uint32_t)nseg, mask0, nwg, fcnt + nseg, b.x + n_new,
                               passes ? b.sc.cnt : (uint32_t *)nullptr, d_new_ids, d_new_aux, b.pairs);
            if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
        }
        pairs = b.pairs;
        // the first pass reads d_new_flow in place (its counts: k_sl_count's); X and Y are the sort's own
        int where = 0;
        if (!rc && passes)
            rc = rs_sort(ctx, b.x, b.x + n_new, b.y, b.y + n_new, n_new, bits, b.sc, s, where, &pl, true, d_new_flow);
        if (!rc && passes) {
            const uint32_t *keys = where ? b.y : b.x;
            perm = keys + n_new;
            hipLaunchKernelGGL(k_sl_starts, dim3(nwg), dim3(SL_BLOCK), 0, s, keys, (uint32_t)n_new, (uint32_t)nseg, fcnt);
            if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
        }
        // the call's one mid-way wait: validity and capacity are decided here
        if (!rc && (hipMemcpyAsync(h_cnt, fcnt, (nseg + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
                    hipStreamSynchronize(s) != hipSuccess))
            rc = QK_E_HIP;
        if (!rc && h_cnt[nseg] != SL_NONE) rc = QK_E_INVAL;
        if (!rc) {
            if (!passes) h_cnt[0] = 0;   // one flow: its run is the whole batch
            if (!sl_counts_from_starts(h_cnt, nseg, n_new)) rc = QK_E_HIP;
        }
    }
    // the counts add up to n_new (sl_counts_from_starts), so the result holds
    // `total` entries: over capacity, offsets_out is written and no item is
    size_t ni = 0;
    if (!rc) {
        ni = sl_plan(offsets, drain, n_new ? h_cnt : nullptr, nseg, offsets_out, total > cap ? nullptr : items);
        if (total > cap) rc = QK_E_CAPACITY;
    }
    if (!rc && ni) {
        hipLaunchKernelGGL(k_log_update, dim3((uint32_t)((ni + SL_WAVES - 1) / SL_WAVES)), dim3(SL_BLOCK), 0, s, d_items,
                           (uint32_t)ni, d_log, d_aux, d_new_ids, d_new_aux, pairs, perm, d_log_out, d_aux_out);
        if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
    }
    // the pinned items and the arenas must outlive what was enqueued (the sort too, when the call fails)
    if ((n_new || ni) && hipStreamSynchronize(s) != hipSuccess && !rc) rc = QK_E_HIP;
    return rc;
}

// The drain once offsets and drain are known to be valid (left entries stay,
// in ni copy items): capacity, then the pointers, then the copy.  *planned:
// offsets_out was written together with the items (one pass over the flows,
// as the update plans; 10^5 flows: a pass costs a tenth of the call).
static int sl_drain_copy(qk_ctx *ctx, const uint32_t *d_log, const uint32_t *d_aux, const uint64_t *offsets,
                         const uint64_t *drain, size_t nseg, uint32_t *d_log_out, uint32_t *d_aux_out, size_t cap,
                         uint64_t *offsets_out, void *stream, uint64_t left, size_t ni, bool *planned) {
    const uint64_t n = offsets[nseg] - offsets[0];
    if (left > cap) return QK_E_CAPACITY;
    if (left == 0) return QK_OK;
    if (!dev_words(d_log) || !dev_words(d_log_out) || (d_aux && (!dev_words(d_aux) || !dev_words(d_aux_out))))
        return QK_E_INVAL;
    const void *in[2] = {d_log + offsets[0], d_aux ? d_aux + offsets[0] : nullptr};
    const void *out[2] = {d_log_out, d_aux_out};
    for (int o = 0; o < 2; ++o)
        for (int i = 0; i < 2; ++i)
            if (ranges_overlap(out[o], left * 4, in[i], n * 4)) return QK_E_INVAL;
    if (ranges_overlap(d_log_out, left * 4, d_aux_out, left * 4)) return QK_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    QK_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    if (ni > 0xFFFFFFFFull) return QK_E_INVAL;
    if (int e = ensure_items(ctx, ni * sizeof(DrItem))) return e;
    sl_plan(offsets, drain, nullptr, nseg, offsets_out, (DrItem *)ctx->h_items);
    *planned = true;
    hipLaunchKernelGGL(k_log_update, dim3((uint32_t)((ni + SL_WAVES - 1) / SL_WAVES)), dim3(SL_BLOCK), 0, s,
                       (const DrItem *)ctx->h_items_dev, (uint32_t)ni, d_log, d_aux, (const uint32_t *)nullptr,
                       (const uint32_t *)nullptr, (const uint2 *)nullptr, (const uint32_t *)nullptr, d_log_out, d_aux_out);
    int rc = hipGetLastError() == hipSuccess ? QK_OK : QK_E_HIP;
    // the pinned items must outlive the kernel
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = QK_E_HIP;
    return rc;
}

// seqno_ids.drain(..idx+1) for all flows without new entries: the update's
// plan with an empty batch (counts == nullptr: kept items only) and its copy
// kernel, behind the drain's own argument rules (drain required, aux and
// aux_out together, capacity decided before any pointer is classified).
extern "C" int qk_u32_log_drain_segments_device(qk_ctx *ctx, const uint32_t *d_log, const uint32_t *d_aux,
                                                const uint64_t *offsets, const uint64_t *drain, size_t nseg,
                                                uint32_t *d_log_out, uint32_t *d_aux_out, size_t cap,
                                                uint64_t *offsets_out, void *stream) {
    if (!ctx) return QK_E_INVAL;
    if (nseg == 0) {
        if (offsets_out) offsets_out[0] = 0;
        return QK_OK;
    }
    if (!offsets || !drain || !offsets_out || (d_aux == nullptr) != (d_aux_out == nullptr)) return QK_E_INVAL;
    uint64_t left = 0;
    size_t ni = 0;
    if (!sl_check(offsets, drain, nseg, &left, &ni)) return QK_E_INVAL;
    bool planned = false;
    const int rc = sl_drain_copy(ctx, d_log, d_aux, offsets, drain, nseg, d_log_out, d_aux_out, cap, offsets_out, stream,
                                 left, ni, &planned);
    // valid offsets and drain: offsets_out is written whatever else the call returns
    if (!planned) sl_plan(offsets, drain, nullptr, nseg, offsets_out, nullptr);
    return rc;
}
