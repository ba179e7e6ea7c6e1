// senderlog.h — the host plan of the device-resident sender log's update
// (senderlog.hip): seqno_ids.push((seqno, id)) for a batch
// of sent packets (media_client.rs:110, :318-322) fused with
// seqno_ids.drain(..idx+1) (:298, :316), for nseg flows whose logs lie
// grouped in one device array.
//
// The plan is plain C++ (tests/native/senderlog_plan_check.cpp checks it
// against a per-flow list model): the output offsets from the input offsets,
// the drain and the batch's per-flow counts, and the copy items, one wave
// each.  Segment g of the output is
//     [ kept: input entries offsets[g] + drain[g] .. offsets[g + 1] )
//     [ new:  the batch's entries of flow g, in send order           )
// The batch arrives ungrouped; a stable sort by flow index (radix.h) leaves
// flow g's entries, in send order, at positions first[g] .. first[g] +
// counts[g] of the sorted batch, first = the exclusive prefix of counts.  A
// kept item's src is a position in the input arrays, a new item's src a
// position in the sorted batch.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace qk {

constexpr uint32_t DR_ITEM = 2048;   // entries per copy item, one wave each
constexpr uint32_t DR_KEPT = 0, DR_NEW = 1;
struct DrItem {
    uint64_t src, dst;   // positions in the input (kept) or the sorted batch (new) / the output arrays
    uint32_t n, kind;    // kind: DR_KEPT a straight copy, DR_NEW a gather through the sort's permutation
};

// decreasing offsets or a drain longer than its segment: false.  Otherwise
// *kept = the entries that stay, *kept_items = the copy items they take.
inline bool sl_check(const uint64_t *offsets, const uint64_t *drain, size_t nseg, uint64_t *kept, size_t *kept_items) {
    uint64_t k = 0;
    size_t ni = 0;
    for (size_t g = 0; g < nseg; ++g) {
        if (offsets[g + 1] < offsets[g]) return false;
        const uint64_t len = offsets[g + 1] - offsets[g], d = drain ? drain[g] : 0;
        if (d > len) return false;
        k += len - d;
        ni += (size_t)((len - d + DR_ITEM - 1) / DR_ITEM);
    }
    *kept = k;
    *kept_items = ni;
    return true;
}

// h[g]: the position of flow g's first entry in the batch sorted by flow, or
// SL_NONE for a flow without traffic (k_sl_starts).  In place: h[g] = the
// flow's number of entries.  False when the starts are no ascending cover of
// 0 .. n_new, so the counts always add up to n_new.
constexpr uint32_t SL_NONE = 0xFFFFFFFFu;
inline bool sl_counts_from_starts(uint32_t *h, size_t nseg, uint64_t n_new) {
    uint64_t next = n_new;
    for (size_t g = nseg; g-- > 0;) {
        const uint32_t s = h[g];
        if (s == SL_NONE) {
            h[g] = 0;
            continue;
        }
        if (s >= next) return false;
        h[g] = (uint32_t)(next - s);
        next = s;
    }
    return next == 0;
}

// an upper bound of the plan's item count that needs no counts: the kept
// items exactly, and n_new entries over at most min(nseg, n_new) flows
inline size_t sl_items_bound(size_t kept_items, size_t nseg, uint64_t n_new) {
    return kept_items + (size_t)(n_new / DR_ITEM) + (size_t)(n_new < nseg ? n_new : nseg);
}

// offsets_out[0 .. nseg] and, where items != nullptr, the items, flow by flow,
// kept before new, in one pass.  counts == nullptr: an empty batch.  Returns
// the number of items of the plan (written or not).
inline size_t sl_plan(const uint64_t *offsets, const uint64_t *drain, const uint32_t *counts, size_t nseg,
                      uint64_t *offsets_out, DrItem *items) {
    size_t k = 0;
    uint64_t first = 0, at = 0;   // flow g's place in the sorted batch / in the output
    offsets_out[0] = 0;
    for (size_t g = 0; g < nseg; ++g) {
        const uint64_t d = drain ? drain[g] : 0, kept = offsets[g + 1] - offsets[g] - d, add = counts ? counts[g] : 0;
        if (items) {
            for (uint64_t o = 0; o < kept; o += DR_ITEM)
                items[k++] = {offsets[g] + d + o, at + o, (uint32_t)(kept - o < DR_ITEM ? kept - o : DR_ITEM), DR_KEPT};
            for (uint64_t o = 0; o < add; o += DR_ITEM)
                items[k++] = {first + o, at + kept + o, (uint32_t)(add - o < DR_ITEM ? add - o : DR_ITEM), DR_NEW};
        } else {
            k += (size_t)((kept + DR_ITEM - 1) / DR_ITEM) + (size_t)((add + DR_ITEM - 1) / DR_ITEM);
        }
        first += add;
        at += kept + add;
        offsets_out[g + 1] = at;
    }
    return k;
}

} // namespace qk

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace qk {

// n words src -> dst by one wave: 16 bytes per lane where the two addresses
// share their alignment, a scalar head up to the first 16-byte boundary
__device__ __forceinline__ void dr_copy(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, uint32_t n,
                                        uint32_t lane) {
    const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst;
    if (((a ^ b) & 15) != 0) {
        for (uint32_t i = lane; i < n; i += 64) dst[i] = src[i];
        return;
    }
    const uint32_t h4 = (uint32_t)((16 - (a & 15)) & 15) / 4, head = h4 < n ? h4 : n;
    if (lane < head) dst[lane] = src[lane];
    const uint32_t nv = (n - head) / 4;
    const uint4 *sv = reinterpret_cast<const uint4 *>(src + head);
    uint4 *dv = reinterpret_cast<uint4 *>(dst + head);
    for (uint32_t v = lane; v < nv; v += 64) dv[v] = sv[v];
    const uint32_t done = head + 4 * nv;
    if (done + lane < n) dst[done + lane] = src[done + lane];
}

} // namespace qk
#endif
