// segdecode.h — internal: the batched per-flow decode (segdecode.hip) as its
// two callers see it: qk_u32_decode_segments_device, which decodes the
// caller's diff records, and the batched sender step (sender.hip), which forms
// the diff records on the device first and subtracts the hits afterwards.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "ctx.h"
#include "segments.h"

namespace qk {

constexpr int SD_BLOCK = 256;
constexpr uint32_t SD_ITEM = QK_SEG_DECODE_ITEM;   // log entries per work item
constexpr uint32_t SD_WORDS = SD_ITEM / 64;        // hit-mask words per work item
static_assert(SD_ITEM % SD_BLOCK == 0 && SD_WORDS <= 64, "k_seg_hit_write: one lane per mask word");
// LDS words for the coefficient rows of one packed work item: a run of short
// segments ends after SD_COEF_WORDS / T segments (at most SD_MAXSEG)
constexpr uint32_t SD_COEF_WORDS = QK_SEG_DECODE_COEF_WORDS;
constexpr uint32_t SD_MAXSEG = QK_SEG_DECODE_MAXSEG;

struct SdItem {
    uint64_t lo;     // first log position
    uint32_t n;      // entries, 1..SD_ITEM
    uint32_t seg0;   // first segment
    uint32_t nseg;   // segments (1: possibly a slice of a long one)
    uint32_t pad;
};

inline uint32_t sd_maxseg(uint32_t T) { return std::max(1u, std::min(SD_MAXSEG, SD_COEF_WORDS / T)); }

#if defined(__HIPCC__)
// the item's segment boundaries, relative to its first entry and clamped to
// the item, into so[0 .. nseg]
__device__ __forceinline__ void sd_stage_offsets(const SdItem &it, const uint64_t *__restrict__ offs, uint32_t *so) {
    for (uint32_t k = threadIdx.x; k <= it.nseg; k += SD_BLOCK) {
        const uint64_t o = offs[(uint64_t)it.seg0 + k];
        so[k] = o <= it.lo ? 0u : o - it.lo >= it.n ? it.n : (uint32_t)(o - it.lo);
    }
}
// the segment (relative to seg0) of entry i of the item: the last r with
// so[r] <= i, so an empty segment never owns an entry
__device__ __forceinline__ uint32_t sd_segment_of(const uint32_t *so, uint32_t nseg, uint32_t i) {
    uint32_t lo = 0, hi = nseg;   // so[lo] <= i < so[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (so[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}
#endif

// per-segment device buffers, carved from the context's per-flow arena
struct SdSeg {
    uint32_t *rec = nullptr;   // the records (the caller's, when they are device memory)
    uint32_t *coef = nullptr, *deg = nullptr, *segcnt = nullptr;
    int32_t *status = nullptr;
    uint64_t *offs = nullptr, *total = nullptr;
    unsigned long long *stop = nullptr;
};

// One batched decode: the work items of its log, and where its buffers lie in
// the two arenas (per-segment ones in d_flow[1], per-item ones in d_flow[0]).
struct SdPlan {
    std::vector<SdItem> items;
    uint32_t maxseg = 1;   // the most segments any item holds (sizes the LDS of a launch)
    uint64_t n = 0;        // log entries
    uint64_t hcap = 0;     // hit positions kept on the device
    SdSeg b;
    uint64_t *d_mask = nullptr, *d_base = nullptr, *d_hit = nullptr;
    uint32_t *d_icnt = nullptr;
    const SdItem *d_items = nullptr;
};

// the work items of offsets[0 .. nseg] and the hit room for a caller's `cap`
void sd_plan(SdPlan &p, const uint64_t *offsets, size_t nseg, uint32_t T, size_t cap);
// the plan's buffers from the two arenas (measuring when the carves have no
// base): a caller with buffers of its own takes them from the same carves
void sd_carve_plan(Carve &seg, Carve &item, SdPlan &p, size_t nseg, uint32_t T, bool host_rec);
// the items into the pinned buffer the kernels read, the offsets uploaded, the
// stop positions and counts reset
int sd_upload(qk_ctx *ctx, SdPlan &p, const uint64_t *offsets, size_t nseg, hipStream_t s);
// Newton, root test, hit count, scan and hit write, enqueued on s after
// sd_upload (diffs: nseg records, host or device)
int sd_enqueue(qk_ctx *ctx, SdPlan &p, const uint8_t *diffs, bool host_rec, const uint32_t *d_log, size_t nseg,
               uint32_t T, int stop_at_last, hipStream_t s);
// the two ends of sd_enqueue for a caller with a root test of its own
// (sendersteps.hip): Newton over nseg device or host records into b.coef /
// b.deg / b.status; the scan of the item counts and the hit write over the
// plan's mask
int sd_newton(qk_ctx *ctx, const uint8_t *diffs, bool host_rec, size_t nseg, uint32_t T, SdSeg &b, hipStream_t s);
int sd_compact(SdPlan &p, hipStream_t s);
// after the caller has waited for s (status and segcnt copied back by it):
// hit_offsets, *n_hits and the hits themselves
int sd_collect(const SdPlan &p, const int32_t *status, const uint32_t *segcnt, uint64_t total, size_t nseg,
               uint64_t *hits, size_t cap, uint64_t *hit_offsets, size_t *n_hits);

} // namespace qk
