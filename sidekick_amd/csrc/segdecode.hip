// segdecode.hip — batched per-flow decode: one pass over nseg (diff, log
// segment) pairs, the decode twin of the segmented encode (segments.hip).
//
// A sender that serves many flows gets one quACK per flow (what SidekickMulti
// emits, sidekick_multi.rs:65-90) and runs media_client.rs:296-313 per flow:
//     diff.sub_assign(quack); coeffs = diff.to_coeffs();
//     for id in log { if Some(id) == diff.last_value() { break }
//                     if eval(&coeffs, id) == 0 { missing.push } }
// Here the diffs are nseg qk_u32 records and the logs one grouped device
// array with CSR offsets, as qk_u32_encode_segments_device takes them.
//   k_seg_newton<G>   Newton's identities (host.cpp qk_u32_to_coeffs), a group
//                     of G lanes per segment, the S and c rows in LDS
//   k_seg_root_test   one workgroup per work item (<= QK_SEG_DECODE_ITEM log
//                     entries: a slice of one long segment, or a run of whole
//                     short segments), the items' coefficient rows in LDS;
//                     one hit bit per entry, atomicMin of the stop position
//   k_seg_hit_count   drops the hit bits at or after their segment's stop,
//                     counts per item and per segment
//   k_seg_scan        exclusive scan of the item counts
//   k_seg_hit_write   the surviving positions, in log order, at their rank
// The hit list is compacted in order on the device (count, scan, write): it is
// ascending and deterministic with no sort, and the host's per-call work is
// O(nseg): the work items, and the prefix sum of the segment counts.
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx.h"
#include "field.h"
#include "segdecode.h"
#include "segments.h"

namespace qk {

QK_WARM_KERNEL(segdecode)

static_assert(sizeof(qk_u32) == 16, "qk_u32 header is 4 words");

// ------------------------------------------------------------------ Newton
// c[i] = -(S[i] + sum_{j<i} S[j] c[i-j-1]) / (i+1), i = 0..d-1 (host.cpp:368).
// The recurrence in i is sequential; the sum is shared by the G lanes of the
// segment's group (lane j takes terms j, j+G, ...) and added up by a xor
// butterfly.  Every product is lazy (< 2^32) and the 64-bit sum of at most
// 1024 of them cannot overflow; c[i] is canonical.  The workgroup runs to its
// largest degree, a barrier per step (groups of smaller degree idle).
// Rows are 2T + G words apart so that the groups of a wave start G banks apart.
template <int G>
__global__ __launch_bounds__(SD_BLOCK) void k_seg_newton(const uint32_t *__restrict__ rec, uint32_t nseg, uint32_t T,
                                                         const uint32_t *__restrict__ inv,
                                                         uint32_t *__restrict__ coef, uint32_t *__restrict__ deg,
                                                         int32_t *__restrict__ status) {
    extern __shared__ uint32_t sd_sm[];
    __shared__ uint32_t s_dmax;
    constexpr uint32_t SEGS = SD_BLOCK / G;
    const uint32_t j = threadIdx.x % G, grp = threadIdx.x / G;
    const uint64_t g = (uint64_t)blockIdx.x * SEGS + grp;
    uint32_t *S = sd_sm + (size_t)grp * (2 * T + G), *c = S + T;
    if (threadIdx.x == 0) s_dmax = 0;
    __syncthreads();
    uint32_t d = 0;
    if (g < nseg) {
        const uint32_t *h = rec + g * (4 + T);
        const uint32_t thr = h[0], cnt = h[1];
        const int32_t st = thr != T ? QK_E_MISMATCH : cnt > T ? QK_E_UNDECODABLE : QK_OK;
        d = st == QK_OK ? cnt : 0u;
        if (j == 0) {
            status[g] = st;
            deg[g] = d;
            if (d) atomicMax(&s_dmax, d);
        }
        for (uint32_t k = j; k < d; k += G) S[k] = h[4 + k];
    }
    __syncthreads();
    const uint32_t dmax = s_dmax;
    for (uint32_t i = 0; i < dmax; ++i) {
        uint64_t acc = 0;
        if (i < d)
            for (uint32_t k = j; k < i; k += G) acc += mul32_lazy(S[k], c[i - k - 1]);
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) {
            const uint32_t lo = __shfl_xor((int)(uint32_t)acc, off, 64);
            const uint32_t hi = __shfl_xor((int)(uint32_t)(acc >> 32), off, 64);
            acc += ((uint64_t)hi << 32) | lo;
        }
        if (i < d && j == 0) c[i] = mul32(neg32(canon32(fold64_32(acc + S[i]))), inv[i + 1]);
        __syncthreads();
    }
    if (g < nseg)
        for (uint32_t k = j; k < T; k += G) coef[g * T + k] = k < d ? c[k] : 0u;
}

// --------------------------------------------------------------- root test
// maxseg: the most segments any item of the launch holds (sizes the LDS).
// LDS: so[maxseg + 1], sdeg[maxseg], sstop[maxseg], suse[maxseg], then the
// coefficient rows, T + 1 words apart (lanes of different segments read
// coefficient k of their rows from different banks).  A wave may hold lanes of
// several segments: it loops to its largest degree, each lane stepping only
// below its own (decode.hip is_root32's body, runtime degree).
__global__ __launch_bounds__(SD_BLOCK) void k_seg_root_test(const uint32_t *__restrict__ log,
                                                            const SdItem *__restrict__ items,
                                                            const uint64_t *__restrict__ offs,
                                                            const uint32_t *__restrict__ rec,
                                                            const uint32_t *__restrict__ coef,
                                                            const uint32_t *__restrict__ deg, uint32_t T,
                                                            uint32_t maxseg, int stop_at_last,
                                                            unsigned long long *__restrict__ stop,
                                                            uint64_t *__restrict__ mask) {
    extern __shared__ uint32_t sd_sm[];
    uint32_t *so = sd_sm, *sdeg = so + maxseg + 1, *sstop = sdeg + maxseg, *suse = sstop + maxseg;
    uint32_t *sc = suse + maxseg;
    const SdItem it = items[blockIdx.x];
    // the item's entries first: their loads are in flight while the rows are staged
    uint32_t idv[SD_ITEM / SD_BLOCK];
#pragma unroll
    for (uint32_t u = 0; u < SD_ITEM / SD_BLOCK; ++u) {
        const uint32_t i = u * SD_BLOCK + threadIdx.x;
        idv[u] = i < it.n ? log[it.lo + i] : 0u;
    }
    sd_stage_offsets(it, offs, so);
    for (uint32_t k = threadIdx.x; k < it.nseg; k += SD_BLOCK) {
        const uint32_t *h = rec + ((uint64_t)it.seg0 + k) * (4 + T);
        sdeg[k] = deg[(uint64_t)it.seg0 + k];
        suse[k] = stop_at_last && h[2];
        sstop[k] = h[3];
    }
    for (uint32_t idx = threadIdx.x; idx < it.nseg * T; idx += SD_BLOCK) {
        const uint32_t r = idx / T, k = idx - r * T;
        sc[r * (T + 1) + k] = coef[(uint64_t)it.seg0 * T + idx];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t u = 0; u < SD_ITEM / SD_BLOCK; ++u) {
        const uint32_t base = u * SD_BLOCK;
        if (base >= it.n) break;
        const uint32_t i = base + threadIdx.x;
        const bool valid = i < it.n;
        const uint32_t id = idv[u];
        const uint32_t r = valid && it.nseg > 1 ? sd_segment_of(so, it.nseg, i) : 0u;
        const uint32_t d = valid ? sdeg[r] : 0u;
        uint32_t dm = d;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)dm, off, 64);
            dm = o > dm ? o : dm;
        }
        const uint32_t x = canon32(id), x5 = times5_32(x);
        const uint32_t *c = sc + r * (T + 1);
        uint32_t lo = 1, hi = 0;
        for (uint32_t k = 0; k < dm; ++k)
            if (k < d) tstep32(lo, hi, x, x5, c[k]);
        const bool hit = d > 0 && canon32(fold64_32(((uint64_t)hi << 32) | lo)) == 0;
        if (valid && suse[r] && id == sstop[r])
            atomicMin(&stop[(uint64_t)it.seg0 + r], (unsigned long long)(it.lo + i));
        const uint64_t m = __ballot(hit);
        if (lane == 0) mask[(uint64_t)blockIdx.x * SD_WORDS + base / 64 + wave] = m;
    }
}

// The `break` at last_value, per segment: a hit survives when it lies before
// its segment's stop position (~0: none).  Rewrites the mask words in place.
__global__ __launch_bounds__(SD_BLOCK) void k_seg_hit_count(const SdItem *__restrict__ items,
                                                            const uint64_t *__restrict__ offs, uint32_t maxseg,
                                                            const unsigned long long *__restrict__ stop,
                                                            uint64_t *__restrict__ mask, uint32_t *__restrict__ itemcnt,
                                                            uint32_t *__restrict__ segcnt) {
    extern __shared__ uint32_t sd_sm[];
    __shared__ uint32_t s_cnt;
    uint32_t *so = sd_sm;
    const SdItem it = items[blockIdx.x];
    sd_stage_offsets(it, offs, so);
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t cnt = 0;
    for (uint32_t base = 0; base < it.n; base += SD_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        uint64_t *w = mask + (uint64_t)blockIdx.x * SD_WORDS + base / 64 + wave;
        const uint64_t m = *w;
        bool keep = false;
        if ((m >> lane) & 1) {   // implies i < it.n
            const uint32_t r = it.nseg > 1 ? sd_segment_of(so, it.nseg, i) : 0u;
            keep = it.lo + i < stop[(uint64_t)it.seg0 + r];
            if (keep) atomicAdd(&segcnt[(uint64_t)it.seg0 + r], 1u);
        }
        const uint64_t k = __ballot(keep);
        if (lane == 0) {
            if (k != m) *w = k;
            cnt += (uint32_t)__popcll(k);
        }
    }
    if (lane == 0 && cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (threadIdx.x == 0) itemcnt[blockIdx.x] = s_cnt;
}

// exclusive scan of the item counts by one workgroup (each thread a
// contiguous run); total[0] = all hits
constexpr int SD_SCAN = 1024;
__global__ __launch_bounds__(SD_SCAN) void k_seg_scan(const uint32_t *__restrict__ itemcnt, uint32_t nitems,
                                                      uint64_t *__restrict__ itembase, uint64_t *__restrict__ total) {
    __shared__ uint64_t part[SD_SCAN];
    const uint32_t per = (nitems + SD_SCAN - 1) / SD_SCAN;
    const uint64_t b = (uint64_t)threadIdx.x * per, e = b + per < nitems ? b + per : nitems;
    uint64_t s = 0;
    for (uint64_t k = b; k < e; ++k) s += itemcnt[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < SD_SCAN; off <<= 1) {   // inclusive scan of the partials
        const uint64_t v = threadIdx.x >= (uint32_t)off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t run = part[threadIdx.x] - s;
    for (uint64_t k = b; k < e; ++k) {
        itembase[k] = run;
        run += itemcnt[k];
    }
    if (threadIdx.x == SD_SCAN - 1) total[0] = part[SD_SCAN - 1];
}

// one wave per work item, lane l its mask word l: the positions of the set
// bits, ascending, from the item's rank on (only ranks below cap are written)
__global__ __launch_bounds__(64) void k_seg_hit_write(const SdItem *__restrict__ items,
                                                      const uint64_t *__restrict__ mask,
                                                      const uint64_t *__restrict__ itembase,
                                                      uint64_t *__restrict__ hits, uint64_t cap) {
    const SdItem it = items[blockIdx.x];
    const uint32_t l = threadIdx.x;
    uint64_t m = l * 64 < it.n ? mask[(uint64_t)blockIdx.x * SD_WORDS + l] : 0;
    const uint32_t cnt = (uint32_t)__popcll(m);
    uint32_t incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, off, 64);
        if (l >= (uint32_t)off) incl += v;
    }
    uint64_t rank = itembase[blockIdx.x] + (incl - cnt);
    while (m) {
        const int b = __ffsll((unsigned long long)m) - 1;
        if (rank < cap) hits[rank] = it.lo + l * 64 + (uint32_t)b;
        ++rank;
        m &= m - 1;
    }
}

// ------------------------------------------------------------------- host
// inverses of 1 .. QK_MAX_THRESHOLD by the recurrence of qk_u32_to_coeffs
// (host.cpp), computed once per context and kept on the device: one table
// serves every threshold (entry i does not depend on it)
static int sd_inverses(qk_ctx *ctx, hipStream_t s) {
    if (ctx->d_seg_inv) return QK_OK;
    ctx->h_seg_inv.assign(QK_MAX_THRESHOLD + 2, 1u);
    for (uint32_t i = 2; i <= QK_MAX_THRESHOLD; ++i)
        ctx->h_seg_inv[i] = mul32(P32 - P32 / i, ctx->h_seg_inv[P32 % i]);
    if (hipMalloc((void **)&ctx->d_seg_inv, ctx->h_seg_inv.size() * 4) != hipSuccess) {
        (void)hipGetLastError();
        ctx->d_seg_inv = nullptr;
        return QK_E_NOMEM;
    }
    if (hipMemcpyAsync(ctx->d_seg_inv, ctx->h_seg_inv.data(), ctx->h_seg_inv.size() * 4, hipMemcpyHostToDevice, s) !=
        hipSuccess)
        return QK_E_HIP;
    return QK_OK;
}

static void sd_carve(Carve &cv, SdSeg &b, size_t nseg, uint32_t T, bool host_rec, bool decode) {
    if (host_rec) b.rec = cv.take<uint32_t>(nseg * (4 + T));
    b.coef = cv.take<uint32_t>(nseg * T);
    b.deg = cv.take<uint32_t>(nseg);
    b.status = cv.take<int32_t>(nseg);
    if (decode) {
        b.offs = cv.take<uint64_t>(nseg + 1);
        b.stop = cv.take<unsigned long long>(nseg);
        b.segcnt = cv.take<uint32_t>(nseg);
        b.total = cv.take<uint64_t>(1);
    }
}

// records onto the device (host records: threshold checked here) and the
// Newton kernel enqueued
int sd_newton(qk_ctx *ctx, const uint8_t *diffs, bool host_rec, size_t nseg, uint32_t T, SdSeg &b,
                     hipStream_t s) {
    const size_t rec = qk_u32_size(T);
    if (host_rec) {
        for (size_t g = 0; g < nseg; ++g)
            if (((const qk_u32 *)(diffs + g * rec))->threshold != T) return QK_E_MISMATCH;
        QK_HIP_TRY(hipMemcpyAsync(b.rec, diffs, nseg * rec, hipMemcpyHostToDevice, s));
    } else {
        b.rec = (uint32_t *)diffs;
    }
    if (int e = sd_inverses(ctx, s)) return e;
    hipEvent_t e0 = prof_begin(ctx, s);
#define QK_NEWTON(G_)                                                                                              \
    hipLaunchKernelGGL((k_seg_newton<G_>), dim3((uint32_t)((nseg + SD_BLOCK / G_ - 1) / (SD_BLOCK / G_))),         \
                       dim3(SD_BLOCK), (SD_BLOCK / G_) * (2 * T + G_) * sizeof(uint32_t), s, b.rec, (uint32_t)nseg, T, \
                       ctx->d_seg_inv, b.coef, b.deg, b.status)
    if (T <= 32) QK_NEWTON(8);
    else if (T <= 128) QK_NEWTON(16);
    else QK_NEWTON(64);
#undef QK_NEWTON
    prof_end(ctx, s, e0);
    return hipGetLastError() == hipSuccess ? QK_OK : QK_E_HIP;
}


// long segments cut into items of SD_ITEM entries; runs of whole short
// segments packed up to SD_ITEM entries and sd_maxseg(T) segments
static std::vector<SdItem> sd_items(const uint64_t *offs, size_t nseg, uint32_t T) {
    std::vector<SdItem> items;
    const uint32_t maxseg = sd_maxseg(T);
    size_t g = 0;
    while (g < nseg) {
        const uint64_t len = offs[g + 1] - offs[g];
        if (len > SD_ITEM) {
            for (uint64_t lo = offs[g]; lo < offs[g + 1]; lo += SD_ITEM)
                items.push_back({lo, (uint32_t)std::min<uint64_t>(SD_ITEM, offs[g + 1] - lo), (uint32_t)g, 1u, 0u});
            ++g;
            continue;
        }
        const size_t g0 = g;
        uint64_t tot = 0;
        while (g < nseg && g - g0 < maxseg && offs[g + 1] - offs[g] <= SD_ITEM - tot) tot += offs[g + 1] - offs[g], ++g;
        if (tot) items.push_back({offs[g0], (uint32_t)tot, (uint32_t)g0, (uint32_t)(g - g0), 0u});
    }
    return items;
}

void sd_plan(SdPlan &p, const uint64_t *offsets, size_t nseg, uint32_t T, size_t cap) {
    p.items = sd_items(offsets, nseg, T);
    p.maxseg = 1;   // the LDS of a launch follows its fullest item, not the packing limit
    for (const SdItem &it : p.items) p.maxseg = std::max(p.maxseg, it.nseg);
    p.n = offsets[nseg] - offsets[0];
    p.hcap = std::min<uint64_t>(cap, p.n);
}

void sd_carve_plan(Carve &seg, Carve &item, SdPlan &p, size_t nseg, uint32_t T, bool host_rec) {
    const size_t ni = p.items.size();
    sd_carve(seg, p.b, nseg, T, host_rec, true);
    p.d_mask = item.take<uint64_t>(ni * SD_WORDS);
    p.d_base = item.take<uint64_t>(ni);
    p.d_icnt = item.take<uint32_t>(ni);
    p.d_hit = item.take<uint64_t>(p.hcap);
}

int sd_upload(qk_ctx *ctx, SdPlan &p, const uint64_t *offsets, size_t nseg, hipStream_t s) {
    const size_t ni = p.items.size();
    if (ni) {
        if (int e = ensure_items(ctx, ni * sizeof(SdItem))) return e;
        memcpy(ctx->h_items, p.items.data(), ni * sizeof(SdItem));
    }
    p.d_items = (const SdItem *)ctx->h_items_dev;
    if (hipMemcpyAsync(p.b.offs, offsets, (nseg + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemsetAsync(p.b.stop, 0xFF, nseg * 8, s) != hipSuccess ||
        hipMemsetAsync(p.b.segcnt, 0, nseg * 4, s) != hipSuccess || hipMemsetAsync(p.b.total, 0, 8, s) != hipSuccess)
        return QK_E_HIP;
    return QK_OK;
}

int sd_enqueue(qk_ctx *ctx, SdPlan &p, const uint8_t *diffs, bool host_rec, const uint32_t *d_log, size_t nseg,
               uint32_t T, int stop_at_last, hipStream_t s) {
    if (int e = sd_newton(ctx, diffs, host_rec, nseg, T, p.b, s)) return e;
    const size_t ni = p.items.size();
    if (!ni) return QK_OK;
    const SdSeg &b = p.b;
    const uint32_t maxseg = p.maxseg;
    const size_t lds_rt = ((size_t)maxseg * 4 + 1 + (size_t)maxseg * (T + 1)) * sizeof(uint32_t);
    const size_t lds_cnt = ((size_t)maxseg + 1) * sizeof(uint32_t);
    hipEvent_t e0 = prof_begin(ctx, s);
    hipLaunchKernelGGL(k_seg_root_test, dim3((uint32_t)ni), dim3(SD_BLOCK), lds_rt, s, d_log, p.d_items, b.offs, b.rec,
                       b.coef, b.deg, T, maxseg, stop_at_last ? 1 : 0, b.stop, p.d_mask);
    prof_end(ctx, s, e0);
    hipLaunchKernelGGL(k_seg_hit_count, dim3((uint32_t)ni), dim3(SD_BLOCK), lds_cnt, s, p.d_items, b.offs, maxseg,
                       b.stop, p.d_mask, p.d_icnt, b.segcnt);
    return sd_compact(p, s);
}

int sd_compact(SdPlan &p, hipStream_t s) {
    const size_t ni = p.items.size();
    if (!ni) return QK_OK;
    hipLaunchKernelGGL(k_seg_scan, dim3(1), dim3(SD_SCAN), 0, s, p.d_icnt, (uint32_t)ni, p.d_base, p.b.total);
    hipLaunchKernelGGL(k_seg_hit_write, dim3((uint32_t)ni), dim3(64), 0, s, p.d_items, p.d_mask, p.d_base, p.d_hit,
                       p.hcap);
    return hipGetLastError() == hipSuccess ? QK_OK : QK_E_HIP;
}

int sd_collect(const SdPlan &p, const int32_t *status, const uint32_t *segcnt, uint64_t total, size_t nseg,
               uint64_t *hits, size_t cap, uint64_t *hit_offsets, size_t *n_hits) {
    for (size_t g = 0; g < nseg; ++g)
        if (status[g] == QK_E_MISMATCH) return QK_E_MISMATCH;
    hit_offsets[0] = 0;
    for (size_t g = 0; g < nseg; ++g) hit_offsets[g + 1] = hit_offsets[g] + segcnt[g];
    *n_hits = (size_t)total;
    if (hit_offsets[nseg] != total) return QK_E_HIP;   // the two counts are kept by different kernels
    if (total > cap) return QK_E_CAPACITY;
    if (total) QK_HIP_TRY(hipMemcpy(hits, p.d_hit, total * 8, hipMemcpyDeviceToHost));
    return QK_OK;
}

} // namespace qk

using namespace qk;

extern "C" int qk_u32_to_coeffs_segments_device(qk_ctx *ctx, const uint8_t *diffs, size_t nseg, uint32_t threshold,
                                                uint32_t *coeffs, uint32_t *degrees, int32_t *status, void *stream) {
    if (int e = check_ctx_threshold(ctx, threshold)) return e;
    if (nseg == 0) return QK_OK;
    if (!diffs || !coeffs || !degrees || !status || nseg > 0xFFFFFFFFull) return QK_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    QK_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    const uint32_t T = threshold;
    const bool host_rec = !is_device_ptr(diffs);
    Carve probe{nullptr};
    SdSeg b;
    sd_carve(probe, b, nseg, T, host_rec, false);
    if (int e = ensure_flow(ctx, 1, probe.off, s)) return e;
    Carve cv{(char *)ctx->d_flow[1]};
    sd_carve(cv, b, nseg, T, host_rec, false);
    int rc = sd_newton(ctx, diffs, host_rec, nseg, T, b, s);
    if (!rc && (hipMemcpyAsync(coeffs, b.coef, nseg * T * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(degrees, b.deg, nseg * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(status, b.status, nseg * 4, hipMemcpyDeviceToHost, s) != hipSuccess))
        rc = QK_E_HIP;
    // the arena and the host records must outlive what was enqueued
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = QK_E_HIP;
    if (rc) return rc;
    for (size_t g = 0; g < nseg; ++g)
        if (status[g] == QK_E_MISMATCH) return QK_E_MISMATCH;
    return QK_OK;
}

extern "C" int qk_u32_decode_segments_device(qk_ctx *ctx, const uint8_t *diffs, const uint32_t *d_log,
                                             const uint64_t *offsets, size_t nseg, uint32_t threshold,
                                             int stop_at_last, uint64_t *hits, size_t cap, uint64_t *hit_offsets,
                                             int32_t *status, size_t *n_hits, void *stream) {
    if (int e = check_ctx_threshold(ctx, threshold)) return e;
    if (n_hits) *n_hits = 0;
    if (nseg == 0) {
        if (hit_offsets) hit_offsets[0] = 0;
        return QK_OK;
    }
    if (!diffs || !offsets || !hit_offsets || !status || !n_hits || (cap && !hits) || nseg > 0xFFFFFFFFull)
        return QK_E_INVAL;
    for (size_t g = 0; g < nseg; ++g)
        if (offsets[g + 1] < offsets[g]) return QK_E_INVAL;
    const uint64_t n = offsets[nseg] - offsets[0];
    if (n && (!d_log || !is_device_ptr(d_log))) return QK_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    QK_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    const uint32_t T = threshold;
    const bool host_rec = !is_device_ptr(diffs);
    SdPlan p;
    sd_plan(p, offsets, nseg, T, cap);
    // per-segment buffers in the per-flow arena, per-item ones in the per-packet arena
    for (int pass = 0; pass < 2; ++pass) {
        Carve cs{pass ? (char *)ctx->d_flow[1] : nullptr}, ci{pass ? (char *)ctx->d_flow[0] : nullptr};
        sd_carve_plan(cs, ci, p, nseg, T, host_rec);
        if (!pass) {
            if (int e = ensure_flow(ctx, 1, cs.off, s)) return e;
            if (int e = ensure_flow(ctx, 0, ci.off, s)) return e;
        }
    }
    int rc = sd_upload(ctx, p, offsets, nseg, s);
    if (!rc) rc = sd_enqueue(ctx, p, diffs, host_rec, d_log, nseg, T, stop_at_last, s);
    std::vector<uint32_t> segcnt(nseg);
    uint64_t total = 0;
    if (!rc && (hipMemcpyAsync(status, p.b.status, nseg * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(segcnt.data(), p.b.segcnt, nseg * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(&total, p.b.total, 8, hipMemcpyDeviceToHost, s) != hipSuccess))
        rc = QK_E_HIP;
    // the one wait for the kernels (the pinned items, the host records and
    // the offsets must outlive them); the hit copy after it is sized by `total`
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = QK_E_HIP;
    if (rc) return rc;
    return sd_collect(p, status, segcnt.data(), total, nseg, hits, cap, hit_offsets, n_hits);
}
