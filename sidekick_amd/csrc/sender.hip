// sender.hip — the batched sender step: what listen_for_quacks_power_sum
// (media_client.rs:223-323) does per quACK before and after the decode, for
// nseg flows whose sent logs lie grouped in one device array.
//
// Per flow with a quACK (receiver.py QuackReceiver.on_quack is the same loop):
//     if quack.last_value() == my_quack.last_value() { continue }        :233
//     idx = log.position(|id| id == quack.last_value())                  :240-246
//     my_quack.insert(log[..=idx])                                       :247-252
//     reset0 = idx.is_none(); reset1 = mine.count < quack.count;
//     reset2 = mine.count > quack.count + threshold                      :257-261
//     diff = mine - quack; missing = decode(diff, log)                   :295-313
//     log.drain(..=idx); for id in missing { my_quack.remove(id) }       :316-322
//   k_snd_find       one workgroup per work item of the batched decode
//                    (segdecode.h SdItem): atomicMin of the first position
//                    whose raw id equals the peer's last value, per segment
//   k_snd_prefix     power sums of the entries up to that position, u64 rows
//                    [nseg][T]: a wave per packed segment (it owns the row's
//                    contribution), four waves striped over a slice
//   k_snd_classify   a lane group per segment: mine1 = mine + prefix into
//                    mine_out, the reset bits, action, drain, the diff record
//                    (count 0 where the flow must not decode)
//   sd_enqueue       Newton, root test, hit count, scan, hit write over the
//                    diff records (segdecode.hip), stop_at_last = 1
//   k_snd_remove     every surviving hit bit adds p - x^k to its segment's row
//   k_snd_finish     the rows of the segments with hits back into mine_out
// Every sum is an integer sum of values below 2^32 in a 64-bit word, folded
// once at the end: exact and independent of the order of the atomics.
#include <string.h>

#include <algorithm>
#include <vector>

#include "bsgs.h"
#include "ctx.h"
#include "field.h"
#include "segdecode.h"
#include "segments.h"

namespace qk {

QK_WARM_KERNEL(sender)

constexpr uint32_t SN_WAVES = SD_BLOCK / 64;
constexpr uint32_t SN_GROUP = 16;   // lanes per segment of k_snd_classify / k_snd_finish
constexpr unsigned long long SN_NONE = ~0ull;

// the flow has a quACK and its last_value differs from mine, compared as the
// Option it is (:233); hm, hp: the headers of mine and of the peer's record
__device__ __forceinline__ bool sn_active(const uint32_t *hm, const uint32_t *hp, const uint8_t *present, uint64_t g) {
    if (present && !present[g]) return false;
    const bool ps = hp[2] != 0, ms = hm[2] != 0;
    return !(ps == ms && (!ps || hp[3] == hm[3]));
}

// ------------------------------------------------------------------- find
// LDS: so[maxseg + 1], suse[maxseg], sval[maxseg].  The stop mechanism of
// k_seg_root_test, keyed on the peer's record: equality is on the raw id.
__global__ __launch_bounds__(SD_BLOCK) void k_snd_find(const uint32_t *__restrict__ log,
                                                       const SdItem *__restrict__ items,
                                                       const uint64_t *__restrict__ offs,
                                                       const uint32_t *__restrict__ mine,
                                                       const uint32_t *__restrict__ peer,
                                                       const uint8_t *__restrict__ present, uint32_t T,
                                                       uint32_t maxseg, unsigned long long *__restrict__ fstop) {
    extern __shared__ uint32_t sn_sm[];
    __shared__ uint32_t s_any;
    uint32_t *so = sn_sm, *suse = so + maxseg + 1, *sval = suse + maxseg;
    const SdItem it = items[blockIdx.x];
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    sd_stage_offsets(it, offs, so);
    for (uint32_t k = threadIdx.x; k < it.nseg; k += SD_BLOCK) {
        const uint64_t g = (uint64_t)it.seg0 + k;
        const uint32_t *hm = mine + g * (4 + T), *hp = peer + g * (4 + T);
        const bool use = hp[2] != 0 && sn_active(hm, hp, present, g);
        suse[k] = use;
        sval[k] = hp[3];
        if (use) s_any = 1;
    }
    __syncthreads();
    if (!s_any) return;   // absent and idle flows only: the item's entries are not read
    for (uint32_t i = threadIdx.x; i < it.n; i += SD_BLOCK) {
        const uint32_t r = it.nseg > 1 ? sd_segment_of(so, it.nseg, i) : 0u;
        if (suse[r] && log[it.lo + i] == sval[r]) atomicMin(&fstop[(uint64_t)it.seg0 + r], (unsigned long long)(it.lo + i));
    }
}

// ----------------------------------------------------------------- prefix
// G lanes per id, lane j a chain of K powers j+1, j+1+G, ... (G * K >= T;
// field.h group_chain32, as the segmented encode's groups).
// An item of fewer than SN_WAVES segments (a slice of a long one among them)
// is walked by all waves, striped; otherwise wave w takes segments w, w +
// SN_WAVES, ...: either way a wave adds up its own entries of ONE segment in
// registers and hands the sums to that segment's row, T atomics per wave.
// A segment with no stop, or whose stop lies before the item, costs nothing.
// LDS: so[maxseg + 1].
template <int G, int K>
__global__ __launch_bounds__(SD_BLOCK) void k_snd_prefix(const uint32_t *__restrict__ log,
                                                         const SdItem *__restrict__ items,
                                                         const uint64_t *__restrict__ offs,
                                                         const unsigned long long *__restrict__ fstop, uint32_t T,
                                                         unsigned long long *__restrict__ acc_out) {
    extern __shared__ uint32_t sn_sm[];
    uint32_t *so = sn_sm;
    const SdItem it = items[blockIdx.x];
    if (it.nseg == 1) {   // the whole workgroup leaves before staging anything
        const unsigned long long st = fstop[it.seg0];
        if (st == SN_NONE || st < it.lo) return;
    }
    sd_stage_offsets(it, offs, so);
    __syncthreads();
    constexpr uint32_t PER = 64 / G;   // ids per wave and step
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = (int)(lane % G);
    const uint32_t slot = lane / G;
    const bool striped = it.nseg < SN_WAVES;
    const uint32_t first = striped ? wave * PER + slot : slot, stride = striped ? SN_WAVES * PER : PER;
    for (uint32_t r = striped ? 0u : wave; r < it.nseg; r += striped ? 1u : SN_WAVES) {
        const uint64_t g = (uint64_t)it.seg0 + r;
        const unsigned long long st = fstop[g];
        const uint32_t b = so[r];
        uint32_t e = so[r + 1];
        if (st == SN_NONE || st < it.lo + b || b == e) continue;
        if (st - it.lo < e) e = (uint32_t)(st - it.lo) + 1;
        uint64_t acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = 0;
        // terms < 6 * 2^32, at most SD_ITEM of them
        for (uint32_t i = b + first; i < e; i += stride) group_chain32<G, K>(acc, canon32(log[it.lo + i]), j);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            uint64_t v = fold64_32(acc[k]);
#pragma unroll
            for (int off = 32; off >= G; off >>= 1) v += bsgs::shfl_xor_u64(v, off);   // < 2^38
            const uint32_t m = lane + (uint32_t)k * G;
            if (lane < G && m < T && v) atomicAdd(&acc_out[g * T + m], (unsigned long long)v);
        }
    }
}

// --------------------------------------------------------------- classify
// SN_GROUP lanes per segment, every lane with the header, lane j the sums j,
// j + SN_GROUP, ...  mine1 goes straight to mine_out: on a reset the caller
// keeps the prefix insert (the reference inserts before it tests, :247-261,
// and a debounced reset leaves my_quack as it then is).  The row is left
// holding mine1's sums for k_snd_remove to subtract from.
__global__ __launch_bounds__(SD_BLOCK) void k_snd_classify(
    const uint32_t *__restrict__ mine, const uint32_t *__restrict__ peer, const uint8_t *__restrict__ present,
    const uint32_t *__restrict__ log, const uint64_t *__restrict__ offs, const unsigned long long *__restrict__ fstop,
    unsigned long long *__restrict__ acc, uint32_t T, uint32_t nseg, uint32_t *__restrict__ mine_out,
    uint32_t *__restrict__ diff, uint8_t *__restrict__ action, uint64_t *__restrict__ drain,
    uint32_t *__restrict__ err) {
    const uint32_t j = threadIdx.x % SN_GROUP;
    const uint64_t g = (uint64_t)blockIdx.x * (SD_BLOCK / SN_GROUP) + threadIdx.x / SN_GROUP;
    if (g >= nseg) return;
    const size_t W = 4 + (size_t)T;
    const uint32_t *hm = mine + g * W, *hp = peer + g * W;
    uint32_t *mo = mine_out + g * W, *df = diff + g * W;
    const bool has = !present || present[g];
    const bool bad = hm[0] != T || (has && hp[0] != T);
    if (bad && j == 0) atomicOr(err, 1u);
    const bool active = !bad && sn_active(hm, hp, present, g);
    const unsigned long long st = active ? fstop[g] : SN_NONE;
    const bool found = st != SN_NONE;
    uint32_t c1 = hm[1], hl = hm[2], lv = hm[3];
    uint64_t idx = 0;
    if (found) {
        idx = st - offs[g];
        c1 += (uint32_t)(idx + 1);
        hl = 1;
        lv = log[st];
    }
    uint32_t bits = 0;
    if (active) {
        const uint32_t pc = hp[1];
        if (!found) bits |= QK_SND_RESET_REORDERED;
        if (c1 < pc) bits |= QK_SND_RESET_RETX;
        if (c1 > pc + T) bits |= QK_SND_RESET_EXCEEDS;   // u32: the sum wraps as the reference's does
    }
    const bool decode = active && !bits;
    if (j == 0) {
        mo[0] = T, mo[1] = c1, mo[2] = hl, mo[3] = lv;
        df[0] = T, df[1] = decode ? c1 - hp[1] : 0u, df[2] = decode ? 1u : 0u, df[3] = lv;
        action[g] = (uint8_t)(!active ? QK_SND_IDLE : bits ? bits : QK_SND_ADVANCED);
        drain[g] = decode ? idx + 1 : 0;
    }
    for (uint32_t k = j; k < T; k += SN_GROUP) {
        uint32_t m = hm[4 + k];
        if (found) m = add32(m, canon32(fold64_32(acc[g * T + k])));
        mo[4 + k] = m;
        if (decode) {
            df[4 + k] = sub32(m, hp[4 + k]);
            acc[g * T + k] = m;
        }
    }
}

// ----------------------------------------------------------------- remove
// after k_seg_hit_count: the mask holds the surviving hits.  One lane per
// hit, T steps: my_quack.remove(id) (:319) as p - x^k added to the row.  An
// item whose rows fit `rows` LDS words adds them up there first (ds_add_u64)
// and hands each touched word to the global row once; a fatter item (many
// short segments at a large T) goes to the global rows directly.  10^5 flows
// of 10^3 entries, T = 32, 10 hits a flow: 1.66 ms direct, every hit's 32
// atomics on its flow's one row (profiles/sender_step/).
// LDS: lrow[rows] (u64), then so[maxseg + 1].
constexpr uint32_t SN_REM_ROWS = 4096;
__global__ __launch_bounds__(SD_BLOCK) void k_snd_remove(const uint32_t *__restrict__ log,
                                                         const SdItem *__restrict__ items,
                                                         const uint64_t *__restrict__ offs,
                                                         const uint64_t *__restrict__ mask,
                                                         const uint32_t *__restrict__ itemcnt, uint32_t T,
                                                         uint32_t rows, unsigned long long *__restrict__ acc) {
    extern __shared__ unsigned long long sn_sm64[];
    unsigned long long *lrow = sn_sm64;
    uint32_t *so = reinterpret_cast<uint32_t *>(sn_sm64 + rows);
    if (itemcnt[blockIdx.x] == 0) return;
    const SdItem it = items[blockIdx.x];
    const uint32_t words = it.nseg * T;
    const bool local = words <= rows;
    sd_stage_offsets(it, offs, so);
    if (local)
        for (uint32_t k = threadIdx.x; k < words; k += SD_BLOCK) lrow[k] = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < it.n; i += SD_BLOCK) {
        if (!((mask[(uint64_t)blockIdx.x * SD_WORDS + i / 64] >> (i & 63)) & 1)) continue;
        const uint32_t r = it.nseg > 1 ? sd_segment_of(so, it.nseg, i) : 0u;
        unsigned long long *row = local ? lrow + (size_t)r * T : acc + ((uint64_t)it.seg0 + r) * T;
        const uint32_t x = canon32(log[it.lo + i]);
        uint32_t pw = 1;
        for (uint32_t k = 0; k < T; ++k) {
            pw = mul32(pw, x);
            atomicAdd(&row[k], (unsigned long long)(P32 - pw));   // at most SD_ITEM terms below 2^32
        }
    }
    if (!local) return;
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < words; k += SD_BLOCK)
        if (lrow[k]) atomicAdd(&acc[(uint64_t)it.seg0 * T + k], lrow[k]);
}

// the rows of the segments with hits, canonical, and their counts
__global__ __launch_bounds__(SD_BLOCK) void k_snd_finish(const uint32_t *__restrict__ segcnt,
                                                         const unsigned long long *__restrict__ acc, uint32_t T,
                                                         uint32_t nseg, uint32_t *__restrict__ mine_out) {
    const uint32_t j = threadIdx.x % SN_GROUP;
    const uint64_t g = (uint64_t)blockIdx.x * (SD_BLOCK / SN_GROUP) + threadIdx.x / SN_GROUP;
    if (g >= nseg) return;
    const uint32_t c = segcnt[g];
    if (!c) return;
    uint32_t *mo = mine_out + g * (4 + (size_t)T);
    if (j == 0) mo[1] -= c;
    for (uint32_t k = j; k < T; k += SN_GROUP) mo[4 + k] = canon32(fold64_32(acc[g * T + k]));
}

// ------------------------------------------------------------------- host
// the step's own per-segment buffers, beside the decode's in the per-flow arena
struct SnSeg {
    unsigned long long *fstop = nullptr, *acc = nullptr;
    uint32_t *diff = nullptr, *err = nullptr;
    uint8_t *action = nullptr;
    uint64_t *drain = nullptr;
};

static void sn_carve(Carve &cv, SnSeg &b, size_t nseg, uint32_t T) {
    b.fstop = cv.take<unsigned long long>(nseg);
    b.acc = cv.take<unsigned long long>(nseg * T);
    b.diff = cv.take<uint32_t>(nseg * (4 + (size_t)T));
    b.err = cv.take<uint32_t>(1);
    b.action = cv.take<uint8_t>(nseg);
    b.drain = cv.take<uint64_t>(nseg);
}

// G = 1 up to 32 powers, then the smallest power of two with T / G <= 32
// (segments.hip seg_choose): a group of more than one lane always has K = 32
template <int G, int K>
static void sn_prefix_gk(const uint32_t *log, const SdPlan &p, uint32_t T, const SnSeg &b, hipStream_t s) {
    hipLaunchKernelGGL((k_snd_prefix<G, K>), dim3((uint32_t)p.items.size()), dim3(SD_BLOCK),
                       ((size_t)p.maxseg + 1) * sizeof(uint32_t), s, log, p.d_items, p.b.offs, b.fstop, T, b.acc);
}
static void sn_prefix(const uint32_t *log, const SdPlan &p, uint32_t T, const SnSeg &b, hipStream_t s) {
    if (T <= 4) sn_prefix_gk<1, 4>(log, p, T, b, s);
    else if (T <= 8) sn_prefix_gk<1, 8>(log, p, T, b, s);
    else if (T <= 16) sn_prefix_gk<1, 16>(log, p, T, b, s);
    else if (T <= 32) sn_prefix_gk<1, 32>(log, p, T, b, s);
    else if (T <= 64) sn_prefix_gk<2, 32>(log, p, T, b, s);
    else if (T <= 128) sn_prefix_gk<4, 32>(log, p, T, b, s);
    else if (T <= 256) sn_prefix_gk<8, 32>(log, p, T, b, s);
    else if (T <= 512) sn_prefix_gk<16, 32>(log, p, T, b, s);
    else sn_prefix_gk<32, 32>(log, p, T, b, s);
}

} // namespace qk

using namespace qk;

extern "C" int qk_u32_sender_step_segments_device(qk_ctx *ctx, const uint8_t *d_mine, const uint8_t *d_peer,
                                                  const uint8_t *d_present, const uint32_t *d_log,
                                                  const uint64_t *offsets, size_t nseg, uint32_t threshold,
                                                  uint8_t *d_mine_out, uint8_t *action, uint64_t *drain,
                                                  uint64_t *hits, size_t cap, uint64_t *hit_offsets, size_t *n_hits,
                                                  void *stream) {
    if (int e = check_ctx_threshold(ctx, threshold)) return e;
    if (n_hits) *n_hits = 0;
    if (nseg == 0) {
        if (hit_offsets) hit_offsets[0] = 0;
        return QK_OK;
    }
    if (!offsets || !action || !drain || !hit_offsets || !n_hits || (cap && !hits) || nseg > 0xFFFFFFFFull)
        return QK_E_INVAL;
    for (size_t g = 0; g < nseg; ++g)
        if (offsets[g + 1] < offsets[g]) return QK_E_INVAL;
    const uint32_t T = threshold;
    const size_t rec = qk_u32_size(T);
    const uint64_t n = offsets[nseg] - offsets[0];
    if (!dev_words(d_mine) || !dev_words(d_peer) || !dev_words(d_mine_out) || (d_present && !is_device_ptr(d_present)) ||
        (n && !dev_words(d_log)))
        return QK_E_INVAL;
    if (is_device_ptr(action) || is_device_ptr(drain) || is_device_ptr(hit_offsets) || (cap && is_device_ptr(hits)))
        return QK_E_INVAL;
    if (ranges_overlap(d_mine_out, nseg * rec, d_mine, nseg * rec) || ranges_overlap(d_mine_out, nseg * rec, d_peer, nseg * rec) ||
        ranges_overlap(d_mine_out, nseg * rec, d_present, nseg) ||
        ranges_overlap(d_mine_out, nseg * rec, n ? d_log + offsets[0] : nullptr, n * 4))
        return QK_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    QK_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    SdPlan p;
    sd_plan(p, offsets, nseg, T, cap);
    SnSeg b;
    // the step's buffers and the decode's, one pass over the two arenas
    for (int pass = 0; pass < 2; ++pass) {
        Carve cs{pass ? (char *)ctx->d_flow[1] : nullptr}, ci{pass ? (char *)ctx->d_flow[0] : nullptr};
        sd_carve_plan(cs, ci, p, nseg, T, false);
        sn_carve(cs, b, nseg, T);
        if (!pass) {
            if (int e = ensure_flow(ctx, 1, cs.off, s)) return e;
            if (int e = ensure_flow(ctx, 0, ci.off, s)) return e;
        }
    }
    const size_t ni = p.items.size();
    const uint32_t *mine = (const uint32_t *)d_mine, *peer = (const uint32_t *)d_peer;
    uint32_t *mine_out = (uint32_t *)d_mine_out;
    const dim3 gseg((uint32_t)((nseg + SD_BLOCK / SN_GROUP - 1) / (SD_BLOCK / SN_GROUP)));
    const size_t lds_so = ((size_t)p.maxseg + 1) * sizeof(uint32_t);
    int rc = sd_upload(ctx, p, offsets, nseg, s);
    if (!rc && (hipMemsetAsync(b.fstop, 0xFF, nseg * 8, s) != hipSuccess ||
                hipMemsetAsync(b.acc, 0, nseg * (size_t)T * 8, s) != hipSuccess ||
                hipMemsetAsync(b.err, 0, 4, s) != hipSuccess))
        rc = QK_E_HIP;
    if (!rc) {
        if (ni) {
            hipEvent_t e0 = prof_begin(ctx, s);
            hipLaunchKernelGGL(k_snd_find, dim3((uint32_t)ni), dim3(SD_BLOCK),
                               ((size_t)p.maxseg * 3 + 1) * sizeof(uint32_t), s, d_log, p.d_items, p.b.offs, mine, peer,
                               d_present, T, p.maxseg, b.fstop);
            prof_end(ctx, s, e0);
            e0 = prof_begin(ctx, s);
            sn_prefix(d_log, p, T, b, s);
            prof_end(ctx, s, e0);
        }
        hipLaunchKernelGGL(k_snd_classify, gseg, dim3(SD_BLOCK), 0, s, mine, peer, d_present, d_log, p.b.offs, b.fstop,
                           b.acc, T, (uint32_t)nseg, mine_out, b.diff, b.action, b.drain, b.err);
        if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
    }
    if (!rc) rc = sd_enqueue(ctx, p, (const uint8_t *)b.diff, false, d_log, nseg, T, 1, s);
    if (!rc && ni) {
        const uint32_t rows = std::min<uint32_t>(p.maxseg * T, SN_REM_ROWS);
        hipLaunchKernelGGL(k_snd_remove, dim3((uint32_t)ni), dim3(SD_BLOCK), (size_t)rows * 8 + lds_so, s, d_log,
                           p.d_items, p.b.offs, p.d_mask, p.d_icnt, T, rows, b.acc);
        hipLaunchKernelGGL(k_snd_finish, gseg, dim3(SD_BLOCK), 0, s, p.b.segcnt, b.acc, T, (uint32_t)nseg, mine_out);
        if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
    }
    std::vector<uint32_t> segcnt(nseg);
    std::vector<int32_t> status(nseg);
    uint64_t total = 0;
    uint32_t err = 0;
    if (!rc && (hipMemcpyAsync(action, b.action, nseg, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(drain, b.drain, nseg * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(&err, b.err, 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(status.data(), p.b.status, nseg * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(segcnt.data(), p.b.segcnt, nseg * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(&total, p.b.total, 8, hipMemcpyDeviceToHost, s) != hipSuccess))
        rc = QK_E_HIP;
    // the one wait for the kernels (the pinned items and the offsets must outlive them)
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = QK_E_HIP;
    if (rc) return rc;
    if (err) return QK_E_MISMATCH;
    return sd_collect(p, status.data(), segcnt.data(), total, nseg, hits, cap, hit_offsets, n_hits);
}
