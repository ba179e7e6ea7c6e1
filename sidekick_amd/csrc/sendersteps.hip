// sendersteps.hip — every queued quACK of a flow stepped in one call
// (DESIGN.md §3.6.7): the loop of listen_for_quacks_power_sum
// (media_client.rs:223-323) over ALL datagrams a batch brought for a flow, one
// after the other, where wire.hip's ingest and sender.hip's step take the
// newest only.
//
// Ingest (qk_u32_wire_ingest_queue_device):
//   k_wq_validate  a wave per datagram: wire.h wire_validate (the rule set of
//                  the newest-only ingest), the flow index tested; the sort key
//                  of datagram i is its flow, or nseg when it is not accepted;
//                  the accepted datagrams counted per flow (integer atomics:
//                  the counts do not depend on the order of execution)
//   (D2H, wait)    the flag, the counts: a flow index out of range and the
//                  capacity are decided here, before d_queue is written
//   radix.h        stable LSD sort of (key, i): flow by flow, ascending i
//   k_wq_place     a wave per accepted datagram: its image into record r of
//                  the queue, r its rank in the sorted order
// Step (qk_u32_sender_steps_segments_device), sender.hip's chain once per
// round j = 0 .. max k_g - 1 over the same work items (segdecode.h SdItem),
// every kernel keyed on a per-flow device `begin` (the entries the flow's
// earlier quACKs of this call drained: an offset, the log is not moved) and an
// `alive` flag (cleared by the flow's first reset):
//   k_sq_init      the queue's threshold fields; every q_action UNSTEPPED
//   k_sq_find      first position at or after begin whose raw id equals the
//                  round's quACK's last value
//   k_sq_prefix    power sums of [begin, stop]
//   k_sq_classify  mine_out += prefix in place, reset bits, the diff record
//   (segdecode)    Newton over the diff records
//   k_sq_root_test the root test over [begin, stop) only: one mask bit per log
//                  entry, kept over the rounds (the intervals of successive
//                  quACKs are disjoint), the round's hits counted per flow
//   k_sq_remove    the round's hits out of mine_out's row
//   k_sq_finish    rows and counts into mine_out, begin += the round's drain
// and after the last round k_sq_item_count and segdecode's scan and hit write:
// one compaction, the hits ascending over the whole call.  All rounds are
// enqueued back to back; the call waits once.  A work item outside its flow's
// current interval leaves before it stages anything.  Integer only.
#include <string.h>

#include <algorithm>
#include <vector>

#include "bsgs.h"
#include "ctx.h"
#include "field.h"
#include "radix.h"
#include "segdecode.h"
#include "segments.h"
#include "sendersteps.h"
#include "wire.h"

namespace qk {

QK_WARM_KERNEL(sendersteps)

constexpr uint32_t SQ_WAVES = SD_BLOCK / 64;
constexpr uint32_t SQ_GROUP = 16;   // lanes per flow of k_sq_classify / k_sq_finish
constexpr unsigned long long SQ_NONE = ~0ull;

// what a round reads of the rounds before it, per flow
struct SqFlow {
    const uint64_t *offs;    // [nseg + 1] the log's CSR index
    const uint64_t *qoffs;   // [nseg + 1] the queue's
    uint64_t *begin;         // [nseg] entries drained so far by this call
    uint8_t *alive;          // [nseg] 0 after the flow's first reset
    // flow g steps a quACK in round j
    __device__ __forceinline__ bool turn(uint64_t g, uint32_t j) const {
        return alive[g] && j < qoffs[g + 1] - qoffs[g];
    }
    // the first log position of flow g's current interval
    __device__ __forceinline__ uint64_t first(uint64_t g) const { return offs[g] + begin[g]; }
};

// position a of the log relative to an item, clamped to it
__device__ __forceinline__ uint32_t sq_clamp(const SdItem &it, uint64_t a) {
    return a <= it.lo ? 0u : a - it.lo >= it.n ? it.n : (uint32_t)(a - it.lo);
}

// mine's and the quACK's last_value differ, compared as the Option they are (:233)
__device__ __forceinline__ bool sq_active(uint32_t m_has, uint32_t m_last, const uint32_t *hp) {
    const bool ps = hp[2] != 0, ms = m_has != 0;
    return !(ps == ms && (!ps || hp[3] == m_last));
}

// --------------------------------------------------------------------- init
__global__ __launch_bounds__(SD_BLOCK) void k_sq_init(const uint32_t *__restrict__ mine,
                                                      const uint32_t *__restrict__ queue, uint32_t nseg, uint32_t nq,
                                                      uint32_t T, uint8_t *__restrict__ q_action,
                                                      uint64_t *__restrict__ q_drain, uint32_t *__restrict__ qcnt,
                                                      uint32_t *__restrict__ err) {
    const uint64_t i = (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x;
    const size_t W = 4 + (size_t)T;
    bool bad = false;
    if (i < nseg) bad = mine[i * W] != T;
    if (i < nq) {
        bad |= queue[i * W] != T;
        q_action[i] = (uint8_t)QK_SND_UNSTEPPED;
        q_drain[i] = 0;
        qcnt[i] = 0;
    }
    if (bad) atomicOr(err, 1u);
}

// --------------------------------------------------------------------- find
// LDS: so[maxseg + 1], suse[maxseg], sval[maxseg], sbeg[maxseg]
__global__ __launch_bounds__(SD_BLOCK) void k_sq_find(const uint32_t *__restrict__ log,
                                                      const SdItem *__restrict__ items, SqFlow fl,
                                                      const uint32_t *__restrict__ mine,
                                                      const uint32_t *__restrict__ queue, uint32_t j, uint32_t T,
                                                      uint32_t maxseg, unsigned long long *__restrict__ fstop) {
    extern __shared__ uint32_t sq_sm[];
    __shared__ uint32_t s_any;
    uint32_t *so = sq_sm, *suse = so + maxseg + 1, *sval = suse + maxseg, *sbeg = sval + maxseg;
    const SdItem it = items[blockIdx.x];
    if (it.nseg == 1)   // a slice behind the flow's turn or before its interval: nothing staged
        if (!fl.turn(it.seg0, j) || fl.first(it.seg0) >= it.lo + it.n) return;
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    sd_stage_offsets(it, fl.offs, so);
    const size_t W = 4 + (size_t)T;
    for (uint32_t k = threadIdx.x; k < it.nseg; k += SD_BLOCK) {
        const uint64_t g = (uint64_t)it.seg0 + k;
        bool use = false;
        uint32_t val = 0, beg = 0;
        if (fl.turn(g, j)) {
            const uint32_t *hm = mine + g * W, *hp = queue + (fl.qoffs[g] + j) * W;
            use = hp[2] != 0 && sq_active(hm[2], hm[3], hp);
            val = hp[3];
            beg = sq_clamp(it, fl.first(g));
        }
        suse[k] = use;
        sval[k] = val;
        sbeg[k] = beg;
        if (use) s_any = 1;
    }
    __syncthreads();
    if (!s_any) return;
    for (uint32_t i = threadIdx.x; i < it.n; i += SD_BLOCK) {
        const uint32_t r = it.nseg > 1 ? sd_segment_of(so, it.nseg, i) : 0u;
        if (suse[r] && i >= sbeg[r] && log[it.lo + i] == sval[r])
            atomicMin(&fstop[(uint64_t)it.seg0 + r], (unsigned long long)(it.lo + i));
    }
}

// ------------------------------------------------------------------- prefix
// sender.hip k_snd_prefix from the flow's begin on.  An item of fewer than
// SQ_WAVES segments is walked by all waves, striped, only where the interval
// is long: a wave's share ends in K butterfly reductions and T atomics
// whatever it holds, which for an interval of SQ_SHORT entries or fewer (a few
// chain steps per lane) costs more than the walk, so one wave takes such an
// interval whole.  LDS: so[maxseg + 1].
constexpr uint32_t SQ_SHORT = 512;
template <int G, int K>
__global__ __launch_bounds__(SD_BLOCK) void k_sq_prefix(const uint32_t *__restrict__ log,
                                                        const SdItem *__restrict__ items, SqFlow fl,
                                                        const unsigned long long *__restrict__ fstop, uint32_t T,
                                                        unsigned long long *__restrict__ acc_out) {
    extern __shared__ uint32_t sq_sm[];
    uint32_t *so = sq_sm;
    const SdItem it = items[blockIdx.x];
    if (it.nseg == 1) {   // the whole workgroup leaves before staging anything
        const unsigned long long st = fstop[it.seg0];
        if (st == SQ_NONE || st < it.lo || fl.first(it.seg0) >= it.lo + it.n) return;
    }
    sd_stage_offsets(it, fl.offs, so);
    __syncthreads();
    constexpr uint32_t PER = 64 / G;   // ids per wave and step
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int jj = (int)(lane % G);
    const uint32_t slot = lane / G;
    const bool few = it.nseg < SQ_WAVES;
    for (uint32_t r = few ? 0u : wave; r < it.nseg; r += few ? 1u : SQ_WAVES) {
        const uint64_t g = (uint64_t)it.seg0 + r;
        const unsigned long long st = fstop[g];
        uint32_t b = so[r], e = so[r + 1];
        if (st == SQ_NONE || st < it.lo + b || b == e) continue;
        b = std::max(b, sq_clamp(it, fl.first(g)));
        if (st - it.lo < e) e = (uint32_t)(st - it.lo) + 1;
        const bool striped = few && e - b > SQ_SHORT;   // wave-uniform, as everything above
        if (few && !striped && r != wave) continue;     // r < SQ_WAVES: the short interval is wave r's
        const uint32_t first = striped ? wave * PER + slot : slot, stride = striped ? SQ_WAVES * PER : PER;
        uint64_t acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = 0;
        // terms < 6 * 2^32, at most SD_ITEM of them
        for (uint32_t i = b + first; i < e; i += stride) group_chain32<G, K>(acc, canon32(log[it.lo + i]), jj);
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

// ----------------------------------------------------------------- classify
// SQ_GROUP lanes per flow.  mine_out is the flow's running record: read, then
// written in place by the same lanes (the header by lane 0, after every lane
// of the group has read it: the group lies in one wave).  A flow without a
// turn gets an empty diff record, so Newton gives it degree 0.
__global__ __launch_bounds__(SD_BLOCK) void k_sq_classify(
    const uint32_t *__restrict__ queue, const uint32_t *__restrict__ log, SqFlow fl,
    const unsigned long long *__restrict__ fstop, unsigned long long *__restrict__ acc, uint32_t j, uint32_t T,
    uint32_t nseg, uint32_t *mine_out, uint32_t *__restrict__ diff, uint8_t *__restrict__ q_action,
    uint64_t *__restrict__ q_drain, uint64_t *__restrict__ rdrain, uint32_t *__restrict__ rcnt,
    uint32_t *__restrict__ stepped) {
    const uint32_t jl = threadIdx.x % SQ_GROUP;
    const uint64_t g = (uint64_t)blockIdx.x * (SD_BLOCK / SQ_GROUP) + threadIdx.x / SQ_GROUP;
    if (g >= nseg) return;
    const size_t W = 4 + (size_t)T;
    uint32_t *mo = mine_out + g * W, *df = diff + g * W;
    if (!fl.turn(g, j)) {
        if (jl == 0) {
            df[0] = T, df[1] = 0, df[2] = 0, df[3] = 0;
            rdrain[g] = 0;
            rcnt[g] = 0;
        }
        return;
    }
    const uint64_t q = fl.qoffs[g] + j;
    const uint32_t *hp = queue + q * W;
    uint32_t c1 = mo[1], hl = mo[2], lv = mo[3];
    const bool active = sq_active(hl, lv, hp);
    const unsigned long long st = active ? fstop[g] : SQ_NONE;
    const bool found = st != SQ_NONE;
    uint64_t idx = 0;
    if (found) {
        idx = st - fl.first(g);
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
    for (uint32_t k = jl; k < T; k += SQ_GROUP) {
        uint32_t m = mo[4 + k];
        if (found) m = add32(m, canon32(fold64_32(acc[g * T + k])));
        mo[4 + k] = m;
        if (decode) {
            df[4 + k] = sub32(m, hp[4 + k]);
            acc[g * T + k] = m;
        }
    }
    if (jl == 0) {
        mo[0] = T, mo[1] = c1, mo[2] = hl, mo[3] = lv;
        df[0] = T, df[1] = decode ? c1 - hp[1] : 0u, df[2] = decode ? 1u : 0u, df[3] = lv;
        q_action[q] = (uint8_t)(!active ? QK_SND_IDLE : bits ? bits : QK_SND_ADVANCED);
        q_drain[q] = decode ? idx + 1 : 0;
        rdrain[g] = decode ? idx + 1 : 0;
        rcnt[g] = 0;
        stepped[g] = j + 1;
        if (bits) fl.alive[g] = 0;
    }
}

// ---------------------------------------------------------------- root test
// segdecode.hip k_seg_root_test over the flows' current intervals [begin,
// stop) only; the hit bits are OR-ed into the call's mask, the round's hits
// counted per flow.  LDS: so[maxseg + 1], sdeg, slo, shi [maxseg], then the
// coefficient rows, T + 1 words apart.
__global__ __launch_bounds__(SD_BLOCK) void k_sq_root_test(const uint32_t *__restrict__ log,
                                                           const SdItem *__restrict__ items, SqFlow fl,
                                                           const unsigned long long *__restrict__ fstop,
                                                           const uint32_t *__restrict__ coef,
                                                           const uint32_t *__restrict__ deg, uint32_t T,
                                                           uint32_t maxseg, uint64_t *__restrict__ mask,
                                                           uint32_t *__restrict__ rcnt) {
    extern __shared__ uint32_t sq_sm[];
    __shared__ uint32_t s_any;
    uint32_t *so = sq_sm, *sdeg = so + maxseg + 1, *slo = sdeg + maxseg, *shi = slo + maxseg;
    uint32_t *sc = shi + maxseg;
    const SdItem it = items[blockIdx.x];
    if (it.nseg == 1) {   // a slice of a flow that does not decode, or outside its interval: nothing staged
        const unsigned long long st = fstop[it.seg0];
        if (deg[it.seg0] == 0 || st == SQ_NONE || st <= it.lo || fl.first(it.seg0) >= it.lo + it.n) return;
    }
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    sd_stage_offsets(it, fl.offs, so);
    for (uint32_t k = threadIdx.x; k < it.nseg; k += SD_BLOCK) {
        const uint64_t g = (uint64_t)it.seg0 + k;
        const uint32_t d = deg[g];
        const unsigned long long st = fstop[g];
        const bool use = d != 0 && st != SQ_NONE;   // a degree comes with a stop; both tested
        sdeg[k] = use ? d : 0u;
        slo[k] = use ? sq_clamp(it, fl.first(g)) : 0u;
        shi[k] = use ? sq_clamp(it, st) : 0u;
        if (use) s_any = 1;
    }
    __syncthreads();
    if (!s_any) return;
    for (uint32_t idx = threadIdx.x; idx < it.nseg * T; idx += SD_BLOCK) {
        const uint32_t r = idx / T, k = idx - r * T;
        sc[r * (T + 1) + k] = coef[(uint64_t)it.seg0 * T + idx];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t base = 0; base < it.n; base += SD_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        const bool valid = i < it.n;
        const uint32_t r = valid && it.nseg > 1 ? sd_segment_of(so, it.nseg, i) : 0u;
        const uint32_t d = valid && i >= slo[r] && i < shi[r] ? sdeg[r] : 0u;
        uint32_t dm = d;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)dm, off, 64);
            dm = o > dm ? o : dm;
        }
        if (dm == 0) continue;   // wave-uniform: the wave's 64 entries lie outside every interval
        const uint32_t x = canon32(d ? log[it.lo + i] : 0u), x5 = times5_32(x);
        const uint32_t *c = sc + r * (T + 1);
        uint32_t lo = 1, hi = 0;
        for (uint32_t k = 0; k < dm; ++k)
            if (k < d) tstep32(lo, hi, x, x5, c[k]);
        const bool hit = d > 0 && canon32(fold64_32(((uint64_t)hi << 32) | lo)) == 0;
        if (hit) atomicAdd(&rcnt[(uint64_t)it.seg0 + r], 1u);
        const uint64_t m = __ballot(hit);
        // the word is this wave's alone, in every round
        if (lane == 0 && m) mask[(uint64_t)blockIdx.x * SD_WORDS + base / 64 + wave] |= m;
    }
}

// ------------------------------------------------------------------- remove
// sender.hip k_snd_remove for the round's hits: the mask bits inside the
// current interval of a flow that counted hits this round.
// LDS: lrow[rows] (u64), then so[maxseg + 1], slo[maxseg], shi[maxseg].
constexpr uint32_t SQ_REM_ROWS = 4096;
__global__ __launch_bounds__(SD_BLOCK) void k_sq_remove(const uint32_t *__restrict__ log,
                                                        const SdItem *__restrict__ items, SqFlow fl,
                                                        const unsigned long long *__restrict__ fstop,
                                                        const uint64_t *__restrict__ mask,
                                                        const uint32_t *__restrict__ rcnt, uint32_t T, uint32_t rows,
                                                        uint32_t maxseg, unsigned long long *__restrict__ acc) {
    extern __shared__ unsigned long long sq_sm64[];
    __shared__ uint32_t s_any;
    unsigned long long *lrow = sq_sm64;
    uint32_t *so = reinterpret_cast<uint32_t *>(sq_sm64 + rows), *slo = so + maxseg + 1, *shi = slo + maxseg;
    const SdItem it = items[blockIdx.x];
    if (it.nseg == 1) {
        const unsigned long long st = fstop[it.seg0];
        if (rcnt[it.seg0] == 0 || st == SQ_NONE || st <= it.lo || fl.first(it.seg0) >= it.lo + it.n) return;
    }
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    const uint32_t words = it.nseg * T;
    const bool local = words <= rows;
    sd_stage_offsets(it, fl.offs, so);
    for (uint32_t k = threadIdx.x; k < it.nseg; k += SD_BLOCK) {
        const uint64_t g = (uint64_t)it.seg0 + k;
        const unsigned long long st = fstop[g];
        const bool use = rcnt[g] != 0 && st != SQ_NONE;
        slo[k] = use ? sq_clamp(it, fl.first(g)) : 0u;
        shi[k] = use ? sq_clamp(it, st) : 0u;
        if (use) s_any = 1;
    }
    __syncthreads();
    if (!s_any) return;
    if (local)
        for (uint32_t k = threadIdx.x; k < words; k += SD_BLOCK) lrow[k] = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < it.n; i += SD_BLOCK) {
        if (!((mask[(uint64_t)blockIdx.x * SD_WORDS + i / 64] >> (i & 63)) & 1)) continue;
        const uint32_t r = it.nseg > 1 ? sd_segment_of(so, it.nseg, i) : 0u;
        if (i < slo[r] || i >= shi[r]) continue;   // a hit of an earlier round
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

// the rows of the flows with hits this round, canonical, their counts, and
// the round's drain onto begin
__global__ __launch_bounds__(SD_BLOCK) void k_sq_finish(SqFlow fl, const uint32_t *__restrict__ rcnt,
                                                        const uint64_t *__restrict__ rdrain,
                                                        const unsigned long long *__restrict__ acc, uint32_t j,
                                                        uint32_t T, uint32_t nseg, uint32_t *__restrict__ mine_out,
                                                        uint32_t *__restrict__ qcnt) {
    const uint32_t jl = threadIdx.x % SQ_GROUP;
    const uint64_t g = (uint64_t)blockIdx.x * (SD_BLOCK / SQ_GROUP) + threadIdx.x / SQ_GROUP;
    if (g >= nseg) return;
    const uint32_t c = rcnt[g];
    const uint64_t d = rdrain[g];
    if (c) {   // hits: the flow had its turn
        uint32_t *mo = mine_out + g * (4 + (size_t)T);
        if (jl == 0) {
            mo[1] -= c;
            qcnt[fl.qoffs[g] + j] = c;
        }
        for (uint32_t k = jl; k < T; k += SQ_GROUP) mo[4 + k] = canon32(fold64_32(acc[g * T + k]));
    }
    if (jl == 0 && d) fl.begin[g] += d;
}

// the call's hits per work item: a wave per item, lane l its mask word l
__global__ __launch_bounds__(64) void k_sq_item_count(const uint64_t *__restrict__ mask, uint32_t *__restrict__ itemcnt) {
    const uint32_t l = threadIdx.x;
    uint32_t c = l < SD_WORDS ? (uint32_t)__popcll(mask[(uint64_t)blockIdx.x * SD_WORDS + l]) : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += (uint32_t)__shfl_xor((int)c, off, 64);
    if (l == 0) itemcnt[blockIdx.x] = c;
}

// ------------------------------------------------------------------- ingest
constexpr uint32_t WQ_BLOCK = 256;
constexpr uint32_t WQ_WAVES = WQ_BLOCK / 64;

// key[i]: the flow of an accepted datagram, nseg for any other; val[i] = i;
// cnt[nseg] is the flag of a flow index out of range
__global__ __launch_bounds__(WQ_BLOCK) void k_wq_validate(const uint8_t *__restrict__ wire, uint64_t stride,
                                                          const uint32_t *__restrict__ len,
                                                          const uint32_t *__restrict__ flow, uint32_t n, uint32_t T,
                                                          uint32_t nseg, int32_t *__restrict__ status,
                                                          uint32_t *__restrict__ key, uint32_t *__restrict__ val,
                                                          uint32_t *__restrict__ cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * WQ_WAVES + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (i >= n) return;
    const int mine = wire_validate(wire + i * stride, len[i], stride, T, lane, 64);
    // every rule before the sums answers alike in all lanes; a sum >= p in any lane's share is QK_E_FORMAT
    const int st = __any(mine == QK_E_FORMAT) ? QK_E_FORMAT : mine;
    if (lane) return;
    status[i] = st;
    const uint32_t f = flow[i];
    const bool ok = st == QK_OK && f < nseg;
    key[i] = ok ? f : nseg;
    val[i] = (uint32_t)i;
    if (f >= nseg) atomicOr(&cnt[nseg], 1u);
    else if (ok) atomicAdd(&cnt[f], 1u);
}

// record r of the queue from datagram perm[r], r < m
__global__ __launch_bounds__(WQ_BLOCK) void k_wq_place(const uint8_t *__restrict__ wire, uint64_t stride,
                                                       const uint32_t *__restrict__ len,
                                                       const uint32_t *__restrict__ perm, uint32_t m, uint32_t n,
                                                       uint32_t T, uint32_t *__restrict__ queue) {
    const uint64_t r = (uint64_t)blockIdx.x * WQ_WAVES + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (r >= m) return;
    const uint32_t i = perm[r];
    if (i >= n) return;   // the sort's values are 0 .. n - 1
    const uint8_t *buf = wire + i * stride;
    uint32_t *row = queue + r * (4 + (uint64_t)T);
    if (lane == 0) {
        uint32_t count, has_last, last;
        wire_header(buf, len[i], T, count, has_last, last);
        row[0] = T;
        row[1] = count;
        row[2] = has_last;
        row[3] = last;
    }
    for (uint32_t k = lane; k < T; k += 64) row[4 + k] = wire_get32(buf + 8 + 4 * (uint64_t)k);
}

// --------------------------------------------------------------------- host
// the step's own buffers beside the decode's, in the per-flow arena
struct SqSeg {
    unsigned long long *fstop = nullptr, *acc = nullptr;
    uint32_t *diff = nullptr, *err = nullptr, *stepped = nullptr, *qcnt = nullptr;
    uint64_t *qoffs = nullptr, *begin = nullptr, *rdrain = nullptr, *q_drain = nullptr;
    uint8_t *alive = nullptr, *q_action = nullptr;
};

static void sq_carve(Carve &cv, SqSeg &b, const SqSizes &z) {
    b.fstop = cv.take<unsigned long long>(z.nseg);
    b.acc = cv.take<unsigned long long>(z.nseg * z.T);
    b.diff = cv.take<uint32_t>(z.nseg * (4 + z.T));
    b.err = cv.take<uint32_t>(1);
    b.stepped = cv.take<uint32_t>(z.nseg);
    b.qcnt = cv.take<uint32_t>(z.nq);
    b.qoffs = cv.take<uint64_t>(z.nseg + 1);
    b.begin = cv.take<uint64_t>(z.nseg);
    b.rdrain = cv.take<uint64_t>(z.nseg);
    b.q_drain = cv.take<uint64_t>(z.nq);
    b.alive = cv.take<uint8_t>(z.nseg);
    b.q_action = cv.take<uint8_t>(z.nq);
}

template <int G, int K>
static void sq_prefix_gk(const uint32_t *log, const SdPlan &p, const SqFlow &fl, uint32_t T, const SqSeg &b,
                         hipStream_t s) {
    hipLaunchKernelGGL((k_sq_prefix<G, K>), dim3((uint32_t)p.items.size()), dim3(SD_BLOCK),
                       ((size_t)p.maxseg + 1) * sizeof(uint32_t), s, log, p.d_items, fl, b.fstop, T, b.acc);
}
// sender.hip sn_prefix's dispatch
static void sq_prefix(const uint32_t *log, const SdPlan &p, const SqFlow &fl, uint32_t T, const SqSeg &b,
                      hipStream_t s) {
    if (T <= 4) sq_prefix_gk<1, 4>(log, p, fl, T, b, s);
    else if (T <= 8) sq_prefix_gk<1, 8>(log, p, fl, T, b, s);
    else if (T <= 16) sq_prefix_gk<1, 16>(log, p, fl, T, b, s);
    else if (T <= 32) sq_prefix_gk<1, 32>(log, p, fl, T, b, s);
    else if (T <= 64) sq_prefix_gk<2, 32>(log, p, fl, T, b, s);
    else if (T <= 128) sq_prefix_gk<4, 32>(log, p, fl, T, b, s);
    else if (T <= 256) sq_prefix_gk<8, 32>(log, p, fl, T, b, s);
    else if (T <= 512) sq_prefix_gk<16, 32>(log, p, fl, T, b, s);
    else sq_prefix_gk<32, 32>(log, p, fl, T, b, s);
}

} // namespace qk

using namespace qk;

extern "C" int qk_u32_sender_steps_segments_device(qk_ctx *ctx, const uint8_t *d_mine, const uint8_t *d_queue,
                                                   const uint64_t *q_offsets, const uint32_t *d_log,
                                                   const uint64_t *offsets, size_t nseg, uint32_t threshold,
                                                   uint8_t *d_mine_out, uint8_t *q_action, uint64_t *q_drain,
                                                   uint32_t *stepped, uint64_t *drain, uint64_t *hits, size_t cap,
                                                   uint64_t *hit_offsets, size_t *n_hits, void *stream) {
    if (int e = check_ctx_threshold(ctx, threshold)) return e;
    if (n_hits) *n_hits = 0;
    if (nseg == 0) {
        if (hit_offsets) hit_offsets[0] = 0;
        return QK_OK;
    }
    if (!offsets || !q_offsets || !stepped || !drain || !hit_offsets || !n_hits || (cap && !hits) ||
        nseg > 0xFFFFFFFFull)
        return QK_E_INVAL;
    uint64_t maxk = 0;
    if (!sq_check(offsets, q_offsets, nseg, &maxk)) return QK_E_INVAL;
    const uint64_t nq = q_offsets[nseg];
    if (nq > 0xFFFFFFFFull || (nq && (!q_action || !q_drain))) return QK_E_INVAL;
    const uint32_t T = threshold;
    const size_t rec = qk_u32_size(T);
    const uint64_t n = offsets[nseg] - offsets[0];
    if (!dev_words(d_mine) || !dev_words(d_mine_out) || (nq && !dev_words(d_queue)) || (n && !dev_words(d_log)))
        return QK_E_INVAL;
    if (is_device_ptr(offsets) || is_device_ptr(q_offsets) || is_device_ptr(stepped) || is_device_ptr(drain) ||
        is_device_ptr(hit_offsets) || (nq && (is_device_ptr(q_action) || is_device_ptr(q_drain))) ||
        (cap && is_device_ptr(hits)))
        return QK_E_INVAL;
    if (ranges_overlap(d_mine_out, nseg * rec, d_mine, nseg * rec) ||
        ranges_overlap(d_mine_out, nseg * rec, nq ? d_queue : nullptr, (size_t)nq * rec) ||
        ranges_overlap(d_mine_out, nseg * rec, n ? d_log + offsets[0] : nullptr, n * 4))
        return QK_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    QK_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    SdPlan p;
    sd_plan(p, offsets, nseg, T, cap);
    const SqSizes z{nseg, (size_t)nq, T};
    SqSeg b;
    for (int pass = 0; pass < 2; ++pass) {
        Carve cs{pass ? (char *)ctx->d_flow[1] : nullptr}, ci{pass ? (char *)ctx->d_flow[0] : nullptr};
        sd_carve_plan(cs, ci, p, nseg, T, false);
        sq_carve(cs, b, z);
        if (!pass) {
            if (int e = ensure_flow(ctx, 1, cs.off, s)) return e;
            if (int e = ensure_flow(ctx, 0, ci.off, s)) return e;
        }
    }
    const size_t ni = p.items.size();
    const uint32_t *mine = (const uint32_t *)d_mine, *queue = (const uint32_t *)d_queue;
    uint32_t *mine_out = (uint32_t *)d_mine_out;
    const dim3 gseg((uint32_t)((nseg + SD_BLOCK / SQ_GROUP - 1) / (SD_BLOCK / SQ_GROUP)));
    const uint32_t ms = p.maxseg;
    const SqLds lds = sq_lds(ms, T, std::min<uint32_t>(ms * T, SQ_REM_ROWS));
    int rc = sd_upload(ctx, p, offsets, nseg, s);
    const SqFlow fl{p.b.offs, b.qoffs, b.begin, b.alive};
    if (!rc && (hipMemcpyAsync(b.qoffs, q_offsets, (nseg + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
                hipMemcpyAsync(mine_out, mine, nseg * rec, hipMemcpyDeviceToDevice, s) != hipSuccess ||
                hipMemsetAsync(b.begin, 0, nseg * 8, s) != hipSuccess ||
                hipMemsetAsync(b.alive, 1, nseg, s) != hipSuccess ||
                hipMemsetAsync(b.stepped, 0, nseg * 4, s) != hipSuccess ||
                hipMemsetAsync(b.err, 0, 4, s) != hipSuccess ||
                (ni && hipMemsetAsync(p.d_mask, 0, ni * SD_WORDS * 8, s) != hipSuccess)))
        rc = QK_E_HIP;
    if (!rc) {
        const uint64_t m = std::max<uint64_t>(nseg, nq);
        hipLaunchKernelGGL(k_sq_init, dim3((uint32_t)((m + SD_BLOCK - 1) / SD_BLOCK)), dim3(SD_BLOCK), 0, s, mine, queue,
                           (uint32_t)nseg, (uint32_t)nq, T, b.q_action, b.q_drain, b.qcnt, b.err);
        if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
    }
    for (uint32_t j = 0; !rc && j < maxk; ++j) {
        if (hipMemsetAsync(b.fstop, 0xFF, nseg * 8, s) != hipSuccess ||
            hipMemsetAsync(b.acc, 0, nseg * (size_t)T * 8, s) != hipSuccess) {
            rc = QK_E_HIP;
            break;
        }
        if (ni) {
            hipLaunchKernelGGL(k_sq_find, dim3((uint32_t)ni), dim3(SD_BLOCK), lds.find, s, d_log, p.d_items, fl,
                               (const uint32_t *)mine_out, queue, j, T, ms, b.fstop);
            sq_prefix(d_log, p, fl, T, b, s);
        }
        hipLaunchKernelGGL(k_sq_classify, gseg, dim3(SD_BLOCK), 0, s, queue, d_log, fl, b.fstop, b.acc, j, T,
                           (uint32_t)nseg, mine_out, b.diff, b.q_action, b.q_drain, b.rdrain, p.b.segcnt, b.stepped);
        if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
        if (!rc) rc = sd_newton(ctx, (const uint8_t *)b.diff, false, nseg, T, p.b, s);
        if (!rc && ni) {
            hipLaunchKernelGGL(k_sq_root_test, dim3((uint32_t)ni), dim3(SD_BLOCK), lds.root, s, d_log, p.d_items, fl,
                               b.fstop, p.b.coef, p.b.deg, T, ms, p.d_mask, p.b.segcnt);
            hipLaunchKernelGGL(k_sq_remove, dim3((uint32_t)ni), dim3(SD_BLOCK), lds.remove, s, d_log, p.d_items, fl,
                               b.fstop, p.d_mask, p.b.segcnt, T, lds.rows, ms, b.acc);
        }
        if (!rc) {
            hipLaunchKernelGGL(k_sq_finish, gseg, dim3(SD_BLOCK), 0, s, fl, p.b.segcnt, b.rdrain, b.acc, j, T,
                               (uint32_t)nseg, mine_out, b.qcnt);
            if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
        }
    }
    if (!rc && ni) {
        hipLaunchKernelGGL(k_sq_item_count, dim3((uint32_t)ni), dim3(64), 0, s, p.d_mask, p.d_icnt);
        if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
        if (!rc) rc = sd_compact(p, s);
    }
    std::vector<uint32_t> qcnt(nq);
    uint64_t total = 0;
    uint32_t err = 0;
    if (!rc && (hipMemcpyAsync(stepped, b.stepped, nseg * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(drain, b.begin, nseg * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(&err, b.err, 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(&total, p.b.total, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
                (nq && (hipMemcpyAsync(q_action, b.q_action, nq, hipMemcpyDeviceToHost, s) != hipSuccess ||
                        hipMemcpyAsync(q_drain, b.q_drain, nq * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
                        hipMemcpyAsync(qcnt.data(), b.qcnt, nq * 4, hipMemcpyDeviceToHost, s) != hipSuccess))))
        rc = QK_E_HIP;
    // the one wait for the kernels (the pinned items and the offsets must outlive them)
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = QK_E_HIP;
    if (rc) return rc;
    if (err) return QK_E_MISMATCH;
    hit_offsets[0] = 0;
    for (size_t q = 0; q < nq; ++q) hit_offsets[q + 1] = hit_offsets[q] + qcnt[q];
    *n_hits = (size_t)total;
    if (hit_offsets[nq] != total) return QK_E_HIP;   // the two counts are kept by different kernels
    if (total > cap) return QK_E_CAPACITY;
    if (total) QK_HIP_TRY(hipMemcpy(hits, p.d_hit, total * 8, hipMemcpyDeviceToHost));
    return QK_OK;
}

extern "C" int qk_u32_wire_ingest_queue_device(qk_ctx *ctx, const uint8_t *d_wire, size_t stride,
                                               const uint32_t *d_len, const uint32_t *d_flow, size_t n,
                                               uint32_t threshold, size_t nseg, uint8_t *d_queue, size_t cap,
                                               uint64_t *q_offsets, int32_t *status, size_t *n_accepted,
                                               void *stream) {
    if (int e = check_ctx_threshold(ctx, threshold)) return e;
    if (!n_accepted || !q_offsets || stride == 0 || n > 0xFFFFFFFFull || nseg >= 0xFFFFFFFFull ||
        (n && (nseg == 0 || !status)))
        return QK_E_INVAL;
    *n_accepted = 0;
    const uint32_t T = threshold;
    const size_t rec = qk_u32_size(T);
    std::lock_guard<std::mutex> lk(ctx->mu);
    QK_HIP_TRY(hipSetDevice(ctx->device));
    if (is_device_ptr(q_offsets)) return QK_E_INVAL;
    if (cap && !dev_words(d_queue)) return QK_E_INVAL;
    if (n && (!d_wire || !is_device_ptr(d_wire) || !dev_words(d_len) || !dev_words(d_flow) || is_device_ptr(status)))
        return QK_E_INVAL;
    const void *in[3] = {d_wire, d_len, d_flow};
    const size_t inb[3] = {n * stride, n * 4, n * 4};
    for (int i = 0; i < 3; ++i)
        if (ranges_overlap(d_queue, cap * rec, in[i], inb[i])) return QK_E_INVAL;
    if (n == 0) {
        for (size_t g = 0; g <= nseg; ++g) q_offsets[g] = 0;
        return QK_OK;
    }
    hipStream_t s = pick_stream(ctx, stream);
    const RsPlan pl = rs_plan(ctx, n, 4);
    uint32_t *x = nullptr, *y = nullptr, *cnt = nullptr;
    int32_t *d_status = nullptr;
    RsScratch sc{};
    for (int pass = 0; pass < 2; ++pass) {
        Carve cp{pass ? (char *)ctx->d_flow[0] : nullptr}, cf{pass ? (char *)ctx->d_flow[1] : nullptr};
        x = cp.take<uint32_t>(wq_region_words(n));
        y = cp.take<uint32_t>(wq_region_words(n));
        d_status = cp.take<int32_t>(n);
        sc.take(cp, pl.nwg, n);
        cnt = cf.take<uint32_t>(nseg + 1);
        if (!pass) {
            if (int e = ensure_flow(ctx, 0, cp.off, s)) return e;
            if (int e = ensure_flow(ctx, 1, cf.off, s)) return e;
        }
    }
    const dim3 grid((uint32_t)((n + WQ_WAVES - 1) / WQ_WAVES));
    QK_HIP_TRY(hipMemsetAsync(cnt, 0, (nseg + 1) * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_wq_validate, grid, dim3(WQ_BLOCK), 0, s, d_wire, (uint64_t)stride, d_len, d_flow, (uint32_t)n,
                       T, (uint32_t)nseg, d_status, x, x + n, cnt);
    int rc = hipGetLastError() == hipSuccess ? QK_OK : QK_E_HIP;
    // the call's one mid-way wait: a flow index out of range and the capacity
    // are decided here, before any output array is written
    std::vector<uint32_t> h_cnt(nseg + 1);
    if (!rc && hipMemcpyAsync(h_cnt.data(), cnt, (nseg + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s) != hipSuccess)
        rc = QK_E_HIP;
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = QK_E_HIP;
    if (rc) return rc;
    if (h_cnt[nseg]) return QK_E_INVAL;
    const uint64_t m = wq_offsets(h_cnt.data(), nseg, q_offsets);
    *n_accepted = (size_t)m;
    if (m > n) return QK_E_HIP;
    if (m <= cap && m) {
        int where = 0;
        rc = rs_sort(ctx, x, x + n, y, y + n, n, bit_width32((uint32_t)nseg), sc, s, where, &pl);
        if (!rc) {
            const uint32_t *perm = (where ? y : x) + n;
            hipLaunchKernelGGL(k_wq_place, dim3((uint32_t)((m + WQ_WAVES - 1) / WQ_WAVES)), dim3(WQ_BLOCK), 0, s, d_wire,
                               (uint64_t)stride, d_len, perm, (uint32_t)m, (uint32_t)n, T, (uint32_t *)d_queue);
            if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
        }
    }
    if (!rc && hipMemcpyAsync(status, d_status, n * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess)
        rc = QK_E_HIP;
    // the arenas must outlive what was enqueued
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = QK_E_HIP;
    if (rc) return rc;
    return m > cap ? QK_E_CAPACITY : QK_OK;
}
