// pktsnap.hip — the proxy's frequency loop over captured packets
// (qk_u32_snapshot_flows_device):
//     for each captured packet (sidekick_multi.rs:256-286)
//         Insert { addr_key, id } => { let quack = sc.insert(addr_key, id);
//                                      if quack.count() % frequency_pkts == 0 { send(serialize(&quack)) } }
//         Reset  { .. }           => sc = SidekickMulti::new(..)            (:263-266)
// against a flow table held by AddrKey in device memory (flowtable.hip's flow
// array): every quACK the loop would have sent, in the order it would have
// sent them, and the table after the batch's last packet.
//
// Per call: the packet front's extract over the batch (flowfront.h: filters,
// AddrKey, hash table; one pass over the records) with the Reset positions
// listed from its (slot, id) output (k_ps_resets).  The batch falls into
// epochs between Resets (pktsnap.h); a batch without one, the common case, is
// one epoch and reuses that extract, a batch with Resets reruns it per epoch
// (the records read twice, and a third time when the caps may be too small
// and a counting pass over the epochs comes first: Resets are rare, one per
// receiver request, media_client.rs:272).  Per epoch:
//   flow_key_order / flow_rank_keys   the epoch's flows in AddrKey order
//   flow_slots_to_ranks, k_ps_iota, rs_sort, flow_rank_offsets
//                     the Inserts grouped stably by flow rank, each carrying
//                     its packet index; the flows' offsets
//   ft_join_merge     merge path of the table's keys with the epoch's
//                     (flowjoin.h), when the epoch builds on the table
//   k_ps_match, k_ps_base   one base record per flow: the table's, or
//                     qk_u32_init's for a new key or behind a Reset
//   (D2H, wait)       offsets and base counts: the host knows every cut
//                     (snapshots.h), the capacity is decided before any output
//   k_ps_gather       ids and arrival indices into grouped order; marks the
//                     packets that emit
//   k_row_scan, k_tot_scan   (radix.h) prefix sums of the marks: a snapshot's
//                     send-order row is its packet's rank among the marked
//   k_ps_dest         that row, per emitting grouped position
//   sn_walk_run       the snapshot walk (snapwalk.h) writes every snapshot at
//                     that row with its key and index, and the tail epoch's
//                     end-of-batch records
//   k_ps_upsert       the table after the batch: the join's union, a matched
//                     row replaced by its end-of-batch record, one pass
// No library sort or scan; integer only.
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx.h"
#include "field.h"
#include "flowfront.h"
#include "flowjoin.h"
#include "pktsnap.h"
#include "radix.h"
#include "segments.h"
#include "snapshots.h"
#include "snapwalk.h"

namespace qk {

QK_WARM_KERNEL(pktsnap)

constexpr uint32_t PS_BLOCK = 256;
enum : uint32_t { PS_F_ORDER = 1, PS_F_MISMATCH = 2 };

// the caller's table: every record of threshold T, the keys strictly
// ascending in memcmp order
__global__ __launch_bounds__(PS_BLOCK) void k_ps_check(const uint32_t *__restrict__ keys,
                                                       const uint32_t *__restrict__ rec, uint32_t nt, uint32_t T,
                                                       uint32_t *__restrict__ flags) {
    const uint32_t j = blockIdx.x * PS_BLOCK + threadIdx.x;
    if (j >= nt) return;
    uint32_t f = rec[(size_t)j * (4 + T)] != T ? PS_F_MISMATCH : 0u;
    if (j) {
        const uint32_t *a = keys + 3 * (size_t)(j - 1), *b = a + 3;
        int c = 0;
        for (int w = 0; w < 3 && c == 0; ++w) {
            const uint32_t x = __builtin_bswap32(a[w]), y = __builtin_bswap32(b[w]);
            c = x < y ? -1 : x > y ? 1 : 0;
        }
        if (c >= 0) f |= PS_F_ORDER;
    }
    if (f) atomicOr(flags, f);
}

// the positions of the Reset packets, in any order (the extract's marker)
__global__ __launch_bounds__(PS_BLOCK) void k_ps_resets(const uint32_t *__restrict__ slots,
                                                        const uint32_t *__restrict__ ids, uint64_t n,
                                                        uint32_t *__restrict__ list, uint32_t cap,
                                                        uint32_t *__restrict__ count) {
    const uint64_t stride = (uint64_t)gridDim.x * PS_BLOCK;
    for (uint64_t i = (uint64_t)blockIdx.x * PS_BLOCK + threadIdx.x; i < n; i += stride)
        if (slots[i] == SLOT_NONE && ids[i] == FLOW_ID_RESET) {
            const uint32_t k = atomicAdd(count, 1u);
            if (k < cap) list[k] = (uint32_t)i;
        }
}

__global__ __launch_bounds__(PS_BLOCK) void k_ps_iota(uint32_t *__restrict__ idx, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * PS_BLOCK;
    for (uint64_t i = (uint64_t)blockIdx.x * PS_BLOCK + threadIdx.x; i < n; i += stride) idx[i] = (uint32_t)i;
}

// match[ib] = the table row of batch flow ib's key (FT_NONE: a new key), from
// the join's (a index, b index) pairs
__global__ __launch_bounds__(PS_BLOCK) void k_ps_match(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ sb,
                                                       const uint32_t *__restrict__ tilecnt, uint32_t ntiles,
                                                       uint32_t na, uint32_t nb, uint32_t *__restrict__ match) {
    const uint64_t x = (uint64_t)blockIdx.x * PS_BLOCK + threadIdx.x;
    const uint64_t k = x / FT_SLOTS;
    const uint32_t e = (uint32_t)(x % FT_SLOTS);
    if (k >= ntiles || e >= min(tilecnt[k], FT_SLOTS)) return;
    const uint32_t ia = sa[x], ib = sb[x];
    if (ib < nb) match[ib] = ia < na ? ia : FT_NONE;
}

// base[g] = the table's record of flow g's key, or qk_u32_init's (match ==
// null: every flow is new); cnt[g] = its count
__global__ __launch_bounds__(PS_BLOCK) void k_ps_base(const uint32_t *__restrict__ rec,
                                                      const uint32_t *__restrict__ match, uint32_t nf, uint32_t T,
                                                      uint32_t *__restrict__ base, uint32_t *__restrict__ cnt) {
    const uint32_t W = 4 + T;
    const uint64_t words = (uint64_t)nf * W, stride = (uint64_t)gridDim.x * PS_BLOCK;
    for (uint64_t i = (uint64_t)blockIdx.x * PS_BLOCK + threadIdx.x; i < words; i += stride) {
        const uint32_t g = (uint32_t)(i / W), w = (uint32_t)(i - (uint64_t)g * W);
        const uint32_t ia = match ? match[g] : FT_NONE;
        const uint32_t v = ia != FT_NONE ? rec[(uint64_t)ia * W + w] : (w == 0 ? T : 0u);
        base[i] = v;
        if (w == 1) cnt[g] = v;
    }
}

// Grouped position p (flow key[p], packet idx[p] of the epoch): its id and its
// arrival index in the batch; the packet is marked when it brings its flow's
// wrapping u32 count to a multiple of f (snapshots.h: the walk's own rule)
__global__ __launch_bounds__(PS_BLOCK) void k_ps_gather(const uint32_t *__restrict__ key,
                                                        const uint32_t *__restrict__ idx, uint64_t m,
                                                        const uint64_t *__restrict__ offs,
                                                        const uint32_t *__restrict__ cnt, uint32_t f,
                                                        const uint32_t *__restrict__ ids, uint32_t arr0,
                                                        uint32_t *__restrict__ gids, uint32_t *__restrict__ arr,
                                                        uint32_t *__restrict__ mark) {
    const uint64_t stride = (uint64_t)gridDim.x * PS_BLOCK;
    for (uint64_t p = (uint64_t)blockIdx.x * PS_BLOCK + threadIdx.x; p < m; p += stride) {
        const uint32_t g = key[p], i = idx[p];
        gids[p] = ids[i];
        arr[p] = arr0 + i;
        const uint32_t c = cnt[g] + (uint32_t)(p - offs[g]) + 1u;   // wrapping
        if (c % f == 0) mark[i] = 1u;
    }
}

// dest[p] = the send-order row of the snapshot that grouped position p emits:
// row0 + the marked packets of the epoch in front of its own (pktsnap.h
// ps_rank over the scan's two levels); written at the emitting positions only
__global__ __launch_bounds__(PS_BLOCK) void k_ps_dest(const uint32_t *__restrict__ key,
                                                      const uint32_t *__restrict__ idx, uint64_t m,
                                                      const uint64_t *__restrict__ offs,
                                                      const uint32_t *__restrict__ cnt, uint32_t f,
                                                      const uint32_t *__restrict__ rows,
                                                      const uint32_t *__restrict__ within, uint64_t row0,
                                                      uint32_t *__restrict__ dest) {
    const uint64_t stride = (uint64_t)gridDim.x * PS_BLOCK;
    for (uint64_t p = (uint64_t)blockIdx.x * PS_BLOCK + threadIdx.x; p < m; p += stride) {
        const uint32_t g = key[p];
        const uint32_t c = cnt[g] + (uint32_t)(p - offs[g]) + 1u;   // wrapping, as k_ps_gather
        if (c % f == 0) dest[p] = (uint32_t)(row0 + ps_rank(rows, within, idx[p]));   // < 2^32: at most one row per packet
    }
}

// The table after the batch: the join's union in key order.  A key of the
// batch takes its end-of-batch record (replacing the table's: the walk
// started from it), every other row is copied.  Chunks as k_ft_move's.
__global__ __launch_bounds__(PS_BLOCK) void k_ps_upsert(
    const uint32_t *__restrict__ ra, const uint32_t *__restrict__ fin, const uint32_t *__restrict__ ka,
    const uint32_t *__restrict__ kb, const uint32_t *__restrict__ sa, const uint32_t *__restrict__ sb,
    const uint32_t *__restrict__ tilecnt, const uint64_t *__restrict__ tilebase, uint32_t na, uint32_t nb, uint32_t T,
    uint32_t *__restrict__ rout, uint32_t *__restrict__ kout) {
    const uint32_t tid = threadIdx.x, W = 4 + T;
    const uint32_t k = blockIdx.x / FT_CPT, lo = (blockIdx.x % FT_CPT) * FT_CHUNK;
    const uint32_t cnt = min(tilecnt[k], FT_SLOTS);
    if (lo >= cnt) return;
    const uint32_t m = min(FT_CHUNK, cnt - lo);
    const uint64_t slot0 = (uint64_t)k * FT_SLOTS + lo, out0 = tilebase[k] + lo;
    const uint32_t total = m * W, dr = PS_BLOCK / W, dc = PS_BLOCK % W;
    uint32_t r = tid / W, c = tid % W;
    for (uint32_t v = tid; v < total; v += PS_BLOCK) {
        const uint32_t ia = sa[slot0 + r], ib = sb[slot0 + r];
        if (ib < nb) rout[(out0 + r) * W + c] = fin[(uint64_t)ib * W + c];
        else if (ia < na) rout[(out0 + r) * W + c] = ra[(uint64_t)ia * W + c];
        r += dr;
        c += dc;
        if (c >= W) {
            c -= W;
            ++r;
        }
    }
    for (uint32_t x = tid; x < 3 * m; x += PS_BLOCK) {
        const uint32_t q = x / 3, w = x % 3;
        const uint32_t ia = sa[slot0 + q], ib = sb[slot0 + q];
        if (ib < nb) kout[(out0 + q) * 3 + w] = kb[(uint64_t)ib * 3 + w];
        else if (ia < na) kout[(out0 + q) * 3 + w] = ka[(uint64_t)ia * 3 + w];
    }
}

static uint32_t ps_grid(const qk_ctx *ctx, uint64_t items) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + PS_BLOCK - 1) / PS_BLOCK, (uint64_t)ctx->num_cus * 8));
}

} // namespace qk

using namespace qk;

extern "C" int qk_u32_snapshot_flows_device(qk_ctx *ctx, const uint8_t *d_bufs, size_t n, size_t stride,
                                            const qk_pkt_meta *d_meta, const uint8_t my_addr[6], uint32_t threshold,
                                            uint32_t frequency_pkts, const qk_flow_key *d_keys, const uint8_t *d_sk,
                                            size_t n_table, qk_flow_key *d_keys_out, uint8_t *d_sk_out,
                                            size_t table_cap, size_t *n_table_out, uint8_t *d_snap_out,
                                            qk_flow_key *d_snap_key_out, uint32_t *d_snap_index_out, size_t snap_cap,
                                            size_t *n_snap, qk_pkt_stats *stats, void *stream) {
    if (int e = check_ctx_threshold(ctx, threshold)) return e;
    if (frequency_pkts == 0 || !n_table_out || !n_snap) return QK_E_INVAL;
    if (stride < QK_BUFFER_SIZE || stride > 512) return QK_E_INVAL;
    if (n >= (1ull << 32) || n_table >= (1ull << 31)) return QK_E_INVAL;   // packet indices are u32, table rows the join's
    const uint32_t T = threshold, f = frequency_pkts, nt = (uint32_t)n_table;
    const size_t W = 4 + (size_t)T, rec = W * 4;
    std::lock_guard<std::mutex> lk(ctx->mu);
    QK_HIP_TRY(hipSetDevice(ctx->device));
    if (is_device_ptr(n_table_out) || is_device_ptr(n_snap) || (stats && is_device_ptr(stats)) ||
        (my_addr && is_device_ptr(my_addr)))
        return QK_E_INVAL;
    if ((n && !is_device_ptr(d_bufs)) || (d_meta && !dev_words(d_meta))) return QK_E_INVAL;
    if (nt && (!dev_words(d_keys) || !dev_words(d_sk))) return QK_E_INVAL;
    // a call of these caps writes at most table_cap rows and min(snap_cap, one snapshot per packet) snapshots
    const size_t sw = std::min<uint64_t>(snap_cap, n);
    if (table_cap && (!dev_words(d_keys_out) || !dev_words(d_sk_out))) return QK_E_INVAL;
    if (sw && (!dev_words(d_snap_out) || !dev_words(d_snap_key_out) || !dev_words(d_snap_index_out))) return QK_E_INVAL;
    {
        const void *in[4] = {d_bufs, d_meta, d_keys, d_sk};
        const size_t inb[4] = {n * stride, d_meta ? n * sizeof(qk_pkt_meta) : 0, (size_t)nt * 12, (size_t)nt * rec};
        const void *out[5] = {d_keys_out, d_sk_out, d_snap_out, d_snap_key_out, d_snap_index_out};
        const size_t outb[5] = {table_cap * 12, table_cap * rec, sw * rec, sw * 12, sw * 4};
        for (int a = 0; a < 5; ++a) {
            for (int i = 0; i < 4; ++i)
                if (ranges_overlap(out[a], outb[a], in[i], inb[i])) return QK_E_INVAL;
            for (int b = a + 1; b < 5; ++b)
                if (ranges_overlap(out[a], outb[a], out[b], outb[b])) return QK_E_INVAL;
        }
    }
    hipStream_t s = pick_stream(ctx, stream);
    const uint64_t my_key = flow_my_key(my_addr);
    const uint32_t *tkeys = (const uint32_t *)d_keys, *trec = (const uint32_t *)d_sk;
    qk_pkt_stats st = {0, 0, 0, 0, -1};
    *n_table_out = 0;
    *n_snap = 0;

    // arena 0, per packet: slot / rank key and packet index with their sorted
    // copies (radix.h: a value array behind its key array), the ids, the
    // grouped ids and arrival indices, the marks and their two scan levels
    const uint64_t rows_max = ps_rows(n);
    uint32_t *slots = nullptr, *idx = nullptr, *key_s = nullptr, *idx_s = nullptr, *ids = nullptr, *gids = nullptr;
    uint32_t *arr = nullptr, *dest = nullptr, *mark = nullptr, *within = nullptr, *rtot = nullptr, *rpre = nullptr, *flags = nullptr;
    uint32_t *rlist = nullptr;
    unsigned long long *counters = nullptr;
    RsScratch rs{};
    auto layout0 = [&](Carve &c) {
        slots = c.take<uint32_t>(n); idx = c.take<uint32_t>(n); key_s = c.take<uint32_t>(n); idx_s = c.take<uint32_t>(n);
        ids = c.take<uint32_t>(n); gids = c.take<uint32_t>(n); arr = c.take<uint32_t>(n); dest = c.take<uint32_t>(n);
        mark = c.take<uint32_t>(rows_max * PS_ROW); within = c.take<uint32_t>(rows_max * PS_ROW);
        rtot = c.take<uint32_t>(rows_max); rpre = c.take<uint32_t>(rows_max);
        counters = c.take<unsigned long long>(FLOW_COUNTERS);
        flags = c.take<uint32_t>(2);   // [0] the table's check, [1] the Resets listed
        rs.take(c, rs_plan(ctx, n, RS_WGPC_MAX).nwg, n);
    };
    {
        Carve probe{nullptr};
        layout0(probe);
        if (int e = ensure_flow(ctx, 0, probe.off, s)) return e;
        Carve cv{(char *)ctx->d_flow[0]};
        layout0(cv);
    }
    if (int e = scratch_acquire(ctx, s)) return e;
    int rc = QK_OK;
    auto finish = [&](int code) {
        (void)hipStreamSynchronize(s);   // the arenas are reused by the next call
        if (int e = scratch_release(ctx, s))
            if (!code) code = e;
        if (stats) *stats = st;
        return code;
    };

    // the table's own check, then the extract over the whole batch
    uint32_t hflags[2] = {0, 0};
    if (hipMemsetAsync(flags, 0, 8, s) != hipSuccess) return finish(QK_E_HIP);
    if (nt) {
        hipLaunchKernelGGL(k_ps_check, dim3((nt + PS_BLOCK - 1) / PS_BLOCK), dim3(PS_BLOCK), 0, s, tkeys, trec, nt, T, flags);
        if (hipGetLastError() != hipSuccess) return finish(QK_E_HIP);
    }
    FlowFront ff;
    flow_front_init(ctx, n, ff);
    if (n) rc = flow_extract(ctx, s, d_bufs, n, stride, d_meta, my_key, slots, ids, counters, nullptr, 1, ff);
    if (rc) return finish(rc);
    const uint64_t all_inserts = ff.hc[0], nreset = ff.hc[1];
    st.resets = nreset;
    st.filtered = n - all_inserts - nreset;
    st.last_reset_index = (int64_t)ff.hc[4] - 1;
    std::vector<uint32_t> h_resets(nreset);
    if (nreset) {
        // the list in the context's scratch: read back before the epochs carve it
        if (int e = ensure_scratch(ctx, nreset * 4, s)) return finish(e);
        rlist = (uint32_t *)ctx->d_scratch;
        hipLaunchKernelGGL(k_ps_resets, dim3(ps_grid(ctx, n)), dim3(PS_BLOCK), 0, s, slots, ids, (uint64_t)n, rlist,
                           (uint32_t)nreset, flags + 1);
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(h_resets.data(), rlist, nreset * 4, hipMemcpyDeviceToHost, s) != hipSuccess)
            return finish(QK_E_HIP);
    }
    if (hipMemcpyAsync(hflags, flags, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return finish(QK_E_HIP);
    if (hflags[0] & PS_F_ORDER) return finish(QK_E_INVAL);
    if (hflags[0] & PS_F_MISMATCH) return finish(QK_E_MISMATCH);
    if (hflags[1] != nreset) return finish(QK_E_HIP);   // the extract's count and its markers are kept apart
    std::vector<PsEpoch> epochs(nreset + 1);
    epochs.resize(ps_epochs(h_resets.data(), nreset, n, epochs.data()));

    // One epoch.  write: the outputs are written, after the capacity check at
    // the point where the epoch's counts are known; else it only counts.
    // reuse: the extract over the whole batch is the epoch's own.
    uint64_t tot_snap = 0, n_tab = nreset ? 0 : nt, tail_ins = 0;
    auto run_epoch = [&](const PsEpoch &ep, bool write, bool reuse, uint64_t row0) -> int {
        const uint64_t pn = ep.hi - ep.lo;
        if (!reuse)
            if (int e = flow_extract(ctx, s, d_bufs + ep.lo * stride, pn, stride, d_meta ? d_meta + ep.lo : nullptr,
                                     my_key, slots, ids, counters, nullptr, 1, ff))
                return e;
        const uint64_t ins = ff.hc[0];
        const uint32_t nf = (uint32_t)ff.hc[2];
        if (ff.hc[1]) return QK_E_HIP;   // (an epoch holds no Reset)
        ctx->flow_hint = nf;
        if (ep.tail) tail_ins = ins;
        const bool keyed = !ep.fresh && nt > 0;   // the epoch builds on the caller's table
        if (nf == 0) {
            if (ep.tail) n_tab = keyed ? nt : 0;
            if (ep.tail && write) {
                if (n_tab > table_cap) return QK_E_CAPACITY;
                if (n_tab && (hipMemcpyAsync(d_keys_out, d_keys, (size_t)nt * 12, hipMemcpyDeviceToDevice, s) != hipSuccess ||
                              hipMemcpyAsync(d_sk_out, d_sk, (size_t)nt * rec, hipMemcpyDeviceToDevice, s) != hipSuccess))
                    return QK_E_HIP;
            }
            return QK_OK;
        }
        // per flow, in the context's scratch: the join, the key ordering, the
        // epoch's keys, offsets, base counts and records, end-of-batch records
        const size_t ntiles = keyed ? ((size_t)nt + nf + FT_TILE - 1) / FT_TILE : 0;
        FtBuf fb;
        FlowKeyBuf kb;
        uint8_t *bkeys = nullptr;
        uint64_t *d_offs = nullptr;
        uint32_t *cnt = nullptr, *match = nullptr, *base = nullptr, *fin = nullptr;
        auto layout1 = [&](Carve &c) {
            if (keyed) ft_carve(c, fb, ntiles, nt, false);
            kb.take(c, ctx, ff.C, nf);
            bkeys = c.take<uint8_t>((size_t)nf * 12);
            d_offs = c.take<uint64_t>((size_t)nf + 1);
            cnt = c.take<uint32_t>(nf);
            match = c.take<uint32_t>(nf);
            base = c.take<uint32_t>((size_t)nf * W);
            fin = ep.tail ? c.take<uint32_t>((size_t)nf * W) : nullptr;
        };
        {
            Carve probe{nullptr};
            layout1(probe);
            if (int e = ensure_scratch(ctx, probe.off, s)) return e;
            Carve cv{(char *)ctx->d_scratch};
            layout1(cv);
        }
        // the flows in AddrKey order; the Inserts grouped by flow rank, stably,
        // each with its packet index
        const uint32_t *sorted = nullptr;
        if (int e = flow_key_order(ctx, s, ff, nf, kb, &sorted)) return e;
        if (int e = flow_rank_keys(s, ff, sorted, nf, bkeys)) return e;
        if (int e = flow_slots_to_ranks(ctx, s, slots, ff, pn, nf)) return e;
        hipLaunchKernelGGL(k_ps_iota, dim3(ps_grid(ctx, pn)), dim3(PS_BLOCK), 0, s, idx, pn);
        if (hipGetLastError() != hipSuccess) return QK_E_HIP;
        int where = 0;
        if (int e = rs_sort(ctx, slots, idx, key_s, idx_s, pn, bit_width32(nf), rs, s, where)) return e;
        const uint32_t *gkey = where ? key_s : slots, *gidx = where ? idx_s : idx;
        if (int e = flow_rank_offsets(ctx, s, gkey, ins, nf, d_offs)) return e;
        // one base record per flow, by key
        uint64_t n_union = nf;
        if (keyed) {
            uint64_t res[FT_RES_WORDS] = {0, 0, 0, 0};
            if (int e = ft_join_merge(ctx, s, tkeys, nt, (const uint32_t *)bkeys, nf, fb, ntiles, res)) return e;
            if (res[FT_FLAGS] & FT_F_ORDER) return QK_E_INVAL;
            if (res[FT_TOTAL] != (uint64_t)nt + nf - res[FT_MATCH]) return QK_E_HIP;
            n_union = res[FT_TOTAL];
            hipLaunchKernelGGL(k_ps_match, dim3((uint32_t)((ntiles * FT_SLOTS + PS_BLOCK - 1) / PS_BLOCK)), dim3(PS_BLOCK),
                               0, s, fb.sa, fb.sb, fb.tilecnt, (uint32_t)ntiles, nt, nf, match);
        }
        hipLaunchKernelGGL(k_ps_base, dim3(ps_grid(ctx, (uint64_t)nf * W)), dim3(PS_BLOCK), 0, s, trec,
                           keyed ? match : (const uint32_t *)nullptr, nf, T, base, cnt);
        if (hipGetLastError() != hipSuccess) return QK_E_HIP;
        // the epoch's mid-way wait: offsets and base counts, hence every cut
        std::vector<uint64_t> h_offs((size_t)nf + 1), h_snoff((size_t)nf + 1);
        std::vector<uint32_t> h_cnt(nf);
        if (hipMemcpyAsync(h_offs.data(), d_offs, ((size_t)nf + 1) * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(h_cnt.data(), cnt, (size_t)nf * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return QK_E_HIP;
        if (h_offs[0] != 0 || h_offs[nf] != ins || !sn_check(h_offs.data(), nf)) return QK_E_HIP;
        const uint64_t total = sn_plan_counts(h_offs.data(), h_cnt.data(), nf, f, h_snoff.data());
        tot_snap = row0 + total;
        if (ep.tail) n_tab = n_union;
        if (!write) return QK_OK;
        if (tot_snap > snap_cap || (ep.tail && n_tab > table_cap)) return QK_E_CAPACITY;
        if (!total && !ep.tail) return QK_OK;
        // send order: the marked packets' prefix sums
        const uint64_t rows = ps_rows(pn);
        if (hipMemsetAsync(mark, 0, rows * PS_ROW * 4, s) != hipSuccess) return QK_E_HIP;
        hipLaunchKernelGGL(k_ps_gather, dim3(ps_grid(ctx, ins)), dim3(PS_BLOCK), 0, s, gkey, gidx, ins, d_offs, cnt, f,
                           ids, (uint32_t)ep.lo, gids, arr, mark);
        hipLaunchKernelGGL(rsort::k_row_scan<256>, dim3((uint32_t)rows), dim3(256), 0, s, mark, PS_ROW, within, rtot);
        hipLaunchKernelGGL(rsort::k_tot_scan<1024>, dim3(1), dim3(1024), 0, s, rtot, (uint32_t)rows, rpre);
        hipLaunchKernelGGL(k_ps_dest, dim3(ps_grid(ctx, ins)), dim3(PS_BLOCK), 0, s, gkey, gidx, ins, d_offs, cnt, f, rpre,
                           within, row0, dest);
        if (hipGetLastError() != hipSuccess) return QK_E_HIP;
        // the walk: every snapshot at its send-order row, the tail's end-of-batch records
        if (int e = ensure_flow(ctx, 1, sn_arena_bytes(nf, sn_items(h_offs.data(), nf), T), s)) return e;
        SnOut o{};
        o.snap = (uint32_t *)d_snap_out, o.arr = d_snap_index_out, o.fin = fin;
        o.dest = dest;
        o.keys = (const uint32_t *)bkeys, o.key_out = (uint32_t *)d_snap_key_out;
        if (int e = sn_walk_run(ctx, s, base, gids, arr, h_offs.data(), h_snoff.data(), nf, T, f, o, 0)) return e;
        if (!ep.tail) return QK_OK;
        // the table after the batch
        if (keyed) {
            hipLaunchKernelGGL(k_ps_upsert, dim3((uint32_t)(ntiles * FT_CPT)), dim3(PS_BLOCK), 0, s, trec, fin, tkeys,
                               (const uint32_t *)bkeys, fb.sa, fb.sb, fb.tilecnt, fb.tilebase, nt, nf, T,
                               (uint32_t *)d_sk_out, (uint32_t *)d_keys_out);
            if (hipGetLastError() != hipSuccess) return QK_E_HIP;
        } else if (hipMemcpyAsync(d_keys_out, bkeys, (size_t)nf * 12, hipMemcpyDeviceToDevice, s) != hipSuccess ||
                   hipMemcpyAsync(d_sk_out, fin, (size_t)nf * rec, hipMemcpyDeviceToDevice, s) != hipSuccess) {
            return QK_E_HIP;
        }
        return hipStreamSynchronize(s) == hipSuccess ? QK_OK : QK_E_HIP;   // (the scratch is carved again by the next epoch)
    };
    auto run_all = [&](bool write) -> int {
        tot_snap = 0;
        n_tab = nreset ? 0 : nt;
        tail_ins = 0;
        for (const PsEpoch &ep : epochs)
            if (int e = run_epoch(ep, write, nreset == 0, tot_snap)) return e;
        return QK_OK;
    };
    // A batch with Resets knows its totals only after its last epoch: unless
    // the caps hold whatever the batch brings (one snapshot, one flow per
    // Insert), a counting pass over the epochs decides the capacity before
    // anything is written.
    const bool sure = snap_cap >= all_inserts && table_cap >= all_inserts;
    if (nreset && !sure) {
        rc = run_all(false);
        if (!rc && (tot_snap > snap_cap || n_tab > table_cap)) rc = QK_E_CAPACITY;
    }
    if (!rc) rc = run_all(true);
    if (!rc && epochs.empty() && n_tab) {   // no packets at all: the table is copied
        if (n_tab > table_cap) rc = QK_E_CAPACITY;
        else if (hipMemcpyAsync(d_keys_out, d_keys, (size_t)nt * 12, hipMemcpyDeviceToDevice, s) != hipSuccess ||
                 hipMemcpyAsync(d_sk_out, d_sk, (size_t)nt * rec, hipMemcpyDeviceToDevice, s) != hipSuccess)
            rc = QK_E_HIP;
    }
    if (!rc || rc == QK_E_CAPACITY) {
        *n_snap = (size_t)tot_snap;
        *n_table_out = (size_t)n_tab;
        st.inserted = tail_ins;
        st.discarded = all_inserts - tail_ins;
    }
    return finish(rc);
}
