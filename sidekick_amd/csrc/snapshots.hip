// snapshots.hip — per-flow quACK snapshots: the quACK after every packet that
// brings its flow's count to a multiple of frequency_pkts
// (sidekick_multi.rs:271-283), for a batch grouped by flow
// (qk_u32_snapshot_segments_device).  A segmented prefix
// encode: snapshot r of flow g holds base_g plus the power sums of the flow's
// ids up to its r-th cut.
//
// Per call:
//   k_sn_base       the base counts (one word per flow) and a flag for a record
//                   of another threshold
//   (D2H, wait)     counts and flag into pinned memory: the call's one mid-way
//                   wait.  The host, which has the offsets, then knows every
//                   cut: snap_offsets, the capacity decision and the plan
//                   (snapshots.h) come before any output is written
//   k_sn_walk<KC>   a wave per item of SN_ITEM consecutive positions of the
//                   grouped id array.  Per tile of 64 ids: lane = id writes the
//                   id's powers x^1 .. x^KC into LDS (one modular product
//                   each), then lane = power walks the 64 ids in order, its
//                   column's running sum in a register, and stores it at every
//                   cut — consecutive lanes on consecutive words of the
//                   snapshot's row.  The interval sums and their scan down a
//                   flow's rows are one pass: a row is written once.  Flow
//                   ends, cuts and the wrap of the count are wave-uniform.
//                   A flow that began in an earlier item starts from zero; the
//                   wave leaves its sum in part[item].  A flow that runs on
//                   past the item leaves its full value in carry[item + 1]
//   k_sn_chain      flows over three items or more: carry down their middle
//                   items, one workgroup per flow, a thread per power
//   k_sn_carry      a workgroup per item whose first flow began earlier: adds
//                   carry[item] to that flow's rows in the item, and writes
//                   the flow's final record where it ends there
//   k_sn_empty      final records of the flows without ids: their base rows
// No workgroup waits on another inside a kernel: kernel boundaries order them.
#include <algorithm>

#include "ctx.h"
#include "field.h"
#include "segments.h"
#include "snapshots.h"
#include "snapwalk.h"

namespace qk {

QK_WARM_KERNEL(snapshots)

static_assert(sizeof(qk_u32) == 16, "qk_u32 header is 4 words");

constexpr uint32_t SN_BLOCK = 256;

__global__ __launch_bounds__(SN_BLOCK) void k_sn_base(const uint32_t *__restrict__ base, uint32_t nseg, uint32_t T,
                                                      uint32_t *__restrict__ cnt) {
    const uint32_t g = blockIdx.x * SN_BLOCK + threadIdx.x;
    if (g >= nseg) return;
    const uint32_t *b = base + (size_t)g * (4 + T);
    cnt[g] = b[1];
    if (b[0] != T) cnt[nseg] = 1;   // the host put 0 there
}

// the final record of flow g, which holds ids: header by one lane
__device__ __forceinline__ void sn_final_header(uint32_t *fin, uint32_t T, uint32_t count, uint32_t last) {
    fin[0] = T;
    fin[1] = count;
    fin[2] = 1u;
    fin[3] = last;
}

// DEST: the rows go where o.dest sends them, with key and packet index (the
// packet path); else by flow, with seg, pos and arrival: the by-flow form is
// compiled without any of the other's loads and tests
template <uint32_t KC, bool DEST>
__device__ __forceinline__ void sn_walk_body(const uint32_t *__restrict__ base, const uint32_t *__restrict__ ids,
                                             const uint32_t *__restrict__ arrival, const uint64_t *__restrict__ offs,
                                             const uint64_t *__restrict__ snoff, const uint32_t *__restrict__ g0s,
                                             uint32_t nseg, uint32_t T, uint32_t f, const SnOut &o,
                                             uint32_t *__restrict__ carry, uint32_t *__restrict__ part) {
    constexpr uint32_t LD = KC + 1;   // odd: lane = id writes its row without bank conflicts
    __shared__ uint32_t tile[64 * LD];
    __shared__ uint32_t raw[64];
    __shared__ uint32_t l_dest[DEST ? 64 : 1], l_arr[DEST ? 64 : 1];
    const uint32_t lane = threadIdx.x, item = blockIdx.x;
    const size_t W = 4 + (size_t)T;
    const uint64_t lo = offs[0] + (uint64_t)item * SN_ITEM, end = offs[nseg];
    const uint64_t hi = lo + SN_ITEM < end ? lo + SN_ITEM : end;

    for (uint32_t k0 = 0; k0 < T; k0 += KC) {   // one pass over the item per KC powers
        const uint32_t nk = T - k0 < KC ? T - k0 : KC, col = k0 + lane;
        const bool act = lane < nk, head = k0 == 0 && lane == 0;
        // the flow under the walk (wave-uniform)
        uint32_t g = g0s[item];
        uint64_t fb = offs[g], fe = offs[g + 1];
        bool whole = fb >= lo;   // it begins in this item: its sums start from the base row
        uint32_t c0 = base[g * W + 1];
        uint64_t r = sn_ncuts(c0, f, lo > fb ? lo - fb : 0);
        uint64_t cut = fb + sn_cut_pos(c0, f, r);
        uint32_t run = whole && act ? canon32(base[g * W + 4 + col]) : 0u;

        for (uint64_t tb = lo; tb < hi; tb += 64) {
            const uint32_t nt = hi - tb < 64 ? (uint32_t)(hi - tb) : 64u;
            const uint32_t id = lane < nt ? ids[tb + lane] : 0u;
            const uint32_t x = canon32(id);
            uint32_t pw = k0 ? pow32(x, k0) : 1u;
            __syncthreads();   // the tile before this one has been read
            raw[lane] = id;
            // what a cut needs besides the sums, loaded with the tile (a load at the cut would stall the walk)
            if constexpr (DEST) {
                l_dest[lane] = lane < nt ? o.dest[tb + lane] : 0u;
                if (k0 == 0) l_arr[lane] = lane < nt ? arrival[tb + lane] : 0u;
            }
#pragma unroll 4
            for (uint32_t j = 0; j < nk; ++j) {
                pw = mul32_lazy(pw, x);
                tile[lane * LD + j] = canon32(pw);
            }
            __syncthreads();
            for (uint32_t l = 0; l < nt; ++l) {
                const uint64_t pos = tb + l;
                if (pos == fe) {
                    // the flow ends in front of pos, the next one with ids begins at it
                    if (whole) {
                        if (o.fin) {
                            if (act) o.fin[g * W + 4 + col] = run;
                            if (head) sn_final_header(o.fin + g * W, T, c0 + (uint32_t)(fe - fb), ids[fe - 1]);
                        }
                    } else if (act) {
                        part[(size_t)item * T + col] = run;
                    }
                    uint32_t q = g + 1;
                    for (;;) {
                        const uint32_t idx = q + lane;
                        const uint64_t e = idx < nseg ? offs[idx + 1] : ~0ull;
                        const unsigned long long m = __ballot(e > pos);
                        if (m) {
                            q += (uint32_t)__ffsll((long long)m) - 1u;
                            break;
                        }
                        q += 64;
                    }
                    g = q < nseg ? q : nseg - 1;
                    fb = offs[g], fe = offs[g + 1];
                    whole = true;
                    c0 = base[g * W + 1];
                    r = 0;
                    cut = fb + sn_cut_pos(c0, f, 0);
                    run = act ? canon32(base[g * W + 4 + col]) : 0u;
                }
                if (act) run = add32(run, tile[l * LD + lane]);
                if (pos == cut) {
                    uint64_t row;
                    if constexpr (DEST) row = l_dest[l];
                    else row = snoff[g] + r;
                    if (act) o.snap[row * W + 4 + col] = run;
                    if (head) {
                        uint32_t *h = o.snap + row * W;
                        h[0] = T;
                        h[1] = c0 + (uint32_t)(pos - fb) + 1u;   // wrapping
                        h[2] = 1u;
                        h[3] = raw[l];
                        if constexpr (DEST) {
                            o.arr[row] = l_arr[l];
                        } else {
                            o.seg[row] = g;
                            o.pos[row] = pos;
                            if (o.arr) o.arr[row] = arrival[pos];
                        }
                    }
                    if constexpr (DEST)
                        if (k0 == 0 && lane < 3) o.key_out[row * 3 + lane] = o.keys[(size_t)g * 3 + lane];
                    ++r;
                    cut = fb + sn_cut_pos(c0, f, r);
                }
            }
        }
        // the item's end
        if (fe == hi) {
            if (whole) {
                if (o.fin) {
                    if (act) o.fin[g * W + 4 + col] = run;
                    if (head) sn_final_header(o.fin + g * W, T, c0 + (uint32_t)(fe - fb), ids[fe - 1]);
                }
            } else if (act) {
                part[(size_t)item * T + col] = run;
            }
        } else if (act) {
            if (whole) carry[((size_t)item + 1) * T + col] = run;   // base and every id so far
            else part[(size_t)item * T + col] = run;                // the whole item is the flow's
        }
    }
}

template <uint32_t KC>
__global__ __launch_bounds__(64) void k_sn_walk(const uint32_t *__restrict__ base, const uint32_t *__restrict__ ids,
                                                const uint32_t *__restrict__ arrival,
                                                const uint64_t *__restrict__ offs,
                                                const uint64_t *__restrict__ snoff, const uint32_t *__restrict__ g0s,
                                                uint32_t nseg, uint32_t T, uint32_t f, SnOut o,
                                                uint32_t *__restrict__ carry, uint32_t *__restrict__ part) {
    sn_walk_body<KC, false>(base, ids, arrival, offs, snoff, g0s, nseg, T, f, o, carry, part);
}
template <uint32_t KC>
__global__ __launch_bounds__(64) void k_sn_walk_dest(const uint32_t *__restrict__ base,
                                                     const uint32_t *__restrict__ ids,
                                                     const uint32_t *__restrict__ arrival,
                                                     const uint64_t *__restrict__ offs,
                                                     const uint64_t *__restrict__ snoff,
                                                     const uint32_t *__restrict__ g0s, uint32_t nseg, uint32_t T,
                                                     uint32_t f, SnOut o, uint32_t *__restrict__ carry,
                                                     uint32_t *__restrict__ part) {
    sn_walk_body<KC, true>(base, ids, arrival, offs, snoff, g0s, nseg, T, f, o, carry, part);
}

__global__ __launch_bounds__(SN_BLOCK) void k_sn_chain(const SnChain *__restrict__ chains, uint32_t T,
                                                       uint32_t *__restrict__ carry,
                                                       const uint32_t *__restrict__ part) {
    const SnChain c = chains[blockIdx.x];
    for (uint32_t col = threadIdx.x; col < T; col += SN_BLOCK) {
        uint32_t v = carry[(size_t)c.first * T + col];
        for (uint32_t i = 0; i < c.count; ++i) {
            v = add32(v, part[((size_t)c.first + i) * T + col]);
            carry[((size_t)c.first + i + 1) * T + col] = v;
        }
    }
}

// item = blockIdx.x + 1 (the first item has no flow from before)
__global__ __launch_bounds__(SN_BLOCK) void k_sn_carry(const uint32_t *__restrict__ base,
                                                       const uint32_t *__restrict__ ids,
                                                       const uint32_t *__restrict__ arrival,
                                                       const uint64_t *__restrict__ offs,
                                                       const uint64_t *__restrict__ snoff,
                                                       const uint32_t *__restrict__ g0s, uint32_t nseg, uint32_t T,
                                                       uint32_t f, SnOut o, const uint32_t *__restrict__ carry,
                                                       const uint32_t *__restrict__ part) {
    uint32_t *__restrict__ snap = o.snap, *__restrict__ fin = o.fin;
    const uint32_t item = blockIdx.x + 1;
    const size_t W = 4 + (size_t)T;
    const uint64_t lo = offs[0] + (uint64_t)item * SN_ITEM, end = offs[nseg];
    const uint64_t hi = lo + SN_ITEM < end ? lo + SN_ITEM : end;
    const uint32_t g = g0s[item];
    const uint64_t fb = offs[g], fe = offs[g + 1];
    if (fb >= lo) return;
    const uint64_t e = fe < hi ? fe : hi;
    const uint32_t c0 = base[g * W + 1];
    const uint64_t r0 = sn_ncuts(c0, f, lo - fb);   // the flow's cuts in front of the item
    // (the cut's position only where dest needs it: by flow the row is plain arithmetic, as it was)
    auto at = [&](uint32_t row) -> uint64_t {
        return o.dest ? (uint64_t)o.dest[fb + sn_cut_pos(c0, f, r0 + row)] : snoff[g] + r0 + row;
    };
    const uint32_t nrows = (uint32_t)(sn_ncuts(c0, f, e - fb) - sn_ncuts(c0, f, lo - fb));   // <= SN_ITEM
    const uint32_t *cin = carry + (size_t)item * T;
    if (T <= SN_BLOCK) {
        // a thread keeps its column: rows SN_BLOCK / T apart
        const uint32_t per = SN_BLOCK / T, col = threadIdx.x % T, sub = threadIdx.x / T;
        if (sub < per) {
            const uint32_t c = cin[col];
            for (uint32_t row = sub; row < nrows; row += per) {
                uint32_t *p = snap + at(row) * W + 4 + col;
                *p = add32(*p, c);
            }
        }
    } else {
        for (uint32_t col = threadIdx.x; col < T; col += SN_BLOCK) {
            const uint32_t c = cin[col];
            for (uint32_t row = 0; row < nrows; ++row) {
                uint32_t *p = snap + at(row) * W + 4 + col;
                *p = add32(*p, c);
            }
        }
    }
    if (fin && fe <= hi) {
        for (uint32_t col = threadIdx.x; col < T; col += SN_BLOCK)
            fin[g * W + 4 + col] = add32(cin[col], part[(size_t)item * T + col]);
        if (threadIdx.x == 0) sn_final_header(fin + g * W, T, c0 + (uint32_t)(fe - fb), ids[fe - 1]);
    }
}

__global__ __launch_bounds__(SN_BLOCK) void k_sn_empty(const uint32_t *__restrict__ base,
                                                       const uint64_t *__restrict__ offs, uint64_t words, uint32_t W,
                                                       uint32_t *__restrict__ fin) {
    const uint64_t stride = (uint64_t)gridDim.x * SN_BLOCK;
    for (uint64_t i = (uint64_t)blockIdx.x * SN_BLOCK + threadIdx.x; i < words; i += stride) {
        const uint64_t g = i / W;
        if (offs[g] == offs[g + 1]) fin[i] = base[i];
    }
}

} // namespace qk

using namespace qk;

extern "C" int qk_u32_snapshot_segments_device(qk_ctx *ctx, const uint8_t *d_base, const uint32_t *d_ids,
                                               const uint32_t *d_arrival, const uint64_t *offsets, size_t nseg,
                                               uint32_t threshold, uint32_t frequency_pkts, uint8_t *d_snap_out,
                                               uint32_t *d_snap_seg_out, uint64_t *d_snap_pos_out,
                                               uint32_t *d_snap_arrival_out, size_t cap, uint64_t *snap_offsets,
                                               size_t *n_snap, uint8_t *d_final_out, void *stream) {
    if (int e = check_ctx_threshold(ctx, threshold)) return e;
    if (frequency_pkts == 0 || !snap_offsets || !n_snap) return QK_E_INVAL;
    if (nseg == 0) {
        snap_offsets[0] = 0;
        *n_snap = 0;
        return QK_OK;
    }
    if (!offsets || nseg > 0xFFFFFFFFull || (d_arrival == nullptr) != (d_snap_arrival_out == nullptr))
        return QK_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    QK_HIP_TRY(hipSetDevice(ctx->device));
    // (before the offsets are read: a device pointer is not the host's to follow)
    if (is_device_ptr(offsets) || is_device_ptr(snap_offsets) || is_device_ptr(n_snap)) return QK_E_INVAL;
    if (!sn_check(offsets, nseg)) return QK_E_INVAL;
    const uint32_t T = threshold, f = frequency_pkts;
    const size_t W = 4 + (size_t)T, rec = W * 4;
    const uint64_t n = offsets[nseg] - offsets[0];
    const size_t ni = sn_items(offsets, nseg);
    if (!dev_words(d_base) || (n && !dev_words(d_ids)) || (d_arrival && !dev_words(d_arrival))) return QK_E_INVAL;
    if ((d_snap_out && !dev_words(d_snap_out)) || (d_snap_seg_out && !dev_words(d_snap_seg_out)) ||
        (d_snap_pos_out && !dev_words(d_snap_pos_out)) || (d_snap_arrival_out && !dev_words(d_snap_arrival_out)) ||
        (d_final_out && !dev_words(d_final_out)))
        return QK_E_INVAL;
    // a call of this cap writes at most min(cap, one snapshot per id) rows
    const uint64_t wr = std::min<uint64_t>(cap, n);
    if (wr && (!d_snap_out || !d_snap_seg_out || !d_snap_pos_out)) return QK_E_INVAL;
    const void *in[3] = {d_base, n ? d_ids + offsets[0] : nullptr, d_arrival && n ? d_arrival + offsets[0] : nullptr};
    const size_t inb[3] = {nseg * rec, (size_t)n * 4, (size_t)n * 4};
    const void *out[5] = {d_snap_out, d_snap_seg_out, d_snap_pos_out, d_snap_arrival_out, d_final_out};
    const size_t outb[5] = {(size_t)wr * rec, (size_t)wr * 4, (size_t)wr * 8, (size_t)wr * 4, nseg * rec};
    for (int a = 0; a < 5; ++a) {
        for (int i = 0; i < 3; ++i)
            if (ranges_overlap(out[a], outb[a], in[i], inb[i])) return QK_E_INVAL;
        for (int b = a + 1; b < 5; ++b)
            if (ranges_overlap(out[a], outb[a], out[b], outb[b])) return QK_E_INVAL;
    }
    hipStream_t s = pick_stream(ctx, stream);

    // pinned: the counts and the flag, then (sn_walk_run) the items' first
    // flows and the chains — their number bounded by the offsets alone, so the
    // buffer never moves under the copy
    const size_t cnt_bytes = (((nseg + 1) * sizeof(uint32_t)) + 15) & ~(size_t)15;
    if (int e = ensure_items(ctx, cnt_bytes + sn_pinned_bytes(nseg, ni))) return e;
    uint32_t *h_cnt = (uint32_t *)ctx->h_items;

    uint32_t *d_cnt = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        Carve cv{pass ? (char *)ctx->d_flow[1] : nullptr};
        d_cnt = cv.take<uint32_t>(nseg + 1);
        if (!pass)
            if (int e = ensure_flow(ctx, 1, cv.off + sn_arena_bytes(nseg, ni, T), s)) return e;
    }
    const uint32_t *base = (const uint32_t *)d_base;
    const uint32_t seg_blocks = (uint32_t)((nseg + SN_BLOCK - 1) / SN_BLOCK);

    int rc = QK_OK;
    if (hipMemsetAsync(d_cnt + nseg, 0, sizeof(uint32_t), s) != hipSuccess) rc = QK_E_HIP;
    if (!rc) {
        hipLaunchKernelGGL(k_sn_base, dim3(seg_blocks), dim3(SN_BLOCK), 0, s, base, (uint32_t)nseg, T, d_cnt);
        if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
    }
    // the call's one mid-way wait: the thresholds and the capacity are decided here
    if (!rc && (hipMemcpyAsync(h_cnt, d_cnt, (nseg + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess))
        rc = QK_E_HIP;
    if (rc) return rc;
    if (h_cnt[nseg]) return QK_E_MISMATCH;
    const uint64_t total = sn_plan_counts(offsets, h_cnt, nseg, f, snap_offsets);
    *n_snap = (size_t)total;
    if (total > cap) return QK_E_CAPACITY;
    if (!n && !d_final_out) return QK_OK;

    SnOut o{};
    o.snap = (uint32_t *)d_snap_out, o.seg = d_snap_seg_out, o.pos = d_snap_pos_out, o.arr = d_snap_arrival_out;
    o.fin = (uint32_t *)d_final_out;
    return sn_walk_run(ctx, s, base, d_ids, d_arrival, offsets, snap_offsets, nseg, T, f, o, cnt_bytes);
}

// bytes of pinned memory and of arena 1 that sn_walk_run takes
size_t qk::sn_pinned_bytes(size_t nseg, size_t ni) {
    return ((ni * sizeof(uint32_t) + 15) & ~(size_t)15) + std::min(nseg, ni) * sizeof(SnChain) + 16;
}
size_t qk::sn_arena_bytes(size_t nseg, size_t ni, uint32_t T) {
    Carve cv{nullptr};
    cv.take<uint64_t>(nseg + 1);
    cv.take<uint64_t>(nseg + 1);
    cv.take<uint32_t>((ni + 1) * T);
    cv.take<uint32_t>(ni * T);
    return cv.off + 256;
}

int qk::sn_walk_run(qk_ctx *ctx, hipStream_t s, const uint32_t *base, const uint32_t *d_ids, const uint32_t *d_arrival,
                    const uint64_t *offsets, const uint64_t *snap_offsets, size_t nseg, uint32_t T, uint32_t f,
                    const SnOut &o, size_t pinned_off) {
    const size_t W = 4 + (size_t)T;
    const size_t ni = sn_items(offsets, nseg);
    const size_t g0_bytes = ((ni * sizeof(uint32_t)) + 15) & ~(size_t)15;
    if (int e = ensure_items(ctx, pinned_off + sn_pinned_bytes(nseg, ni))) return e;
    uint32_t *h_g0 = (uint32_t *)((char *)ctx->h_items + pinned_off);
    SnChain *h_chain = (SnChain *)((char *)ctx->h_items + pinned_off + g0_bytes);
    const uint32_t *d_g0 = (const uint32_t *)((const char *)ctx->h_items_dev + pinned_off);
    const SnChain *d_chain = (const SnChain *)((const char *)ctx->h_items_dev + pinned_off + g0_bytes);
    // arena 1, from its end: the caller's own use of it comes first
    if (ctx->flow_bytes[1] < sn_arena_bytes(nseg, ni, T)) return QK_E_HIP;
    uint32_t *d_carry = nullptr, *d_part = nullptr;
    uint64_t *d_offs = nullptr, *d_snoff = nullptr;
    {
        // rounded up: never below the caller's own bytes (sn_arena_bytes holds 256 bytes of slack for it)
        const size_t at = (ctx->flow_bytes[1] - sn_arena_bytes(nseg, ni, T) + 255) & ~(size_t)255;
        Carve cv{(char *)ctx->d_flow[1] + at};
        d_offs = cv.take<uint64_t>(nseg + 1);
        d_snoff = cv.take<uint64_t>(nseg + 1);
        d_carry = cv.take<uint32_t>((ni + 1) * T);
        d_part = cv.take<uint32_t>(ni * T);
    }
    if (o.dest && (!d_arrival || !o.arr || !o.keys || !o.key_out)) return QK_E_INVAL;   // the packet form writes all of them
    int rc = QK_OK;
    const size_t nc = ni ? sn_plan_items(offsets, nseg, h_g0, h_chain) : 0;
    if (hipMemcpyAsync(d_offs, offsets, (nseg + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d_snoff, snap_offsets, (nseg + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess)
        rc = QK_E_HIP;
    uint32_t *fin = o.fin;
    if (!rc && ni) {
        if (o.dest && T <= SN_KC_SMALL)
            hipLaunchKernelGGL(k_sn_walk_dest<SN_KC_SMALL>, dim3((uint32_t)ni), dim3(64), 0, s, base, d_ids, d_arrival,
                               d_offs, d_snoff, d_g0, (uint32_t)nseg, T, f, o, d_carry, d_part);
        else if (o.dest)
            hipLaunchKernelGGL(k_sn_walk_dest<SN_KC>, dim3((uint32_t)ni), dim3(64), 0, s, base, d_ids, d_arrival, d_offs,
                               d_snoff, d_g0, (uint32_t)nseg, T, f, o, d_carry, d_part);
        else if (T <= SN_KC_SMALL)
            hipLaunchKernelGGL((k_sn_walk<SN_KC_SMALL>), dim3((uint32_t)ni), dim3(64), 0, s, base, d_ids, d_arrival,
                               d_offs, d_snoff, d_g0, (uint32_t)nseg, T, f, o, d_carry, d_part);
        else
            hipLaunchKernelGGL((k_sn_walk<SN_KC>), dim3((uint32_t)ni), dim3(64), 0, s, base, d_ids, d_arrival, d_offs,
                               d_snoff, d_g0, (uint32_t)nseg, T, f, o, d_carry, d_part);
        if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
    }
    if (!rc && nc) {
        hipLaunchKernelGGL(k_sn_chain, dim3((uint32_t)nc), dim3(SN_BLOCK), 0, s, d_chain, T, d_carry, d_part);
        if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
    }
    if (!rc && ni > 1) {
        hipLaunchKernelGGL(k_sn_carry, dim3((uint32_t)(ni - 1)), dim3(SN_BLOCK), 0, s, base, d_ids, d_arrival, d_offs,
                           d_snoff, d_g0, (uint32_t)nseg, T, f, o, d_carry, d_part);
        if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
    }
    if (!rc && fin) {
        const uint64_t words = (uint64_t)nseg * W;
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((words + SN_BLOCK - 1) / SN_BLOCK, 1u << 16);
        hipLaunchKernelGGL(k_sn_empty, dim3(blocks), dim3(SN_BLOCK), 0, s, base, d_offs, words, (uint32_t)W, fin);
        if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
    }
    // the pinned plan, the arena and the caller's offsets must outlive what was enqueued
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = QK_E_HIP;
    return rc;
}
