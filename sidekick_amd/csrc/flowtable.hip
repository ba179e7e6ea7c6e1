// flowtable.hip — the device-resident flow table: SidekickMulti's
// `senders: HashMap<AddrKey, PowerSumQuackU32>` (sidekick_multi.rs:36,65-90)
// kept in HBM as a flow array (keys strictly ascending in memcmp order, one
// qk_u32 record per key: what qk_u32_encode_flows_device writes), and the
// three operations on it:
//   merge    table ∪ batch, qk_u32_merge per shared key (sidekick_multi.rs:65-90)
//   diff     mine - peer's per shared key (media_client.rs:295-296), in a's order
//   lookup   SidekickMulti::quack(&addr_key) (sidekick_multi.rs:92-94) for nk keys
//
// The join is a merge path over the two key arrays; kernel boundaries are its
// only inter-workgroup ordering (no look-back, no flag another workgroup
// spins on):
//   k_ft_join<DIFF>   one workgroup per QK_FLOW_JOIN_TILE keys of a and b
//                     together: the tile's two diagonals are searched on the
//                     global keys, its keys staged in LDS (byte-swapped words,
//                     so word order is memcmp order), strict ascent checked,
//                     then every thread merges FT_IPT positions: per output
//                     element its source index in a and in b.  Merge: into the
//                     tile's own FT_SLOTS slots, with the tile's output count.
//                     Diff: the b index (or none) at the a index.
//   k_ft_scan         exclusive scan of the tile counts, the total to res[0]
//   k_ft_move<..>     one workgroup per chunk of FT_CHUNK slots, its threads
//                     striding over the chunk's output *words* (or 16-byte
//                     vectors), so reads and writes stay coalesced whatever the
//                     record length; keys and `due` in the same pass (merge)
//   k_ft_lookup       a wave per queried key: binary search, then its lanes
//                     copy the record into staging
// A cut never falls between an a key and its equal b key: merged order puts a
// before b on a tie, so only the cut right after that a key can split the
// pair, and it is moved one b key on (ft_cut_*).  A tile therefore holds at
// most QK_FLOW_JOIN_TILE + 1 keys.
#include <string.h>

#include <algorithm>

#include "ctx.h"
#include "field.h"
#include "flowjoin.h"
#include "segments.h"

namespace qk {

QK_WARM_KERNEL(flowtable)

static_assert(sizeof(qk_u32) == 16 && sizeof(qk_flow_key) == 12, "record header 4 words, key 3 words");

constexpr int FT_BLOCK = 256;
// (FT_TILE, FT_SLOTS, FT_CPT, FT_CHUNK, FT_NONE, the res[] words: flowjoin.h)
constexpr uint32_t FT_IPT = (FT_SLOTS + FT_BLOCK - 1) / FT_BLOCK;     // merged positions per thread
static_assert(FT_SLOTS * 12 <= 24 * 1024 + 12, "the staged keys take 24 KB of LDS");

// a key as three big-endian words: comparing them most significant first is
// memcmp on the 12 bytes
struct FtKey {
    uint32_t w0, w1, w2;
};
__device__ __forceinline__ FtKey ft_load(const uint32_t *__restrict__ k, uint64_t i) {
    const uint32_t *p = k + 3 * i;
    return {__builtin_bswap32(p[0]), __builtin_bswap32(p[1]), __builtin_bswap32(p[2])};
}
__device__ __forceinline__ int ft_cmp(const FtKey &x, const FtKey &y) {
    if (x.w0 != y.w0) return x.w0 < y.w0 ? -1 : 1;
    if (x.w1 != y.w1) return x.w1 < y.w1 ? -1 : 1;
    if (x.w2 != y.w2) return x.w2 < y.w2 ? -1 : 1;
    return 0;
}

// The cut of diagonal d (d <= na + nb): i keys of a and j = d - i of b come
// first in merged order (a before b on a tie).  Every index read lies in
// [0, na) / [0, nb) whatever the keys hold, sorted or not.
__device__ void ft_cut_global(const uint32_t *__restrict__ ka, uint32_t na, const uint32_t *__restrict__ kb,
                              uint32_t nb, uint64_t d, uint32_t &ci, uint32_t &cj) {
    uint32_t lo = d > nb ? (uint32_t)(d - nb) : 0u, hi = d < na ? (uint32_t)d : na;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ft_cmp(ft_load(ka, mid), ft_load(kb, d - 1 - mid)) <= 0) lo = mid + 1;
        else hi = mid;
    }
    uint32_t i = lo, j = (uint32_t)(d - lo);
    if (i > 0 && j < nb && ft_cmp(ft_load(ka, i - 1), ft_load(kb, j)) == 0) ++j;   // keep the pair together
    ci = i;
    cj = j;
}

// the staged keys: word c of key e at s[c * FT_LD + e]; a's ca keys first
constexpr uint32_t FT_LD = FT_SLOTS + 3;
__device__ __forceinline__ FtKey ft_lds(const uint32_t *s, uint32_t e) {
    return {s[e], s[FT_LD + e], s[2 * FT_LD + e]};
}
__device__ void ft_cut_lds(const uint32_t *s, uint32_t ca, uint32_t cb, uint32_t d, uint32_t &ci, uint32_t &cj) {
    uint32_t lo = d > cb ? d - cb : 0u, hi = d < ca ? d : ca;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (ft_cmp(ft_lds(s, mid), ft_lds(s, ca + d - 1 - mid)) <= 0) lo = mid + 1;
        else hi = mid;
    }
    uint32_t i = lo, j = d - lo;
    if (i > 0 && j < cb && ft_cmp(ft_lds(s, i - 1), ft_lds(s, ca + j)) == 0) ++j;
    ci = i;
    cj = j;
}

// One thread's stretch of the tile's merge, [i, ie) of a and [j, je) of b:
// returns its output elements (a pair is one) and adds its pairs to `matches`.
// EMIT: merge writes (a index, b index) into slot base + rank (ranks past the
// tile's slots are dropped: only unsorted input gets there); diff writes the
// b index at the a index.
template <bool EMIT, bool DIFF>
__device__ __forceinline__ uint32_t ft_walk(const uint32_t *s, uint32_t ca, uint32_t i, uint32_t ie, uint32_t j,
                                            uint32_t je, uint32_t i0, uint32_t j0, uint32_t *__restrict__ sa,
                                            uint32_t *__restrict__ sb, uint64_t slot0, uint32_t rank,
                                            uint32_t &matches) {
    uint32_t cnt = 0;
    while (i < ie || j < je) {
        int c;
        if (i < ie && j < je) c = ft_cmp(ft_lds(s, i), ft_lds(s, ca + j));
        else c = i < ie ? -1 : 1;
        const uint32_t ia = c <= 0 ? i0 + i : FT_NONE, ib = c >= 0 ? j0 + j : FT_NONE;
        if (EMIT) {
            if (DIFF) {
                if (c <= 0) sb[ia] = ib;
            } else if (rank + cnt < FT_SLOTS) {
                sa[slot0 + rank + cnt] = ia;
                sb[slot0 + rank + cnt] = ib;
            }
        }
        matches += c == 0;
        i += c <= 0;
        j += c >= 0;
        ++cnt;
    }
    return cnt;
}

template <bool DIFF>
__global__ __launch_bounds__(FT_BLOCK) void k_ft_join(const uint32_t *__restrict__ ka, uint32_t na,
                                                      const uint32_t *__restrict__ kb, uint32_t nb,
                                                      uint32_t *__restrict__ sa, uint32_t *__restrict__ sb,
                                                      uint32_t *__restrict__ tilecnt, unsigned long long *res) {
    __shared__ uint32_t s_k[3 * FT_LD];
    __shared__ uint32_t s_cut[4];
    __shared__ uint32_t s_ci[FT_BLOCK + 1], s_cj[FT_BLOCK + 1];
    __shared__ uint32_t s_scan[FT_BLOCK];
    __shared__ uint32_t s_match;
    const uint32_t tid = threadIdx.x, tile = blockIdx.x;
    const uint64_t N = (uint64_t)na + nb;
    if (tid < 2) {
        const uint64_t d = std::min<uint64_t>(((uint64_t)tile + tid) * FT_TILE, N);
        ft_cut_global(ka, na, kb, nb, d, s_cut[2 * tid], s_cut[2 * tid + 1]);
    }
    if (tid == 0) s_match = 0;
    __syncthreads();
    const uint32_t i0 = s_cut[0], j0 = s_cut[1], i1 = s_cut[2], j1 = s_cut[3];
    // sorted input gives i0 <= i1, j0 <= j1 and at most FT_SLOTS keys; anything
    // else is input out of order, and the tile writes nothing
    if (i1 < i0 || j1 < j0 || (uint64_t)(i1 - i0) + (j1 - j0) > FT_SLOTS) {
        if (tid == 0) {
            atomicOr(&res[FT_FLAGS], FT_F_ORDER);
            if (!DIFF) tilecnt[tile] = 0;
        }
        return;
    }
    const uint32_t ca = i1 - i0, cb = j1 - j0, n = ca + cb;
    for (uint32_t x = tid; x < 3 * ca; x += FT_BLOCK)
        s_k[(x % 3) * FT_LD + x / 3] = __builtin_bswap32(ka[3 * (uint64_t)i0 + x]);
    for (uint32_t x = tid; x < 3 * cb; x += FT_BLOCK)
        s_k[(x % 3) * FT_LD + ca + x / 3] = __builtin_bswap32(kb[3 * (uint64_t)j0 + x]);
    __syncthreads();
    // strict ascent of both inputs, the pair across the tile's start included
    bool bad = false;
    for (uint32_t e = tid; e < n; e += FT_BLOCK) {
        const bool isa = e < ca;
        const uint32_t first = isa ? 0u : ca, g0 = isa ? i0 : j0;
        if (e == first && g0 == 0) continue;
        const FtKey prev = e > first ? ft_lds(s_k, e - 1) : ft_load(isa ? ka : kb, g0 - 1);
        bad |= ft_cmp(prev, ft_lds(s_k, e)) >= 0;
    }
    if (bad) atomicOr(&res[FT_FLAGS], FT_F_ORDER);
    // every thread's own cut of the tile
    ft_cut_lds(s_k, ca, cb, std::min(tid * FT_IPT, n), s_ci[tid], s_cj[tid]);
    if (tid == 0) {
        s_ci[FT_BLOCK] = ca;
        s_cj[FT_BLOCK] = cb;
    }
    __syncthreads();
    const uint32_t i = s_ci[tid], j = s_cj[tid];
    // (unsorted input can put a later cut before an earlier one: that side of
    // the stretch is then empty)
    const uint32_t ie = std::max(i, s_ci[tid + 1]), je = std::max(j, s_cj[tid + 1]);
    uint32_t matches = 0, unused = 0;
    if (DIFF) {
        ft_walk<true, true>(s_k, ca, i, ie, j, je, i0, j0, sa, sb, 0, 0, matches);
    } else {
        const uint32_t cnt = ft_walk<false, false>(s_k, ca, i, ie, j, je, i0, j0, sa, sb, 0, 0, matches);
        s_scan[tid] = cnt;
        __syncthreads();
        for (int off = 1; off < FT_BLOCK; off <<= 1) {   // inclusive scan of the thread counts
            const uint32_t v = tid >= (uint32_t)off ? s_scan[tid - off] : 0u;
            __syncthreads();
            s_scan[tid] += v;
            __syncthreads();
        }
        ft_walk<true, false>(s_k, ca, i, ie, j, je, i0, j0, sa, sb, (uint64_t)tile * FT_SLOTS, s_scan[tid] - cnt,
                             unused);
        if (tid == FT_BLOCK - 1) tilecnt[tile] = std::min(s_scan[tid], FT_SLOTS);
    }
    if (matches) atomicAdd(&s_match, matches);
    __syncthreads();
    if (tid == 0 && s_match) atomicAdd(&res[FT_MATCH], (unsigned long long)s_match);
}

// exclusive scan of the tile counts by one workgroup (each thread a contiguous
// run); res[FT_TOTAL] = the union's size
constexpr int FT_SCAN = 1024;
__global__ __launch_bounds__(FT_SCAN) void k_ft_scan(const uint32_t *__restrict__ tilecnt, uint32_t ntiles,
                                                     uint64_t *__restrict__ tilebase, unsigned long long *res) {
    __shared__ uint64_t part[FT_SCAN];
    const uint32_t per = (ntiles + FT_SCAN - 1) / FT_SCAN;
    const uint64_t b = std::min<uint64_t>((uint64_t)threadIdx.x * per, ntiles), e = std::min<uint64_t>(b + per, ntiles);
    uint64_t s = 0;
    for (uint64_t k = b; k < e; ++k) s += tilecnt[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < FT_SCAN; off <<= 1) {
        const uint64_t v = threadIdx.x >= (uint32_t)off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t run = part[threadIdx.x] - s;
    for (uint64_t k = b; k < e; ++k) {
        tilebase[k] = run;
        run += tilecnt[k];
    }
    if (threadIdx.x == FT_SCAN - 1) res[FT_TOTAL] = part[FT_SCAN - 1];
}

// --------------------------------------------------------------- move/combine
// header of qk_u32_merge(a, b) (host.cpp): counts add (wrapping), last from b
// when b has one; of qk_u32_sub_assign: counts subtract, last stays a's
template <bool DIFF> __device__ __forceinline__ uint4 ft_header(const uint4 &a, const uint4 &b) {
    uint4 r = a;
    if (DIFF) {
        r.y = a.y - b.y;
    } else {
        r.y = a.y + b.y;
        if (b.z) {
            r.z = 1;
            r.w = b.w;
        }
    }
    return r;
}
template <bool DIFF> __device__ __forceinline__ uint32_t ft_sum(uint32_t a, uint32_t b) {
    return DIFF ? sub32(a, b) : add32(a, b);
}

// One workgroup per chunk of FT_CHUNK slots.  Merge: chunk c is quarter c %
// FT_CPT of tile c / FT_CPT, output record = the tile's base + the slot's rank.
// Diff: slot = output record = a index.  VEC: the unit is a 16-byte vector
// (unit 0 of a record is its header), else a dword (units 0..3).
// A source index that is not below its array's size counts as none: after
// unsorted input (the call fails) index slots may hold anything.
template <bool DIFF, bool VEC>
__global__ __launch_bounds__(FT_BLOCK) void k_ft_move(
    const uint32_t *__restrict__ ra, const uint32_t *__restrict__ rb, uint32_t *__restrict__ rout,
    const uint32_t *__restrict__ ka, const uint32_t *__restrict__ kb, uint32_t *__restrict__ kout,
    uint8_t *__restrict__ due, const uint32_t *__restrict__ sa, const uint32_t *__restrict__ sb,
    const uint32_t *__restrict__ tilecnt, const uint64_t *__restrict__ tilebase, uint32_t na, uint32_t nb, uint32_t T,
    uint32_t freq, unsigned long long *res) {
    const uint32_t tid = threadIdx.x, W = 4 + T;
    uint64_t slot0, out0;
    uint32_t m;
    if (DIFF) {
        slot0 = out0 = (uint64_t)blockIdx.x * FT_CHUNK;
        if (slot0 >= na) return;
        m = (uint32_t)std::min<uint64_t>(FT_CHUNK, na - slot0);
    } else {
        const uint32_t k = blockIdx.x / FT_CPT, lo = (blockIdx.x % FT_CPT) * FT_CHUNK;
        const uint32_t cnt = std::min(tilecnt[k], FT_SLOTS);
        if (lo >= cnt) return;
        m = std::min(FT_CHUNK, cnt - lo);
        slot0 = (uint64_t)k * FT_SLOTS + lo;
        out0 = tilebase[k] + lo;
    }
    const uint32_t U = VEC ? W / 4 : W, total = m * U;
    const uint32_t dr = FT_BLOCK / U, dc = FT_BLOCK % U;
    uint32_t rec = tid / U, col = tid % U;
    bool mismatch = false;
    for (uint32_t v = tid; v < total; v += FT_BLOCK) {
        uint32_t ia = DIFF ? (uint32_t)(slot0 + rec) : sa[slot0 + rec], ib = sb[slot0 + rec];
        if (ia >= na) ia = FT_NONE;
        if (ib >= nb) ib = FT_NONE;
        const uint64_t o = (out0 + rec) * W, pa = (uint64_t)ia * W, pb = (uint64_t)ib * W;
        if (ia != FT_NONE || ib != FT_NONE) {
            if (VEC) {
                const uint4 *va = (const uint4 *)(ra + pa) + col, *vb = (const uint4 *)(rb + pb) + col;
                uint4 r;
                if (ia != FT_NONE && ib != FT_NONE) {
                    const uint4 a = *va, b = *vb;
                    if (col == 0) {
                        mismatch |= a.x != T || b.x != T;
                        r = ft_header<DIFF>(a, b);
                    } else {
                        r = {ft_sum<DIFF>(a.x, b.x), ft_sum<DIFF>(a.y, b.y), ft_sum<DIFF>(a.z, b.z),
                             ft_sum<DIFF>(a.w, b.w)};
                    }
                } else {
                    r = ia != FT_NONE ? *va : *vb;
                    if (col == 0) mismatch |= r.x != T;
                }
                *((uint4 *)(rout + o) + col) = r;
            } else {
                uint32_t r;
                if (ia != FT_NONE && ib != FT_NONE) {
                    const uint32_t a = ra[pa + col], b = rb[pb + col];
                    if (col >= 4) {
                        r = ft_sum<DIFF>(a, b);
                    } else if (col == 0) {
                        mismatch |= a != T || b != T;
                        r = a;
                    } else if (col == 1) {
                        r = DIFF ? a - b : a + b;
                    } else {   // has_last, last_value: b's when a merge's b has one
                        const bool fromb = !DIFF && rb[pb + 2] != 0;
                        r = fromb ? (col == 2 ? 1u : b) : a;
                    }
                } else {
                    r = ia != FT_NONE ? ra[pa + col] : rb[pb + col];
                    if (col == 0) mismatch |= r != T;
                }
                rout[o + col] = r;
            }
        }
        rec += dr;
        col += dc;
        if (col >= U) {
            col -= U;
            ++rec;
        }
    }
    if (mismatch) atomicOr(&res[FT_FLAGS], FT_F_MISMATCH);
    if (DIFF) return;
    // the union's keys, and the flows whose count crossed a multiple of freq
    for (uint32_t x = tid; x < 3 * m; x += FT_BLOCK) {
        const uint32_t r = x / 3, c = x % 3;
        const uint32_t ia = sa[slot0 + r], ib = sb[slot0 + r];
        if (ia < na) kout[(out0 + r) * 3 + c] = ka[(uint64_t)ia * 3 + c];
        else if (ib < nb) kout[(out0 + r) * 3 + c] = kb[(uint64_t)ib * 3 + c];
    }
    if (due)
        for (uint32_t r = tid; r < m; r += FT_BLOCK) {
            const uint32_t ia = sa[slot0 + r], ib = sb[slot0 + r];
            uint8_t d = 0;
            if (freq && ib < nb) {
                const uint64_t before = ia < na ? ra[(uint64_t)ia * W + 1] : 0u;
                const uint64_t after = before + rb[(uint64_t)ib * W + 1];
                d = after / freq > before / freq;
            }
            due[out0 + r] = d;
        }
}

// ------------------------------------------------------------------- lookup
// a wave per queried key: the lower bound of the key in the table, every lane
// the same search; then the lanes copy the record (or write qk_u32_init's)
__global__ __launch_bounds__(FT_BLOCK) void k_ft_lookup(const uint32_t *__restrict__ keys, uint32_t n,
                                                        const uint32_t *__restrict__ rec, uint32_t T,
                                                        const uint32_t *__restrict__ q, uint32_t nk,
                                                        uint32_t *__restrict__ out, uint8_t *__restrict__ found,
                                                        unsigned long long *res) {
    const uint64_t w = ((uint64_t)blockIdx.x * FT_BLOCK + threadIdx.x) / 64;
    const uint32_t lane = threadIdx.x & 63, W = 4 + T;
    if (w >= nk) return;
    const FtKey k = ft_load(q, w);
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ft_cmp(ft_load(keys, mid), k) < 0) lo = mid + 1;
        else hi = mid;
    }
    const bool f = lo < n && ft_cmp(ft_load(keys, lo), k) == 0;
    for (uint32_t c = lane; c < W; c += 64) {
        uint32_t v = c == 0 ? T : 0u;
        if (f) {
            v = rec[(uint64_t)lo * W + c];
            if (c == 0 && v != T) atomicOr(&res[FT_FLAGS], FT_F_MISMATCH);
        }
        out[w * W + c] = v;
    }
    if (lane == 0) found[w] = f;
}

// --------------------------------------------------------------------- host
// a device array of `bytes` bytes, 4-byte aligned (an empty one may be anything)
static bool ft_dev(const void *p, size_t bytes) { return !bytes || dev_words(p); }
static bool ft_vec(uint32_t T, const void *a, const void *b, const void *o) {
    return T % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)o) & 15) == 0;
}

// scratch of the join, carved from ctx->d_scratch (FtBuf: flowjoin.h)
void ft_carve(Carve &cv, FtBuf &b, size_t ntiles, size_t na, bool diff) {
    b.res = cv.take<unsigned long long>(FT_RES_WORDS);
    if (diff) {
        b.sb = cv.take<uint32_t>(na);
    } else {
        b.sa = cv.take<uint32_t>(ntiles * FT_SLOTS);
        b.sb = cv.take<uint32_t>(ntiles * FT_SLOTS);
        b.tilecnt = cv.take<uint32_t>(ntiles);
        b.tilebase = cv.take<uint64_t>(ntiles);
    }
}
// res[] into the pinned words, after everything enqueued on s
int ft_read_res(qk_ctx *ctx, const FtBuf &b, hipStream_t s, uint64_t *out) {
    QK_HIP_TRY(hipMemcpyAsync(ctx->h_flow, b.res, FT_RES_WORDS * 8, hipMemcpyDeviceToHost, s));
    QK_HIP_TRY(hipStreamSynchronize(s));
    std::copy(ctx->h_flow, ctx->h_flow + FT_RES_WORDS, out);
    return QK_OK;
}

int ft_join_merge(qk_ctx *ctx, hipStream_t s, const uint32_t *ka, uint32_t na, const uint32_t *kb, uint32_t nb,
                  const FtBuf &b, size_t ntiles, uint64_t *res) {
    QK_HIP_TRY(hipMemsetAsync(b.res, 0, FT_RES_WORDS * 8, s));
    hipLaunchKernelGGL((k_ft_join<false>), dim3((uint32_t)ntiles), dim3(FT_BLOCK), 0, s, ka, na, kb, nb, b.sa, b.sb,
                       b.tilecnt, b.res);
    hipLaunchKernelGGL(k_ft_scan, dim3(1), dim3(FT_SCAN), 0, s, b.tilecnt, (uint32_t)ntiles, b.tilebase, b.res);
    if (hipGetLastError() != hipSuccess) return QK_E_HIP;
    return ft_read_res(ctx, b, s, res);
}

} // namespace qk

using namespace qk;

extern "C" int qk_u32_flows_merge_device(qk_ctx *ctx, const qk_flow_key *d_keys_a, const uint8_t *d_sk_a, size_t na,
                                         const qk_flow_key *d_keys_b, const uint8_t *d_sk_b, size_t nb,
                                         uint32_t threshold, uint32_t frequency_pkts, qk_flow_key *d_keys_out,
                                         uint8_t *d_sk_out, uint8_t *d_due_out, size_t cap, size_t *n_out,
                                         void *stream) {
    if (int e = check_ctx_threshold(ctx, threshold)) return e;
    if (!n_out || na >= ((size_t)1 << 31) || nb >= ((size_t)1 << 31)) return QK_E_INVAL;
    *n_out = 0;
    const uint32_t T = threshold;
    const size_t rec = qk_u32_size(T);
    std::lock_guard<std::mutex> lk(ctx->mu);
    QK_HIP_TRY(hipSetDevice(ctx->device));
    if (!ft_dev(d_keys_a, na * 12) || !ft_dev(d_sk_a, na * rec) || !ft_dev(d_keys_b, nb * 12) ||
        !ft_dev(d_sk_b, nb * rec) || !ft_dev(d_keys_out, cap * 12) || !ft_dev(d_sk_out, cap * rec) ||
        (d_due_out && cap && !is_device_ptr(d_due_out)))
        return QK_E_INVAL;
    const void *in[4] = {d_keys_a, d_sk_a, d_keys_b, d_sk_b};
    const size_t inb[4] = {na * 12, na * rec, nb * 12, nb * rec};
    const void *out[3] = {d_keys_out, d_sk_out, d_due_out};
    const size_t outb[3] = {cap * 12, cap * rec, cap};
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 4; ++i)
            if (ranges_overlap(out[o], outb[o], in[i], inb[i])) return QK_E_INVAL;
        for (int p = 0; p < o; ++p)
            if (ranges_overlap(out[o], outb[o], out[p], outb[p])) return QK_E_INVAL;
    }
    const size_t N = na + nb;
    if (N == 0) return QK_OK;
    hipStream_t s = pick_stream(ctx, stream);
    const size_t ntiles = (N + FT_TILE - 1) / FT_TILE;
    Carve probe{nullptr};
    FtBuf b;
    ft_carve(probe, b, ntiles, na, false);
    if (int e = scratch_acquire(ctx, s)) return e;
    if (int e = ensure_scratch(ctx, probe.off, s)) return e;
    Carve cv{(char *)ctx->d_scratch};
    ft_carve(cv, b, ntiles, na, false);
    const uint32_t *ka = (const uint32_t *)d_keys_a, *kb = (const uint32_t *)d_keys_b;
    int rc = QK_OK;
    uint64_t res[FT_RES_WORDS] = {0, 0, 0, 0};
    // the one place the union's size is known: QK_E_CAPACITY (and input out of
    // order) is decided here, before anything is written to the outputs
    rc = ft_join_merge(ctx, s, ka, (uint32_t)na, kb, (uint32_t)nb, b, ntiles, res);
    if (!rc && (res[FT_FLAGS] & FT_F_ORDER)) rc = QK_E_INVAL;
    if (!rc) {
        *n_out = (size_t)res[FT_TOTAL];
        if (res[FT_TOTAL] != N - res[FT_MATCH]) rc = QK_E_HIP;   // the two counts are kept by different kernels
        else if (res[FT_TOTAL] > cap) rc = QK_E_CAPACITY;
    }
    if (!rc) {
        const uint32_t *ra = (const uint32_t *)d_sk_a, *rb = (const uint32_t *)d_sk_b;
        uint32_t *ro = (uint32_t *)d_sk_out, *ko = (uint32_t *)d_keys_out;
        const dim3 grid((uint32_t)(ntiles * FT_CPT));
        if (ft_vec(T, d_sk_a, d_sk_b, d_sk_out))
            hipLaunchKernelGGL((k_ft_move<false, true>), grid, dim3(FT_BLOCK), 0, s, ra, rb, ro, ka, kb, ko, d_due_out,
                               b.sa, b.sb, b.tilecnt, b.tilebase, (uint32_t)na, (uint32_t)nb, T, frequency_pkts, b.res);
        else
            hipLaunchKernelGGL((k_ft_move<false, false>), grid, dim3(FT_BLOCK), 0, s, ra, rb, ro, ka, kb, ko, d_due_out,
                               b.sa, b.sb, b.tilecnt, b.tilebase, (uint32_t)na, (uint32_t)nb, T, frequency_pkts, b.res);
        if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
        if (!rc) rc = ft_read_res(ctx, b, s, res);
        if (!rc && (res[FT_FLAGS] & FT_F_MISMATCH)) rc = QK_E_MISMATCH;
    }
    if (int e = scratch_release(ctx, s))
        if (!rc) rc = e;
    return rc;
}

extern "C" int qk_u32_flows_diff_device(qk_ctx *ctx, const qk_flow_key *d_keys_a, const uint8_t *d_sk_a, size_t na,
                                        const qk_flow_key *d_keys_b, const uint8_t *d_sk_b, size_t nb,
                                        uint32_t threshold, uint8_t *d_diffs_out, size_t *n_matched, void *stream) {
    if (int e = check_ctx_threshold(ctx, threshold)) return e;
    if (!n_matched || na >= ((size_t)1 << 31) || nb >= ((size_t)1 << 31)) return QK_E_INVAL;
    *n_matched = 0;
    const uint32_t T = threshold;
    const size_t rec = qk_u32_size(T);
    std::lock_guard<std::mutex> lk(ctx->mu);
    QK_HIP_TRY(hipSetDevice(ctx->device));
    if (!ft_dev(d_keys_a, na * 12) || !ft_dev(d_sk_a, na * rec) || !ft_dev(d_keys_b, nb * 12) ||
        !ft_dev(d_sk_b, nb * rec) || !ft_dev(d_diffs_out, na * rec))
        return QK_E_INVAL;
    if (ranges_overlap(d_diffs_out, na * rec, d_keys_a, na * 12) || ranges_overlap(d_diffs_out, na * rec, d_sk_a, na * rec) ||
        ranges_overlap(d_diffs_out, na * rec, d_keys_b, nb * 12) || ranges_overlap(d_diffs_out, na * rec, d_sk_b, nb * rec))
        return QK_E_INVAL;
    const size_t N = na + nb;
    if (N == 0) return QK_OK;
    hipStream_t s = pick_stream(ctx, stream);
    const size_t ntiles = (N + FT_TILE - 1) / FT_TILE;
    Carve probe{nullptr};
    FtBuf b;
    ft_carve(probe, b, ntiles, na, true);
    if (int e = scratch_acquire(ctx, s)) return e;
    if (int e = ensure_scratch(ctx, probe.off, s)) return e;
    Carve cv{(char *)ctx->d_scratch};
    ft_carve(cv, b, ntiles, na, true);
    const uint32_t *ka = (const uint32_t *)d_keys_a, *kb = (const uint32_t *)d_keys_b;
    int rc = QK_OK;
    uint64_t res[FT_RES_WORDS] = {0, 0, 0, 0};
    if (hipMemsetAsync(b.res, 0, FT_RES_WORDS * 8, s) != hipSuccess) rc = QK_E_HIP;
    if (!rc) {
        hipLaunchKernelGGL((k_ft_join<true>), dim3((uint32_t)ntiles), dim3(FT_BLOCK), 0, s, ka, (uint32_t)na, kb,
                           (uint32_t)nb, (uint32_t *)nullptr, b.sb, (uint32_t *)nullptr, b.res);
        if (na) {
            const uint32_t *ra = (const uint32_t *)d_sk_a, *rb = (const uint32_t *)d_sk_b;
            uint32_t *ro = (uint32_t *)d_diffs_out;
            const dim3 grid((uint32_t)((na + FT_CHUNK - 1) / FT_CHUNK));
            if (ft_vec(T, d_sk_a, d_sk_b, d_diffs_out))
                hipLaunchKernelGGL((k_ft_move<true, true>), grid, dim3(FT_BLOCK), 0, s, ra, rb, ro, ka, kb,
                                   (uint32_t *)nullptr, (uint8_t *)nullptr, (const uint32_t *)nullptr, b.sb,
                                   (const uint32_t *)nullptr, (const uint64_t *)nullptr, (uint32_t)na, (uint32_t)nb, T,
                                   0u, b.res);
            else
                hipLaunchKernelGGL((k_ft_move<true, false>), grid, dim3(FT_BLOCK), 0, s, ra, rb, ro, ka, kb,
                                   (uint32_t *)nullptr, (uint8_t *)nullptr, (const uint32_t *)nullptr, b.sb,
                                   (const uint32_t *)nullptr, (const uint64_t *)nullptr, (uint32_t)na, (uint32_t)nb, T,
                                   0u, b.res);
        }
        if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
    }
    if (!rc) rc = ft_read_res(ctx, b, s, res);
    else (void)hipStreamSynchronize(s);
    if (!rc && (res[FT_FLAGS] & FT_F_ORDER)) rc = QK_E_INVAL;
    if (!rc && (res[FT_FLAGS] & FT_F_MISMATCH)) rc = QK_E_MISMATCH;
    if (!rc) *n_matched = (size_t)res[FT_MATCH];
    if (int e = scratch_release(ctx, s))
        if (!rc) rc = e;
    return rc;
}

extern "C" int qk_u32_flows_lookup_device(qk_ctx *ctx, const qk_flow_key *d_keys, const uint8_t *d_sk, size_t n,
                                          uint32_t threshold, const qk_flow_key *keys, size_t nk, uint8_t *sketches,
                                          uint8_t *found, void *stream) {
    if (int e = check_ctx_threshold(ctx, threshold)) return e;
    if (n >= ((size_t)1 << 31) || nk >= ((size_t)1 << 31)) return QK_E_INVAL;
    if (nk == 0) return QK_OK;
    if (!keys || !sketches || !found) return QK_E_INVAL;
    const uint32_t T = threshold;
    const size_t rec = qk_u32_size(T);
    std::lock_guard<std::mutex> lk(ctx->mu);
    QK_HIP_TRY(hipSetDevice(ctx->device));
    if (!ft_dev(d_keys, n * 12) || !ft_dev(d_sk, n * rec)) return QK_E_INVAL;
    if (is_device_ptr(keys) || is_device_ptr(sketches) || is_device_ptr(found)) return QK_E_INVAL;
    hipStream_t s = pick_stream(ctx, stream);
    unsigned long long *d_res = nullptr;
    uint32_t *d_q = nullptr, *d_out = nullptr;
    uint8_t *d_found = nullptr;
    if (int e = scratch_acquire(ctx, s)) return e;
    for (int pass = 0; pass < 2; ++pass) {
        Carve cv{pass ? (char *)ctx->d_scratch : nullptr};
        d_res = cv.take<unsigned long long>(FT_RES_WORDS);
        d_q = cv.take<uint32_t>(nk * 3);
        d_out = cv.take<uint32_t>(nk * (rec / 4));
        d_found = cv.take<uint8_t>(nk);
        if (!pass)
            if (int e = ensure_scratch(ctx, cv.off, s)) return e;
    }
    int rc = QK_OK;
    uint64_t res[FT_RES_WORDS] = {0, 0, 0, 0};
    if (hipMemsetAsync(d_res, 0, FT_RES_WORDS * 8, s) != hipSuccess ||
        hipMemcpyAsync(d_q, keys, nk * 12, hipMemcpyHostToDevice, s) != hipSuccess)
        rc = QK_E_HIP;
    if (!rc) {
        hipLaunchKernelGGL(k_ft_lookup, dim3((uint32_t)((nk + FT_BLOCK / 64 - 1) / (FT_BLOCK / 64))), dim3(FT_BLOCK), 0,
                           s, (const uint32_t *)d_keys, (uint32_t)n, (const uint32_t *)d_sk, T, d_q, (uint32_t)nk, d_out,
                           d_found, d_res);
        if (hipGetLastError() != hipSuccess) rc = QK_E_HIP;
    }
    if (!rc && (hipMemcpyAsync(sketches, d_out, nk * rec, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(found, d_found, nk, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(ctx->h_flow, d_res, FT_RES_WORDS * 8, hipMemcpyDeviceToHost, s) != hipSuccess))
        rc = QK_E_HIP;
    // the host keys and the staging must outlive what was enqueued
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = QK_E_HIP;
    if (!rc) std::copy(ctx->h_flow, ctx->h_flow + FT_RES_WORDS, res);
    if (!rc && (res[FT_FLAGS] & FT_F_MISMATCH)) rc = QK_E_MISMATCH;
    if (int e = scratch_release(ctx, s))
        if (!rc) rc = e;
    return rc;
}
