// encode.hip — batch power-sum encode on gfx950 (the hot path).
//
// Replaces the reference's per-id loop `for id in ids { quack.insert(id) }`
// (sidekick/src/sidekick.rs:42 inside the sniff loop :76-124; quack's
// benchmark_construct, figures/fig2_microbenchmarks.py:220-228) for an id
// array resident in HBM.
//
// Kernels and dispatch (`enc32` / `enc64` below):
//   * 5 <= t <= 80 (u32) — the headline kernel k_encode_u32_bsgs<NB,NA,SG>
//     (bsgs.h; the shape of each threshold: QK_U32_SHAPES below): baby steps x^1..x^NB and giant steps x^(NB a) per id, lane
//     private, then S_(NB a + b) += A_a * B_b as 64-bit multiply-accumulates
//     whose wraps are counted per wave on the scalar unit.  t = 32 is
//     (NB, NA) = (8, 4): 9 lazy modmuls + 24 MACs + 8 row-0 mads per id =
//     4.47 SIMD-cycles of VALU issue per id (the algorithmic anchor,
//     tools/issue_model.py); the kernel issues 1.19 VALU + 0.76 SALU
//     wave-instructions per id, each id's MAC phase at raised wave priority
//     (s_setprio, bsgs.h Cfg PRIO).  Streams below 2^32 ids take the dynamic
//     form k_encode_u32_bsgs_dyn (knob enc_dyn): one round of resident
//     workgroups whose waves claim 4 096-id chunks from eight counters; only
//     the wave that finds the chunks exhausted at counter 0 runs masked trips
//     and the head / tail (bsgs.h body_dyn, run_encode_dyn below).  Longer
//     streams and enc_dyn = 0 take the static grid-stride form over three
//     rounds of resident workgroups (knob grid_mult; also the u64 kernels,
//     the chains and, at one round, the passes).  It runs at 0.86-0.89 of the
//     anchor at the bench run's own shader clock (bench.py roofline.valu,
//     DESIGN.md §4) and ~0.20-0.21 of the HBM read roofline (4 B/id; the
//     line moves with the box's shader clock, 2.0-2.1 GHz).
//   * t = 31..32 (u32) — k_encode_u32_basis / k_encode_u32_basis_dyn (knob
//     u32_basis, default 1): the same kernel bodies with the 32 powers from
//     the nine-power basis of basis32.h, 8 lazy modmuls per id instead of the
//     (8, 4) grid's 9 (bsgs.h CfgBasis); the ids whose lazy chain is wrong
//     are looked up in an LDS table once per trip (basis_filter.h).
//     u32_basis = 2 finds them by the minimum of each id's products instead;
//     u32_basis = 0 and the all-VALU fallback take the grid.
//   * 14 <= t <= 80 (u64) — k_encode_u64_bsgs<NA,SG> (bsgs64.h): the
//     same split with the babies/giants of a 256-id tile shared through LDS,
//     each wave owning two babies' MAC rows (paired, at raised priority).
//   * t > 80 — passes of the BSGS kernels (offset giants x^(base + 8a)).
//   * small t (u32 t <= 4, u64 t <= 13) — power chains: a lane group of G
//     lanes owns one id, lane j computes powers j+1, j+1+G, ... with step
//     x^G and K lazy accumulators (G K >= t).
//   The ids are never reduced mod p up front (x^k is congruent either way).
//   Lane partials -> wavefront butterfly -> LDS across the waves -> one
//   partial per (power, block), stored [power][block] -> a finalize kernel
//   (one workgroup per power) writes the canonical partial vector.
// Integer-issue bound; no MFMA (north_star).  (The int8 matrix-core variant
// measured in rounds 2-3, DESIGN.md §3.9, was removed from the sources in
// round 4; it lives in the git history.)
#include <algorithm>
#include <type_traits>
#include <utility>

#include "ctx.h"
#include "field.h"
#include "bsgs.h"
#include "bsgs64.h"

namespace qk {

QK_WARM_KERNEL(encode)

using bsgs::BLOCK;
using bsgs::WAVES;
using bsgs::shfl_xor_u64;

// ------------------------------------------------------------------ u32
// Power chains in t-form (field.h: tstep32, chain32, group_powers32); x and
// x5 = 5x are canonical.

// four independent ids in lockstep (ILP for the dependent modmul chains);
// the four t-form values of a power are summed before the accumulate
// (each < 6*2^32, so the sum and the lane accumulator stay far below 2^64).
template <int K>
__device__ __forceinline__ void chain32x4(uint64_t (&acc)[K], uint4 w) {
    const uint32_t x0 = canon32(w.x), x1 = canon32(w.y), x2 = canon32(w.z), x3 = canon32(w.w);
    const uint32_t f0 = times5_32(x0), f1 = times5_32(x1), f2 = times5_32(x2), f3 = times5_32(x3);
    uint64_t t0 = x0, t1 = x1, t2 = x2, t3 = x3;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        acc[k] += t0;
        acc[k] += t1;
        acc[k] += t2;
        acc[k] += t3;
        if (k + 1 < K) {
            t0 = tstep32p(t0, x0, f0, 0u);
            t1 = tstep32p(t1, x1, f1, 0u);
            t2 = tstep32p(t2, x2, f2, 0u);
            t3 = tstep32p(t3, x3, f3, 0u);
        }
    }
}

// ---- baby-step / giant-step encode, the shapes of QK_U32_SHAPES below (bsgs.h)
// waves per SIMD the register budget is sized for (tools/tune_bsgs.hip: 5 for
// (8,4) beat 4 by 2-3 %; its three spilled VGPRs live outside the loop)
// Every encode kernel runs each id's accumulation at raised wave priority —
// row 0 at 1, the MAC rows at 2, the powers at 0 (bsgs.h Cfg PRIO; t = 32:
// 2.60 / 2.67 vs 2.66 / 2.73 ms for the MAC phase at 1, vs 2.77 ms for none,
// profiles/r04/prio/tune_bsgs_prio_levels*.json)
template <int NB, int NA, int SG>
__global__ __launch_bounds__(BLOCK, (NB * NA == 32 ? 5 : NB * NA > 64 ? 2 : NB * NA > 40 ? 3 : 4)) void k_encode_u32_bsgs(const uint32_t *__restrict__ ids,
                                                                                  uint64_t n, uint32_t head,
                                                                                  uint32_t T,
                                                                                  uint64_t *__restrict__ partials) {
    bsgs::body<bsgs::Cfg<NB, NA, SG, true>>(ids, n, head, T, partials);
}

// The same with the ids handed out dynamically (bsgs.h body_dyn): the waves
// claim chunks of 64 x DYN_CH 16-byte groups from the counter `ctr`, whose
// value before this launch is `cbase`.
template <int NB, int NA, int SG>
__global__ __launch_bounds__(BLOCK, (NB * NA == 32 ? 5 : NB * NA > 64 ? 2 : NB * NA > 40 ? 3 : 4)) void k_encode_u32_bsgs_dyn(
    const uint32_t *__restrict__ ids, uint64_t n, uint32_t head, uint32_t T, uint64_t *__restrict__ partials,
    const bsgs::DynArgs da) {
    bsgs::body_dyn<bsgs::Cfg<NB, NA, SG, true>>(ids, n, head, T, partials, da);
}

// t = 31..32 from the nine-power basis (basis32.h, bsgs.h CfgBasis; knob
// u32_basis): 8 lazy products per id instead of the (8,4) grid's 9, the same
// accumulators, wrap counting and priorities.  Static and dynamic form.
// FILT 1: wrong ids by the table of basis_filter.h (16 KiB of LDS per
// workgroup); 0: by the minimum of the products (knob u32_basis = 2).
template <int FILT = 1>
__global__ __launch_bounds__(BLOCK, 5) void k_encode_u32_basis(const uint32_t *__restrict__ ids, uint64_t n,
                                                              uint32_t head, uint32_t T,
                                                              uint64_t *__restrict__ partials) {
    bsgs::body<bsgs::CfgBasis<true, FILT>>(ids, n, head, T, partials);
}
template <int FILT = 1>
__global__ __launch_bounds__(BLOCK, 5) void k_encode_u32_basis_dyn(const uint32_t *__restrict__ ids, uint64_t n,
                                                                  uint32_t head, uint32_t T,
                                                                  uint64_t *__restrict__ partials,
                                                                  const bsgs::DynArgs da) {
    bsgs::body_dyn<bsgs::CfgBasis<true, FILT>>(ids, n, head, T, partials, da);
}

// Pass 0 of a multi-pass encode (powers 1..80) that also writes x^80 per id
// for pass 1 (the x^base cache, enc_passes_chunk)
template <int SG>
__global__ __launch_bounds__(BLOCK, 2) void k_encode_u32_bsgs_x80(const uint32_t *__restrict__ ids, uint64_t n,
                                                                 uint32_t head, uint32_t T,
                                                                 uint64_t *__restrict__ partials,
                                                                 const uint32_t *xin,
                                                                 uint32_t *xout) {
    (void)xin;
    bsgs::body<bsgs::Cfg<8, 10, SG, true, 2>>(ids, n, head, T, partials, 0, nullptr, xout);
}

// Offset pass for thresholds > 80 (several passes over the ids): powers
// base+1 .. base+8*NA with giants x^(base + 8a), a = 0..NA-1 (bsgs.h OFF).
// XC: x^base from the previous pass's per-id cache (bit 0) / x^(base + 8 NA)
// to the next pass's (bit 1) instead of square-and-multiply per pass.
template <int NA, int SG, int XC = 0>
__global__ __launch_bounds__(BLOCK, (NA > 6 ? 2 : NA > 5 ? 3 : 4)) void k_encode_u32_bsgs_off(
    const uint32_t *__restrict__ ids, uint64_t n, uint32_t head, uint32_t T, uint32_t base,
    uint64_t *__restrict__ partials, const uint32_t *xin, uint32_t *xout) {
    bsgs::body<bsgs::Cfg<8, NA, SG, true, XC, true>>(ids, n, head, T, partials, base, xin, xout);
}

// Reduce per-lane accumulators to one partial per (power, block).
// acc[k] of lane with (lane % G) == j belongs to power m = j + k*G (0-based).
template <int G, int K, typename Fold>
__device__ __forceinline__ void block_store(const uint64_t (&acc)[K], uint32_t T, uint64_t *partials,
                                            uint64_t *sm, Fold fold) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        uint64_t v = fold(acc[k]);                   // < 2^32
#pragma unroll
        for (int off = 32; off >= G; off >>= 1) v += shfl_xor_u64(v, off); // < 2^38
        if (lane < G) sm[wave * (G * K) + lane + k * G] = v;
    }
    __syncthreads();
    for (uint32_t m = threadIdx.x; m < T; m += BLOCK) {
        uint64_t s = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) s += sm[w * (G * K) + m];   // < 2^40
        partials[(size_t)m * gridDim.x + blockIdx.x] = s;
    }
}

struct Fold32 {
    __device__ uint64_t operator()(uint64_t a) const { return fold64_32(a); }
};

// G == 1: each lane streams ids with 16-byte loads.
template <int K>
__global__ __launch_bounds__(BLOCK) void k_encode_u32_g1(const uint32_t *__restrict__ ids, uint64_t n,
                                                         uint32_t head, uint32_t T,
                                                         uint64_t *__restrict__ partials) {
    __shared__ uint64_t sm[WAVES * K];
    uint64_t acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0;

    const uint64_t gtid = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint64_t nthr = (uint64_t)gridDim.x * BLOCK;
    const uint64_t h = head < n ? head : n;
    const uint64_t body = (n - h) >> 2;
    const uint4 *__restrict__ v = reinterpret_cast<const uint4 *>(ids + h);

    for (uint64_t i = gtid; i < body; i += nthr) chain32x4<K>(acc, v[i]);
    // unaligned head (< 4 ids) and tail (< 4 ids)
    const uint64_t tail0 = h + (body << 2);
    if (gtid < h) chain32<K>(acc, ids[gtid], canon32(ids[gtid]));
    if (gtid < n - tail0) chain32<K>(acc, ids[tail0 + gtid], canon32(ids[tail0 + gtid]));

    block_store<1, K>(acc, T, partials, sm, Fold32{});
}

// G > 1: lane groups share one id (scalar loads; G lanes read one address).
template <int G, int K>
__global__ __launch_bounds__(BLOCK) void k_encode_u32_gn(const uint32_t *__restrict__ ids, uint64_t n,
                                                         uint32_t head, uint32_t T,
                                                         uint64_t *__restrict__ partials) {
    (void)head;
    __shared__ uint64_t sm[WAVES * G * K];
    uint64_t acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0;
    const int j = threadIdx.x % G;
    const uint64_t grp = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) / G;
    const uint64_t ngrp = (uint64_t)gridDim.x * BLOCK / G;
    for (uint64_t i = grp; i < n; i += ngrp) {
        uint32_t start, step;
        group_powers32<G>(ids[i], j, start, step);
        chain32<K>(acc, start, step);
    }
    block_store<G, K>(acc, T, partials, sm, Fold32{});
}

// Sum block partials of power m = blockIdx.x; write canonical S_m to out[m]
// (or add it in when accumulate).  The launch with meta != nullptr also
// writes count and last id there (meta[0], meta[1]): out + T for a single-pass
// encode; in a multi-pass encode out is the partial vector + the pass's base
// and only pass 0 has a meta.
__global__ __launch_bounds__(BLOCK) void k_finalize_u32(const uint64_t *__restrict__ partials,
                                                        uint32_t nblocks, uint32_t T,
                                                        const uint32_t *__restrict__ ids, uint64_t n,
                                                        uint64_t *__restrict__ out,
                                                        uint64_t *__restrict__ meta, int accumulate) {
    __shared__ uint64_t sm[WAVES];
    const uint32_t m = blockIdx.x;
    uint64_t s = 0;
    for (uint32_t b = threadIdx.x; b < nblocks; b += BLOCK) s += partials[(size_t)m * nblocks + b]; // < 2^60
    s = fold64_32(s);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += shfl_xor_u64(s, off);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t tot = 0;
        for (int w = 0; w < WAVES; ++w) tot += sm[w];
        const uint32_t c = canon32(fold64_32(tot));
        out[m] = accumulate ? (uint64_t)add32((uint32_t)out[m], c) : (uint64_t)c;
        if (m == 0 && meta) {
            meta[0] = accumulate ? meta[0] + n : n;
            if (n) meta[1] = ids[n - 1];
            else if (!accumulate) meta[1] = 0;
        }
    }
}

// ------------------------------------------------------------------ u64
// Power chain over p64 = 2^64 - 59, hand-scheduled (gfx950 ISA).  State:
// t = t0 + t1*2^32 + th*2^64 (th <= 59; t0:t1 pinned in v[2:3] so the step can
// address the halves of its 64-bit pairs).  One step, for a step value x < 2^64:
//   V  = (t0:t1) + 59*th            v_mad_u64_u32; wraps past 2^64 only when
//                                   V < 59*60, then V += 59 (2^64 == 59) exactly
//   P  = V*x < 2^128                four v_mad_u64_u32:
//        A = V.lo*x0, B = V.hi*x0 + A.hi, C = V.lo*x1 + B (carry cc),
//        PH = V.hi*x1 + C.hi + cc*2^32, P_L = A.lo + C.lo*2^32
//   t' = P_L + 59*PH  (< 60*2^64)   two v_mad_u64_u32: E = P_L + 59*PH.lo
//                                   (carry ce), F = E.hi + ce*2^32 + 59*PH.hi;
//                                   t0' = E.lo, t1' = F.lo, th' = F.hi
// and the previous power's value is added into its 96-bit accumulator
// (a0, a1, a2) with a carry chain in the same block: 7 multiplies + 14 simple
// ops per power (the compiler's rendering of field.h tstep64 plus the
// accumulate spends 8 multiplies and ~20 moves/adds/compares).  Every
// VALU-written carry is read >= 2 wait states later (gfx950 VALU SGPR-write ->
// VALU read hazard).
#define QK_U64_STEP_ASM                                                                            \
    "v_add_co_u32_e64 %[a0], %[sc], %[a0], v2\n\t"                                                   \
    "v_mad_u64_u32 v[4:5], %[cw], %[th], 59, v[2:3]\n\t"                                             \
    "v_mov_b32_e32 v11, 0\n\t"                                                                     \
    "v_addc_co_u32_e64 %[a1], %[sc], %[a1], v3, %[sc]\n\t"                                           \
    "v_cndmask_b32_e64 %[tmp], 0, 59, %[cw]\n\t"                                                     \
    "v_add_u32_e32 v4, v4, %[tmp]\n\t"                                                               \
    "v_addc_co_u32_e64 %[a2], %[cx], %[a2], %[th], %[sc]\n\t"                                        \
    "v_mad_u64_u32 v[6:7], %[cx], v4, %[x0], 0\n\t"                                                  \
    "v_mov_b32_e32 v10, v7\n\t"                                                                    \
    "v_mad_u64_u32 v[8:9], %[cx], v5, %[x0], v[10:11]\n\t"                                           \
    "v_mad_u64_u32 v[8:9], %[cc], v4, %[x1], v[8:9]\n\t"                                             \
    "v_mov_b32_e32 v7, v8\n\t"                                                                     \
    "v_mov_b32_e32 v10, v9\n\t"                                                                    \
    "v_cndmask_b32_e64 v11, 0, 1, %[cc]\n\t"                                                         \
    "v_mad_u64_u32 v[4:5], %[cx], v5, %[x1], v[10:11]\n\t"                                           \
    "v_mad_u64_u32 v[2:3], %[ce], v4, 59, v[6:7]\n\t"                                                \
    "v_mov_b32_e32 v8, v3\n\t"                                                                     \
    "s_nop 0\n\t"                                                                                  \
    "v_cndmask_b32_e64 v9, 0, 1, %[ce]\n\t"                                                          \
    "v_mad_u64_u32 v[8:9], %[cx], v5, 59, v[8:9]\n\t"                                                \
    "v_mov_b32_e32 v3, v8\n\t"                                                                     \
    "v_mov_b32_e32 %[th], v9\n\t"

template <int K>
__device__ __forceinline__ void chain64(uint32_t (&a0)[K], uint32_t (&a1)[K], uint32_t (&a2)[K], uint64_t start,
                                        uint64_t step) {
    // start, step: any values < 2^64 (t-form with th = 0)
    uint64_t t = start;
    uint32_t th = 0;
    const uint32_t x0 = (uint32_t)step, x1 = (uint32_t)(step >> 32);
#pragma unroll
    for (int k = 0; k + 1 < K; ++k) {
        uint64_t sc, cw, cx, cc, ce;
        uint32_t tmp;
        asm volatile(QK_U64_STEP_ASM
                     : [a0] "+v"(a0[k]), [a1] "+v"(a1[k]), [a2] "+v"(a2[k]), "+{v[2:3]}"(t), [th] "+v"(th),
                       [sc] "=&s"(sc), [cw] "=&s"(cw), [cx] "=&s"(cx), [cc] "=&s"(cc), [ce] "=&s"(ce),
                       [tmp] "=&v"(tmp)
                     : [x0] "v"(x0), [x1] "v"(x1)
                     : "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11");
    }
    uint64_t sc, cx;
    asm volatile("v_add_co_u32_e64 %[a0], %[sc], %[a0], v2\n\t"
                 "s_nop 1\n\t"
                 "v_addc_co_u32_e64 %[a1], %[sc], %[a1], v3, %[sc]\n\t"
                 "s_nop 1\n\t"
                 "v_addc_co_u32_e64 %[a2], %[cx], %[a2], %[th], %[sc]\n\t"
                 : [a0] "+v"(a0[K - 1]), [a1] "+v"(a1[K - 1]), [a2] "+v"(a2[K - 1]), [sc] "=&s"(sc), [cx] "=&s"(cx)
                 : "{v[2:3]}"(t), [th] "v"(th));
}

// (lo, hi) -> a 64-bit value through an opaque move, so the 32-bit
// accumulators are not kept as zero-extended / shifted 64-bit pairs
__device__ __forceinline__ uint64_t pack64(uint32_t lo, uint32_t hi) {
    uint64_t v;
    asm volatile("v_mov_b32_e32 v12, %1\n\tv_mov_b32_e32 v13, %2" : "={v[12:13]}"(v) : "v"(lo), "v"(hi));
    return v;
}

// t-form value -> a value < 2^64 congruent to it (chain starts and steps)
__device__ __forceinline__ uint64_t vfold64(uint32_t t0, uint32_t t1, uint32_t th) {
    const uint64_t t = ((uint64_t)t1 << 32) | t0;
    const uint64_t v = t + (uint64_t)th * C64;
    return v < t ? v + C64 : v; // wrapped: v < 59*60 and 2^64 == 59
}

// The step without an accumulate (chain setup): t <- t*x, t-form in/out.
#define QK_U64_MUL_ASM                                                                             \
    "v_mad_u64_u32 v[4:5], %[cw], %[th], 59, v[2:3]\n\t"                                             \
    "v_mov_b32_e32 v11, 0\n\t"                                                                     \
    "s_nop 0\n\t"                                                                                  \
    "v_cndmask_b32_e64 %[tmp], 0, 59, %[cw]\n\t"                                                     \
    "v_add_u32_e32 v4, v4, %[tmp]\n\t"                                                               \
    "v_mad_u64_u32 v[6:7], %[cx], v4, %[x0], 0\n\t"                                                  \
    "v_mov_b32_e32 v10, v7\n\t"                                                                    \
    "v_mad_u64_u32 v[8:9], %[cx], v5, %[x0], v[10:11]\n\t"                                           \
    "v_mad_u64_u32 v[8:9], %[cc], v4, %[x1], v[8:9]\n\t"                                             \
    "v_mov_b32_e32 v7, v8\n\t"                                                                     \
    "v_mov_b32_e32 v10, v9\n\t"                                                                    \
    "v_cndmask_b32_e64 v11, 0, 1, %[cc]\n\t"                                                         \
    "v_mad_u64_u32 v[4:5], %[cx], v5, %[x1], v[10:11]\n\t"                                           \
    "v_mad_u64_u32 v[2:3], %[ce], v4, 59, v[6:7]\n\t"                                                \
    "v_mov_b32_e32 v8, v3\n\t"                                                                     \
    "s_nop 0\n\t"                                                                                  \
    "v_cndmask_b32_e64 v9, 0, 1, %[ce]\n\t"                                                          \
    "v_mad_u64_u32 v[8:9], %[cx], v5, 59, v[8:9]\n\t"                                                \
    "v_mov_b32_e32 v3, v8\n\t"                                                                     \
    "v_mov_b32_e32 %[th], v9\n\t"

__device__ __forceinline__ void tmul64_asm(uint64_t &t, uint32_t &th, uint32_t x0, uint32_t x1) {
    uint64_t cw, cx, cc, ce;
    uint32_t tmp;
    asm volatile(QK_U64_MUL_ASM
                 : "+{v[2:3]}"(t), [th] "+v"(th), [cw] "=&s"(cw), [cx] "=&s"(cx), [cc] "=&s"(cc), [ce] "=&s"(ce),
                   [tmp] "=&v"(tmp)
                 : [x0] "v"(x0), [x1] "v"(x1)
                 : "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11");
}

// Lane j of a group of G starts at x^(j+1) and steps by x^G: x^2 .. x^G by
// the same step, each folded below 2^64.
template <int G>
__device__ __forceinline__ void group_powers64(uint64_t x, int j, uint64_t &start, uint64_t &step) {
    const uint32_t x0 = (uint32_t)x, x1 = (uint32_t)(x >> 32);
    uint64_t t = x;
    uint32_t th = 0;
    start = x;
    step = x;
#pragma unroll
    for (int g = 1; g < G; ++g) {
        tmul64_asm(t, th, x0, x1);
        const uint64_t v = vfold64((uint32_t)t, (uint32_t)(t >> 32), th);
        if (g == j) start = v;
        step = v; // after the last iteration: x^G
    }
}

// u64 partials: two 32-bit limbs per power, stored [2m + limb][block].
template <int G, int K>
__device__ __forceinline__ void block_store64(const uint32_t (&a0)[K], const uint32_t (&a1)[K],
                                              const uint32_t (&a2)[K], uint32_t T, uint64_t *partials,
                                              uint64_t *sm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint64_t f = fold96_64(a2[k], pack64(a0[k], a1[k]));
        uint64_t a = (uint32_t)f, b = f >> 32;
#pragma unroll
        for (int off = 32; off >= G; off >>= 1) {
            a += shfl_xor_u64(a, off);
            b += shfl_xor_u64(b, off);
        }
        if (lane < G) {
            sm[wave * (2 * G * K) + 2 * (lane + k * G)] = a;
            sm[wave * (2 * G * K) + 2 * (lane + k * G) + 1] = b;
        }
    }
    __syncthreads();
    for (uint32_t m = threadIdx.x; m < 2 * T; m += BLOCK) {
        uint64_t s = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) s += sm[w * (2 * G * K) + m];
        partials[(size_t)m * gridDim.x + blockIdx.x] = s;
    }
}

template <int K>
__global__ __launch_bounds__(BLOCK) void k_encode_u64_g1(const uint64_t *__restrict__ ids, uint64_t n,
                                                         uint32_t head, uint32_t T,
                                                         uint64_t *__restrict__ partials) {
    __shared__ uint64_t sm[WAVES * 2 * K];
    uint32_t a0[K], a1[K], a2[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { a0[k] = 0; a1[k] = 0; a2[k] = 0; }
    const uint64_t gtid = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint64_t nthr = (uint64_t)gridDim.x * BLOCK;
    const uint64_t h = head < n ? head : n;
    const uint64_t body = (n - h) >> 1;
    const ulonglong2 *__restrict__ v = reinterpret_cast<const ulonglong2 *>(ids + h);
    for (uint64_t i = gtid; i < body; i += nthr) {
        const ulonglong2 w = v[i];
        chain64<K>(a0, a1, a2, w.x, w.x);
        chain64<K>(a0, a1, a2, w.y, w.y);
    }
    const uint64_t tail0 = h + (body << 1);
    if (gtid < h) chain64<K>(a0, a1, a2, ids[gtid], ids[gtid]);
    if (gtid < n - tail0) chain64<K>(a0, a1, a2, ids[tail0 + gtid], ids[tail0 + gtid]);
    block_store64<1, K>(a0, a1, a2, T, partials, sm);
}

template <int G, int K>
__global__ __launch_bounds__(BLOCK) void k_encode_u64_gn(const uint64_t *__restrict__ ids, uint64_t n,
                                                         uint32_t head, uint32_t T,
                                                         uint64_t *__restrict__ partials) {
    (void)head;
    __shared__ uint64_t sm[WAVES * 2 * G * K];
    uint32_t a0[K], a1[K], a2[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { a0[k] = 0; a1[k] = 0; a2[k] = 0; }
    const int j = threadIdx.x % G;
    const uint64_t grp = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) / G;
    const uint64_t ngrp = (uint64_t)gridDim.x * BLOCK / G;
    for (uint64_t i = grp; i < n; i += ngrp) {
        uint64_t start, step;
        group_powers64<G>(ids[i], j, start, step);
        chain64<K>(a0, a1, a2, start, step);
    }
    block_store64<G, K>(a0, a1, a2, T, partials, sm);
}

// Sum block limb partials of power m = blockIdx.x; write canonical S_m as
// two 32-bit limbs out[2m], out[2m+1] (or add it in when accumulate); the
// launch with meta != nullptr also writes count and last id (meta[0..1]):
// out + 2 T for a single-pass encode, pass 0 alone in a multi-pass one.
__global__ __launch_bounds__(BLOCK) void k_finalize_u64(const uint64_t *__restrict__ partials,
                                                        uint32_t nblocks, uint32_t T,
                                                        const uint64_t *__restrict__ ids, uint64_t n,
                                                        uint64_t *__restrict__ out,
                                                        uint64_t *__restrict__ meta, int accumulate) {
    __shared__ uint64_t sm[2][WAVES];
    const uint32_t m = blockIdx.x; // power index
    uint64_t a = 0, b = 0;         // limb sums, each < nblocks * 2^40
    for (uint32_t i = threadIdx.x; i < nblocks; i += BLOCK) {
        a += partials[(size_t)(2 * m) * nblocks + i];
        b += partials[(size_t)(2 * m + 1) * nblocks + i];
    }
    // fold each limb sum to < 2^64 congruent, then re-split to limbs so the
    // cross-lane sums cannot overflow: value = a + b*2^32.
    {
        const uint64_t av = canon64(a), bv = mul64_lazy(canon64(b), 1ull << 32);
        const uint64_t vv = canon64(add64(canon64(av), canon64(bv)));
        a = (uint32_t)vv;
        b = vv >> 32;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a += shfl_xor_u64(a, off);
        b += shfl_xor_u64(b, off);
    }
    if ((threadIdx.x & 63) == 0) { sm[0][threadIdx.x >> 6] = a; sm[1][threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t sa = 0, sb = 0;
        for (int w = 0; w < WAVES; ++w) { sa += sm[0][w]; sb += sm[1][w]; } // < 2^40
        uint64_t v = add64(canon64(sa), mul64(canon64(sb), 1ull << 32));
        if (accumulate) v = add64(canon64(out[2 * m] | (out[2 * m + 1] << 32)), v);
        out[2 * m] = (uint32_t)v;
        out[2 * m + 1] = v >> 32;
        if (m == 0 && meta) {
            meta[0] = accumulate ? meta[0] + n : n;
            if (n) meta[1] = ids[n - 1];
            else if (!accumulate) meta[1] = 0;
        }
    }
}

// u64 baby-step / giant-step (bsgs64.h): 256-id tiles, babies and giants
// shared through LDS, the MAC powers split over the 4 waves.  The babies'
// B * 2^32 are recomputed by their owner wave instead of stored and x^8
// is read from baby 8: 32 KB of LDS per workgroup at t = 80, 4 per CU
// (tools/tune_u64.hip: 24.1 vs 25.6 ms per 1e9 ids with 50 KB at 3 per CU).
// The first SG MACs of a wave's tile count their carries on the scalar unit;
// with two babies per wave the two MACs of a giant row are issued as one
// interleaved block.  The MAC step runs at raised wave priority (the row-0
// sums at 1, the MACs at 2: ~1 % over one level).
template <int NA, int SG>
__global__ __launch_bounds__(bsgs64::BLOCK, 4) void k_encode_u64_bsgs(const uint64_t *__restrict__ ids, uint64_t n,
                                                                      uint32_t head, uint32_t T,
                                                                      uint64_t *__restrict__ partials) {
    (void)head;
    bsgs64::body<bsgs64::Cfg<NA, 8, SG>>(ids, n, T, partials);
}

// the same with four babies per id (one per wave) and NA giant rows of 4
// powers: t <= 40 (bsgs64.h NBT)
template <int NA>
__global__ __launch_bounds__(bsgs64::BLOCK, 4) void k_encode_u64_bsgs4(const uint64_t *__restrict__ ids, uint64_t n,
                                                                       uint32_t head, uint32_t T,
                                                                       uint64_t *__restrict__ partials) {
    (void)head;
    bsgs64::body<bsgs64::Cfg<NA, 4, 16>>(ids, n, T, partials);
}

// Pass 0 of a u64 multi-pass encode that also writes x^80 per id for pass 1
__global__ __launch_bounds__(bsgs64::BLOCK, 4) void k_encode_u64_bsgs_x80(const uint64_t *__restrict__ ids,
                                                                          uint64_t n, uint32_t head, uint32_t T,
                                                                          uint64_t *__restrict__ partials,
                                                                          uint64_t *xout) {
    (void)head;
    bsgs64::body<bsgs64::Cfg<10, 8, 16, 2>>(ids, n, T, partials, 0, nullptr, xout);
}

// Offset pass for u64 thresholds > 80: powers base+1 .. base+8NA with giants
// x^(base + 8a) (bsgs64.h OFF); the ids are read once per pass.
// XC: the per-id x^base cache between passes (bsgs64.h)
template <int NA, int XC = 0>
__global__ __launch_bounds__(bsgs64::BLOCK, 4) void k_encode_u64_bsgs_off(const uint64_t *__restrict__ ids,
                                                                          uint64_t n, uint32_t head, uint32_t T,
                                                                          uint32_t base,
                                                                          uint64_t *__restrict__ partials,
                                                                          const uint64_t *xin,
                                                                          uint64_t *xout) {
    (void)head;
    bsgs64::body<bsgs64::Cfg<NA, 8, 16, XC, true>>(ids, n, T, partials, base, xin, xout);
}

// ------------------------------------------------------------- dispatch
template <int... Vs>
using ints = std::integer_sequence<int, Vs...>;

// A runtime integer as a template argument: f(std::integral_constant<int, V>)
// for the V of Vs equal to v, `none` when there is no such V.
template <int... Vs, class F>
static int with_int(int v, ints<Vs...>, int none, F &&f) {
    int rc = none;
    (void)((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return rc;
}

// units / per_block workgroups, at most `mult` rounds of the resident ones
// (mult <= 0: knob grid_mult), or the override.
static uint32_t grid_clamp(const qk_ctx *ctx, uint64_t units, uint32_t per_block, uint64_t blocks_per_cu, int mult) {
    if (ctx->grid_override) return ctx->grid_override;
    const uint64_t full = (uint64_t)ctx->num_cus * blocks_per_cu * (uint64_t)(mult > 0 ? mult : ctx->knobs.grid_mult);
    uint64_t need = (units + per_block - 1) / per_block;
    if (need < 1) need = 1;
    return (uint32_t)(need < full ? need : full);
}

template <typename KernelT>
static uint32_t grid_for(qk_ctx *ctx, KernelT kern, uint64_t units, uint32_t per_block, int mult = 0) {
    int occ = 0;
    if (ctx->grid_override || hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, BLOCK, 0) != hipSuccess ||
        occ < 1)
        occ = 1;
    // knob grid_mult: resident workgroups x this.  The static encode kernels
    // (the u64 kernels, the chains, the u32 BSGS kernels at enc_dyn = 0 or
    // n >= 2^32) split the ids evenly over the grid; with one round of
    // workgroups the launch ends with the slowest CU's share, with three the
    // shares are a third as long and the CUs that finish early take the
    // later workgroups (the dynamic form asks for one round: mult = 1)
    // (mult > 0: fixed by the caller — u32 t > 48 and the u32 passes measured
    // 0.4-2.3 % slower at three rounds, profiles/r04/grid_mult/)
    return grid_clamp(ctx, units, per_block, (uint64_t)occ, mult);
}

// An upper bound on grid_for over every kernel a multi-pass encode may
// launch, whatever its occupancy: the device's resident threads per CU
// (hipDeviceAttributeMaxThreadsPerMultiProcessor, read at context creation)
// in workgroups of BLOCK threads.  The x^base cache is placed after the
// largest partials this allows.
static uint32_t grid_cap(const qk_ctx *ctx, uint64_t units, uint32_t per_block, int mult = 0) {
    return grid_clamp(ctx, units, per_block, ctx->max_blocks_per_cu(BLOCK), mult);
}

template <class KernelT, class... Args>
static void launch(KernelT kern, uint32_t nb, hipStream_t s, Args... args) {
    hipLaunchKernelGGL(kern, dim3(nb), dim3(BLOCK), 0, s, args...);
}

// The launch sequence of every encode: room for the partials of nb
// workgroups, the scratch hand-off, main(nb, partials) — the main kernel,
// between the profiling events — then fin(nb, partials), the finalize.
template <class Main, class Fin>
static int launch_encode(qk_ctx *ctx, uint32_t nb, size_t scratch_bytes, hipStream_t s, Main &&main, Fin &&fin) {
    if (int rc = ensure_scratch(ctx, scratch_bytes, s)) return rc;
    uint64_t *partials = (uint64_t *)ctx->d_scratch;
    if (int rc = scratch_acquire(ctx, s)) return rc;
    hipEvent_t e0 = prof_begin(ctx, s);
    main(nb, partials);
    prof_end(ctx, s, e0);
    QK_HIP_TRY(hipGetLastError());
    fin(nb, partials);
    QK_HIP_TRY(hipGetLastError());
    return scratch_release(ctx, s);
}

// The finalize of T powers into out, count and last id into meta (nullptr:
// not written; out + T words of a single-pass encode), as launch_encode's fin.
template <typename IdT>
static auto finalize_to(uint32_t T, const IdT *ids, size_t n, uint64_t *out, uint64_t *meta, int acc, hipStream_t s) {
    return [=](uint32_t nb, const uint64_t *partials) {
        if constexpr (sizeof(IdT) == 4)
            hipLaunchKernelGGL(k_finalize_u32, dim3(T), dim3(BLOCK), 0, s, partials, nb, T, ids, (uint64_t)n, out, meta,
                               acc);
        else
            hipLaunchKernelGGL(k_finalize_u64, dim3(T), dim3(BLOCK), 0, s, partials, nb, T, ids, (uint64_t)n, out, meta,
                               acc);
    };
}

// A single-pass encode with a kernel of the plain form (ids, n, head, T,
// partials) that keeps GK partial rows per workgroup.
template <typename IdT, typename KernelT>
static int run_encode(qk_ctx *ctx, KernelT kern, uint32_t GK, const IdT *d_ids, size_t n, uint32_t head, uint32_t T,
                      uint64_t units, uint32_t per_block, uint64_t *d_partial, int accumulate, hipStream_t s,
                      int mult = 0) {
    constexpr uint32_t W = sizeof(IdT) / 4;   // 32-bit limbs, each a partial row and an output word, per power
    const uint32_t nb = grid_for(ctx, kern, units, per_block, mult);
    return launch_encode(
        ctx, nb, (size_t)nb * W * GK * sizeof(uint64_t), s,
        [&](uint32_t, uint64_t *partials) { launch(kern, nb, s, d_ids, (uint64_t)n, head, T, partials); },
        finalize_to(T, d_ids, n, d_partial, d_partial + W * T, accumulate, s));
}

// The dynamic form of a single-pass u32 BSGS encode (bsgs.h body_dyn): one
// round of resident workgroups (or the override) whose waves claim chunks of
// ids from the counters at d_small[ENC_CLAIM], one per region of the chunks.
// The counters are never reset: a launch of nb workgroups moves each by its
// region's chunks + nb * WAVES (every wave ends with one failed claim at
// every counter), and the context keeps their values for the next launch's
// bases.  Launches are ordered by the scratch hand-off (launch_encode), so a
// launch finds the counters at its bases whatever stream it runs on.
static_assert((size_t)bsgs::DYN_NCTR * bsgs::DYN_CTR_STRIDE <= ENC_CLAIM_WORDS &&
                  bsgs::DYN_NCTR == sizeof(qk_ctx::enc_claim_base) / sizeof(uint64_t),
              "ctx.h: room for the dynamic encode's counters and their bases");
template <typename KernelT>
static int run_encode_dyn(qk_ctx *ctx, KernelT kern, uint32_t GK, const uint32_t *d_ids, size_t n, uint32_t head,
                          uint32_t T, uint64_t *d_partial, int accumulate, hipStream_t s) {
    const uint32_t nb = grid_for(ctx, kern, ((uint64_t)n + 3) / 4, BLOCK, 1);
    const uint64_t h = head < n ? head : n;
    const uint64_t nchunks = ((n - h) >> 2) / bsgs::DYN_GROUPS;
    bsgs::DynArgs da;
    da.ctr = (unsigned long long *)(ctx->d_small + ENC_CLAIM);
    da.region = (nchunks + bsgs::DYN_NCTR - 1) / bsgs::DYN_NCTR;
    for (int k = 0; k < bsgs::DYN_NCTR; ++k) da.base[k] = ctx->enc_claim_base[k];
    auto fin = finalize_to(T, d_ids, n, d_partial, d_partial + T, accumulate, s);
    return launch_encode(
        ctx, nb, (size_t)nb * GK * sizeof(uint64_t), s,
        [&](uint32_t, uint64_t *partials) { launch(kern, nb, s, d_ids, (uint64_t)n, head, T, partials, da); },
        [&](uint32_t, const uint64_t *partials) {   // the main kernel is enqueued: its claims move the counters
            for (int k = 0; k < bsgs::DYN_NCTR; ++k)
                ctx->enc_claim_base[k] += bsgs::dyn_region_len(nchunks, da.region, (uint32_t)k) + (uint64_t)nb * WAVES;
            fin(nb, partials);
        });
}

// sums of per-block partials [power][block] -> canonical S_1..S_T in out[0..T)
int launch_finalize_powers_u32(const uint64_t *partials, uint32_t nblocks, uint32_t T, uint64_t *out,
                               hipStream_t s) {
    finalize_to(T, (const uint32_t *)nullptr, 0, out, nullptr, 0, s)(nblocks, partials);
    return hipGetLastError() == hipSuccess ? QK_OK : QK_E_HIP;
}

// Thresholds 81..1024 by baby-step/giant-step passes: pass 0 is the (8,10)
// kernel (powers 1..80), each further pass the offset kernel with giants
// from x^base (the ids are read once per pass; HBM has the bandwidth, the
// passes are integer-issue bound like the single-pass kernels).
static int enc_passes_chunk(qk_ctx *ctx, const uint32_t *ids, size_t n, uint32_t head, uint32_t T, uint64_t *out,
                            int acc, hipStream_t s) {
    // pass 0: powers 1..80 with the single-pass (8,10) kernel; then passes of
    // <= 48 powers with the offset (8,6) kernel (142 VGPRs, 3 waves/SIMD;
    // every row of an offset pass is a MAC row: the 80-power form spills, a
    // 64-power (8,8) form at 2 waves/SIMD measured the same as 48)
    //
    // Each pass hands x^(next base) to the next one through a per-id cache
    // (4 B per id read + 4 B written per pass) instead of every offset pass
    // raising x^8 to base/8 (~4-8 of its ~16-22 modmuls per id): pass 0
    // writes x^80, the middle passes read and write, the last one reads.  The
    // cache lives in the scratch after the partials, sized once for every
    // pass (a regrow between passes would drop it), with the ids' address
    // modulo 16 so that both are read in the same 16-byte groups.
    const uint32_t npass = T <= 80 ? 0 : (T - 80 + 47) / 48;   // offset passes
    uint32_t *xc = nullptr;
    if (npass >= 1) {
        const uint32_t nbmax = grid_cap(ctx, (n + 3) / 4, BLOCK, 1);   // run_pass: one round
        const size_t poff = ((size_t)nbmax * 80 * sizeof(uint64_t) + 255) & ~(size_t)255;
        if (ensure_scratch(ctx, poff + 16 + (size_t)n * 4, s) == QK_OK)
            xc = (uint32_t *)((char *)ctx->d_scratch + poff + ((uintptr_t)ids & 15));
        // else: no room for the cache, each pass raises x^8 itself
    }
    uint32_t pass = 0;
    for (uint32_t base = 0; base < T; ++pass) {
        const uint32_t Tp = std::min<uint32_t>(base == 0 ? 80 : 48, T - base);
        // one pass: main(nb, partials) launches kern (GK partial rows per
        // workgroup); its powers go to out + base, count and last id with pass 0
        auto run_pass = [&](auto kern, uint32_t GK, auto main) {
            const uint32_t nb = grid_for(ctx, kern, (n + 3) / 4, BLOCK, 1);
            return launch_encode(ctx, nb, (size_t)nb * GK * sizeof(uint64_t), s, main,
                                 finalize_to(Tp, ids, n, out + base, base == 0 ? out + T : nullptr, acc, s));
        };
        // an offset pass of NA giant rows; XC: x^base from the cache (bit 0),
        // x^(base + 8 NA) to it (bit 1)
        auto off = [&](auto na, auto x) {
            constexpr int NA = decltype(na)::value, XC = decltype(x)::value;
            auto kern = k_encode_u32_bsgs_off<NA, 2 * NA, XC>;
            return run_pass(kern, 8 * NA, [&](uint32_t nb, uint64_t *partials) {
                launch(kern, nb, s, ids, (uint64_t)n, head, Tp, base, partials, (const uint32_t *)(XC & 1 ? xc : nullptr),
                       XC & 2 ? xc : nullptr);
            });
        };
        // XC: pass 0 writes the cache, the middle passes read and write it, the last reads it
        const int xcm = !xc ? 0 : (pass > 0 ? 1 : 0) | (pass < npass ? 2 : 0);
        int rc;
        if (base == 0 && xc) {
            auto kern = k_encode_u32_bsgs_x80<16>;
            rc = run_pass(kern, 80, [&](uint32_t nb, uint64_t *partials) {
                launch(kern, nb, s, ids, (uint64_t)n, head, Tp, partials, (const uint32_t *)nullptr, xc);
            });
        } else if (base == 0) {
            auto kern = k_encode_u32_bsgs<8, 10, 16>;
            rc = run_pass(kern, 80, [&](uint32_t nb, uint64_t *partials) {
                launch(kern, nb, s, ids, (uint64_t)n, head, Tp, partials);
            });
        } else if (Tp <= 40) {   // the last pass (npass >= 1): NA = ceil(Tp / 8) giant rows; <= 8 powers: one (x^base)
            rc = with_int((Tp + 7) / 8, ints<1, 2, 3, 4, 5>{}, QK_E_THRESHOLD, [&](auto na) {
                return with_int(xcm & 1, ints<0, 1>{}, QK_E_THRESHOLD, [&](auto x) { return off(na, x); });
            });
        } else {
            rc = with_int(xcm, ints<0, 1, 2, 3>{}, QK_E_THRESHOLD,
                          [&](auto x) { return off(std::integral_constant<int, 6>{}, x); });
        }
        if (rc) return rc;
        base += Tp;
    }
    return QK_OK;
}

// u64 thresholds > 80: pass 0 is the single-pass (8 babies, 10 giants)
// kernel for powers 1..80, then offset passes of <= 80 powers (giants
// x^(base + 8a), every row a MAC row; NA = ceil(Tp / 8)).  Each pass reads the
// 8-byte ids once more: at ~25 ms of integer issue per pass over 1e9 ids, the
// extra 1 ms of HBM reads is noise.
static int enc_passes_chunk(qk_ctx *ctx, const uint64_t *ids, size_t n, uint32_t head, uint32_t T, uint64_t *out,
                            int acc, hipStream_t s) {
    // x^(next base) goes from pass to pass through a per-id cache (8 B read +
    // 8 B written per id and pass; pass 0 writes x^80) instead of each offset
    // pass raising x^8 to base/8 (as the u32 passes).  The cache follows the
    // partials in the scratch, sized once.
    const uint32_t npass = (T - 80 + 79) / 80;
    const uint64_t tiles = (n + bsgs64::BLOCK - 1) / bsgs64::BLOCK;
    uint64_t *xc = nullptr;
    if (npass >= 1) {
        const uint32_t nbmax = grid_cap(ctx, tiles, 1);
        const size_t poff = ((size_t)nbmax * 2 * 80 * sizeof(uint64_t) + 255) & ~(size_t)255;
        if (ensure_scratch(ctx, poff + (size_t)n * 8, s) == QK_OK) xc = (uint64_t *)((char *)ctx->d_scratch + poff);
    }
    // one pass of Tp powers from base + 1: main(nb, partials) launches its
    // kernel on the grid of kern (8 NA x 2 partial rows per workgroup); count
    // and last id go with pass 0
    auto run_pass = [&](auto kern, uint32_t NA, uint32_t Tp, uint32_t base, auto main) {
        const uint32_t nb = grid_for(ctx, kern, tiles, 1);
        return launch_encode(ctx, nb, (size_t)nb * 2 * 8 * NA * sizeof(uint64_t), s, main,
                             finalize_to(Tp, ids, n, out + 2 * base, base == 0 ? out + 2 * T : nullptr, acc, s));
    };
    // pass 0: powers 1..80 (+ x^80 per id for pass 1 when the cache is on)
    if (int rc = run_pass(k_encode_u64_bsgs<10, 14>, 10, 80, 0, [&](uint32_t nb, uint64_t *partials) {
            if (xc) launch(k_encode_u64_bsgs_x80, nb, s, ids, (uint64_t)n, head, 80u, partials, xc);
            else launch(k_encode_u64_bsgs<10, 14>, nb, s, ids, (uint64_t)n, head, 80u, partials);
        }))
        return rc;
    uint32_t pass = 1;
    for (uint32_t base = 80; base < T; ++pass) {
        const uint32_t Tp = std::min<uint32_t>(80, T - base);
        // an offset pass of NA giant rows; XC: the cache read (bit 0) and written (bit 1)
        auto off = [&](auto na, auto x) {
            constexpr int NA = decltype(na)::value, XC = decltype(x)::value;
            auto kern = k_encode_u64_bsgs_off<NA, XC>;
            uint64_t *c = XC ? xc : nullptr;
            return run_pass(kern, NA, Tp, base, [&](uint32_t nb, uint64_t *partials) {
                launch(kern, nb, s, ids, (uint64_t)n, head, Tp, base, partials, (const uint64_t *)c, c);
            });
        };
        // pass 0 wrote the cache; the middle passes read and write it (all
        // full 80-power passes), the last one reads it
        const int xcm = !xc ? 0 : 1 | (pass < npass ? 2 : 0);
        int rc;
        if (xcm & 2)   // a middle pass: Tp = 80
            rc = off(std::integral_constant<int, 10>{}, std::integral_constant<int, 3>{});
        else   // a last pass of <= 8 powers: one giant row (x^base)
            rc = with_int((Tp + 7) / 8, ints<1, 2, 3, 4, 5, 6, 7, 8, 9, 10>{}, QK_E_THRESHOLD, [&](auto na) {
                return with_int(xcm & 1, ints<0, 1>{}, QK_E_THRESHOLD, [&](auto x) { return off(na, x); });
            });
        if (rc) return rc;
        base += Tp;
    }
    return QK_OK;
}

// The x^base cache holds one word of the id's width per id for the whole
// array: above 1 GiB of it (2^28 u32 ids, 2^27 u64 ids) the passes run chunk
// by chunk (each chunk all its passes, the later chunks accumulating into
// out), so the scratch stays <= 1 GiB.
template <typename IdT>
static int enc_passes(qk_ctx *ctx, const IdT *ids, size_t n, uint32_t head, uint32_t T, uint64_t *out, int acc,
                      hipStream_t s) {
    constexpr size_t CHUNK = ((size_t)1 << 30) / sizeof(IdT);
    if (n <= CHUNK) return enc_passes_chunk(ctx, ids, n, head, T, out, acc, s);
    for (size_t c0 = 0; c0 < n; c0 += CHUNK) {
        const IdT *p = ids + c0;
        const uint32_t hd = (uint32_t)(((16 - ((uintptr_t)p & 15)) & 15) / sizeof(IdT));
        if (int rc = enc_passes_chunk(ctx, p, std::min(CHUNK, n - c0), hd, T, out, c0 ? 1 : acc, s)) return rc;
    }
    return QK_OK;
}

// Power chains, (G, K): the smallest G whose K = ceil(T/G) fits the register
// budget KMAX, then the smallest instantiated K >= ceil(T/G) — of KG1 at
// G = 1, of KGN above; gk(G, K) runs the encode.
using K32_G1 = ints<1, 2, 4, 8, 12, 16, 20, 24, 28, 32>;
using K32_GN = ints<20, 24, 28, 32>;
using K64_G1 = ints<1, 2, 4, 8, 12, 16, 20, 24, 32, 40>;
using K64_GN = ints<12, 16, 20, 24, 32, 40>;

template <int... Ks>
static int pick_k(uint32_t kneed, ints<Ks...>) {
    int K = 0;
    for (int k : {Ks...}) {
        K = k;
        if ((uint32_t)k >= kneed) break;
    }
    return K;
}

template <int KMAX, class KG1, class KGN, int... Gs, class F>
static int enc_chain(uint32_t T, ints<Gs...> gs, F &&gk) {
    int G = 1;
    while ((T + G - 1) / G > (uint32_t)KMAX) G *= 2;
    const uint32_t kneed = (T + G - 1) / G;
    return with_int(G, gs, QK_E_THRESHOLD, [&](auto g) {
        using KS = std::conditional_t<decltype(g)::value == 1, KG1, KGN>;
        return with_int(pick_k(kneed, KS{}), KS{}, QK_E_THRESHOLD, [&](auto k) { return gk(g, k); });
    });
}

// The single-pass u32 BSGS shapes with scalar-counted wraps, by threshold:
//   X(t_lo, t_hi, NB, NA, SG)
// 5..28: four babies and ceil(T / 4) giant rows (every group 4 wide); above,
// the round-3 shapes: the (NB, NA) with the fewest issue cycles for the
// powers actually needed — modmuls NB - 1 + NA - 2 at ~17 cycles, MACs
// NB (NA - 1) and row-0 adds NB at ~4.2, measured ((6,4) /
// (8,4) computed 24 / 32 powers at 17..28): 29..30 (6,5), 33..36 (6,6),
// 41..42 (6,7), 65..72 (8,9).  tools/issue_model.py u32_shape prices the same
// rows (tests/test_issue_model.py holds the two together).
#define QK_U32_SHAPES(X)           \
    X(5, 8, 4, 2, 1)               \
    X(9, 12, 4, 3, 3)              \
    X(13, 16, 4, 4, 4)             \
    X(17, 20, 4, 5, 5)             \
    X(21, 24, 4, 6, 6)             \
    X(25, 28, 4, 7, 7)             \
    X(29, 30, 6, 5, 5)             \
    X(31, 32, 8, 4, 8)             \
    X(33, 36, 6, 6, 6)             \
    X(37, 40, 8, 5, 10)            \
    X(41, 42, 6, 7, 7)             \
    X(43, 48, 8, 6, 12)            \
    X(49, 56, 8, 7, 14)            \
    X(57, 64, 8, 8, 16)            \
    X(65, 72, 8, 9, 14)            \
    X(73, 80, 8, 10, 16)

static int enc32(qk_ctx *ctx, const uint32_t *ids, size_t n, uint32_t T, uint64_t *out, int acc, hipStream_t s) {
    if (T == 0 || T > QK_MAX_THRESHOLD) return QK_E_THRESHOLD;
    const uintptr_t a = (uintptr_t)ids;
    if (a & 3) return QK_E_INVAL;
    const uint32_t head = (uint32_t)(((16 - (a & 15)) & 15) / 4);
    if (n >= (1ull << 40)) return QK_E_INVAL; // 4 TB of ids: beyond any HBM; keeps per-lane trip counts 32-bit
    // baby-step / giant-step for the thresholds of QK_U32_SHAPES (fewer
    // modmuls per id) and, in passes, above them; the power chain otherwise
    // Scalar-counted BSGS groups (bsgs.h) keep per-wave 32-bit wrap totals: a
    // wave sees at most 64 * (4 * trips + 2) wraps per accumulator, so trips
    // must stay < 2^24 - 1 — true for any n < 2^40 at >= 1 workgroup per CU;
    // a tiny override grid over a huge n takes the all-VALU form.
    const uint64_t min_grid = ctx->grid_override ? ctx->grid_override : (uint64_t)ctx->num_cus;
    const bool sc_ok = n / (4ull * BLOCK * min_grid) < (1ull << 24) - 2;
    // Dynamic form (knob enc_dyn): a wave's scalar wrap totals are 32-bit and
    // its share of the ids is not fixed, so n stays below 2^32 (one wave
    // alone could take every chunk: < 2^32 wraps per accumulator); longer
    // streams keep the static split.
    const bool dyn = ctx->knobs.enc_dyn != 0 && n < (1ull << 32);
#define QK_BSGS_STATIC(NB_, NA_, G_)                                                                      \
    run_encode(ctx, k_encode_u32_bsgs<NB_, NA_, G_>, NB_ * NA_, ids, n, head, T, (n + 3) / 4, BLOCK, out, acc, s, \
               NB_ * NA_ > 48 ? 1 : 0)
#define QK_BSGS(NB_, NA_, G_)                                                                             \
    (dyn ? run_encode_dyn(ctx, k_encode_u32_bsgs_dyn<NB_, NA_, G_>, NB_ * NA_, ids, n, head, T, out, acc, s) \
         : QK_BSGS_STATIC(NB_, NA_, G_))
#define QK_BSGS_ROW(LO_, HI_, NB_, NA_, G_) \
    if (T >= LO_ && T <= HI_) return QK_BSGS(NB_, NA_, G_);
    if (sc_ok) {
        if (T >= 31 && T <= 32 && ctx->knobs.u32_basis == 1)   // the nine-power basis (basis32.h), ids filtered
            return dyn ? run_encode_dyn(ctx, k_encode_u32_basis_dyn<1>, 32, ids, n, head, T, out, acc, s)
                       : run_encode(ctx, k_encode_u32_basis<1>, 32, ids, n, head, T, (n + 3) / 4, BLOCK, out, acc,
                                    s, 0);
        if (T >= 31 && T <= 32 && ctx->knobs.u32_basis == 2)   // ... with the minimum tracked per product
            return dyn ? run_encode_dyn(ctx, k_encode_u32_basis_dyn<0>, 32, ids, n, head, T, out, acc, s)
                       : run_encode(ctx, k_encode_u32_basis<0>, 32, ids, n, head, T, (n + 3) / 4, BLOCK, out, acc,
                                    s, 0);
        QK_U32_SHAPES(QK_BSGS_ROW)
        if (T > 80) return enc_passes(ctx, ids, n, head, T, out, acc, s);
    } else {
        // the all-VALU forms that fit the registers; t 33..80 would spill, so
        // a grid too small for scalar counts takes the power chain there
        // (static only: !sc_ok needs n >= 2^34, beyond the dynamic form)
        if (T >= 9 && T <= 12) return QK_BSGS_STATIC(4, 3, 0);
        if (T >= 13 && T <= 16) return QK_BSGS_STATIC(4, 4, 0);
        if (T >= 17 && T <= 24) return QK_BSGS_STATIC(6, 4, 0);
        if (T >= 25 && T <= 32) return QK_BSGS_STATIC(8, 4, 0);
    }
#undef QK_BSGS_ROW
#undef QK_BSGS
#undef QK_BSGS_STATIC
    return enc_chain<32, K32_G1, K32_GN>(T, ints<1, 2, 4, 8, 16, 32>{}, [&](auto g, auto k) {
        constexpr int G = decltype(g)::value, K = decltype(k)::value;
        if constexpr (G == 1)   // each lane streams ids with 16-byte loads
            return run_encode(ctx, k_encode_u32_g1<K>, K, ids, n, head, T, (n + 3) / 4, BLOCK, out, acc, s);
        else
            return run_encode(ctx, k_encode_u32_gn<G, K>, G * K, ids, n, head, T, n, BLOCK / G, out, acc, s);
    });
}

static int enc64(qk_ctx *ctx, const uint64_t *ids, size_t n, uint32_t T, uint64_t *out, int acc, hipStream_t s) {
    if (T == 0 || T > QK_MAX_THRESHOLD) return QK_E_THRESHOLD;
    const uintptr_t a = (uintptr_t)ids;
    if (a & 7) return QK_E_INVAL;
    const uint32_t head = (uint32_t)(((16 - (a & 15)) & 15) / 8);
    // baby-step / giant-step for 14 <= T <= 80 (configs[2] is T = 80; below
    // 14 powers the 8 modmuls of the babies and x^8 cost more than the chain
    // they save: profiles/r03/shapes/sweep64_tmin_ab.jsonl — 21 before round
    // 3, BSGS +3..9 % at t = 14..20): NA = ceil(T / 8) giant rows; its
    // per-wave 32-bit carry totals need < 2^31 ids per workgroup.  Every form
    // runs with s_setprio around the MACs.
    const uint64_t min_grid64 = ctx->grid_override ? ctx->grid_override : (uint64_t)ctx->num_cus;
    const bool bsgs_ok = n / min_grid64 < (1ull << 30);
    if (T >= 14 && T <= 80 && bsgs_ok) {
        const uint64_t tiles = (n + bsgs64::BLOCK - 1) / bsgs64::BLOCK;
        // four babies per id and ceil(T/4) giant rows where 8 babies would
        // compute 4+ powers more: t = 14..20, 25..28, 33..36 (+8..17 %,
        // profiles/r03/shapes/sweep64_four_babies_ab.jsonl; at t = 21..24,
        // 29..32 even, at 37..40 7 % slower: not used)
        const int rc4 = with_int(T <= 36 ? (T + 3) / 4 : 0, ints<4, 5, 7, 9>{}, 1, [&](auto na) {
            constexpr int NA = decltype(na)::value;
            return run_encode(ctx, k_encode_u64_bsgs4<NA>, 4 * NA, ids, n, head, T, tiles, 1, out, acc, s);
        });
        if (rc4 <= 0) return rc4;   // 1: no four-baby form at this T (a status is <= 0)
        return with_int((T + 7) / 8, ints<2, 3, 4, 5, 6, 7, 8, 9, 10>{}, QK_E_THRESHOLD, [&](auto na) {
            // NA <= 9: a wave's <= 16 MACs all scalar-counted
            // NA = 10: 14 of the 18 MACs scalar-counted with the paired-MAC form
            // (22.65 vs 23.19 ms at 16, twice, profiles/r04/prio/tune_u64_prio.json)
            constexpr int NA = decltype(na)::value, SG = NA == 10 ? 14 : 16;
            return run_encode(ctx, k_encode_u64_bsgs<NA, SG>, 8 * NA, ids, n, head, T, tiles, 1, out, acc, s);
        });
    }
    if (T > 80 && bsgs_ok) return enc_passes(ctx, ids, n, head, T, out, acc, s);
    // K <= 40 accumulators per lane (120 VGPRs, 3 waves/SIMD) beat K <= 20 at
    // 5 waves by needing fewer lanes per id (t = 80: 2 x (39 + 1) steps vs
    // 4 x (19 + 3)).
    return enc_chain<40, K64_G1, K64_GN>(T, ints<1, 2, 4, 8, 16, 32, 64>{}, [&](auto g, auto k) {
        constexpr int G = decltype(g)::value, K = decltype(k)::value;
        if constexpr (G == 1)
            return run_encode(ctx, k_encode_u64_g1<K>, K, ids, n, head, T, (n + 1) / 2, BLOCK, out, acc, s);
        else
            return run_encode(ctx, k_encode_u64_gn<G, K>, G * K, ids, n, head, T, n, BLOCK / G, out, acc, s);
    });
}

int launch_encode_u32(qk_ctx *ctx, const uint32_t *d_ids, size_t n, uint32_t t, uint64_t *d_partial, hipStream_t s) {
    return enc32(ctx, d_ids, n, t, d_partial, 0, s);
}
int launch_encode_u64(qk_ctx *ctx, const uint64_t *d_ids, size_t n, uint32_t t, uint64_t *d_partial, hipStream_t s) {
    return enc64(ctx, d_ids, n, t, d_partial, 0, s);
}
int launch_encode_u32_acc(qk_ctx *ctx, const uint32_t *d_ids, size_t n, uint32_t t, uint64_t *d_partial,
                          hipStream_t s) {
    return enc32(ctx, d_ids, n, t, d_partial, 1, s);
}
int launch_encode_u64_acc(qk_ctx *ctx, const uint64_t *d_ids, size_t n, uint32_t t, uint64_t *d_partial,
                          hipStream_t s) {
    return enc64(ctx, d_ids, n, t, d_partial, 1, s);
}

} // namespace qk
