// bsgs.h — baby-step / giant-step u32 encode body for 9 <= t <= 32 (the
// headline kernel).  Shared by encode.hip (product kernel)
// and tools/tune_bsgs.hip (A/B harness), so the tuned code is the shipped code.
//
// Power m+1 = a*NB + b + 1 with B_b = x^(b+1) (b < NB) and A_a = x^(a*NB)
// (a < NA; A_0 = 1), so S_{m+1} = sum_i A_a(x_i) * B_b(x_i): NB-1 + NA-2
// lazy modmuls per id, then (NA-1)*NB 32x32->64 multiply-accumulates into
// 64-bit accumulators whose wraps are counted (2^64 == 25 mod p), plus NB
// 64-bit adds for the a = 0 row, which cannot wrap.
//
// Wrap counting, per accumulator group of four (Cfg SG):
//   VALU form   v_mad_u64_u32 writes its carry to an SGPR pair,
//               v_addc_co_u32 adds it into a per-lane 32-bit counter.  gfx950
//               needs two wait states between a VALU SGPR write and a VALU
//               carry-in read (hipcc pads with s_nop), so four ops with four
//               distinct carry pairs are issued back to back first: every
//               v_addc reads a carry written >= 3 VALU instructions earlier.
//   SALU form   only the SUM over lanes of a power's wraps matters (the block
//               reduction adds every lane), so the carry mask is counted per
//               wave on the scalar unit (s_bcnt1 + s_add, issued beside the
//               VALU stream).  Needs EXEC = all lanes at the op (wave-uniform
//               control flow; lanes past their range feed id 0).
//
// Ids are not reduced mod p first: every product below is exact for any
// 32-bit operand and x == id (mod p) either way.
//
// Two loop structures walk the ids with the same per-id code (four / one):
//   body_gen   static: grid-stride over 16-byte groups, an unmasked main loop
//              and <= 2 masked trips per wave, head and tail in every
//              workgroup (the flow, segment and packet kernels, the offset
//              passes, and the single-pass kernels at enc_dyn = 0)
//   body_dyn   dynamic: waves claim chunks of DYN_CH x 64 groups from
//              counters, every claimed trip unmasked; one wave of the launch
//              walks the ragged rest, the head and the tail (the single-pass
//              kernels' default, DESIGN.md §3.2 "Grid")
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "basis32.h"
#include "basis_filter.h"
#include "field.h"

namespace qk {
namespace bsgs {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
    const uint32_t lo = __shfl_xor((int)(uint32_t)v, m, 64);
    const uint32_t hi = __shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return ((uint64_t)hi << 32) | lo;
}

// ---- multiply-accumulate groups, carries counted ---------------------------
// The carry masks live in explicitly named SGPR pairs, and consecutive groups
// alternate between two disjoint sets (SET 0: s[40:47] + temp s56, SET 1:
// s[48:55] + temp s57).  hipcc treats an inline-asm block's SGPR definitions
// conservatively and pads "s_nop 0" between two blocks that define the same
// SGPRs (8 nops per id with compiler-allocated pairs; 3-5 remain at blocks
// with "+s" operands — one fused asm statement per id measured no faster).
// The blocks are volatile so the compiler keeps them in this alternating
// order.  Inside a block every VALU carry-in read is >= 3 VALU instructions
// after its write.
#define QK_MAC4V(P0, P1, P2, P3)                                                                       \
    "v_mad_u64_u32 %0, " P0 ", %8, %9, %0\n\t"                                                         \
    "v_mad_u64_u32 %1, " P1 ", %8, %10, %1\n\t"                                                        \
    "v_mad_u64_u32 %2, " P2 ", %8, %11, %2\n\t"                                                        \
    "v_mad_u64_u32 %3, " P3 ", %8, %12, %3\n\t"                                                        \
    "v_addc_co_u32_e64 %4, " P0 ", %4, 0, " P0 "\n\t"                                                  \
    "v_addc_co_u32_e64 %5, " P1 ", %5, 0, " P1 "\n\t"                                                  \
    "v_addc_co_u32_e64 %6, " P2 ", %6, 0, " P2 "\n\t"                                                  \
    "v_addc_co_u32_e64 %7, " P3 ", %7, 0, " P3
#define QK_MAC4S(P0, P1, P2, P3, T)                                                                       \
    "v_mad_u64_u32 %0, " P0 ", %8, %9, %0\n\t"                                                         \
    "v_mad_u64_u32 %1, " P1 ", %8, %10, %1\n\t"                                                        \
    "v_mad_u64_u32 %2, " P2 ", %8, %11, %2\n\t"                                                        \
    "v_mad_u64_u32 %3, " P3 ", %8, %12, %3\n\t"                                                        \
    "s_bcnt1_i32_b64 " T ", " P0 "\n\ts_add_u32 %4, %4, " T "\n\t"                                          \
    "s_bcnt1_i32_b64 " T ", " P1 "\n\ts_add_u32 %5, %5, " T "\n\t"                                          \
    "s_bcnt1_i32_b64 " T ", " P2 "\n\ts_add_u32 %6, %6, " T "\n\t"                                          \
    "s_bcnt1_i32_b64 " T ", " P3 "\n\ts_add_u32 %7, %7, " T
#define QK_SET0 "s[40:41]", "s[42:43]", "s[44:45]", "s[46:47]"
#define QK_SET1 "s[48:49]", "s[50:51]", "s[52:53]", "s[54:55]"
// scalar-form temps: one per set, so adjacent blocks never share a definition
#define QK_SET0T QK_SET0, "s56"
#define QK_SET1T QK_SET1, "s57"
#define QK_CLOB0 "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47"
#define QK_CLOB1 "s48", "s49", "s50", "s51", "s52", "s53", "s54", "s55"
#define QK_EXPAND(M, ...) M(__VA_ARGS__)
// pair form (the nine-power basis, below): each multiply-add has its own two
// operands, acc_j += l_j * r_j
#define QK_MAC4PS(P0, P1, P2, P3, T)                                                                      \
    "v_mad_u64_u32 %0, " P0 ", %8, %9, %0\n\t"                                                         \
    "v_mad_u64_u32 %1, " P1 ", %10, %11, %1\n\t"                                                       \
    "v_mad_u64_u32 %2, " P2 ", %12, %13, %2\n\t"                                                       \
    "v_mad_u64_u32 %3, " P3 ", %14, %15, %3\n\t"                                                       \
    "s_bcnt1_i32_b64 " T ", " P0 "\n\ts_add_u32 %4, %4, " T "\n\t"                                          \
    "s_bcnt1_i32_b64 " T ", " P1 "\n\ts_add_u32 %5, %5, " T "\n\t"                                          \
    "s_bcnt1_i32_b64 " T ", " P2 "\n\ts_add_u32 %6, %6, " T "\n\t"                                          \
    "s_bcnt1_i32_b64 " T ", " P3 "\n\ts_add_u32 %7, %7, " T

// acc_j += A * b_j (64-bit), wraps counted per lane (c_j) or per wave (s_j)
template <int SET>
__device__ __forceinline__ void mac4v(uint64_t &a0, uint64_t &a1, uint64_t &a2, uint64_t &a3, uint32_t &c0,
                                      uint32_t &c1, uint32_t &c2, uint32_t &c3, uint32_t A, uint32_t b0,
                                      uint32_t b1, uint32_t b2, uint32_t b3) {
    if constexpr (SET == 0)
        asm volatile(QK_EXPAND(QK_MAC4V, QK_SET0)
            : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3)
            : "v"(A), "v"(b0), "v"(b1), "v"(b2), "v"(b3)
            : QK_CLOB0);
    else
        asm volatile(QK_EXPAND(QK_MAC4V, QK_SET1)
            : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3)
            : "v"(A), "v"(b0), "v"(b1), "v"(b2), "v"(b3)
            : QK_CLOB1);
}
template <int SET>
__device__ __forceinline__ void mac4s(uint64_t &a0, uint64_t &a1, uint64_t &a2, uint64_t &a3, uint32_t &s0,
                                      uint32_t &s1, uint32_t &s2, uint32_t &s3, uint32_t A, uint32_t b0,
                                      uint32_t b1, uint32_t b2, uint32_t b3) {
    if constexpr (SET == 0)
        asm volatile(QK_EXPAND(QK_MAC4S, QK_SET0T)
            : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3)
            : "v"(A), "v"(b0), "v"(b1), "v"(b2), "v"(b3)
            : "scc", "s56", QK_CLOB0);
    else
        asm volatile(QK_EXPAND(QK_MAC4S, QK_SET1T)
            : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3)
            : "v"(A), "v"(b0), "v"(b1), "v"(b2), "v"(b3)
            : "scc", "s57", QK_CLOB1);
}
// acc_j += l_j * r_j (64-bit), wraps counted per wave (s_j)
template <int SET>
__device__ __forceinline__ void mac4ps(uint64_t &a0, uint64_t &a1, uint64_t &a2, uint64_t &a3, uint32_t &s0,
                                       uint32_t &s1, uint32_t &s2, uint32_t &s3, uint32_t l0, uint32_t r0,
                                       uint32_t l1, uint32_t r1, uint32_t l2, uint32_t r2, uint32_t l3,
                                       uint32_t r3) {
    if constexpr (SET == 0)
        asm volatile(QK_EXPAND(QK_MAC4PS, QK_SET0T)
            : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3)
            : "v"(l0), "v"(r0), "v"(l1), "v"(r1), "v"(l2), "v"(r2), "v"(l3), "v"(r3)
            : "scc", "s56", QK_CLOB0);
    else
        asm volatile(QK_EXPAND(QK_MAC4PS, QK_SET1T)
            : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3)
            : "v"(l0), "v"(r0), "v"(l1), "v"(r1), "v"(l2), "v"(r2), "v"(l3), "v"(r3)
            : "scc", "s57", QK_CLOB1);
}
// leftovers for NB % 4 != 0 (t = 17..24 uses NB = 6): compiler-allocated
// carries with explicit wait states
__device__ __forceinline__ void mac2v(uint64_t &a0, uint64_t &a1, uint32_t &c0, uint32_t &c1, uint32_t A,
                                      uint32_t b0, uint32_t b1) {
    uint64_t k0, k1;
    asm("v_mad_u64_u32 %0, %4, %6, %7, %0\n\t"
        "v_mad_u64_u32 %1, %5, %6, %8, %1\n\t"
        "s_nop 0\n\t"
        "v_addc_co_u32_e64 %2, %4, %2, 0, %4\n\t"
        "v_addc_co_u32_e64 %3, %5, %3, 0, %5"
        : "+v"(a0), "+v"(a1), "+v"(c0), "+v"(c1), "=&s"(k0), "=&s"(k1)
        : "v"(A), "v"(b0), "v"(b1));
}

// ---- a = 0 row as 64-bit multiply-adds: acc_j += b_j * 1 ------------------
// acc < 2^64 for < 2^32 adds of 32-bit values, so no carry is counted: one
// VALU per add (its carry-out is dead).
#define QK_ROW4M(P0, P1, P2, P3)                                                                       \
    "v_mad_u64_u32 %0, " P0 ", %4, 1, %0\n\t"                                                          \
    "v_mad_u64_u32 %1, " P1 ", %5, 1, %1\n\t"                                                          \
    "v_mad_u64_u32 %2, " P2 ", %6, 1, %2\n\t"                                                          \
    "v_mad_u64_u32 %3, " P3 ", %7, 1, %3"
template <int SET>
__device__ __forceinline__ void row4m(uint64_t &a0, uint64_t &a1, uint64_t &a2, uint64_t &a3, uint32_t b0,
                                      uint32_t b1, uint32_t b2, uint32_t b3) {
    if constexpr (SET == 0)
        asm volatile(QK_EXPAND(QK_ROW4M, QK_SET0)
            : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)
            : "v"(b0), "v"(b1), "v"(b2), "v"(b3)
            : QK_CLOB0);
    else
        asm volatile(QK_EXPAND(QK_ROW4M, QK_SET1)
            : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)
            : "v"(b0), "v"(b1), "v"(b2), "v"(b3)
            : QK_CLOB1);
}
__device__ __forceinline__ void row2m(uint64_t &a0, uint64_t &a1, uint32_t b0, uint32_t b1) {
    uint64_t k0, k1;
    asm("v_mad_u64_u32 %0, %2, %4, 1, %0\n\t"
        "v_mad_u64_u32 %1, %3, %5, 1, %1"
        : "+v"(a0), "+v"(a1), "=&s"(k0), "=&s"(k1)
        : "v"(b0), "v"(b1));
}

// ---- configuration ----------------------------------------------------------
//  NB, NA  baby / giant steps (NB even)
//  SG      the first SG 4-wide accumulator groups count their wraps on the
//          scalar unit.  Group numbering: MAC row a (1..NA-1; an offset pass:
//          0..NA-1) has g = a*(NB/4) + b/4; the a = 0 sum row counts nothing.
//          NB % 4 leftovers always use the VALU form.
//  PRIO    wave priority (s_setprio) over each id's accumulation: row 0 at 1
//          and the MAC rows with their scalar wrap counts at 2, the powers at
//          0.  false: no priority change.
//  XC      bit 0 (offset passes) — x^base per id read from the previous
//          pass's cache instead of square-and-multiply; bit 1 — the next
//          pass's x^base written per id (one more product): x^(base + NB*NA)
//          after an offset pass, x^(NB*NA) after a plain one (pass 0)
//  OFF     offset pass (thresholds > 80, several passes over the ids): the
//          giants are x^(base + a*NB) for a = 0..NA-1 with a runtime base
//          (a multiple of NB), so every row is a MAC row (no a = 0 sum row)
//          and the pass yields powers base+1 .. base+NB*NA
//  BASIS   (CfgBasis) 32 powers from the nine-power basis of basis32.h instead
//          of the (8, 4) grid: 8 lazy products, 8 direct adds and 24 pair MACs
//          per id in the same accumulators (slot -> power from the table,
//          finish())
template <int NB_, int NA_, int SG_, bool PRIO_ = false, int XC_ = 0, bool OFF_ = false>
struct Cfg {
    static constexpr bool BASIS = false;   // CfgBasis (below) sets it
    static constexpr bool FILT = false;    // ... and this
    static constexpr int NB = NB_, NA = NA_, SG = SG_, XC = XC_;
    static constexpr bool PRIO = PRIO_, OFF = OFF_;
    static_assert(OFF_ || (XC_ & 1) == 0, "only an offset pass reads x^base");
    static constexpr int ROWS = OFF_ ? NA_ : NA_ - 1;   // MAC rows
    static constexpr int ROW1 = OFF_ ? 0 : 1;           // group-row number of the first MAC row
    static_assert(NB % 2 == 0 && (NA >= 2 || (OFF_ && NA == 1)), "NB even, NA >= 2 (1: offset pass)");
};
// The basis form: the plain (8, 4) configuration — its accumulators, every MAC
// group scalar-counted — with the flag set.
// FILT 1: the ids whose lazy chain is wrong are found by the table of
// basis_filter.h, once per trip of four ids; 0: by the minimum of each id's
// eight products (knob u32_basis = 2, kept for comparison).
template <bool PRIO_, int FILT_ = 1>
struct CfgBasis : Cfg<8, 4, 8, PRIO_> {
    static constexpr bool BASIS = true;
    static constexpr bool FILT = FILT_ != 0;
};

template <int NB, int NA, int ROWS = NA - 1>
struct Acc {
    uint64_t r0[NB];          // a = 0 row: sum of B_b, 64-bit
    uint64_t m[ROWS][NB];     // MAC rows: sum of A_a * B_b mod 2^64
    uint32_t c[ROWS][NB];     // ... its wraps (lane count, or wave total if scalar)
};

// group rows: 0 = the a = 0 sum row, ROW1.. = the MAC rows (an offset pass
// has no sum row: its MAC rows start at 0)
template <class C>
__host__ __device__ constexpr bool scalar_group(int row, int b) {
    return b / 4 * 4 + 4 <= C::NB && (row > 0 || C::OFF) && row * (C::NB / 4) + b / 4 < C::SG;
}

// x^(NB*q) from xn = x^NB by square-and-multiply over the (wave-uniform) q >= 1
template <class MUL>
__device__ __forceinline__ uint32_t pow_uniform(uint32_t xn, uint32_t q, MUL mul) {
    uint32_t r = 0, sq = xn;
    bool have = false;
    for (;;) {
        if (q & 1) {
            r = have ? mul(r, sq) : sq;
            have = true;
        }
        q >>= 1;
        if (!q) break;
        sq = mul(sq, sq);
    }
    return r;
}

// ---- an id's power chain as one statement -----------------------------------
// The lazy product (field.h mulfold32_min) is three v_mad_u64_u32:
//     P = y * x            Q = P + 5 Ph            R = P + 5 Qh,   r = Rl
// Ph, Qh and the r that feeds the next product are halves of 64-bit pairs, and
// an asm operand cannot name half of a pair, so a statement per product ends
// with the result in a compiler-chosen pair and hipcc pads one s_nop between
// it and the next product's statement.  The whole chain is therefore one
// statement over a fixed window of VGPRs (gfx950 register tuples are 64-bit
// aligned, so every result sits in the even register of a pair):
//     v[6:7]              Q, reused by every product
//     v[8:9]              x^NB (the last baby, A[0]); R is written over P in
//                         place, so v8 = r and v9 is the dead high word
//     v[10:11] .. v[26:27] the giants x^(2 NB), x^(3 NB), ... (up to nine)
//     v[28:29] ..         the babies x^(NB-1) down to x^2: x^2 sits in
//                         v[22 + 2 NB], so a shorter chain is a suffix of a
//                         longer one's text
// (v0 .. v5 are left alone: the kernels' prologues want them, and a window
// from v2 spilled five dwords more in the headline kernel; from v10 the
// small-flow kernel of t = 9..12 needed a 65th VGPR.)  An id costs Q plus one
// pair per product, as the product-by-product form does.  Unlike there, the
// odd halves are clobbered by the statement, so no value that lives across
// the loop can sit in one: body_gen makes up for it by keeping no thread
// index across its loops.  The running minimum of the results (the wrap
// check) is formed in the dead v9 inside the statement.  All carry-outs go to
// the clobbered pair s[58:59], which nothing reads.  Within the statement
// every hazard is a VALU result read by the next VALU, which the hardware
// interlocks.
#define QK_LP(D, DH, Y, X)                                                                             \
    "v_mad_u64_u32 v[" #D ":" #DH "], s[58:59], " Y ", " X ", 0\n\t"                                   \
    "v_mad_u64_u32 v[6:7], s[58:59], v" #DH ", 5, v[" #D ":" #DH "]\n\t"                               \
    "v_mad_u64_u32 v[" #D ":" #DH "], s[58:59], v7, 5, v[" #D ":" #DH "]\n\t"
// babies: x^2 = x * x first, then each by x (operand [id]) down to v[8:9]
#define QK_BT1 QK_LP(8, 9, "v28", "%[id]")
#define QK_BT2 QK_LP(28, 29, "v30", "%[id]") QK_BT1
#define QK_BT3 QK_LP(30, 31, "v32", "%[id]") QK_BT2
#define QK_BT4 QK_LP(32, 33, "v34", "%[id]") QK_BT3
#define QK_BT5 QK_LP(34, 35, "v36", "%[id]") QK_BT4
#define QK_BT6 QK_LP(36, 37, "v38", "%[id]") QK_BT5
#define QK_BABIES4 QK_LP(30, 31, "%[id]", "%[id]") QK_BT2
#define QK_BABIES6 QK_LP(34, 35, "%[id]", "%[id]") QK_BT4
#define QK_BABIES8 QK_LP(38, 39, "%[id]", "%[id]") QK_BT6
#define QK_BMIN4 "v_min3_u32 v9, v30, v28, v8\n\t"
#define QK_BMIN6 QK_BMIN4 "v_min3_u32 v9, v9, v34, v32\n\t"
#define QK_BMIN8 QK_BMIN6 "v_min3_u32 v9, v9, v38, v36\n\t"
#define QK_BOUT4 "=&{v30}"(B[1]), "=&{v28}"(B[2]), "=&{v8}"(B[3])
#define QK_BOUT6 "=&{v34}"(B[1]), "=&{v32}"(B[2]), "=&{v30}"(B[3]), "=&{v28}"(B[4]), "=&{v8}"(B[5])
#define QK_BOUT8                                                                                       \
    "=&{v38}"(B[1]), "=&{v36}"(B[2]), "=&{v34}"(B[3]), "=&{v32}"(B[4]), "=&{v30}"(B[5]), "=&{v28}"(B[6]), \
        "=&{v8}"(B[7])
#define QK_BCLOB4 "v31", "v29"
#define QK_BCLOB6 QK_BCLOB4, "v35", "v33"
#define QK_BCLOB8 QK_BCLOB6, "v39", "v37"
// giants: each by x^NB (v8)
#define QK_GIANTS0
#define QK_GIANTS1 QK_LP(10, 11, "v8", "v8")
#define QK_GIANTS2 QK_GIANTS1 QK_LP(12, 13, "v10", "v8")
#define QK_GIANTS3 QK_GIANTS2 QK_LP(14, 15, "v12", "v8")
#define QK_GIANTS4 QK_GIANTS3 QK_LP(16, 17, "v14", "v8")
#define QK_GIANTS5 QK_GIANTS4 QK_LP(18, 19, "v16", "v8")
#define QK_GIANTS6 QK_GIANTS5 QK_LP(20, 21, "v18", "v8")
#define QK_GIANTS7 QK_GIANTS6 QK_LP(22, 23, "v20", "v8")
#define QK_GIANTS8 QK_GIANTS7 QK_LP(24, 25, "v22", "v8")
#define QK_GIANTS9 QK_GIANTS8 QK_LP(26, 27, "v24", "v8")
#define QK_GMIN0
#define QK_GMIN1 "v_min_u32_e32 v9, v9, v10\n\t"
#define QK_GMIN2 "v_min3_u32 v9, v9, v10, v12\n\t"
#define QK_GMIN3 QK_GMIN2 "v_min_u32_e32 v9, v9, v14\n\t"
#define QK_GMIN4 QK_GMIN2 "v_min3_u32 v9, v9, v14, v16\n\t"
#define QK_GMIN5 QK_GMIN4 "v_min_u32_e32 v9, v9, v18\n\t"
#define QK_GMIN6 QK_GMIN4 "v_min3_u32 v9, v9, v18, v20\n\t"
#define QK_GMIN7 QK_GMIN6 "v_min_u32_e32 v9, v9, v22\n\t"
#define QK_GMIN8 QK_GMIN6 "v_min3_u32 v9, v9, v22, v24\n\t"
#define QK_GMIN9 QK_GMIN8 "v_min_u32_e32 v9, v9, v26\n\t"
#define QK_GOUT0
#define QK_GOUT1 , "=&{v10}"(G[0])
#define QK_GOUT2 QK_GOUT1, "=&{v12}"(G[1])
#define QK_GOUT3 QK_GOUT2, "=&{v14}"(G[2])
#define QK_GOUT4 QK_GOUT3, "=&{v16}"(G[3])
#define QK_GOUT5 QK_GOUT4, "=&{v18}"(G[4])
#define QK_GOUT6 QK_GOUT5, "=&{v20}"(G[5])
#define QK_GOUT7 QK_GOUT6, "=&{v22}"(G[6])
#define QK_GOUT8 QK_GOUT7, "=&{v24}"(G[7])
#define QK_GOUT9 QK_GOUT8, "=&{v26}"(G[8])
#define QK_GCLOB0
#define QK_GCLOB1 , "v11"
#define QK_GCLOB2 QK_GCLOB1, "v13"
#define QK_GCLOB3 QK_GCLOB2, "v15"
#define QK_GCLOB4 QK_GCLOB3, "v17"
#define QK_GCLOB5 QK_GCLOB4, "v19"
#define QK_GCLOB6 QK_GCLOB5, "v21"
#define QK_GCLOB7 QK_GCLOB6, "v23"
#define QK_GCLOB8 QK_GCLOB7, "v25"
#define QK_GCLOB9 QK_GCLOB8, "v27"

// B[b] = x^(b+1) for b = 1..NB-1 (lazy), G[g] = x^(NB (g+2)) for g < NG;
// returns the minimum over all of them.  Only the (NB, NG) listed below are
// fused; any other falls back to a statement per product.
template <int NB, int NG>
struct LazyChain {
    static constexpr bool fused = false;
};
#define QK_CHAIN(NB, NG)                                                                               \
    template <>                                                                                        \
    struct LazyChain<NB, NG> {                                                                         \
        static constexpr bool fused = true;                                                            \
        static __device__ __forceinline__ uint32_t run(uint32_t id, uint32_t (&B)[NB],                 \
                                                       uint32_t (&G)[NG ? NG : 1]) {                   \
            uint32_t mn;                                                                               \
            (void)G;                                                                                   \
            asm(QK_BABIES##NB QK_GIANTS##NG QK_BMIN##NB QK_GMIN##NG                                    \
                : "=&{v9}"(mn), QK_BOUT##NB QK_GOUT##NG                                                \
                : [id] "v"(id)                                                                         \
                : "v6", "v7", QK_BCLOB##NB QK_GCLOB##NG, "s58", "s59");                                \
            return mn;                                                                                 \
        }                                                                                              \
    };
#define QK_CHAINS(NB)                                                                                  \
    QK_CHAIN(NB, 0) QK_CHAIN(NB, 1) QK_CHAIN(NB, 2) QK_CHAIN(NB, 3) QK_CHAIN(NB, 4) QK_CHAIN(NB, 5)    \
    QK_CHAIN(NB, 6) QK_CHAIN(NB, 7) QK_CHAIN(NB, 8) QK_CHAIN(NB, 9)
QK_CHAINS(4)
QK_CHAINS(6)
QK_CHAINS(8)

// ---- the nine-power basis (basis32.h) as one statement ----------------------
// The same window and rules as LazyChain: Q in v[6:7], each result in the even
// register of its own pair v[8:9] .. v[22:23] (V[1] .. V[8] in the order of
// basis32::CHAIN), the odd halves clobbered, carry-outs to s[58:59].  The text
// below is basis32::CHAIN written out (checked underneath): 2 = 1+1, 3 = 2+1,
// 6 = 3+3, 8 = 6+2, 12 = 6+6, 16 = 8+8, 13 = 12+1, 15 = 12+3.  The chain
// carries no wrap check: the ids it gets wrong are known (basis_filter.h).
// QK_BASIS_CHAIN_MIN is the form of CfgBasis<.., 0>: the minimum of the eight
// results formed in the dead v9.
#define QK_BASIS_CHAIN                                                                                 \
    QK_LP(8, 9, "%[id]", "%[id]")                                                                      \
    QK_LP(10, 11, "v8", "%[id]")                                                                       \
    QK_LP(12, 13, "v10", "v10")                                                                        \
    QK_LP(14, 15, "v12", "v8")                                                                         \
    QK_LP(16, 17, "v12", "v12")                                                                        \
    QK_LP(18, 19, "v14", "v14")                                                                        \
    QK_LP(20, 21, "v16", "%[id]")                                                                      \
    QK_LP(22, 23, "v16", "v10")
#define QK_BASIS_CHAIN_MIN                                                                             \
    QK_BASIS_CHAIN                                                                                     \
    "v_min3_u32 v9, v8, v10, v12\n\t"                                                                  \
    "v_min3_u32 v9, v9, v14, v16\n\t"                                                                  \
    "v_min3_u32 v9, v9, v18, v20\n\t"                                                                  \
    "v_min_u32_e32 v9, v9, v22\n\t"
constexpr bool basis_chain_is(const uint8_t (&t)[3 * basis32::NP]) {
    for (int i = 0; i < basis32::NP; ++i)
        if (basis32::CHAIN[i].power != t[3 * i] || basis32::CHAIN[i].left != t[3 * i + 1] ||
            basis32::CHAIN[i].right != t[3 * i + 2])
            return false;
    return true;
}
static_assert(basis_chain_is({2, 1, 1, 3, 2, 1, 6, 3, 3, 8, 6, 2, 12, 6, 6, 16, 8, 8, 13, 12, 1, 15, 12, 3}),
              "QK_BASIS_CHAIN is basis32::CHAIN written out");
// V[0] = id, V[i + 1] = the chain's step i (lazy)
__device__ __forceinline__ void basis_chain(uint32_t id, uint32_t (&V)[basis32::NE]) {
    V[0] = id;
    asm(QK_BASIS_CHAIN
        : "=&{v8}"(V[1]), "=&{v10}"(V[2]), "=&{v12}"(V[3]), "=&{v14}"(V[4]), "=&{v16}"(V[5]), "=&{v18}"(V[6]),
          "=&{v20}"(V[7]), "=&{v22}"(V[8])
        : [id] "v"(id)
        : "v6", "v7", "v9", "v11", "v13", "v15", "v17", "v19", "v21", "v23", "s58", "s59");
}
// ... and returns their minimum
__device__ __forceinline__ uint32_t basis_chain_min(uint32_t id, uint32_t (&V)[basis32::NE]) {
    uint32_t mn;
    V[0] = id;
    asm(QK_BASIS_CHAIN_MIN
        : "=&{v9}"(mn), "=&{v8}"(V[1]), "=&{v10}"(V[2]), "=&{v12}"(V[3]), "=&{v14}"(V[4]), "=&{v16}"(V[5]),
          "=&{v18}"(V[6]), "=&{v20}"(V[7]), "=&{v22}"(V[8])
        : [id] "v"(id)
        : "v6", "v7", "v11", "v13", "v15", "v17", "v19", "v21", "v23", "s58", "s59");
    return mn;
}

// ---- the id filter (basis_filter.h) -----------------------------------------
// The table waits in device memory; every workgroup copies it into LDS once,
// before its first trip (filter_load), and an id's test is one v_and (the
// entry's byte address), one ds_read_b32 and one v_xor: filter_diff(id) is
// below basis_filter::WINDOW iff the id is a candidate.
static __device__ const basis_filter::Table FILTER_TABLE = basis_filter::TABLE;
__device__ __forceinline__ uint32_t *filter_lds() {
    __shared__ __attribute__((aligned(16))) uint32_t tab[basis_filter::SLOTS];
    return tab;
}
__device__ __forceinline__ void filter_load() {
    static_assert(basis_filter::SLOTS % (4 * BLOCK) == 0, "whole 16-byte copies per thread");
    uint4 *dst = reinterpret_cast<uint4 *>(filter_lds());
    const uint4 *src = reinterpret_cast<const uint4 *>(FILTER_TABLE.e);
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)basis_filter::SLOTS / 4; i += BLOCK) dst[i + threadIdx.x] = src[i + threadIdx.x];
    __syncthreads();
}
__device__ __forceinline__ uint32_t filter_diff(uint32_t id) {
    const char *tab = reinterpret_cast<const char *>(filter_lds());
    return *reinterpret_cast<const uint32_t *>(tab + (id & basis_filter::KEY_MASK)) ^ id;
}

// powers of one id; returns a value below WRAP_BELOW if a lazy fold may have
// wrapped (the caller then recomputes exactly): the minimum of the products
// (a wrapped fold leaves a value < 25, field.h).  The comparison is the caller's, so that it can
// place an instruction between the chain's statement and the v_cmp that reads
// its result (hipcc pads one s_nop there otherwise).
// OFF: A[a] = x^(base + a*NB).
constexpr uint32_t WRAP_BELOW = 25u;
template <class C>
__device__ __forceinline__ uint32_t powers(uint32_t id, uint32_t (&B)[C::NB], uint32_t (&A)[C::ROWS],
                                           uint32_t base = 0, uint32_t xb = 0, uint32_t *xnext = nullptr) {
    constexpr int NB = C::NB, NA = C::NA;
    B[0] = id;
    if constexpr (C::OFF) {
        uint32_t mn = 0xFFFFFFFFu;
        if constexpr (LazyChain<NB, 0>::fused) {
            uint32_t G[1];
            mn = LazyChain<NB, 0>::run(id, B, G);
        } else {
#pragma unroll
            for (int b = 1; b < NB; ++b) B[b] = mulfold32_min(B[b - 1], B[0], mn);
        }
        const uint32_t xn = B[NB - 1];                                   // x^NB (B[b] = x^(b+1))
        if constexpr (C::XC & 1) A[0] = xb;
        else A[0] = pow_uniform(xn, base / NB, [&](uint32_t u, uint32_t v) { return mulfold32_min(u, v, mn); });
#pragma unroll
        for (int a = 1; a < NA; ++a) A[a] = mulfold32_min(A[a - 1], xn, mn);
        if constexpr ((C::XC & 2) != 0) *xnext = mulfold32_min(A[NA - 1], xn, mn);
        return mn;
    } else {
        // giants after x^NB, and the next pass's x^(NB NA) as one more of them
        constexpr int NG = NA - 2 + ((C::XC & 2) != 0 ? 1 : 0);
        if constexpr (LazyChain<NB, NG>::fused) {
            uint32_t G[NG ? NG : 1];
            const uint32_t mn = LazyChain<NB, NG>::run(id, B, G);
            A[0] = B[NB - 1];
#pragma unroll
            for (int a = 1; a < NA - 1; ++a) A[a] = G[a - 1];
            if constexpr ((C::XC & 2) != 0) *xnext = G[NA - 2];
            return mn;
        }
        uint32_t mn = 0xFFFFFFFFu;
#pragma unroll
        for (int b = 1; b < NB; ++b) B[b] = mulfold32_min(B[b - 1], B[0], mn);
        A[0] = B[NB - 1];
#pragma unroll
        for (int a = 1; a < NA - 1; ++a) A[a] = mulfold32_min(A[a - 1], A[0], mn);
        if constexpr ((C::XC & 2) != 0) *xnext = mulfold32_min(A[NA - 2], A[0], mn);   // x^(NB NA)
        return mn;
    }
}
template <class C>
__device__ __forceinline__ void powers_exact(uint32_t (&B)[C::NB], uint32_t (&A)[C::ROWS], uint32_t base = 0,
                                             uint32_t xb = 0, uint32_t *xnext = nullptr) {
#pragma unroll
    for (int b = 1; b < C::NB; ++b) B[b] = mulfold32_exact(B[b - 1], B[0]);
    if constexpr (C::OFF) {
        const uint32_t xn = B[C::NB - 1];
        if constexpr (C::XC & 1) A[0] = xb;
        else A[0] = pow_uniform(xn, base / C::NB, [](uint32_t u, uint32_t v) { return mulfold32_exact(u, v); });
#pragma unroll
        for (int a = 1; a < C::NA; ++a) A[a] = mulfold32_exact(A[a - 1], xn);
        if constexpr ((C::XC & 2) != 0) *xnext = mulfold32_exact(A[C::NA - 1], xn);
        return;
    }
    A[0] = B[C::NB - 1];
#pragma unroll
    for (int a = 1; a < C::NA - 1; ++a) A[a] = mulfold32_exact(A[a - 1], A[0]);
    if constexpr ((C::XC & 2) != 0) *xnext = mulfold32_exact(A[C::NA - 2], A[0]);
}

// Groups are issued in the order row 0, row 1, ... and alternate carry-SGPR
// sets (group index parity), so no two adjacent blocks share SGPRs.
template <class C>
__device__ __forceinline__ void accumulate(Acc<C::NB, C::NA, C::ROWS> &S, const uint32_t (&B)[C::NB],
                                           const uint32_t (&A)[C::ROWS]) {
    constexpr int NB = C::NB;
    if constexpr (!C::OFF) {   // the a = 0 sum row (an offset pass has none)
#pragma unroll
        for (int b = 0; b + 4 <= NB; b += 4) {
            if ((b / 4) % 2 == 0) row4m<0>(S.r0[b], S.r0[b + 1], S.r0[b + 2], S.r0[b + 3], B[b], B[b + 1], B[b + 2], B[b + 3]);
            else row4m<1>(S.r0[b], S.r0[b + 1], S.r0[b + 2], S.r0[b + 3], B[b], B[b + 1], B[b + 2], B[b + 3]);
        }
        if constexpr (NB % 4 == 2) row2m(S.r0[NB - 2], S.r0[NB - 1], B[NB - 2], B[NB - 1]);
    }
    if constexpr (C::PRIO) __builtin_amdgcn_s_setprio(2);   // row 0 at 1, the MAC rows at 2
#pragma unroll
    for (int a = 0; a < C::ROWS; ++a) {
#pragma unroll
        for (int b = 0; b + 4 <= NB; b += 4) {
            const int g = (a + C::ROW1) * (NB / 4) + b / 4;   // group index: parity picks the SGPR set
            if (scalar_group<C>(a + C::ROW1, b)) {
                if (g % 2 == 0)
                    mac4s<0>(S.m[a][b], S.m[a][b + 1], S.m[a][b + 2], S.m[a][b + 3], S.c[a][b], S.c[a][b + 1],
                             S.c[a][b + 2], S.c[a][b + 3], A[a], B[b], B[b + 1], B[b + 2], B[b + 3]);
                else
                    mac4s<1>(S.m[a][b], S.m[a][b + 1], S.m[a][b + 2], S.m[a][b + 3], S.c[a][b], S.c[a][b + 1],
                             S.c[a][b + 2], S.c[a][b + 3], A[a], B[b], B[b + 1], B[b + 2], B[b + 3]);
            } else {
                if (g % 2 == 0)
                    mac4v<0>(S.m[a][b], S.m[a][b + 1], S.m[a][b + 2], S.m[a][b + 3], S.c[a][b], S.c[a][b + 1],
                             S.c[a][b + 2], S.c[a][b + 3], A[a], B[b], B[b + 1], B[b + 2], B[b + 3]);
                else
                    mac4v<1>(S.m[a][b], S.m[a][b + 1], S.m[a][b + 2], S.m[a][b + 3], S.c[a][b], S.c[a][b + 1],
                             S.c[a][b + 2], S.c[a][b + 3], A[a], B[b], B[b + 1], B[b + 2], B[b + 3]);
            }
        }
        if constexpr (NB % 4 == 2)
            mac2v(S.m[a][NB - 2], S.m[a][NB - 1], S.c[a][NB - 2], S.c[a][NB - 1], A[a], B[NB - 2], B[NB - 1]);
    }
}

// The basis form's accumulation, in the grid form's shape: two groups of four direct
// adds (the x1 form, priority 1), then six groups of four pair MACs whose
// wraps are counted on the scalar unit (priority 2), alternating SGPR sets.
// Direct accumulator i is S.r0[i], pair accumulator i is S.m[i / 8][i % 8];
// their powers are basis32::DIRECT[i] and basis32::MAC[i] (finish()).
template <class C, int G>
__device__ __forceinline__ void basis_direct4(Acc<8, 4, 3> &S, const uint32_t (&V)[basis32::NE]) {
    constexpr int i = 4 * G;
    row4m<G % 2>(S.r0[i], S.r0[i + 1], S.r0[i + 2], S.r0[i + 3], V[basis32::direct_v(i)],
                 V[basis32::direct_v(i + 1)], V[basis32::direct_v(i + 2)], V[basis32::direct_v(i + 3)]);
}
template <class C, int G>
__device__ __forceinline__ void basis_mac4(Acc<8, 4, 3> &S, const uint32_t (&V)[basis32::NE]) {
    constexpr int i = 4 * G, a = i / 8, b = i % 8;
    static_assert(scalar_group<C>(a + 1, b), "basis form: pair MACs are scalar-counted");
    mac4ps<G % 2>(S.m[a][b], S.m[a][b + 1], S.m[a][b + 2], S.m[a][b + 3], S.c[a][b], S.c[a][b + 1], S.c[a][b + 2],
                  S.c[a][b + 3], V[basis32::mac_l(i)], V[basis32::mac_r(i)], V[basis32::mac_l(i + 1)],
                  V[basis32::mac_r(i + 1)], V[basis32::mac_l(i + 2)], V[basis32::mac_r(i + 2)],
                  V[basis32::mac_l(i + 3)], V[basis32::mac_r(i + 3)]);
}
template <class C>
__device__ __forceinline__ void accumulate_basis(Acc<8, 4, 3> &S, const uint32_t (&V)[basis32::NE]) {
    static_assert(basis32::ND == 8 && basis32::NM == 24, "two direct groups, six pair groups");
    basis_direct4<C, 0>(S, V);
    basis_direct4<C, 1>(S, V);
    if constexpr (C::PRIO) __builtin_amdgcn_s_setprio(2);
    basis_mac4<C, 0>(S, V);
    basis_mac4<C, 1>(S, V);
    basis_mac4<C, 2>(S, V);
    basis_mac4<C, 3>(S, V);
    basis_mac4<C, 4>(S, V);
    basis_mac4<C, 5>(S, V);
}
// the power (1..32) held by the accumulator that finish() numbers (a, b)
constexpr int basis_slot_power(int a, int b) {
    return a == 0 ? basis32::DIRECT[b] : basis32::MAC[(a - 1) * 8 + b];
}

// wave priority around an id's accumulation (Cfg PRIO; accumulate raises it
// further before the MAC rows)
template <class C> __device__ __forceinline__ void prio_enter() {
    if constexpr (C::PRIO) __builtin_amdgcn_s_setprio(1);
}
template <class C> __device__ __forceinline__ void prio_exit() {
    if constexpr (C::PRIO) __builtin_amdgcn_s_setprio(0);
}

// The filtered basis form (CfgBasis FILT).  A trip whose filter test found
// nothing runs the lazy chain for its four ids and accumulates.  In a trip
// with a candidate, the candidates are taken out first (basis_candidates):
// where some lane's id is one, those lanes run the exact chain (always
// congruent, so a candidate that is not wrong costs only this) while the
// others feed id 0, whose powers are all 0, and the id is replaced by 0 for
// the lazy pass that follows.  EXEC is full at every accumulation.
template <class C>
__device__ __forceinline__ void basis_one_lazy(Acc<8, 4, 3> &S, uint32_t id) {
    uint32_t V[basis32::NE];
    basis_chain(id, V);
    prio_enter<C>();
    if constexpr (C::PRIO) __builtin_amdgcn_sched_barrier(0);
    accumulate_basis<C>(S, V);
    prio_exit<C>();
}
template <class C>
__device__ __forceinline__ void basis_candidates(Acc<8, 4, 3> &S, uint32_t &id) {
    const bool c = filter_diff(id) < basis_filter::WINDOW;
    if (!__any(c)) return;
    uint32_t V[basis32::NE];
#pragma unroll
    for (int i = 0; i < basis32::NE; ++i) V[i] = 0;
    if (c) basis32::chain_exact(id, V);
    prio_enter<C>();
    accumulate_basis<C>(S, V);
    prio_exit<C>();
    id = c ? 0u : id;
}

// xb / xnext: an offset pass's cached x^base and the next pass's (Cfg XC)
template <class C>
__device__ __forceinline__ void one(Acc<C::NB, C::NA, C::ROWS> &S, uint32_t id, uint32_t base = 0, uint32_t xb = 0,
                                    uint32_t *xnext = nullptr) {
    if constexpr (C::BASIS && C::FILT) {   // a single id (head, tail): its own filter test
        basis_candidates<C>(S, id);
        basis_one_lazy<C>(S, id);
        return;
    } else if constexpr (C::BASIS) {   // the same steps over the basis's nine values
        uint32_t V[basis32::NE];
        const uint32_t mn = basis_chain_min(id, V);
        prio_enter<C>();
        if constexpr (C::PRIO) __builtin_amdgcn_sched_barrier(0);
        const bool w = mn < WRAP_BELOW;
        if (__builtin_expect(__any(w), 0)) {
            if (w) basis32::chain_exact(id, V);
        }
        accumulate_basis<C>(S, V);
        prio_exit<C>();
        return;
    }
    uint32_t B[C::NB], A[C::ROWS];
    const uint32_t mn = powers<C>(id, B, A, base, xb, xnext);
    // the priority change sits between the chain and the wrap check that reads
    // its minimum, where an s_nop would stand otherwise (the rare redo runs at
    // the accumulation's priority)
    prio_enter<C>();
    if constexpr (C::PRIO) __builtin_amdgcn_sched_barrier(0);
    const bool w = mn < WRAP_BELOW;
    if (__builtin_expect(__any(w), 0)) {
        if (w) powers_exact<C>(B, A, base, xb, xnext);
    }
    accumulate<C>(S, B, A);
    prio_exit<C>();
}

template <class C>
__device__ __forceinline__ void four(Acc<C::NB, C::NA, C::ROWS> &S, uint4 w, uint32_t base,
                                     uint4 xb = make_uint4(0, 0, 0, 0), uint4 *xn = nullptr) {
    if constexpr (C::BASIS && C::FILT) {
        // one test per trip, before the chains: the smallest of the four differences
        const uint32_t d0 = filter_diff(w.x), d1 = filter_diff(w.y), d2 = filter_diff(w.z), d3 = filter_diff(w.w);
        const uint32_t d01 = d0 < d1 ? d0 : d1, d23 = d2 < d3 ? d2 : d3;
        if (__builtin_expect(__any((d01 < d23 ? d01 : d23) < basis_filter::WINDOW), 0)) {
            // rare: the candidates first, on their own (the other lanes feed id 0), then id 0 in their place
            basis_candidates<C>(S, w.x);
            basis_candidates<C>(S, w.y);
            basis_candidates<C>(S, w.z);
            basis_candidates<C>(S, w.w);
        }
        basis_one_lazy<C>(S, w.x);
        basis_one_lazy<C>(S, w.y);
        basis_one_lazy<C>(S, w.z);
        basis_one_lazy<C>(S, w.w);
    } else {
        uint4 t = make_uint4(0, 0, 0, 0);
        one<C>(S, w.x, base, xb.x, &t.x);
        one<C>(S, w.y, base, xb.y, &t.y);
        one<C>(S, w.z, base, xb.z, &t.z);
        one<C>(S, w.w, base, xb.w, &t.w);
        if constexpr ((C::XC & 2) != 0) *xn = t;
    }
}

// Lane partials -> wave butterfly -> LDS -> one sum per power for the
// workgroup: out(m, s) receives power m + 1's sum (< 2^40) in thread m.
// tid: the thread's index in the workgroup (body_gen passes one rebuilt after
// its loops, so that threadIdx.x holds no register across them).
template <class C, class Out>
__device__ __forceinline__ void finish(const Acc<C::NB, C::NA, C::ROWS> &S, uint32_t T, Out out,
                                       uint32_t tid = threadIdx.x) {
    constexpr int NB = C::NB, NA = C::NA;
    __shared__ uint64_t sm[WAVES * NB * NA];
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            // the sum row's value is its 64-bit sum; a MAC row's is m + c * 2^64
            // with 2^64 == 25; a scalar-counted c is the wave's total, added
            // once (by lane 0)
            uint64_t x;
            if (!C::OFF && a == 0) {
                x = S.r0[b];
            } else {
                const uint32_t c = S.c[a - C::ROW1][b];
                const uint32_t cl = scalar_group<C>(a, b) ? (lane == 0 ? c : 0u) : c;
                x = (uint64_t)fold64_32(S.m[a - C::ROW1][b]) + fold64_32((uint64_t)cl * 25u);
            }
            x = fold64_32(x);                                                         // < 2^32
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) x += shfl_xor_u64(x, off);        // < 2^38
            // sm is indexed by power - 1: the grid's a * NB + b, the basis's from its table
            const int m = C::BASIS ? basis_slot_power(a, b) - 1 : a * NB + b;
            if (lane == 0) sm[wave * (NB * NA) + m] = x;
        }
    }
    __syncthreads();
    for (uint32_t m = tid; m < T; m += BLOCK) {
        uint64_t s = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) s += sm[w * (NB * NA) + m];
        out(m, s);
    }
}

// The kernel body: grid-stride over 16-byte groups of ids (+ unaligned head
// and tail), then lane partials -> wave butterfly -> LDS -> one partial per
// (power, block) stored [power][block].
//
// Every lane of a wave runs the wave's trip count (lane 0 has the largest):
// lanes past their range feed id 0, whose powers are all 0, so EXEC is full
// at every scalar-counted op.  The loop is split: while every lane of the
// wave still has a next group, the prefetch is unconditional; the last <= 2
// trips take the masked form.  Per-lane 32-bit trip counts (the host
// guarantees body / nthr < 2^32).
// body_gen: the ids are walked by `nthr` threads of which this is `gtid`
// (the whole grid for the headline kernel, one workgroup for a flow's work
// item); out(m, s) receives the workgroup's sum for power m + 1 (< 2^40) in
// thread m (an offset pass: power base + m + 1).
template <class C>
__device__ __forceinline__ void clear(Acc<C::NB, C::NA, C::ROWS> &S) {
#pragma unroll
    for (int b = 0; b < C::NB; ++b) {
        S.r0[b] = 0;
#pragma unroll
        for (int a = 0; a < C::ROWS; ++a) { S.m[a][b] = 0; S.c[a][b] = 0; }
    }
}

// XC (offset passes): xin / xout are per-id arrays indexed like ids whose
// address is congruent to ids' modulo 16 (the same 16-byte groups).  The
// middle passes read and write the same cache (xin == xout): not restrict —
// each element is read one iteration before its own write, and the source
// order (next load, compute, this store) is the order kept.
template <class C, class Out>
__device__ __forceinline__ void body_gen(const uint32_t *__restrict__ ids, uint64_t n, uint32_t head, uint32_t T,
                                         uint64_t gtid, uint64_t nthr, Out out, uint32_t base = 0,
                                         const uint32_t *xin = nullptr,
                                         uint32_t *xout = nullptr) {
    constexpr bool XI = (C::XC & 1) != 0, XO = (C::XC & 2) != 0;
    Acc<C::NB, C::NA, C::ROWS> S;
    clear<C>(S);
    if constexpr (C::BASIS && C::FILT) filter_load();
    // The loops below leave two or three VGPRs to values that only the head,
    // the tail and finish() read.  gtid - threadIdx.x is the same in every
    // lane (both callers: a workgroup's first thread), so it and the wave's
    // number wait in SGPRs, and the thread's index is rebuilt from the lane
    // number after the loops instead of being kept.
    const uint64_t gbase64 = gtid - threadIdx.x;
    const uint32_t gb_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)gbase64);
    const uint32_t gb_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(gbase64 >> 32));
    const uint32_t wave_s = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t h = head < n ? head : n;
    const uint64_t nbody = (n - h) >> 2;
    const uint4 *__restrict__ v = reinterpret_cast<const uint4 *>(ids + h);
    const uint32_t iters = gtid < nbody ? (uint32_t)((nbody - gtid + nthr - 1) / nthr) : 0u;
    const uint32_t tmax = (uint32_t)__builtin_amdgcn_readfirstlane(iters);           // lane 0: most trips
    const uint32_t tmin = (uint32_t)__builtin_amdgcn_readlane((int)iters, 63);       // lane 63: fewest
    const uint4 *__restrict__ p = v + gtid;
    const uint4 *pc = XI ? reinterpret_cast<const uint4 *>(xin + h) + gtid : nullptr;
    uint4 *po = XO ? reinterpret_cast<uint4 *>(xout + h) + gtid : nullptr;
    // A lane's group number `it` exists (it < iters) iff p < vend at that trip:
    // the masked trips test the pointer the loop carries anyway, against a
    // wave-uniform end, so the trip count holds no VGPR across the main loop.
    const uint4 *const vend = v + nbody;
    uint4 nxt = make_uint4(0, 0, 0, 0), nxc = make_uint4(0, 0, 0, 0), xo = make_uint4(0, 0, 0, 0);
    if (p < vend) {
        nxt = *p;
        if constexpr (XI) nxc = *pc;
    }
    uint32_t it = 0;
    for (; it + 1 < tmin; ++it) {
        const uint4 w = nxt, c = nxc;
        p += nthr;
        nxt = *p;
        if constexpr (XI) {
            pc += nthr;
            nxc = *pc;
        }
        four<C>(S, w, base, c, &xo);
        if constexpr (XO) {
            *po = xo;
            po += nthr;
        }
    }
    for (; it < tmax; ++it) {
        const uint4 w = nxt, c = nxc;
        const bool cur = p < vend;
        p += nthr;
        nxt = make_uint4(0, 0, 0, 0);
        if (p < vend) nxt = *p;
        if constexpr (XI) {
            pc += nthr;
            if (p < vend) nxc = *pc;
        }
        four<C>(S, w, base, c, &xo);
        if constexpr (XO) {
            if (cur) *po = xo;
            po += nthr;
        }
        (void)cur;
    }
    const uint64_t tail0 = h + (nbody << 2);
    const uint32_t tid = wave_s * 64u + __lane_id();
    gtid = (((uint64_t)gb_hi << 32) | gb_lo) + tid;
    {
        const bool in = gtid < h;
        uint32_t xn = 0;
        one<C>(S, in ? ids[gtid] : 0u, base, XI && in ? xin[gtid] : 0u, &xn);
        if (XO && in) xout[gtid] = xn;
    }
    {
        const bool in = gtid < n - tail0;
        uint32_t xn = 0;
        one<C>(S, in ? ids[tail0 + gtid] : 0u, base, XI && in ? xin[tail0 + gtid] : 0u, &xn);
        if (XO && in) xout[tail0 + gtid] = xn;
    }

    finish<C>(S, T, out, tid);
}

// the headline kernel's form: grid-stride, one partial per (power, block)
// stored [power][block]
template <class C>
__device__ __forceinline__ void body(const uint32_t *__restrict__ ids, uint64_t n, uint32_t head, uint32_t T,
                                     uint64_t *__restrict__ partials, uint32_t base = 0,
                                     const uint32_t *xin = nullptr, uint32_t *xout = nullptr) {
    body_gen<C>(
        ids, n, head, T, (uint64_t)blockIdx.x * BLOCK + threadIdx.x, (uint64_t)gridDim.x * BLOCK,
        [=](uint32_t m, uint64_t s) { partials[(size_t)m * gridDim.x + blockIdx.x] = s; }, base, xin, xout);
}

// ---- dynamic form: waves claim chunks of ids (DESIGN.md §3.2 "Grid") --------
// A chunk is DYN_CH consecutive 16-byte groups per lane for the 64 lanes of a
// wave: group j of chunk c for lane l is v[(c DYN_CH + j) 64 + l], a coalesced
// 1 KB per wave and load.  A wave takes its chunks from a counter (one of
// DYN_NCTR, below): lane 0 adds 1 (relaxed, agent scope) and the wave reads the result into SGPRs.  The
// counter only ever grows; the launch's claims are numbered from a base that
// the host keeps: every wave ends with exactly one claim past the counter's
// chunks, so a launch of W waves moves it by those chunks + W.  Nothing is
// reset and no wave waits for another.
//
// A wave claims chunk k+1 before it walks chunk k (the atomic's round trip is
// then covered by the SIMD's other waves, which are in their own chunks; the
// result goes straight to SGPRs, so the claim holds no VGPR across an id), and
// the last trip of a chunk prefetches the first group of the next one.  Every
// trip over a claimed chunk is the unmasked form: all 64 lanes have a group.
// What is no whole chunk — the groups past the last one, the unaligned head
// and the tail — is walked once per launch, by the wave whose claim returns
// exactly the number of chunks, with body_gen's masked form (lanes without
// work feed id 0).  A workgroup whose waves claim nothing stores zero partials.
// Plain single-pass configurations only (no offset pass, no x^base cache).
#ifndef QK_DYN_CH
#define QK_DYN_CH 16   // groups per lane and claim (4 096 ids per chunk)
#endif
constexpr int DYN_CH = QK_DYN_CH;
constexpr uint32_t DYN_GROUPS = DYN_CH * 64;   // 16-byte groups per chunk (4 ids each)

// The claim as one statement: lane 0 alone adds 1 to the counter and the
// returned value goes straight to SGPRs, so no VGPR is held across the chunk
// (hipcc's own rendering of the atomic keeps a lane index and the returned
// pair in VGPRs across the loop: 8 more VGPRs, and spills in the headline
// kernel).  v[6:7] is the power chain's scratch pair and s[58:59] its dead
// carry pair; the wait also covers the prefetched group.
__device__ __forceinline__ uint64_t claim_chunk(unsigned long long *ctr, uint64_t cbase) {
    uint32_t lo, hi;
    asm volatile("v_mov_b32_e32 v6, 1\n\t"
                 "v_mov_b32_e32 v7, 0\n\t"
                 "s_mov_b64 s[58:59], exec\n\t"
                 "s_mov_b64 exec, 1\n\t"
                 "global_atomic_add_x2 v[6:7], v7, v[6:7], %[ctr] sc0\n\t"
                 "s_mov_b64 exec, s[58:59]\n\t"
                 "s_waitcnt vmcnt(0)\n\t"
                 "v_readfirstlane_b32 %[lo], v6\n\t"
                 "v_readfirstlane_b32 %[hi], v7"
                 : [lo] "=s"(lo), [hi] "=s"(hi)
                 : [ctr] "s"(ctr)
                 : "v6", "v7", "s58", "s59", "memory");
    return (((uint64_t)hi << 32) | lo) - cbase;
}

// A chunk's groups are read through a buffer resource on the chunk (base and
// size in SGPRs): the lane's 16-byte slot is the only VGPR an address needs,
// and the group's number within the chunk is a scalar offset.
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t chunk_rsrc(const char *vb, uint64_t g) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(vb + g * 16u), 0, (int)(DYN_GROUPS * 16u),
                                             0x00020000);
}
__device__ __forceinline__ uint4 chunk_group(__amdgpu_buffer_rsrc_t rs, uint32_t slot, uint32_t j) {
    const u32x4_t w = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)slot, (int)(j * 1024u), 0);
    return make_uint4(w.x, w.y, w.z, w.w);
}

// One counter serves about 8e7 claims per second whoever asks (agent-scope
// atomics on one address, measured: 12.5 ns per claim at 4.9e5 and at 2.4e5
// claims per launch), which 4 096-id chunks of a 1e9-id launch exceed.  The
// chunks are therefore split into DYN_NCTR contiguous regions with a counter
// each, DYN_CTR_STRIDE words apart.  A wave starts at the counter of its
// workgroup's number and moves on to the next one when a claim fails, until
// it has failed once at every counter: each counter moves by its region's
// chunks + the launch's waves.  The wave whose claim at counter 0 returns
// exactly that region's length walks the ragged rest at its end.
constexpr int DYN_NCTR = 8;
constexpr int DYN_CTR_STRIDE = 544;   // u64 words: 4 KB + 256 B, another channel whatever the interleave
struct DynArgs {
    unsigned long long *ctr;      // counter k at ctr[k * DYN_CTR_STRIDE]
    uint64_t region;              // chunks per region: ceil(nchunks / DYN_NCTR)
    uint64_t base[DYN_NCTR];      // the counters' values before this launch
};
// chunks of region k (host and device)
__host__ __device__ inline uint64_t dyn_region_len(uint64_t nchunks, uint64_t region, uint32_t k) {
    const uint64_t lo = (uint64_t)k * region;
    return lo >= nchunks ? 0 : (nchunks - lo < region ? nchunks - lo : region);
}

template <class C>
__device__ __forceinline__ void body_dyn(const uint32_t *__restrict__ ids, uint64_t n, uint32_t head, uint32_t T,
                                         uint64_t *__restrict__ partials, const DynArgs &da) {
    static_assert(!C::OFF && C::XC == 0, "dynamic chunks: plain single-pass configurations");
    Acc<C::NB, C::NA, C::ROWS> S;
    clear<C>(S);
    if constexpr (C::BASIS && C::FILT) filter_load();
    // as body_gen: the wave's number waits in an SGPR and the thread's index
    // is rebuilt after the loops
    const uint32_t wave_s = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t h = head < n ? head : n;
    const uint64_t nbody = (n - h) >> 2;
    const uint64_t nchunks = nbody / DYN_GROUPS;
    const char *vb = reinterpret_cast<const char *>(ids + h);
    const uint32_t slot = __lane_id() * 16u;
    constexpr uint64_t NONE = ~0ull;
    // the claim state is wave-uniform (SGPRs)
    uint32_t k = blockIdx.x % (uint32_t)DYN_NCTR, failed = 0;
    bool rest_mine = false;
    auto claim = [&]() -> uint64_t {
        while (failed < (uint32_t)DYN_NCTR) {
            const uint64_t idx = claim_chunk(da.ctr + (size_t)k * DYN_CTR_STRIDE, da.base[k]);
            const uint64_t len = dyn_region_len(nchunks, da.region, k);
            if (idx < len) return (uint64_t)k * da.region + idx;
            if (k == 0 && idx == len) rest_mine = true;
            k = k + 1 == (uint32_t)DYN_NCTR ? 0u : k + 1;
            ++failed;
        }
        return NONE;
    };
    uint4 nxt = make_uint4(0, 0, 0, 0);
    uint64_t cur = claim();
    __amdgpu_buffer_rsrc_t rs = chunk_rsrc(vb, 0);
    if (cur != NONE) {
        rs = chunk_rsrc(vb, cur * DYN_GROUPS);
        nxt = chunk_group(rs, slot, 0);
    }
    while (cur != NONE) {
        const uint64_t next = claim();
        for (uint32_t j = 1; j < (uint32_t)DYN_CH; ++j) {
            const uint4 w = nxt;
            nxt = chunk_group(rs, slot, j);
            four<C>(S, w, 0);
        }
        const uint4 w = nxt;
        if (next != NONE) {
            rs = chunk_rsrc(vb, next * DYN_GROUPS);
            nxt = chunk_group(rs, slot, 0);
        }
        four<C>(S, w, 0);
        cur = next;
    }
    if (rest_mine) {   // one wave of the launch: the ragged rest, masked
        const uint32_t lane = __lane_id();
        const uint32_t rest = (uint32_t)(nbody - nchunks * DYN_GROUPS);   // < DYN_GROUPS
        rs = chunk_rsrc(vb, nchunks * DYN_GROUPS);
        nxt = make_uint4(0, 0, 0, 0);
        if (lane < rest) nxt = chunk_group(rs, slot, 0);
        for (uint32_t j = 0; j * 64u < rest; ++j) {   // <= DYN_CH trips
            const uint4 w = nxt;
            nxt = make_uint4(0, 0, 0, 0);
            if ((j + 1) * 64u + lane < rest) nxt = chunk_group(rs, slot, j + 1);
            four<C>(S, w, 0);
        }
        const uint64_t tail0 = h + (nbody << 2);
        one<C>(S, lane < h ? ids[lane] : 0u);
        one<C>(S, lane < n - tail0 ? ids[tail0 + lane] : 0u);
    }
    finish<C>(
        S, T, [=](uint32_t m, uint64_t s) { partials[(size_t)m * gridDim.x + blockIdx.x] = s; },
        wave_s * 64u + __lane_id());
}

} // namespace bsgs
} // namespace qk
