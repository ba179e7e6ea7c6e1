// basis32.h — the nine-power basis of the u32 t = 31..32 encode (DESIGN.md
// §3.2 "Basis"), as data.  Plain C++17: bsgs.h builds the kernel's chain and
// accumulation from these tables, and the host compiles the same file without
// HIP (tests/native/basis_check.cpp), like field.h.
//
// E = {1, 2, 3, 6, 8, 12, 13, 15, 16}: 1 is the id, every other element is
// the product of two earlier ones (one lazy product each, eight in all), and
// every power 1..32 is an element of E or the product of two.  An exhaustive
// search finds no such set of eight elements for 32 powers; of the 31 sets of
// nine this one has the shallowest chain (depth 5).
//
// An id therefore costs 8 lazy products, 8 direct adds (elements of E) and 24
// multiply-accumulates (pairs): E has nine elements, so one of them (x^2) is
// accumulated as a pair, 1 + 1.
#pragma once
#include <stdint.h>

#include "field.h"

namespace qk {
namespace basis32 {

constexpr int T = 32;    // powers 1..T
constexpr int NE = 9;    // |E|
constexpr int NP = 8;    // lazy products per id
constexpr int ND = 8;    // accumulators fed by an element of E as it is
constexpr int NM = 24;   // accumulators fed by the product of two elements

// x^power = x^left * x^right, in the order the products are issued: no step
// directly follows the one it depends on where the order allows (8 and 12
// both need 6; 16 needs 8; 13 and 15 need 12).  V[0] = x, V[i + 1] = step i.
struct Step {
    uint8_t power, left, right;
};
constexpr Step CHAIN[NP] = {{2, 1, 1},  {3, 2, 1},  {6, 3, 3},   {8, 6, 2},
                            {12, 6, 6}, {16, 8, 8}, {13, 12, 1}, {15, 12, 3}};

// for each power 1..32 its operand pair; right == 0: direct (left == power)
struct Term {
    uint8_t left, right;
};
constexpr Term TERM[T + 1] = {
    {0, 0},                                                                             // (no power 0)
    {1, 0},   {1, 1},   {3, 0},   {3, 1},   {3, 2},   {6, 0},   {6, 1},   {8, 0},    //  1 ..  8
    {8, 1},   {8, 2},   {8, 3},   {12, 0},  {13, 0},  {13, 1},  {15, 0},  {16, 0},   //  9 .. 16
    {16, 1},  {16, 2},  {16, 3},  {12, 8},  {15, 6},  {16, 6},  {15, 8},  {16, 8},   // 17 .. 24
    {13, 12}, {13, 13}, {15, 12}, {16, 12}, {16, 13}, {15, 15}, {16, 15}, {16, 16},  // 25 .. 32
};

// the accumulators' powers in the order they are fed: two groups of four
// direct adds, then six groups of four multiply-accumulates
constexpr uint8_t DIRECT[ND] = {1, 3, 6, 8, 12, 13, 15, 16};
constexpr uint8_t MAC[NM] = {2,  4,  5,  7,  9,  10, 11, 14, 17, 18, 19, 20,
                             21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32};

// index in V of x^e (0: the id; i + 1: CHAIN[i]); -1 if e is not in E
constexpr int vidx(int e) {
    if (e == 1) return 0;
    for (int i = 0; i < NP; ++i)
        if (CHAIN[i].power == e) return i + 1;
    return -1;
}

// ---- invariants -------------------------------------------------------------
constexpr bool chain_ok() {
    for (int i = 0; i < NP; ++i) {
        const Step s = CHAIN[i];
        if (s.power > T || s.left + s.right != s.power) return false;
        const int l = vidx(s.left), r = vidx(s.right);
        if (l < 0 || r < 0 || l > i || r > i) return false;   // produced before use
        for (int j = 0; j < i; ++j)
            if (CHAIN[j].power == s.power) return false;
        if (s.power == 1) return false;
    }
    return true;
}
constexpr bool terms_ok() {
    for (int k = 1; k <= T; ++k) {
        const Term t = TERM[k];
        if (t.left > T || t.right > T || vidx(t.left) < 0) return false;
        if (t.right == 0 ? t.left != k : (vidx(t.right) < 0 || t.left + t.right != k)) return false;
    }
    return true;
}
// every power 1..32 is fed exactly once, the direct ones to DIRECT and the
// pairs to MAC
constexpr bool slots_ok() {
    for (int k = 1; k <= T; ++k) {
        int d = 0, m = 0;
        for (int i = 0; i < ND; ++i) d += DIRECT[i] == k;
        for (int i = 0; i < NM; ++i) m += MAC[i] == k;
        if (d + m != 1 || (d == 1) != (TERM[k].right == 0)) return false;
    }
    return true;
}
static_assert(ND + NM == T && NP + 1 == NE && ND % 4 == 0 && NM % 4 == 0, "basis32: sizes");
static_assert(chain_ok(), "basis32: every chain step is a new power <= 32 whose operands were produced before it");
static_assert(terms_ok(), "basis32: every power is an element of E or the sum of two, none above 32");
static_assert(slots_ok(), "basis32: every power 1..32 has exactly one accumulator, of its own kind");

// the tables as V indices, so that unrolled device code sees constants
struct ChainIdx {
    int8_t l[NP], r[NP];
};
constexpr ChainIdx chain_idx() {
    ChainIdx c{};
    for (int i = 0; i < NP; ++i) {
        c.l[i] = (int8_t)vidx(CHAIN[i].left);
        c.r[i] = (int8_t)vidx(CHAIN[i].right);
    }
    return c;
}
constexpr ChainIdx CIDX = chain_idx();
constexpr int direct_v(int i) { return vidx(DIRECT[i]); }             // accumulator i of the direct ones
constexpr int mac_l(int i) { return vidx(TERM[MAC[i]].left); }        // accumulator i of the pairs
constexpr int mac_r(int i) { return vidx(TERM[MAC[i]].right); }

// ---- the chain --------------------------------------------------------------
// V[0] = id (not reduced: every product is exact for any 32-bit operand).
// Lazy form: returns the minimum of the eight results; below WRAP_BELOW a
// fold may have wrapped and the caller runs the exact form instead (field.h
// mulfold32_min).  The kernel issues the same eight products as one asm
// statement (bsgs.h basis_chain); this is its mirror on the CPU.  Which ids
// the lazy form gets wrong is a fixed set of 61: the kernel looks them up
// (basis_filter.h) instead of forming the minimum, which only the
// u32_basis = 2 form still does.
constexpr uint32_t WRAP_BELOW = 25u;
QK_HD uint32_t chain_min(uint32_t id, uint32_t (&V)[NE]) {
    uint32_t mn = 0xFFFFFFFFu;
    V[0] = id;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < NP; ++i) V[i + 1] = mulfold32_min(V[CIDX.l[i]], V[CIDX.r[i]], mn);
    return mn;
}
// the redo path: always congruent
QK_HD void chain_exact(uint32_t id, uint32_t (&V)[NE]) {
    V[0] = id;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < NP; ++i) V[i + 1] = mulfold32_exact(V[CIDX.l[i]], V[CIDX.r[i]]);
}

} // namespace basis32
} // namespace qk
