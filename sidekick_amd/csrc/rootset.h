// rootset.h — the pure host logic of the decode root test (decode.hip), plain
// C++ checked natively (tests/native/rootset_check.cpp): the hash set of P's
// roots, the u64 baby-step/giant-step coefficient table, the pinned result slots.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "field.h"

namespace qk {

// The root set: 2^b buckets of S slots (words = S 2^b); root r sits in bucket
// rs_hash(r) >> shift (shift = 32 - b); free slots hold all-ones (>= p).
struct RtScanSet {
    uint32_t S = 1, words = 0, m1 = 1, m2 = 1, shift = 28;
};

// lo(x) m1 + hi(x) m2 mod 2^32 (hi = 0 for u32): host builder and device lookup (decode.hip rs_member)
template <typename T> QK_HD uint32_t rs_hash(T x, uint32_t m1, uint32_t m2) {
    uint32_t hh = (uint32_t)x * m1;
    if constexpr (sizeof(T) == 8) hh += (uint32_t)((uint64_t)x >> 32) * m2;
    return hh;
}

// a root set of at most this many bytes travels in the kernel arguments
constexpr size_t RT_KTAB_BYTES = 2048;

// The hash set of the k canonical, distinct roots.  S = 1 for up to 32 roots
// (2^b >= 2 k^2 buckets: a multiplier pair without collisions is found in
// ~1.3 tries on average), else S = 4 with 2^b >= 2k buckets (mean load 1/2).
// compact: S = 1 with 2^b >= k^2 / 6 — a table small enough for the kernel
// arguments (k = 32: 256 words; a collision-free multiplier pair is then
// found in ~e^(k^2 / 2^(b+1)) = 7 tries, a few hundred host hashes).  (S = 4
// with 2^b >= 2k, the other small layout, costs the u32 scan 84 against 65 µs
// at configs[4]: four compares per candidate.)  b >= 4.  Returns false when
// no multipliers fit within the attempt limit.  Deterministic in its arguments.
template <typename T>
inline bool rt_scan_table(const T *roots, uint32_t k, RtScanSet &set, std::vector<T> &out, bool compact = false) {
    set.S = k <= 32 || compact ? 1 : 4;
    uint32_t b = 4;
    const uint64_t want = compact ? ((uint64_t)k * k + 5) / 6 : set.S == 1 ? 2ull * k * k : 2ull * k;
    while ((1ull << b) < want) ++b;
    set.shift = 32 - b;
    const uint32_t nb = 1u << b;
    set.words = nb * set.S;
    out.assign(set.words, (T)~(T)0);
    std::vector<uint32_t> fill(nb);
    uint64_t st = 0x9E3779B97F4A7C15ull ^ k;
    for (int attempt = 0; attempt < 1000; ++attempt) {
        st = splitmix_mix(st + GAMMA);
        set.m1 = (uint32_t)st | 1u;
        set.m2 = (uint32_t)(st >> 32) | 1u;
        std::fill(fill.begin(), fill.end(), 0u);
        std::fill(out.begin(), out.end(), (T)~(T)0);
        bool ok = true;
        for (uint32_t r = 0; r < k && ok; ++r) {
            const T x = roots[r];
            const uint32_t bi = rs_hash<T>(x, set.m1, set.m2) >> set.shift;
            if (fill[bi] == set.S) ok = false;
            else out[(size_t)bi * set.S + fill[bi]++] = x;
        }
        if (ok) return true;
    }
    return false;
}

// The limb-shifted coefficient table of k_root_test_u64_bsgs (coeffs: canonical
// c_1..c_d of the monic polynomial): out[3k + j] = p_k 2^(22j) mod p for the
// coefficient p_k of x^k, k < 8 ceil(d / 8); returns the words written.
inline size_t rt64_bsgs_table(const uint64_t *coeffs, uint32_t d, uint64_t *out) {
    const uint32_t nfull = d / 8, r = d % 8, nblk = nfull + (r ? 1 : 0);
    const size_t words = (size_t)nblk * 24;
    for (size_t i = 0; i < words; ++i) out[i] = 0;
    for (uint32_t k = 0; k < 8 * nblk; ++k) {
        uint64_t pk;   // coefficient of x^k: p_d = 1, p_(d-i) = c_i
        if (k > d) pk = 0;
        else if (k == d) pk = 1;
        else pk = coeffs[d - k - 1];
        unsigned __int128 v = pk;
        for (int j = 0; j < 3; ++j) {
            out[(size_t)k * 3 + j] = (uint64_t)(v % P64);
            v = (v % P64) << 22;
        }
    }
    return words;
}

// Small-buffer layout (u64 words).  Root tests: d_small[0] hit count, [1]
// first stop, [2] the scan's hash multipliers, [3] stops recorded (root-set
// scan), [RT_C ..) the coefficients or the root set — one H2D copy of
// h_small[0 .. RT_C + words) sets all of it.  Results in h_small from
// SMALL_NHITS: count, stop, the overflow flag of the direct form, the
// kernel-argument scan's completion mark, then from SMALL_HITPF the first
// hits and at the end RT_NSTOP stop slots.  Horner's arrive by D2H copies;
// the root-set scan writes its hits and stops there itself (decode.hip
// rt_record) and the host derives count and stop from the slots (RtSlots).
constexpr size_t SMALL_WORDS = 4096;   // >= max partial words (2*1024+2) plus counters
constexpr size_t RT_C = 4;             // root tests: coefficients / root set from d_small[RT_C]
constexpr size_t SMALL_NHITS = 3072;   // h_small: hit count
constexpr size_t SMALL_STOP = 3073;    // h_small: first stop index
constexpr size_t SMALL_OVF = 3074;     // h_small: a hit or stop slot past the direct form's room
constexpr size_t SMALL_DONE = 3075;    // h_small: the kernel-argument scan's completion mark
constexpr size_t SMALL_HITPF = 3076;   // h_small: the first hits
constexpr uint32_t RT_NSTOP = 16;      // stop slots of the direct form
constexpr size_t SMALL_STOPS = SMALL_WORDS - RT_NSTOP;
constexpr size_t SMALL_HITPF_N = SMALL_STOPS - SMALL_HITPF;
// the same slots relative to SMALL_NHITS (the kernel's hout)
constexpr size_t RT_STOP0 = SMALL_STOPS - SMALL_NHITS;
constexpr size_t RT_DONE0 = SMALL_DONE - SMALL_NHITS;
// room of d_small for the coefficients / the root set of the copy form
constexpr size_t RT_SET_BYTES = (SMALL_NHITS - RT_C) * 8;

// what a root test left: hit count, first stop position (~0: none), stop slots
// filled; overflow: a hit or stop found no slot, count and stop are on the device
struct RtSlotRead {
    uint64_t hits = 0, stop = ~0ull, stops = 0;
    bool overflow = false;
};

// The slot protocol over h_small (or its device alias, for a kernel's pointers).
// The host fills every slot with ~0 and clears the overflow flag (clear); the
// scan writes hit k to hit slot k and its j-th stop to stop slot j, or sets the
// flag; the host counts hits up to the first ~0 and takes the stops' minimum.
struct RtSlots {
    uint64_t *h;

    void clear() const {
        std::fill(h + SMALL_HITPF, h + SMALL_WORDS, ~0ull);
        h[SMALL_OVF] = 0;
    }
    RtSlotRead read() const {
        RtSlotRead r;
        r.overflow = h[SMALL_OVF] != 0;
        while (r.hits < SMALL_HITPF_N && h[SMALL_HITPF + r.hits] != ~0ull) ++r.hits;
        for (uint32_t k = 0; k < RT_NSTOP; ++k) {
            r.stop = std::min(r.stop, h[SMALL_STOPS + k]);
            r.stops += h[SMALL_STOPS + k] != ~0ull;
        }
        return r;
    }
    // after a call that read r without overflow: it wrote no other slots
    void restore(const RtSlotRead &r) const {
        std::fill(h + SMALL_HITPF, h + SMALL_HITPF + r.hits, ~0ull);
        std::fill(h + SMALL_STOPS, h + SMALL_WORDS, ~0ull);
    }
    // count and stop as a D2H copy of the device counters to result() left them
    RtSlotRead copied() const { return {h[SMALL_NHITS], h[SMALL_STOP], 0, false}; }
    uint64_t *result() const { return h + SMALL_NHITS; }   // the kernel's hout; the counters' D2H target
    uint64_t *hits() const { return h + SMALL_HITPF; }     // the first SMALL_HITPF_N hits
    const volatile uint64_t *done() const { return h + SMALL_DONE; }
};

} // namespace qk
