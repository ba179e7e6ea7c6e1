// snapshots.h — the host plan of the per-flow quACK snapshots
// (snapshots.hip): the quACK the proxy sends after every
// packet that brings a flow's count to a multiple of frequency_pkts
// (sidekick_multi.rs:271-283), for a batch grouped by flow.
//
// Plain C++ (tests/native/snapshot_plan_check.cpp checks it against a
// per-packet count loop).  A flow with base count c0 reaches, after its
// packet j, the count (c0 + j + 1) mod 2^32; packet j is a cut when that
// value is a multiple of f.  The test runs on the wrapped u32, so a count
// that wraps to 0 is a cut and the cuts after it lie at f, 2f, ... again: the
// cuts are not evenly spaced across the wrap unless f divides 2^32.  A
// segment holds fewer than 2^32 ids, so a flow wraps at most once per call.
//
// The grouped id array is cut into work items of SN_ITEM consecutive
// positions, whatever flows they belong to; one wave walks an item.  A flow
// that begins inside an item starts from its base row; a flow that continues
// from the item before starts from zero, and its rows receive their carry-in
// (base + the flow's earlier items) in a later kernel.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "field.h"

namespace qk {

constexpr uint32_t SN_ITEM = 2048;     // positions of the grouped id array per work item, one wave each
constexpr uint32_t SN_KC_SMALL = 32;   // powers per column pass of a threshold <= SN_KC_SMALL
constexpr uint32_t SN_KC = 64;         // powers per column pass of a larger threshold
constexpr uint64_t SN_WRAP = 1ull << 32;

// the cuts among the first len packets of a flow with base count c0 (len < 2^32)
QK_HD uint64_t sn_ncuts(uint32_t c0, uint32_t f, uint64_t len) {
    const uint64_t e = (uint64_t)c0 + len;   // the count after len packets, not wrapped
    if (e < SN_WRAP) return e / f - c0 / f;
    return (SN_WRAP - 1) / f - c0 / f + (e - SN_WRAP) / f + 1;   // the multiples in (c0, 2^32), then 0, f, 2f, ...
}

// the local position of the flow's r-th cut, r from 0 (may lie past the segment's end)
QK_HD uint64_t sn_cut_pos(uint32_t c0, uint32_t f, uint64_t r) {
    const uint64_t before = (SN_WRAP - 1) / f - c0 / f;   // the cuts in front of the wrap
    if (r < before) return ((uint64_t)(c0 / f) + 1 + r) * f - c0 - 1;
    return SN_WRAP - c0 - 1 + (r - before) * f;
}

// carry[first + i + 1] = carry[first + i] + part[first + i], i = 0 .. count - 1:
// the items in the middle of a flow that spans three items or more
struct SnChain {
    uint32_t first, count;
};

inline size_t sn_items(const uint64_t *offsets, size_t nseg) {
    return (size_t)((offsets[nseg] - offsets[0] + SN_ITEM - 1) / SN_ITEM);
}

// decreasing offsets or a segment of 2^32 ids or more: false
inline bool sn_check(const uint64_t *offsets, size_t nseg) {
    for (size_t g = 0; g < nseg; ++g)
        if (offsets[g + 1] < offsets[g] || offsets[g + 1] - offsets[g] >= SN_WRAP) return false;
    return true;
}

// snap_offsets[0 .. nseg] from the flows' base counts; returns the total
inline uint64_t sn_plan_counts(const uint64_t *offsets, const uint32_t *counts, size_t nseg, uint32_t f,
                               uint64_t *snap_offsets) {
    uint64_t at = 0;
    snap_offsets[0] = 0;
    for (size_t g = 0; g < nseg; ++g) {
        at += sn_ncuts(counts[g], f, offsets[g + 1] - offsets[g]);
        snap_offsets[g + 1] = at;
    }
    return at;
}

// g0[i] = the flow that holds item i's first position; the chains (at most
// min(nseg, items) of them).  Returns the number of chains.
inline size_t sn_plan_items(const uint64_t *offsets, size_t nseg, uint32_t *g0, SnChain *chains) {
    const uint64_t pos0 = offsets[0];
    const size_t ni = sn_items(offsets, nseg);
    size_t nc = 0, i = 0;
    for (size_t g = 0; g < nseg && i < ni; ++g) {
        const uint64_t fb = offsets[g], fe = offsets[g + 1];
        if (fe == fb) continue;
        for (; i < ni && pos0 + (uint64_t)i * SN_ITEM < fe; ++i) g0[i] = (uint32_t)g;
        const uint64_t a = (fb - pos0) / SN_ITEM, b = (fe - 1 - pos0) / SN_ITEM;
        if (b - a >= 2) chains[nc++] = {(uint32_t)(a + 1), (uint32_t)(b - a - 1)};
    }
    return nc;
}

} // namespace qk
