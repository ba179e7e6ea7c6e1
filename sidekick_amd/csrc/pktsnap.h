// pktsnap.h — the host plan of the packet snapshots (pktsnap.hip,
// qk_u32_snapshot_flows_device): the proxy's frequency loop
// over captured packets (sidekick_multi.rs:240-287).
//
// Plain C++ (tests/native/pktsnap_plan_check.cpp checks it against the
// per-packet loop).  A Reset packet replaces the whole map
// (sidekick_multi.rs:263-266), so the batch falls into epochs: maximal runs
// of packets without a Reset.  The chain (extract, grouping, base gather,
// walk) runs once per epoch that holds packets; the epoch in front of the
// first Reset builds on the caller's table, every later one on an empty
// table.  Only the epoch behind the last Reset (the tail) leaves flows in the
// table; when the batch ends in a Reset there is none and the table is empty.
//
// Send order: every snapshot belongs to one packet, so the packets that emit
// are marked, and a snapshot's output row is the number of marked packets in
// front of its own.  The marks are summed in rows of PS_ROW (radix.h
// k_row_scan / k_tot_scan): rank(i) = rows[i / PS_ROW] + within[i].
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "field.h"

namespace qk {

constexpr uint32_t PS_ROW = 1024;   // marks per scan row: four per thread of a 256-thread workgroup

struct PsEpoch {
    uint64_t lo, hi;   // packets [lo, hi), no Reset among them, lo < hi
    bool fresh;        // a Reset lies in front of lo: the epoch starts from an empty table
    bool tail;         // hi is the batch's end: its flows are the table the batch leaves
};

// The epochs of a batch of n packets whose Reset packets lie at resets[0 ..
// nr) (any order, distinct, < n; sorted in place).  out holds up to nr + 1
// epochs; returns their number.  Runs of consecutive Resets, a Reset as packet
// 0 and a Reset as the last packet give no empty epoch.
inline size_t ps_epochs(uint32_t *resets, size_t nr, uint64_t n, PsEpoch *out) {
    std::sort(resets, resets + nr);
    size_t ne = 0;
    uint64_t lo = 0;
    for (size_t k = 0; k <= nr; ++k) {
        const uint64_t hi = k < nr ? resets[k] : n;
        if (hi > lo) out[ne++] = PsEpoch{lo, hi, k > 0, k == nr};
        lo = hi + 1;
    }
    return ne;
}

// rows of the mark scan over an epoch of m packets
inline uint64_t ps_rows(uint64_t m) { return (m + PS_ROW - 1) / PS_ROW; }

// the send-order row of packet i of an epoch (i local), given the scan's two levels
QK_HD uint64_t ps_rank(const uint32_t *rows, const uint32_t *within, uint64_t i) {
    return (uint64_t)rows[i / PS_ROW] + within[i];
}

} // namespace qk
