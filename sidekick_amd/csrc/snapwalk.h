// snapwalk.h — internal: the snapshot walk (snapshots.hip: k_sn_walk,
// k_sn_chain, k_sn_carry, k_sn_empty) behind one host driver, shared by
// qk_u32_snapshot_segments_device and the packet path
// (pktsnap.hip, qk_u32_snapshot_flows_device).  The caller has the offsets, the
// base counts' plan (snapshots.h sn_plan_counts) and the capacity decision;
// the driver plans the work items and runs the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ctx.h"

namespace qk {

// Where the walk writes.  snap: the snapshot records; seg / pos / arr / key_out
// (each may be null): the flow, the grouped position, the arrival index and
// the flow's key (3 words from keys[g]) of every snapshot; fin (may be null):
// the flows' end-of-batch records.
// dest == null: snapshot r of flow g is row snap_offsets[g] + r (by flow).
// dest != null: the snapshot taken at grouped position pos is row dest[pos]
// (read at the cuts only): the caller's prefix sum over the emitting packets
// puts the rows into send order without a sort (pktsnap.hip).
struct SnOut {
    uint32_t *snap = nullptr, *seg = nullptr;
    uint64_t *pos = nullptr;
    uint32_t *arr = nullptr, *fin = nullptr;
    const uint32_t *dest = nullptr;
    const uint32_t *keys = nullptr;
    uint32_t *key_out = nullptr;
};

// bytes of pinned memory (ctx->h_items, from pinned_off) and of arena 1 (its
// end) that the driver takes; the caller ensures the arena
size_t sn_pinned_bytes(size_t nseg, size_t ni);
size_t sn_arena_bytes(size_t nseg, size_t ni, uint32_t T);
// base: nseg device records; d_ids (d_arrival): the grouped ids; offsets,
// snap_offsets: host, nseg + 1 each, checked (sn_check) and planned
// (sn_plan_counts) by the caller.  Synchronous on s.
int sn_walk_run(qk_ctx *ctx, hipStream_t s, const uint32_t *base, const uint32_t *d_ids, const uint32_t *d_arrival,
                const uint64_t *offsets, const uint64_t *snap_offsets, size_t nseg, uint32_t T, uint32_t f,
                const SnOut &o, size_t pinned_off);

} // namespace qk
