// flowfront.h — internal: the packet front of the per-flow batches, shared by
// the end-of-batch encode (flows.hip, qk_u32_encode_flows_device) and the
// every-crossing snapshots from captures (pktsnap.hip,
// qk_u32_snapshot_flows_device).  The kernels live in flows.hip; these are
// their host drivers:
//   flow_extract      the SidekickMulti filters (records.h) and the device hash
//                     table over a run of packets: slot and id per packet, the
//                     counters (sidekick_multi.rs:101-143)
//   flow_key_order    the occupied slots in ascending AddrKey order
//   flow_rank_keys    rank <-> slot, and the key bytes of every rank
//   flow_slots_to_ranks, flow_rank_offsets   the by-rank grouping's two ends
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ctx.h"
#include "radix.h"
#include "segments.h"

namespace qk {

// one slot of the device hash table (flows.hip, "flow table")
struct alignas(16) FlowSlot {
    uint64_t w0, w1;
};
constexpr uint32_t SLOT_NONE = 0xFFFFFFFFu;
constexpr uint64_t FT_OVERFLOW = 1;   // counters[3] flag
// the extract's counters: [0] inserts, [1] resets, [2] distinct flows, [3]
// flags, [4] 1 + the position of the last reset (0: none)
constexpr int FLOW_COUNTERS = 5;
// A Reset packet leaves (slot, id) = (SLOT_NONE, FLOW_ID_RESET), a skipped one
// (SLOT_NONE, 0): the ids of packets without a slot are otherwise unused
constexpr uint32_t FLOW_ID_RESET = 1;

// own dst ip:port as the extract compares it (NULL: no packet is a reset)
inline uint64_t flow_my_key(const uint8_t *my_addr) {
    if (!my_addr) return ~0ull;
    return ((uint64_t)my_addr[0] << 40) | ((uint64_t)my_addr[1] << 32) | ((uint64_t)my_addr[2] << 24) |
           ((uint64_t)my_addr[3] << 16) | ((uint64_t)my_addr[4] << 8) | (uint64_t)my_addr[5];
}

// the table (arena 2) and the counters of the last extract
struct FlowFront {
    uint64_t C = 0, cmax = 0;          // slots now, and the most a batch of this size may need
    FlowSlot *tab = nullptr;
    uint32_t *rank_of_slot = nullptr;
    RsPlan xpl{1, 4};                  // the last extract's chunking
    uint64_t hc[FLOW_COUNTERS] = {0, 0, 0, 0, 0};
};
// the table's first size for a batch of n packets, from the context's flow hint
void flow_front_init(const qk_ctx *ctx, uint64_t n, FlowFront &ff);
// The extract over pn packets from pb: slots[i], ids[i], ff.hc; a table that
// overflows its probe limit is regrown and the pass rerun.  hist != null: the
// by-slot sort's first-digit chunk counts (hg extract chunks per sort chunk).
// Records ctx->flow_ev[0] behind the last extract and waits for the counters.
int flow_extract(qk_ctx *ctx, hipStream_t s, const uint8_t *pb, uint64_t pn, size_t stride, const qk_pkt_meta *pm,
                 uint64_t my_key, uint32_t *slots, uint32_t *ids, unsigned long long *counters, uint32_t *hist,
                 uint32_t hg, FlowFront &ff);

// per-flow scratch of the key ordering
struct FlowKeyBuf {
    uint32_t *kA = nullptr, *vA = nullptr, *kB = nullptr, *vB = nullptr, *used = nullptr, *sl3 = nullptr;
    uint32_t *nsel = nullptr;   // [0] occupied slots found, [1] the caller's
    uint32_t *wcnt = nullptr;
    RsScratch krs{};
    uint32_t unb = 1;
    uint64_t uchunk = 256;
    void take(Carve &c, const qk_ctx *ctx, uint64_t C, uint32_t nf);
};
// the occupied slots in slot order (kb.used) and in ascending AddrKey order (*sorted)
int flow_key_order(qk_ctx *ctx, hipStream_t s, const FlowFront &ff, uint32_t nf, const FlowKeyBuf &kb,
                   const uint32_t **sorted);
// ff.rank_of_slot[slot] = rank, d_keys[rank] = the 12 key bytes
int flow_rank_keys(hipStream_t s, const FlowFront &ff, const uint32_t *sorted, uint32_t nf, uint8_t *d_keys);
// per packet, in place: slot -> flow rank (no slot -> nf, sorting last)
int flow_slots_to_ranks(const qk_ctx *ctx, hipStream_t s, uint32_t *key, const FlowFront &ff, uint64_t n, uint32_t nf);
// segment starts of the rank-sorted keys: d_offs[0 .. nf]
int flow_rank_offsets(const qk_ctx *ctx, hipStream_t s, const uint32_t *key, uint64_t inserted, uint32_t nf,
                      uint64_t *d_offs);

} // namespace qk
