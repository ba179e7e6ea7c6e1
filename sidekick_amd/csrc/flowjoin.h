// flowjoin.h — internal: the merge-path join of two flow-key arrays
// (flowtable.hip k_ft_join / k_ft_scan), shared by the flow table's merge and
// the packet snapshots' base gather and table upsert (pktsnap.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ctx.h"
#include "segments.h"

namespace qk {

constexpr uint32_t FT_TILE = QK_FLOW_JOIN_TILE;
constexpr uint32_t FT_SLOTS = FT_TILE + 1;                            // the moved cut adds one key
constexpr uint32_t FT_CPT = 4;                                        // move chunks per tile
constexpr uint32_t FT_CHUNK = (FT_SLOTS + FT_CPT - 1) / FT_CPT;       // slots per move chunk
constexpr uint32_t FT_NONE = 0xFFFFFFFFu;
// res[] words (device, zeroed per call; copied to the pinned ctx->h_flow)
enum { FT_TOTAL = 0, FT_MATCH = 1, FT_FLAGS = 2, FT_RES_WORDS = 4 };
enum : unsigned long long { FT_F_ORDER = 1, FT_F_MISMATCH = 2 };

// The join's scratch.  Merge form: tile k's output elements are slots
// [k FT_SLOTS, k FT_SLOTS + tilecnt[k]): sa / sb hold each element's index in
// a / in b (FT_NONE: absent), tilebase[k] the output row of the tile's first.
struct FtBuf {
    uint32_t *sa = nullptr, *sb = nullptr, *tilecnt = nullptr;
    uint64_t *tilebase = nullptr;
    unsigned long long *res = nullptr;
};
void ft_carve(Carve &cv, FtBuf &b, size_t ntiles, size_t na, bool diff);
// res[] into the pinned words, after everything enqueued on s (waits)
int ft_read_res(qk_ctx *ctx, const FtBuf &b, hipStream_t s, uint64_t *out);
// The merge-form join of ka (na keys) with kb (nb keys), ntiles = ceil((na +
// nb) / FT_TILE): fills b, waits, and returns res[] (FT_TOTAL the union's
// size, FT_MATCH the shared keys, FT_F_ORDER: an input not strictly ascending).
int ft_join_merge(qk_ctx *ctx, hipStream_t s, const uint32_t *ka, uint32_t na, const uint32_t *kb, uint32_t nb,
                  const FtBuf &b, size_t ntiles, uint64_t *res);

} // namespace qk
