// sendersteps.h — the host plan of the queued sender step and of the ingest
// that feeds it (sendersteps.hip), plain C++ that a native
// CPU program compiles too (tests/native/sender_steps_plan_check.cpp):
//   sq_check     both CSR indices ascending, the queue's starting at 0; the
//                number of rounds = the longest queue of any flow
//   sq_lds       the LDS bytes of the round's kernels for the fullest item
//   wq_offsets   the queue's CSR index from the per-flow counts of accepted
//                datagrams
// The queue holds flow g's accepted datagrams at q_offsets[g] ..
// q_offsets[g + 1], in arrival order; round j steps record q_offsets[g] + j of
// every flow that still has one and has not reset.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace qk {

struct SqSizes {
    size_t nseg, nq;
    uint32_t T;
};

inline bool sq_check(const uint64_t *offsets, const uint64_t *q_offsets, size_t nseg, uint64_t *rounds) {
    uint64_t k = 0;
    if (q_offsets[0] != 0) return false;
    for (size_t g = 0; g < nseg; ++g) {
        if (offsets[g + 1] < offsets[g] || q_offsets[g + 1] < q_offsets[g]) return false;
        const uint64_t kg = q_offsets[g + 1] - q_offsets[g];
        if (kg > k) k = kg;
    }
    *rounds = k;
    return true;
}

struct SqLds {
    size_t find, root, remove;
    uint32_t rows;   // u64 words of k_sq_remove's local rows
};
// maxseg: the most segments any work item holds
inline SqLds sq_lds(uint32_t maxseg, uint32_t T, uint32_t rows) {
    SqLds l;
    l.rows = rows;
    l.find = ((size_t)maxseg * 4 + 1) * sizeof(uint32_t);
    l.root = ((size_t)maxseg * 4 + 1 + (size_t)maxseg * (T + 1)) * sizeof(uint32_t);
    l.remove = (size_t)rows * 8 + ((size_t)maxseg * 3 + 1) * sizeof(uint32_t);
    return l;
}

// a sort region: n keys, then n values; the passes between hold n pairs there
inline size_t wq_region_words(uint64_t n) { return 2 * (size_t)n; }

// q_offsets[0 .. nseg] from counts[0 .. nseg); returns the records
inline uint64_t wq_offsets(const uint32_t *counts, size_t nseg, uint64_t *q_offsets) {
    uint64_t at = 0;
    q_offsets[0] = 0;
    for (size_t g = 0; g < nseg; ++g) {
        at += counts[g];
        q_offsets[g + 1] = at;
    }
    return at;
}

} // namespace qk
