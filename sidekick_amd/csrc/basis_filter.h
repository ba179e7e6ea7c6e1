// basis_filter.h — which ids the lazy chain of basis32.h gets wrong, as a
// table (DESIGN.md §3.2 "Basis").  Plain C++17: bsgs.h copies the table into
// LDS and tests every id against it, and the host compiles the same file
// without HIP (tests/native/basis_filter_check.cpp), like basis32.h.
//
// Whether a lazy fold of the chain wraps is a property of the id alone.  Of
// all 2^32 ids, 61 have a lazy chain that differs mod p from the exact one
// (WRONG below; enumerated by basis_filter_check `enumerate`).  The kernel
// used to re-derive that per id from the minimum of the eight products; it
// now looks the id up and runs the exact chain for the candidates.
//
// The filter is one table of SLOTS 32-bit entries, indexed by the id's bits
// 2..13 (the byte address id & KEY_MASK).  An id is a candidate iff
//     (entry ^ id) < WINDOW.
//   * A slot that holds wrong ids stores the OR of them.  The wrong ids of a
//     slot differ only in bits 0, 1, 16 and 17 (0xFFFDFFFB, 0xFFFEFFFB and
//     0xFFFFFFF8 share their low 16 bits, so no key taken from the low bits
//     parts them), and WINDOW = 0x20004 is the smallest bound that covers
//     those differences.  This is asserted below for every wrong id: there is
//     no false negative.
//   * Every other slot stores a value whose key bits are not the slot's
//     (bit 13 flipped), so an id that lands there differs from it in bit 13.
//   The candidates are counted exactly: an id is one iff it equals its slot's
//   entry in bits 18..31, the key bits match, and bits 14..17 of the difference
//   are at most 8 (at most 7 where bit 13 differs): 36 ids for each of the 57
//   slots in use, 32 for each other slot, CANDIDATES in all, 3.1e-5 of the ids.
//   A trip of four ids per lane therefore takes the slow path with probability
//   about 256 x 3.1e-5 = 0.8 %.  Id 0 (what lanes past their range feed) is no
//   candidate.
// Per id the test costs one v_and (the key), one ds_read_b32 and one v_xor; a
// trip adds three v_min and one v_cmp.
#pragma once
#include <stdint.h>

namespace qk {
namespace basis_filter {

constexpr int NWRONG = 61;
// ascending; tests/golden/basis_wrong_ids.json holds the same list
constexpr uint32_t WRONG[NWRONG] = {
    15362091u,   58005635u,   84325748u,   212215109u,  221073260u,  492279886u,  552143393u,
    622572812u,  639109131u,  957658446u,  998652690u,  1120809293u, 1142778689u, 1248059560u,
    1373385175u, 1606977228u, 1669389704u, 1793818983u, 1820041303u, 1858945430u, 1974274384u,
    2039928669u, 2085787571u, 2173567192u, 2255038622u, 2324401375u, 2337445954u, 2436021861u,
    2474925988u, 2523745003u, 2624686118u, 2625577587u, 2687990063u, 2921582116u, 3046907731u,
    3152188602u, 3277239954u, 3278929599u, 3365160499u, 3493496785u, 3655858160u, 3672394479u,
    3742823898u, 3780479003u, 3802687405u, 3828599332u, 3911878746u, 3927921728u, 4073894031u,
    4082752182u, 4147259949u, 4210641543u, 4236961656u, 4291450497u, 4294836219u, 4294901755u,
    4294967287u, 4294967288u, 4294967293u, 4294967294u, 4294967295u,
};

constexpr uint32_t KEY_MASK = 0x3FFCu;          // the entry's byte address: bits 2..13 of the id
constexpr int SLOTS = (KEY_MASK >> 2) + 1;      // 4 096 entries, 16 KiB
constexpr uint32_t WINDOW = 0x20004u;           // candidate iff (entry ^ id) < WINDOW
constexpr uint32_t EMPTY_HIGH = 0x80000000u;    // bits 14..31 of an unused slot's entry
constexpr uint32_t EMPTY_FLIP = 0x2000u;        // ... and the key bit it has wrong
constexpr int USED_SLOTS = 57;
// ids that are candidates, out of 2^32 (the cap the exhaustive check holds the filter to)
constexpr uint64_t CANDIDATES = (uint64_t)USED_SLOTS * 36u + (uint64_t)(SLOTS - USED_SLOTS) * 32u;

struct Table {
    uint32_t e[SLOTS];
};
constexpr uint32_t slot_of(uint32_t id) { return (id & KEY_MASK) >> 2; }
constexpr Table make_table() {
    Table t{};
    for (int k = 0; k < SLOTS; ++k) t.e[k] = EMPTY_HIGH | (((uint32_t)k << 2) ^ EMPTY_FLIP);
    bool used[SLOTS] = {};
    for (int i = 0; i < NWRONG; ++i) {
        const uint32_t k = slot_of(WRONG[i]);
        t.e[k] = used[k] ? (t.e[k] | WRONG[i]) : WRONG[i];
        used[k] = true;
    }
    return t;
}
constexpr Table TABLE = make_table();

constexpr bool candidate(const Table &t, uint32_t id) { return (t.e[slot_of(id)] ^ id) < WINDOW; }
constexpr bool candidate(uint32_t id) { return candidate(TABLE, id); }

// ---- invariants -------------------------------------------------------------
constexpr bool list_ok() {
    for (int i = 1; i < NWRONG; ++i)
        if (WRONG[i - 1] >= WRONG[i]) return false;
    return true;
}
constexpr bool wrong_are_candidates() {
    for (int i = 0; i < NWRONG; ++i)
        if (!candidate(WRONG[i])) return false;
    return true;
}
constexpr int used_slots() {
    int n = 0;
    for (int k = 0; k < SLOTS; ++k) n += slot_of(TABLE.e[k]) == (uint32_t)k;
    return n;
}
static_assert(list_ok(), "basis_filter: the wrong ids ascend, none twice");
static_assert(wrong_are_candidates(), "basis_filter: every wrong id is a candidate (no false negative)");
static_assert(used_slots() == USED_SLOTS, "basis_filter: slots in use");
static_assert(!candidate(0u), "basis_filter: id 0 (lanes past their range) takes the fast path");
static_assert(sizeof(Table) == 16384, "basis_filter: 16 KiB per workgroup, five workgroups per CU");

} // namespace basis_filter
} // namespace qk
