// basis_filter_check.cpp — CPU check of the id filter of the u32 t = 31..32
// encode (sidekick_amd/csrc/basis_filter.h) against the chains of basis32.h.
//
//   basis_filter_check table              the table as built: every listed id a
//                                         candidate, id 0 none, unused slots can
//                                         never hold their own key
//   basis_filter_check enumerate [N] [T]  ids 0 .. N-1 (default 2^32: all) on T
//                                         threads (default and at most 16):
//     * every id whose lazy chain differs mod p from chain_exact must be a
//       candidate of the filter (no false negative);
//     * those ids must be exactly the header's list below N (all 61 for 2^32);
//     * the candidates are counted: at most basis_filter::CANDIDATES over all
//       ids, and exactly that many when N = 2^32.
//     Prints "wrong ID" for each such id, "flag ID" for each id that trips the
//     parent's test (minimum of the products < 25) and is right, then a
//     summary line.  tests/golden/basis_wrong_ids.json is this output.
//     A fold that wraps leaves a result below 25 (field.h), so the exact chain
//     is run where the minimum is below 25 and, as a cross-check of that
//     shortcut, for every 64th id whatever its minimum.
// Built and run by tests/test_basis_filter_native.py (also under ASan + UBSan
// on a 2^24-id prefix).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "../../sidekick_amd/csrc/basis32.h"
#include "../../sidekick_amd/csrc/basis_filter.h"

using namespace qk;
namespace b32 = qk::basis32;
namespace bf = qk::basis_filter;

static int run_table() {
    int fails = 0;
    for (int i = 0; i < bf::NWRONG; ++i)
        if (!bf::candidate(bf::WRONG[i])) { printf("FAIL: wrong id %u is no candidate\n", bf::WRONG[i]); ++fails; }
    if (bf::candidate(0u)) { printf("FAIL: id 0 is a candidate\n"); ++fails; }
    int used = 0;
    for (int k = 0; k < bf::SLOTS; ++k) {
        const uint32_t e = bf::TABLE.e[k];
        if (bf::slot_of(e) == (uint32_t)k) { ++used; continue; }
        // unused: an id of this slot differs from the entry in the flipped key bit
        if (((e ^ ((uint32_t)k << 2)) & bf::KEY_MASK) != bf::EMPTY_FLIP) { printf("FAIL: slot %d entry %#x\n", k, e); ++fails; }
    }
    if (used != bf::USED_SLOTS) { printf("FAIL: %d slots in use\n", used); ++fails; }
    printf("basis_filter_check table: %s (%d failures, %d slots in use)\n", fails ? "FAIL" : "ok", fails, used);
    return fails ? 1 : 0;
}

struct Found {
    std::vector<uint32_t> wrong, flagged_right;
    uint64_t candidates = 0, missed = 0, shortcut_broken = 0;
};

static bool differs(const uint32_t (&V)[b32::NE], const uint32_t (&E)[b32::NE]) {
    for (int k = 1; k < b32::NE; ++k)
        if (V[k] != E[k] && canon32(V[k]) != canon32(E[k])) return true;
    return false;
}

static int run_enumerate(uint64_t n, int threads) {
    std::vector<Found> found(threads);
    std::vector<std::thread> pool;
    const uint64_t per = (n + threads - 1) / threads;
    for (int t = 0; t < threads; ++t)
        pool.emplace_back([&, t]() {
            Found &f = found[t];
            const uint64_t lo = std::min(n, per * t), hi = std::min(n, lo + per);
            for (uint64_t i = lo; i < hi; ++i) {
                const uint32_t id = (uint32_t)i;
                uint32_t V[b32::NE], E[b32::NE];
                const bool cand = bf::candidate(id);
                f.candidates += cand;
                const bool flagged = b32::chain_min(id, V) < b32::WRAP_BELOW;
                if (!flagged && (id & 63u) != 0) continue;
                b32::chain_exact(id, E);
                const bool wrong = differs(V, E);
                if (wrong && !flagged) ++f.shortcut_broken;
                if (wrong) {
                    f.wrong.push_back(id);
                    if (!cand) ++f.missed;
                } else if (flagged) {
                    f.flagged_right.push_back(id);
                }
            }
        });
    for (auto &th : pool) th.join();
    Found all;
    for (const Found &f : found) {   // the threads' ranges ascend
        all.wrong.insert(all.wrong.end(), f.wrong.begin(), f.wrong.end());
        all.flagged_right.insert(all.flagged_right.end(), f.flagged_right.begin(), f.flagged_right.end());
        all.candidates += f.candidates;
        all.missed += f.missed;
        all.shortcut_broken += f.shortcut_broken;
    }
    for (uint32_t id : all.wrong) printf("wrong %u\n", id);
    for (uint32_t id : all.flagged_right) printf("flag %u\n", id);
    std::vector<uint32_t> listed;
    for (int i = 0; i < bf::NWRONG; ++i)
        if (bf::WRONG[i] < n) listed.push_back(bf::WRONG[i]);
    const bool whole = n == (1ull << 32);
    int fails = 0;
    if (all.missed) { printf("FAIL: %llu wrong ids are no candidates\n", (unsigned long long)all.missed); ++fails; }
    if (all.shortcut_broken) { printf("FAIL: %llu wrong ids with a minimum >= 25\n", (unsigned long long)all.shortcut_broken); ++fails; }
    if (all.wrong != listed) { printf("FAIL: the enumerated ids are not the header's list below %llu\n", (unsigned long long)n); ++fails; }
    if (whole && all.wrong.size() != (size_t)bf::NWRONG) { printf("FAIL: %zu wrong ids\n", all.wrong.size()); ++fails; }
    if (all.candidates > bf::CANDIDATES || (whole && all.candidates != bf::CANDIDATES)) {
        printf("FAIL: %llu candidates, the header says %llu\n", (unsigned long long)all.candidates,
               (unsigned long long)bf::CANDIDATES);
        ++fails;
    }
    printf("basis_filter_check enumerate: %s (%d failures, %llu ids, %zu wrong, %zu flagged and right, %llu candidates, cap %llu)\n",
           fails ? "FAIL" : "ok", fails, (unsigned long long)n, all.wrong.size(), all.flagged_right.size(),
           (unsigned long long)all.candidates, (unsigned long long)bf::CANDIDATES);
    return fails ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "table")) return run_table();
    if (argc >= 2 && !strcmp(argv[1], "enumerate")) {
        const uint64_t n = argc >= 3 ? strtoull(argv[2], 0, 0) : (1ull << 32);
        int threads = argc >= 4 ? atoi(argv[3]) : 16;
        const int hw = (int)std::thread::hardware_concurrency();
        if (hw > 0 && threads > hw) threads = hw;
        if (threads < 1) threads = 1;
        if (threads > 16) threads = 16;
        if (n > (1ull << 32)) { fprintf(stderr, "basis_filter_check: N <= 2^32\n"); return 2; }
        return run_enumerate(n, threads);
    }
    fprintf(stderr, "usage: basis_filter_check table | enumerate [N] [THREADS]\n");
    return 2;
}
