// pktsnap_plan_check.cpp — the host plan of the packet snapshots
// (sidekick_amd/csrc/pktsnap.h) against the per-packet loop it stands for:
//   * ps_epochs: the loop walks the batch once, a Reset empties the table; the
//     plan's epochs must be exactly the maximal Reset-free runs that hold a
//     packet, in order, `fresh` exactly where a Reset came before, `tail`
//     exactly on the run that reaches the batch's end — for Resets given in
//     any order, consecutive, as packet 0, as the last packet, all packets;
//   * ps_rows / ps_rank: the two-level prefix sums of the emitting packets'
//     marks, restated on the host as k_row_scan / k_tot_scan compute them, put
//     the r-th emitting packet at row r.
// Stand-alone: g++ -std=c++17 -I../../sidekick_amd/csrc, plain and under
// -fsanitize=address,undefined (tests/test_pktsnap_plan_native.py).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../sidekick_amd/csrc/pktsnap.h"

using namespace qk;

static uint64_t checks = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        ++checks;                                                         \
        if (!(c)) {                                                       \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);           \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

// the loop: per packet, is it a Reset; the runs it sees
static std::vector<PsEpoch> loop_epochs(const std::vector<uint8_t> &is_reset) {
    std::vector<PsEpoch> out;
    const uint64_t n = is_reset.size();
    bool seen_reset = false, open = false;
    PsEpoch cur{0, 0, false, false};
    for (uint64_t i = 0; i < n; ++i) {
        if (is_reset[i]) {
            if (open) out.push_back(cur);
            open = false;
            seen_reset = true;
            continue;
        }
        if (!open) {
            cur = PsEpoch{i, i, seen_reset, false};
            open = true;
        }
        cur.hi = i + 1;
    }
    if (open) {
        cur.tail = true;
        out.push_back(cur);
    }
    return out;
}

static void check_epochs(const std::vector<uint8_t> &is_reset, std::mt19937_64 &rng) {
    const uint64_t n = is_reset.size();
    std::vector<uint32_t> resets;
    for (uint64_t i = 0; i < n; ++i)
        if (is_reset[i]) resets.push_back((uint32_t)i);
    std::shuffle(resets.begin(), resets.end(), rng);   // the device lists them in any order
    std::vector<PsEpoch> got(resets.size() + 1);
    const size_t ne = ps_epochs(resets.data(), resets.size(), n, got.data());
    CHECK(ne <= resets.size() + 1);
    got.resize(ne);
    CHECK(std::is_sorted(resets.begin(), resets.end()));
    const std::vector<PsEpoch> want = loop_epochs(is_reset);
    CHECK(got.size() == want.size());
    uint64_t covered = 0;
    for (size_t k = 0; k < got.size(); ++k) {
        CHECK(got[k].lo == want[k].lo && got[k].hi == want[k].hi);
        CHECK(got[k].fresh == want[k].fresh && got[k].tail == want[k].tail);
        CHECK(got[k].lo < got[k].hi && got[k].hi <= n);
        for (uint64_t i = got[k].lo; i < got[k].hi; ++i) CHECK(!is_reset[i]);
        covered += got[k].hi - got[k].lo;
    }
    CHECK(covered + resets.size() == n);
    // only the last epoch can be the tail, and it is one iff the last packet is no Reset
    for (size_t k = 0; k + 1 < got.size(); ++k) CHECK(!got[k].tail);
    CHECK((n && !is_reset[n - 1]) == (!got.empty() && got.back().tail));
}

static void check_rank(const std::vector<uint32_t> &mark) {
    const uint64_t m = mark.size(), rows = ps_rows(m);
    CHECK(rows * PS_ROW >= m && (rows == 0 || (rows - 1) * PS_ROW < m));
    std::vector<uint32_t> padded(rows * PS_ROW, 0), within(rows * PS_ROW), tot(rows), rpre(rows);
    std::copy(mark.begin(), mark.end(), padded.begin());
    for (uint64_t r = 0; r < rows; ++r) {   // k_row_scan: exclusive within the row, the row's total
        uint32_t run = 0;
        for (uint32_t c = 0; c < PS_ROW; ++c) {
            within[r * PS_ROW + c] = run;
            run += padded[r * PS_ROW + c];
        }
        tot[r] = run;
    }
    uint32_t run = 0;
    for (uint64_t r = 0; r < rows; ++r) {   // k_tot_scan
        rpre[r] = run;
        run += tot[r];
    }
    uint64_t next = 0;
    for (uint64_t i = 0; i < m; ++i)
        if (mark[i]) CHECK(ps_rank(rpre.data(), within.data(), i) == next++);
}

int main() {
    std::mt19937_64 rng(12345);
    // every pattern of up to 10 packets
    for (uint32_t n = 0; n <= 10; ++n)
        for (uint32_t bits = 0; bits < (1u << n); ++bits) {
            std::vector<uint8_t> r(n);
            for (uint32_t i = 0; i < n; ++i) r[i] = (bits >> i) & 1;
            check_epochs(r, rng);
        }
    // random batches: rare Resets, dense Resets, runs of them
    for (int round = 0; round < 300; ++round) {
        const uint64_t n = 1 + rng() % 5000;
        const double p = round % 3 == 0 ? 0.001 : round % 3 == 1 ? 0.05 : 0.6;
        std::vector<uint8_t> r(n);
        for (auto &x : r) x = (rng() % 100000) < p * 100000;
        if (round % 7 == 0) r[0] = 1;
        if (round % 11 == 0) r[n - 1] = 1;
        if (round % 13 == 0 && n > 3) r[n / 2] = r[n / 2 + 1] = 1;
        check_epochs(r, rng);
    }
    // the send-order ranks: sizes around a scan row, every density
    const uint64_t sizes[] = {0, 1, 2, PS_ROW - 1, PS_ROW, PS_ROW + 1, 3 * PS_ROW, 3 * PS_ROW + 7, 50000};
    for (uint64_t m : sizes)
        for (int d = 0; d < 4; ++d) {
            std::vector<uint32_t> mark(m);
            for (auto &x : mark) x = d == 0 ? 0 : d == 1 ? 1 : (rng() % (d == 2 ? 2 : 97)) == 0;
            check_rank(mark);
        }
    printf("pktsnap_plan_check: ok %llu checks\n", (unsigned long long)checks);
    return 0;
}
