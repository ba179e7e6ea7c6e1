// rootset_check — the pure host logic of the decode root test
// (sidekick_amd/csrc/rootset.h) against literal models written here.
//
//   1. rt_scan_table, both id widths and both layouts, k = 1 .. 256 distinct
//      canonical roots (0, 1, p - 1 and, for u64, values with a zero low or a
//      zero high word among them): the builder succeeds; S and words are what
//      the layout rule states; every root is found by a literal bucket lookup
//      and 1000 non-roots are not; the slots that hold no root are all-ones.
//   2. the fit boundary of the kernel-argument form: the compact set is
//      within RT_KTAB_BYTES up to k = 55 (u32) / 39 (u64) and over it from
//      k = 56 / 40.
//   3. rt64_bsgs_table for d = 8, 9, 15, 16, 17, 255, 256, 1024: entry
//      out[3k + j] = p_k 2^(22j) mod p by unsigned __int128, zero padding
//      coefficients, 24 ceil(d / 8) words.
//   4. the slot reader over hand-built slot images: empty, one hit, exactly
//      SMALL_HITPF_N hits, stops in any order (the minimum wins), overflow;
//      clear and restore leave every slot all-ones.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <set>
#include <vector>

#include "../../sidekick_amd/csrc/rootset.h"

using namespace qk;

static int fails = 0;
static size_t checks = 0;
static void expect(bool ok, const char *what, uint64_t a, uint64_t b) {
    ++checks;
    if (!ok && fails++ < 10) printf("rootset_check: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
}

template <typename T> static constexpr T modulus() { return sizeof(T) == 4 ? (T)P32 : (T)P64; }

template <typename T> static std::vector<T> special_roots() {
    const T p = modulus<T>();
    std::vector<T> s = {0, 1, (T)(p - 1)};
    if (sizeof(T) == 8) {
        const uint64_t more[] = {1ull << 32, 0xFFFFFFFF00000000ull, 0x00000000DEADBEEFull, 5ull << 32, 0xFFFFFFFFull};
        for (uint64_t v : more) s.push_back((T)v);
    }
    return s;
}

// the literal lookup: the bucket of x, then its S slots
template <typename T> static bool lookup(const std::vector<T> &tab, const RtScanSet &set, T x) {
    uint32_t h = (uint32_t)x * set.m1;
    if (sizeof(T) == 8) h += (uint32_t)((uint64_t)x >> 32) * set.m2;
    const size_t bucket = h >> set.shift;
    for (uint32_t j = 0; j < set.S; ++j)
        if (tab[bucket * set.S + j] == x) return true;
    return false;
}

template <typename T> static void check_sets(uint64_t seed) {
    std::mt19937_64 rng(seed);
    const T p = modulus<T>();
    const std::vector<T> special = special_roots<T>();
    for (uint32_t k = 1; k <= 256; ++k) {
        // distinct canonical roots: the specials (rotated, so that small k see all of them), then random ones
        std::vector<T> roots;
        std::set<T> have;
        for (size_t i = 0; i < special.size() && roots.size() < k; ++i) {
            const T v = special[(i + k) % special.size()];
            if (have.insert(v).second) roots.push_back(v);
        }
        while (roots.size() < k) {
            const T v = (T)(rng() % p);
            if (have.insert(v).second) roots.push_back(v);
        }
        std::shuffle(roots.begin(), roots.end(), rng);
        for (int compact = 0; compact < 2; ++compact) {
            RtScanSet set;
            std::vector<T> tab;
            const bool built = rt_scan_table<T>(roots.data(), k, set, tab, compact != 0);
            expect(built, "builder failed", k, compact);
            if (!built) continue;
            // the layout rule: S = 1 with 2^b >= 2 k^2 up to 32 roots, else S = 4
            // with 2^b >= 2k; compact S = 1 with 2^b >= k^2 / 6; b >= 4
            const uint32_t S = compact || k <= 32 ? 1 : 4;
            uint32_t b = 4;
            if (compact) while (6ull << b < (uint64_t)k * k) ++b;
            else if (S == 1) while (1ull << b < 2ull * k * k) ++b;
            else while (1ull << b < 2ull * k) ++b;
            expect(set.S == S, "S", k, set.S);
            expect(set.words == (S << b), "words", k, set.words);
            expect(set.shift == 32 - b, "shift", k, set.shift);
            expect(tab.size() == set.words, "table size", k, tab.size());
            expect((set.m1 & 1) && (set.m2 & 1), "even multiplier", set.m1, set.m2);
            if (tab.size() != set.words) continue;
            for (T r : roots) expect(lookup<T>(tab, set, r), "root not found", k, (uint64_t)r);
            for (int i = 0; i < 1000;) {
                const T v = (T)(rng() % p);
                if (have.count(v)) continue;
                expect(!lookup<T>(tab, set, v), "non-root found", k, (uint64_t)v);
                ++i;
            }
            size_t used = 0;
            for (T w : tab) {
                if (w == (T)~(T)0) continue;
                ++used;
                expect(have.count(w) == 1, "a slot holds neither a root nor all-ones", k, (uint64_t)w);
            }
            expect(used == k, "slots used", k, used);
        }
    }
}

template <typename T> static size_t compact_bytes(uint32_t k) {
    std::vector<T> roots(k), tab;
    for (uint32_t i = 0; i < k; ++i) roots[i] = (T)(1000003ull * (i + 1));
    RtScanSet set;
    expect(rt_scan_table<T>(roots.data(), k, set, tab, true), "builder failed (fit)", k, sizeof(T));
    return set.words * sizeof(T);
}

static void check_fit() {
    expect(RT_KTAB_BYTES == 2048, "RT_KTAB_BYTES", RT_KTAB_BYTES, 2048);
    for (uint32_t k = 1; k <= 55; ++k) expect(compact_bytes<uint32_t>(k) <= RT_KTAB_BYTES, "u32 set must fit", k, 0);
    for (uint32_t k = 56; k <= 64; ++k) expect(compact_bytes<uint32_t>(k) > RT_KTAB_BYTES, "u32 set must not fit", k, 0);
    for (uint32_t k = 1; k <= 39; ++k) expect(compact_bytes<uint64_t>(k) <= RT_KTAB_BYTES, "u64 set must fit", k, 0);
    for (uint32_t k = 40; k <= 64; ++k) expect(compact_bytes<uint64_t>(k) > RT_KTAB_BYTES, "u64 set must not fit", k, 0);
}

static void check_bsgs() {
    std::mt19937_64 rng(64);
    for (uint32_t d : {8u, 9u, 15u, 16u, 17u, 255u, 256u, 1024u}) {
        std::vector<uint64_t> c(d);
        for (auto &v : c) v = rng() % P64;
        c[0] = P64 - 1;
        if (d > 9) c[9] = 0;
        const size_t words = 24 * (size_t)((d + 7) / 8);
        std::vector<uint64_t> out(words + 8, 0xA5A5A5A5A5A5A5A5ull);   // guard words behind
        expect(rt64_bsgs_table(c.data(), d, out.data()) == words, "bsgs words", d, words);
        for (size_t k = 0; k < words / 3; ++k) {
            const uint64_t pk = k > d ? 0 : k == d ? 1 : c[d - k - 1];   // coefficient of x^k
            for (int j = 0; j < 3; ++j) {
                unsigned __int128 v = pk;
                for (int q = 0; q < 22 * j; ++q) v = (v << 1) % P64;
                expect(out[3 * k + j] == (uint64_t)v, "bsgs entry", d, 3 * k + j);
                if (k > d) expect(out[3 * k + j] == 0, "bsgs padding", d, 3 * k + j);
            }
        }
        for (size_t i = words; i < out.size(); ++i) expect(out[i] == 0xA5A5A5A5A5A5A5A5ull, "bsgs wrote past", d, i);
    }
}

static void check_slots() {
    std::vector<uint64_t> img(SMALL_WORDS, 0x1111111111111111ull);
    const RtSlots slots{img.data()};
    auto all_ones = [&] {
        bool ok = img[SMALL_OVF] == 0;
        for (size_t i = SMALL_HITPF; i < SMALL_WORDS; ++i) ok &= img[i] == ~0ull;
        return ok;
    };
    expect(SMALL_HITPF_N + RT_NSTOP == SMALL_WORDS - SMALL_HITPF, "slot counts", SMALL_HITPF_N, RT_NSTOP);
    expect(slots.result() == img.data() + SMALL_NHITS && slots.hits() == img.data() + SMALL_HITPF &&
               slots.done() == img.data() + SMALL_DONE, "slot pointers", 0, 0);
    expect(RT_STOP0 == SMALL_STOPS - SMALL_NHITS && RT_DONE0 == SMALL_DONE - SMALL_NHITS, "kernel offsets", 0, 0);
    // empty
    slots.clear();
    expect(all_ones(), "clear", 0, 0);
    for (size_t i = 0; i < SMALL_NHITS; ++i) expect(img[i] == 0x1111111111111111ull, "clear wrote below the slots", i, 0);
    RtSlotRead r = slots.read();
    expect(r.hits == 0 && r.stop == ~0ull && r.stops == 0 && !r.overflow, "empty image", r.hits, r.stops);
    // one hit
    img[SMALL_HITPF] = 4242;
    r = slots.read();
    expect(r.hits == 1 && r.stop == ~0ull && r.stops == 0 && !r.overflow, "one hit", r.hits, r.stops);
    slots.restore(r);
    expect(all_ones(), "restore after one hit", 0, 0);
    // every hit slot, position 0 among them (a hit at log position 0 is not an empty slot)
    for (size_t i = 0; i < SMALL_HITPF_N; ++i) img[SMALL_HITPF + i] = SMALL_HITPF_N - 1 - i;
    r = slots.read();
    expect(r.hits == SMALL_HITPF_N && r.stops == 0 && r.stop == ~0ull && !r.overflow, "full hit slots", r.hits, r.stops);
    slots.restore(r);
    expect(all_ones(), "restore after full hit slots", 0, 0);
    // stops in any order: the minimum wins, wherever it sits
    const uint64_t stops[] = {900, 17, 5000, 17, 3, 77777};
    for (size_t at = 0; at < 6; ++at) {
        slots.clear();
        for (size_t i = 0; i < 6; ++i) img[SMALL_STOPS + i] = stops[(i + at) % 6];
        img[SMALL_HITPF] = 1;
        img[SMALL_HITPF + 1] = 0;
        r = slots.read();
        expect(r.stop == 3 && r.stops == 6 && r.hits == 2 && !r.overflow, "stops in any order", r.stop, r.stops);
        slots.restore(r);
        expect(all_ones(), "restore after stops", at, 0);
    }
    // every stop slot
    for (uint32_t i = 0; i < RT_NSTOP; ++i) img[SMALL_STOPS + i] = 100 + (i * 7) % RT_NSTOP;
    r = slots.read();
    expect(r.stop == 100 && r.stops == RT_NSTOP && r.hits == 0, "full stop slots", r.stop, r.stops);
    // overflow
    slots.clear();
    img[SMALL_OVF] = 1;
    img[SMALL_HITPF] = 9;
    r = slots.read();
    expect(r.overflow, "overflow flag", 0, 0);
    // the counters a D2H copy left
    img[SMALL_NHITS] = 123456;
    img[SMALL_STOP] = 77;
    r = slots.copied();
    expect(r.hits == 123456 && r.stop == 77 && !r.overflow, "copied counters", r.hits, r.stop);
    slots.clear();
    expect(all_ones(), "clear after overflow", 0, 0);
}

int main() {
    check_sets<uint32_t>(32);
    check_sets<uint64_t>(64);
    check_fit();
    check_bsgs();
    check_slots();
    if (fails) {
        printf("rootset_check: %d failures\n", fails);
        return 1;
    }
    printf("rootset_check: ok %zu checks\n", checks);
    return 0;
}
