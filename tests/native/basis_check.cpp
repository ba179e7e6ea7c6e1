// basis_check.cpp — CPU check of the nine-power basis of the u32 t = 31..32
// encode (sidekick_amd/csrc/basis32.h).
//
//   basis_check table           the table's invariants, recomputed here at run
//                               time independently of the header's static_asserts
//   basis_check chain [IDS]     the lazy chain with the r < 25 redo, then the
//                               table's direct / pair terms, against pow32 for
//                               every power 1..32: IDS random ids (default 10^6)
//                               and the edge ids 0, 1, p-1, p, 2^32-1
//   basis_check wraps P:ID...   each ID's lazy chain must really wrap at the
//                               product of power P (the integer Ql + 5 th passes
//                               2^32 there), trip the redo, and still give every
//                               power right
//   basis_check find [N] [T]    search N ids (default 2^32: all of them) on T
//                               threads for ids whose chain wraps at each of
//                               the eight products; prints "wrap P ID" lines
//                               (up to four per product; tens of seconds)
// Built and run by tests/test_basis_native.py (table and chain also under
// ASan + UBSan).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <thread>
#include <vector>

#include "../../sidekick_amd/csrc/basis32.h"

using namespace qk;
namespace b32 = qk::basis32;

static int fails = 0;
#define EXPECT(c, ...)                                                                             \
    do {                                                                                           \
        if (!(c)) {                                                                                \
            if (fails < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
            ++fails;                                                                               \
        }                                                                                          \
    } while (0)

static int run_table() {
    // E: 1 and the chain's powers, all different, at most 32, operands earlier
    bool in_e[b32::T + 1] = {};
    in_e[1] = true;
    for (int i = 0; i < b32::NP; ++i) {
        const b32::Step s = b32::CHAIN[i];
        EXPECT(s.power >= 2 && s.power <= b32::T, "step %d: power %d", i, s.power);
        EXPECT(s.left + s.right == s.power, "step %d: %d + %d != %d", i, s.left, s.right, s.power);
        EXPECT(s.left <= b32::T && s.right <= b32::T && in_e[s.left] && in_e[s.right],
               "step %d: operand not produced before use", i);
        EXPECT(s.power <= b32::T && !in_e[s.power], "step %d: power %d twice", i, s.power);
        if (s.power <= b32::T) in_e[s.power] = true;
        EXPECT(b32::vidx(s.power) == i + 1, "vidx(%d)", s.power);
    }
    int ne = 0;
    for (int k = 1; k <= b32::T; ++k) ne += in_e[k];
    EXPECT(ne == b32::NE, "|E| = %d", ne);
    // every power: direct (in E) or a pair of elements of E; exactly one accumulator
    int seen[b32::T + 1] = {};
    for (int i = 0; i < b32::ND; ++i) {
        const int k = b32::DIRECT[i];
        EXPECT(k >= 1 && k <= b32::T && in_e[k] && b32::TERM[k].right == 0 && b32::TERM[k].left == k, "direct %d", k);
        if (k >= 1 && k <= b32::T) ++seen[k];
        EXPECT(b32::direct_v(i) == b32::vidx(k), "direct_v(%d)", i);
    }
    for (int i = 0; i < b32::NM; ++i) {
        const int k = b32::MAC[i];
        EXPECT(k >= 1 && k <= b32::T, "pair accumulator %d: power %d", i, k);
        if (k < 1 || k > b32::T) continue;
        const b32::Term t = b32::TERM[k];
        EXPECT(t.right != 0 && t.left <= b32::T && t.right <= b32::T && in_e[t.left] && in_e[t.right] &&
                   t.left + t.right == k,
               "pair %d = %d + %d", k, t.left, t.right);
        ++seen[k];
        EXPECT(b32::mac_l(i) == b32::vidx(t.left) && b32::mac_r(i) == b32::vidx(t.right), "mac_l/r(%d)", i);
    }
    for (int k = 1; k <= b32::T; ++k) EXPECT(seen[k] == 1, "power %d has %d accumulators", k, seen[k]);
    printf("basis_check table: %s (%d failures)\n", fails ? "FAIL" : "ok", fails);
    return fails ? 1 : 0;
}

// the integer sum Ql + 5 th of one lazy product passed 2^32
static bool product_wraps(uint32_t y, uint32_t x) {
    const uint64_t P = (uint64_t)y * x;
    const uint32_t Ph = (uint32_t)(P >> 32);
    const uint64_t Q = P + (uint64_t)Ph * 5u;
    const uint32_t tl = (uint32_t)Q, th = (uint32_t)(Q >> 32) - Ph;
    return (uint64_t)tl + 5ull * th >= (1ull << 32);
}
// bit i set: the chain's product i wraps when every operand is the lazy value
static unsigned chain_wraps(uint32_t id) {
    uint32_t V[b32::NE], mn = 0xFFFFFFFFu;
    unsigned w = 0;
    V[0] = id;
    for (int i = 0; i < b32::NP; ++i) {
        const uint32_t y = V[b32::CIDX.l[i]], x = V[b32::CIDX.r[i]];
        if (product_wraps(y, x)) w |= 1u << i;
        V[i + 1] = mulfold32_min(y, x, mn);
    }
    return w;
}

// what the kernel does with one id; every power against pow32.  Returns
// whether the redo ran.
static bool check_id(uint32_t id) {
    uint32_t V[b32::NE];
    const uint32_t mn = b32::chain_min(id, V);
    const unsigned w = chain_wraps(id);
    const bool redo = mn < b32::WRAP_BELOW;
    EXPECT(!w || redo, "id %u wraps (mask %#x) and the minimum %u does not show it", id, w, mn);
    if (redo) b32::chain_exact(id, V);
    EXPECT(V[0] == id, "V[0]");
    const uint32_t x = id % P32;
    for (int k = 1; k <= b32::T; ++k) {
        const b32::Term t = b32::TERM[k];
        const uint32_t l = V[b32::vidx(t.left)];
        // a direct power is added as it is; a pair as the 64-bit product (the accumulators are folded later)
        const uint32_t got = t.right == 0 ? l % P32 : (uint32_t)((uint64_t)l * V[b32::vidx(t.right)] % P32);
        EXPECT(got == pow32(x, (uint64_t)k), "id %u power %d: %u != %u", id, k, got, pow32(x, (uint64_t)k));
    }
    return redo;
}

static uint64_t rng_state = 0xBA5150032ull;
static uint32_t r32() {
    rng_state += GAMMA;
    return (uint32_t)(splitmix_mix(rng_state) >> 32);
}

static int run_chain(long ids) {
    const uint32_t edges[] = {0u, 1u, P32 - 1, P32, 0xFFFFFFFFu, 2u, 4u, 5u, 0x80000000u};
    long redos = 0;
    for (uint32_t e : edges) redos += check_id(e);
    for (long i = 0; i < ids; ++i) redos += check_id(r32());
    printf("basis_check chain: %s (%d failures, %ld ids, %ld redone)\n", fails ? "FAIL" : "ok", fails, ids, redos);
    return fails ? 1 : 0;
}

static int run_wraps(int argc, char **argv) {
    int n = 0;
    for (int i = 2; i < argc; ++i, ++n) {
        const char *colon = strchr(argv[i], ':');
        if (!colon) { fprintf(stderr, "basis_check wraps: P:ID expected, got %s\n", argv[i]); return 2; }
        const int p = atoi(argv[i]);
        const uint32_t id = (uint32_t)strtoull(colon + 1, 0, 0);
        const int v = p >= 2 && p <= b32::T ? b32::vidx(p) : -1;
        EXPECT(v >= 1, "%d is no product of the chain", p);
        if (v < 1) continue;
        EXPECT(chain_wraps(id) & (1u << (v - 1)), "id %u does not wrap at the product of power %d", id, p);
        EXPECT(check_id(id), "id %u does not trip the redo", id);
    }
    printf("basis_check wraps: %s (%d failures, %d ids)\n", fails ? "FAIL" : "ok", fails, n);
    return fails ? 1 : 0;
}

static int run_find(uint64_t n, int threads) {
    constexpr int KEEP = 4;
    std::vector<std::vector<std::vector<uint32_t>>> found(threads, std::vector<std::vector<uint32_t>>(b32::NP));
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
        pool.emplace_back([&, t]() {
            // thread t walks ids t, t + threads, ... through a bijection of the 32-bit ids
            for (uint64_t i = (uint64_t)t; i < n; i += (uint64_t)threads) {
                const uint32_t id = (uint32_t)i * 2654435761u + 0x9E3779B9u;
                uint32_t V[b32::NE];
                if (b32::chain_min(id, V) >= b32::WRAP_BELOW) continue;
                const unsigned w = chain_wraps(id);
                for (int s = 0; s < b32::NP; ++s)
                    if ((w >> s & 1) && (int)found[t][s].size() < KEEP) found[t][s].push_back(id);
            }
        });
    for (auto &th : pool) th.join();
    int missing = 0;
    for (int s = 0; s < b32::NP; ++s) {
        int k = 0;
        for (int t = 0; t < threads && k < KEEP; ++t)
            for (uint32_t id : found[t][s])
                if (k < KEEP) { printf("wrap %d %u\n", b32::CHAIN[s].power, id); ++k; }
        missing += k == 0;
    }
    printf("basis_check find: %s (%d products without an id, %llu ids searched)\n", missing ? "FAIL" : "ok", missing,
           (unsigned long long)n);
    return missing ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "table")) return run_table();
    if (argc >= 2 && !strcmp(argv[1], "chain")) return run_chain(argc >= 3 ? atol(argv[2]) : 1000000L);
    if (argc >= 3 && !strcmp(argv[1], "wraps")) return run_wraps(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "find")) {
        const uint64_t n = argc >= 3 ? strtoull(argv[2], 0, 0) : (1ull << 32);
        int threads = argc >= 4 ? atoi(argv[3]) : (int)std::thread::hardware_concurrency();
        if (threads < 1) threads = 1;
        if (threads > 64) threads = 64;
        return run_find(n, threads);
    }
    fprintf(stderr, "usage: basis_check table | chain [IDS] | wraps P:ID... | find [N] [THREADS]\n");
    return 2;
}
