// lazy_product_check.cpp — CPU check of the lazy product's remainder taken
// straight from the quotient word (sidekick_amd/csrc/field.h mulfold32_min:
// r = Pl + 5 Qh) against the earlier form r = Ql + 5 (Qh - Ph), written out
// here literally.
//
//   lazy_product_check check              edge operands and random pairs
//   lazy_product_check chain NB NA ID...  each id through the (NB, NA) kernel's
//                                         power chain (NB - 1 babies by x, then
//                                         NA - 2 giants by x^NB) and through
//                                         the 8-step baby chain with 8 giants;
//                                         at least one product of the (NB, NA)
//                                         chain must really wrap
// On every product: old == new; r == y x (mod p) whenever Ql + 5 th < 2^32, and
// r < 25 otherwise; mulfold32_exact is congruent always.
// Built and run by tests/test_lazy_product_native.py (also under ASan + UBSan).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../sidekick_amd/csrc/field.h"

using namespace qk;
typedef unsigned __int128 u128;

static int fails = 0;
static long wraps_seen = 0;
#define EXPECT(c, ...)                                                                             \
    do {                                                                                           \
        if (!(c)) {                                                                                \
            if (fails < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
            ++fails;                                                                               \
        }                                                                                          \
    } while (0)

// the form before the change, literally; *sum is the integer Ql + 5 th
static uint32_t old_mulfold32_min(uint32_t y, uint32_t x, uint64_t *sum) {
    const uint64_t P = (uint64_t)y * x;
    const uint32_t Ph = (uint32_t)(P >> 32);
    const uint64_t Q = P + (uint64_t)Ph * 5u;
    const uint32_t tl = (uint32_t)Q, th = (uint32_t)(Q >> 32) - Ph;
    *sum = (uint64_t)tl + 5ull * th;
    return tl + th * 5u;
}

// one product: all properties; returns the new form's r; *wrapped: the sum passed 2^32
static uint32_t check_product(uint32_t y, uint32_t x, bool *wrapped = nullptr) {
    uint64_t sum;
    const uint32_t ro = old_mulfold32_min(y, x, &sum);
    uint32_t mn = 0xFFFFFFFFu;
    const uint32_t rn = mulfold32_min(y, x, mn);
    const uint32_t want = (uint32_t)((u128)y * x % P32);
    EXPECT(rn == ro, "new %u != old %u (y=%u x=%u)", rn, ro, y, x);
    EXPECT(mn == rn, "minimum not tracked (y=%u x=%u)", y, x);
    EXPECT(sum < (1ull << 32) + 25, "th > 5 (y=%u x=%u)", y, x);
    const bool w = sum >= (1ull << 32);
    if (!w) EXPECT(rn % P32 == want, "r=%u not congruent without a wrap (y=%u x=%u)", rn, y, x);
    else EXPECT(rn < 25u, "wrapped sum left r=%u >= 25 (y=%u x=%u)", rn, y, x);
    if (w) ++wraps_seen;
    if (wrapped) *wrapped = w;
    const uint32_t e = mulfold32_exact(y, x);
    EXPECT(e % P32 == want, "exact %u not congruent (y=%u x=%u)", e, y, x);
    if (!w) EXPECT(e == rn, "exact != lazy without a wrap (y=%u x=%u)", y, x);
    else EXPECT(e == rn + 5u, "exact != r + 5 after a wrap (y=%u x=%u)", y, x);
    return rn;
}

static uint64_t rng_state = 0x51DE1C4;
static uint32_t r32() {
    rng_state += GAMMA;
    return (uint32_t)(splitmix_mix(rng_state) >> 32);
}

static int run_check(long pairs) {
    const uint32_t edges[] = {0u, 1u, 4u, 5u, 6u, P32 - 1, P32, 0xFFFFFFFFu, 0x80000000u, 0xCCCCCCCDu};
    for (uint32_t y : edges)
        for (uint32_t x : edges) check_product(y, x);
    for (uint32_t y : edges)
        for (int i = 0; i < 1000; ++i) {
            const uint32_t x = r32();
            check_product(y, x);
            check_product(x, y);
        }
    for (long i = 0; i < pairs; ++i) check_product(r32(), r32());
    printf("lazy_product_check: %s (%d failures, %ld pairs, %ld wrapped)\n", fails ? "FAIL" : "ok", fails, pairs,
           wraps_seen);
    return fails ? 1 : 0;
}

// the kernels' chain (bsgs.h powers): the id is not reduced first
static long chain(uint32_t id, int NB, int NA) {
    long w = 0;
    bool wr;
    uint32_t b = id;
    for (int k = 1; k < NB; ++k) { b = check_product(b, id, &wr); w += wr; }
    uint32_t a = b;
    for (int k = 1; k < NA - 1; ++k) { a = check_product(a, b, &wr); w += wr; }
    return w;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "check")) return run_check(argc >= 3 ? atol(argv[2]) : 10000000L);
    if (argc >= 5 && !strcmp(argv[1], "chain")) {
        const int NB = atoi(argv[2]), NA = atoi(argv[3]);
        for (int i = 4; i < argc; ++i) {
            const uint32_t id = (uint32_t)strtoull(argv[i], 0, 0);
            EXPECT(chain(id, NB, NA) >= 1, "id %u does not wrap in the (%d, %d) chain", id, NB, NA);
            chain(id, 8, 10);
        }
        printf("lazy_product_check chain %dx%d: %s (%d failures, %ld wrapped products)\n", NB, NA, fails ? "FAIL" : "ok",
               fails, wraps_seen);
        return fails ? 1 : 0;
    }
    fprintf(stderr, "usage: lazy_product_check check [PAIRS] | chain NB NA ID...\n");
    return 2;
}
