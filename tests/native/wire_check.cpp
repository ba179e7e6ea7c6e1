// Native check of wire.h, the per-image rules the device wire leg shares with
// the host: wire_validate over the malformed and edge images of the ingest
// tests against a table of statuses written out here, every image at the end
// of an exactly sized heap block (a read past `len` is an ASan error); and
// wire_byte / wire_dword against a literal packer of the bincode layout.
// Stand-alone: g++ -std=c++17 -I include -I sidekick_amd/csrc wire_check.cpp
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "wire.h"

using namespace qk;

static int checks = 0, failures = 0;
#define EXPECT(cond, ...)                                                                                          \
    do {                                                                                                           \
        ++checks;                                                                                                  \
        if (!(cond)) {                                                                                             \
            ++failures;                                                                                            \
            printf("FAIL %s:%d: ", __FILE__, __LINE__);                                                            \
            printf(__VA_ARGS__);                                                                                   \
            printf("\n");                                                                                          \
        }                                                                                                          \
    } while (0)

typedef std::vector<uint8_t> Bytes;
static void le(Bytes &b, uint64_t v, int n) {
    for (int i = 0; i < n; ++i) b.push_back((uint8_t)(v >> (8 * i)));
}
// the layout, literally: u64 threshold | sums | tag | last (tag 1) | count
static Bytes pack(uint64_t threshold, const std::vector<uint32_t> &sums, int tag, uint32_t last, uint32_t count,
                  bool with_last) {
    Bytes b;
    le(b, threshold, 8);
    for (uint32_t s : sums) le(b, s, 4);
    b.push_back((uint8_t)tag);
    if (with_last) le(b, last, 4);
    le(b, count, 4);
    return b;
}

// every share of the sums, one caller and 64 lanes: the image is accepted when all return QK_OK;
// a refusal is the same in every share that refuses, and any QK_E_FORMAT share makes it QK_E_FORMAT
static int validate(const Bytes &img, uint64_t len, uint64_t room, uint32_t T) {
    // the image's first `len` bytes (or all of it when len is larger: then no byte may be read at all)
    const size_t have = len < img.size() ? (size_t)len : img.size();
    uint8_t *block = (uint8_t *)malloc(have ? have : 1);
    const uint8_t *p = block + (have ? 0 : 1);      // have == 0: one past the block, nothing readable
    if (have) memcpy(block, img.data(), have);
    const int one = wire_validate(p, len, room, T, 0, 1);
    int all = QK_OK;
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const int st = wire_validate(p, len, room, T, lane, 64);
        if (st == QK_E_FORMAT || (st && all == QK_OK)) all = st;
    }
    free(block);
    EXPECT(one == all, "one caller %d, 64 lanes %d", one, all);
    return one;
}

struct Case {
    std::string what;
    Bytes img;
    uint64_t len, room;
    int want;
};

static void validator_table(uint32_t T) {
    std::vector<uint32_t> ok(T), top(T, QK_P32 - 1);
    for (uint32_t k = 0; k < T; ++k) ok[k] = 0x01020304u * (k + 1) % QK_P32;
    const Bytes v1 = pack(T, ok, 1, 0xDEADBEEF, 7, true), v0 = pack(T, ok, 0, 0, 0xFFFFFFFFu, false);
    std::vector<Case> cs;
    auto add = [&](const char *what, Bytes img, int want, uint64_t len = ~0ull, uint64_t room = 1 << 20) {
        cs.push_back({what, img, len == ~0ull ? img.size() : len, room, want});
    };
    add("valid, tag 1", v1, QK_OK);
    add("valid, tag 0", v0, QK_OK);
    add("sums p - 1", pack(T, top, 1, 1, 2, true), QK_OK);
    add("len 0", v1, QK_E_FORMAT, 0);
    add("len 7", v1, QK_E_FORMAT, 7);
    add("len 8", v1, QK_E_FORMAT, 8);
    add("len 4t + 12", v0, QK_E_FORMAT, 4 * (uint64_t)T + 12);
    add("tag 2", pack(T, ok, 2, 5, 6, true), QK_E_FORMAT);
    add("tag 0 at the tag-1 length", pack(T, ok, 0, 5, 6, true), QK_E_FORMAT);
    add("tag 1 at the tag-0 length", pack(T, ok, 1, 0, 6, false), QK_E_FORMAT);
    {
        Bytes x = v1;
        x.push_back(0);
        add("one trailing byte, tag 1", x, QK_E_FORMAT);
        x = v0;
        x.push_back(0);
        add("one trailing byte, tag 0", x, QK_E_FORMAT);
    }
    add("threshold t + 1, consistent", pack(T + 1, std::vector<uint32_t>(T + 1, 3), 1, 5, 6, true), QK_E_MISMATCH);
    add("threshold t - 1, consistent", pack(T - 1, std::vector<uint32_t>(T - 1, 3), 0, 0, 6, false), QK_E_MISMATCH);
    add("threshold t + 1, sums not canonical", pack(T + 1, std::vector<uint32_t>(T + 1, QK_P32), 1, 5, 6, true),
        QK_E_MISMATCH);   // deser's order: the threshold is compared before the sums
    add("threshold 2^32 - 1", pack(0xFFFFFFFFull, ok, 1, 5, 6, true), QK_E_FORMAT);
    add("threshold 2^32", pack(1ull << 32, ok, 1, 5, 6, true), QK_E_FORMAT);
    add("threshold 2^32 + t", pack((1ull << 32) + T, ok, 1, 5, 6, true), QK_E_FORMAT);
    add("threshold 2^63", pack(1ull << 63, ok, 1, 5, 6, true), QK_E_FORMAT);
    add("threshold 2^62 - 2 (4t wraps in 64 bits)", pack((1ull << 62) - 2, ok, 1, 5, 6, true), QK_E_FORMAT);
    // one sum out of range, the others p - 1 or ordinary: the first and last of a 64-lane share's first,
    // second and third trips, and the image's last two
    std::set<uint32_t> bad_at;
    for (uint32_t at : {0u, 1u, 62u, 63u, 64u, 65u, 126u, 127u, 128u, 129u, T - 2, T - 1})
        if (at < T) bad_at.insert(at);
    for (uint32_t at : bad_at) {
        std::vector<uint32_t> s = top;
        s[at] = QK_P32;
        add("sums p - 1 but one equal to p", pack(T, s, at & 1, 5, 6, at & 1), QK_E_FORMAT);
        s[at] = 0xFFFFFFFFu;
        add("sums p - 1 but one equal to 2^32 - 1", pack(T, s, ~at & 1, 5, 6, ~at & 1), QK_E_FORMAT);
        s = ok;
        s[at] = QK_P32;
        add("a sum equal to p", pack(T, s, 1, 5, 6, true), QK_E_FORMAT);
        s[at] = 0xFFFFFFFFu;
        add("a sum equal to 2^32 - 1", pack(T, s, 0, 0, 6, false), QK_E_FORMAT);
    }
    add("len > stride", v1, QK_E_FORMAT, v1.size(), v1.size() - 1);
    add("len > stride, far", v1, QK_E_FORMAT, 0xFFFFFFFFull, v1.size());
    add("len == stride", v1, QK_OK, v1.size(), v1.size());
    for (const Case &c : cs) {
        const int got = validate(c.img, c.len, c.room, T);
        EXPECT(got == c.want, "t=%u %s: status %d, want %d", T, c.what.c_str(), got, c.want);
    }
    // an accepted image's header
    uint32_t count, has_last, last;
    wire_header(v1.data(), v1.size(), T, count, has_last, last);
    EXPECT(count == 7 && has_last == 1 && last == 0xDEADBEEF, "header of tag 1");
    wire_header(v0.data(), v0.size(), T, count, has_last, last);
    EXPECT(count == 0xFFFFFFFFu && has_last == 0 && last == 0, "header of tag 0");
}

// wire_byte / wire_dword of a record against the packer, every offset up to past the longest image
static void image_of_record(uint32_t T, int has_last, uint32_t count, uint32_t fill) {
    std::vector<uint32_t> rec(4 + T);
    rec[0] = T;
    rec[1] = count;
    rec[2] = has_last ? 1 : 0;
    rec[3] = has_last ? 0xA1B2C3D4u : 0;
    std::vector<uint32_t> sums(T);
    for (uint32_t k = 0; k < T; ++k) sums[k] = rec[4 + k] = fill ? fill : 0x9E3779B9u * (k + 1) % QK_P32;
    const Bytes want = pack(T, sums, rec[2], rec[3], count, has_last);
    EXPECT(wire_len(rec.data(), T) == want.size(), "t=%u length", T);
    auto at = [&](size_t q) { return q < want.size() ? want[q] : 0u; };
    for (uint32_t q = 0; q < 4 * T + 17 + 8; ++q) {
        EXPECT(wire_byte(rec.data(), T, q) == at(q), "t=%u byte %u", T, q);
        const uint32_t w = at(q) | at(q + 1) << 8 | at(q + 2) << 16 | (uint32_t)at(q + 3) << 24;
        EXPECT(wire_dword(rec.data(), T, q) == w, "t=%u dword %u", T, q);
    }
}

int main() {
    // t = 1: threshold 0 is an image of its own; 64, 65, 129: a 64-lane share of one, two and three trips
    for (uint32_t T : {1u, 2u, 7u, 32u, 64u, 65u, 129u, 1024u}) validator_table(T);
    for (uint32_t T : {1u, 2u, 7u, 32u, 64u, 65u, 129u, 1024u})
        for (int has_last = 0; has_last < 2; ++has_last) {
            image_of_record(T, has_last, 0, 0);
            image_of_record(T, has_last, 0xFFFFFFFFu, QK_P32 - 1);
            image_of_record(T, has_last, 0x01020304u, 0);
        }
    if (failures) {
        printf("wire_check: %d of %d checks failed\n", failures, checks);
        return 1;
    }
    printf("wire_check: ok %d checks\n", checks);
    return 0;
}
