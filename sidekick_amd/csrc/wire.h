// wire.h — the bincode image of a PowerSumQuackU32 as the device wire leg
// reads and writes it (wire.hip), plain C++ that the kernels
// and a native CPU program both compile (tests/native/wire_check.cpp):
//   wire_validate   the per-image rules of qk_u32_deserialize (host.cpp deser),
//                   in deser's order — the one copy the ingest kernel runs
//   wire_header     count / has_last / last_value of an accepted image
//   wire_byte/dword the image of a qk_u32 record, addressed by byte offset:
//                   what the emit kernel gathers its aligned stores from
// Image: u64 threshold | threshold x u32 sums | u8 tag | u32 last (tag 1) |
// u32 count; little-endian, nothing aligned (sidekick.rs:187,
// media_client.rs:227).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "quack_hip.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define QK_WIRE_FN __host__ __device__ inline
#else
#define QK_WIRE_FN inline
#endif

namespace qk {

QK_WIRE_FN uint32_t wire_get32(const uint8_t *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// The status qk_u32_deserialize gives the `len` bytes at buf for a sketch
// initialised for `threshold`; room = the bytes the slot holds (len > room:
// QK_E_FORMAT).  No byte at or past min(len, room) is read.  The test of the
// sums is shared out: this call takes sums lane, lane + nlanes, ..; the image
// is accepted when every share returns QK_OK (every rule before the sums gives
// all shares the same answer).  One caller: lane 0 of 1.
QK_WIRE_FN int wire_validate(const uint8_t *buf, uint64_t len, uint64_t room, uint32_t threshold, uint32_t lane,
                             uint32_t nlanes) {
    if (len > room || len < 8) return QK_E_FORMAT;
    if (wire_get32(buf + 4) != 0) return QK_E_FORMAT;   // a threshold above 2^32 - 1
    const uint64_t t = wire_get32(buf);
    const uint64_t body = 8 + 4 * t;                    // < 2^35: 64-bit arithmetic throughout
    if (len < body + 1 + 4) return QK_E_FORMAT;
    const uint8_t tag = buf[body];
    if (tag > 1) return QK_E_FORMAT;
    if (len != body + 1 + (tag ? 4 : 0) + 4) return QK_E_FORMAT;
    if (t != threshold) return QK_E_MISMATCH;
    for (uint64_t k = lane; k < t; k += nlanes)
        if (wire_get32(buf + 8 + 4 * k) >= QK_P32) return QK_E_FORMAT;   // ModularInteger values are canonical
    return QK_OK;
}

// words 1..3 of the qk_u32 record of an image wire_validate accepted
QK_WIRE_FN void wire_header(const uint8_t *buf, uint64_t len, uint32_t threshold, uint32_t &count, uint32_t &has_last,
                            uint32_t &last) {
    const uint64_t body = 8 + 4 * (uint64_t)threshold;
    has_last = buf[body];
    last = has_last ? wire_get32(buf + body + 1) : 0u;
    count = wire_get32(buf + len - 4);
}

// ---- the image of a record (rec: its 4 + T aligned words) by byte offset
QK_WIRE_FN uint32_t wire_len(const uint32_t *rec, uint32_t T) { return 4 * T + 13 + (rec[2] ? 4u : 0u); }
// aligned word i < T + 2 of the image's head: the u64 threshold, then the sums
QK_WIRE_FN uint32_t wire_word(const uint32_t *rec, uint32_t T, uint32_t i) {
    return i == 0 ? T : i == 1 ? 0u : rec[2 + i];
}
// byte q of the image; 0 at and past its end
QK_WIRE_FN uint32_t wire_byte(const uint32_t *rec, uint32_t T, uint32_t q) {
    const uint32_t head = 8 + 4 * T;
    if (q < head) return (wire_word(rec, T, q >> 2) >> (8 * (q & 3))) & 255u;
    uint32_t j = q - head;
    if (j == 0) return rec[2] ? 1u : 0u;
    --j;
    if (rec[2]) {
        if (j < 4) return (rec[3] >> (8 * j)) & 255u;
        j -= 4;
    }
    return j < 4 ? (rec[1] >> (8 * j)) & 255u : 0u;
}
// bytes q .. q + 3 as a little-endian word: inside the head two aligned words
// funnelled, across the tag byte by single bytes
QK_WIRE_FN uint32_t wire_dword(const uint32_t *rec, uint32_t T, uint32_t q) {
    if (q + 4 <= 8 + 4 * T) {
        const uint32_t w = q >> 2, s = 8 * (q & 3), lo = wire_word(rec, T, w);
        return s ? (lo >> s) | (wire_word(rec, T, w + 1) << (32 - s)) : lo;
    }
    return wire_byte(rec, T, q) | wire_byte(rec, T, q + 1) << 8 | wire_byte(rec, T, q + 2) << 16 |
           wire_byte(rec, T, q + 3) << 24;
}

} // namespace qk
