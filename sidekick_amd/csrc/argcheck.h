// argcheck.h — argument checks the device entry points share, plain C++
// (tests/native/senderlog_plan_check.cpp checks them on the host).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace qk {

// do the byte ranges [p, p + pn) and [q, q + qn) share a byte?  A null or
// empty range overlaps nothing.
inline bool ranges_overlap(const void *p, size_t pn, const void *q, size_t qn) {
    if (!p || !q || !pn || !qn) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qn && b < a + pn;
}

} // namespace qk
