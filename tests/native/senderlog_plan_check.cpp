// senderlog_plan_check — the host plan of the sender log's update
// (sidekick_amd/csrc/senderlog.h) against a literal per-flow list model.
//
// The model tags every input entry (flow, position) and every entry of the
// sorted batch (flow, rank in the flow's send order) and builds each flow's
// output list: the kept tail, then the new entries.  The plan must give the
// model's offsets, and for every output position exactly one item must cover
// it, of the right kind and with the right source; no item is empty or longer
// than DR_ITEM, and sl_items_bound is no less than the item count.
// Then the entry points' overlap test (argcheck.h ranges_overlap) on byte
// ranges of one buffer.
//
//   senderlog_plan_check          edge shapes, then 300 random shapes
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "../../sidekick_amd/csrc/argcheck.h"
#include "../../sidekick_amd/csrc/senderlog.h"

using namespace qk;

struct Src {
    uint32_t kind;
    uint64_t pos;
};

static int fails = 0;
static void fail(const char *what, size_t shape, uint64_t at) {
    if (fails++ < 10) printf("senderlog_plan_check: %s (shape %zu, at %llu)\n", what, shape, (unsigned long long)at);
}

// lens, drains (empty: NULL drain), counts (empty: NULL counts) per flow; first: offsets[0]
static void check(size_t shape, uint64_t first, const std::vector<uint64_t> &lens, const std::vector<uint64_t> &drains,
                  const std::vector<uint32_t> &counts) {
    const size_t nseg = lens.size();
    std::vector<uint64_t> offs(nseg + 1);
    offs[0] = first;
    for (size_t g = 0; g < nseg; ++g) offs[g + 1] = offs[g] + lens[g];
    const uint64_t *dr = drains.empty() ? nullptr : drains.data();
    const uint32_t *cn = counts.empty() ? nullptr : counts.data();
    uint64_t kept = ~0ull;
    size_t kept_items = ~(size_t)0;
    if (!sl_check(offs.data(), dr, nseg, &kept, &kept_items)) return fail("valid shape refused", shape, 0);
    // the model: per flow a list of sources
    std::vector<Src> want;
    std::vector<uint64_t> want_offs(nseg + 1, 0);
    uint64_t sorted_at = 0, n_new = 0;
    for (size_t g = 0; g < nseg; ++g) {
        std::vector<Src> flow;
        for (uint64_t p = offs[g] + (dr ? dr[g] : 0); p < offs[g + 1]; ++p) flow.push_back({DR_KEPT, p});
        for (uint32_t r = 0; cn && r < cn[g]; ++r) flow.push_back({DR_NEW, sorted_at + r});
        sorted_at += cn ? cn[g] : 0;
        n_new += cn ? cn[g] : 0;
        want.insert(want.end(), flow.begin(), flow.end());
        want_offs[g + 1] = want.size();
    }
    // the counts back from the run starts of the sorted batch
    if (cn) {
        std::vector<uint32_t> h(nseg);
        uint64_t at = 0;
        for (size_t g = 0; g < nseg; ++g) {
            h[g] = cn[g] ? (uint32_t)at : SL_NONE;
            at += cn[g];
        }
        if (!sl_counts_from_starts(h.data(), nseg, n_new)) return fail("valid starts refused", shape, 0);
        for (size_t g = 0; g < nseg; ++g)
            if (h[g] != cn[g]) return fail("counts from starts differ", shape, g);
    }
    if (kept != want.size() - n_new) return fail("sl_check's kept total differs from the model", shape, kept);
    std::vector<uint64_t> out(nseg + 1, ~0ull);
    const size_t ni = sl_plan(offs.data(), dr, cn, nseg, out.data(), nullptr);   // offsets alone (over capacity)
    for (size_t g = 0; g <= nseg; ++g)
        if (out[g] != want_offs[g]) return fail("offsets_out differs from the model", shape, g);
    if (sl_items_bound(kept_items, nseg, n_new) < ni) fail("sl_items_bound below the item count", shape, ni);
    std::vector<DrItem> items(ni + 1, DrItem{~0ull, ~0ull, 0xFFFFFFFFu, 0xFFFFFFFFu});
    out.assign(nseg + 1, ~0ull);
    const size_t k = sl_plan(offs.data(), dr, cn, nseg, out.data(), items.data());
    if (k != ni) return fail("sl_plan wrote another number of items than it counted", shape, k);
    if (items[ni].n != 0xFFFFFFFFu) return fail("sl_plan wrote past its items", shape, ni);
    for (size_t g = 0; g <= nseg; ++g)
        if (out[g] != want_offs[g]) return fail("offsets_out differs from the model (with items)", shape, g);
    size_t nk = 0;
    for (size_t j = 0; j < ni; ++j) nk += items[j].kind == DR_KEPT;
    if (nk != kept_items) return fail("sl_check's kept item count differs from the plan's", shape, nk);
    std::vector<uint32_t> covered(want.size(), 0);
    for (size_t j = 0; j < ni; ++j) {
        const DrItem &it = items[j];
        if (it.n == 0 || it.n > DR_ITEM) return fail("item of a bad length", shape, j);
        if (it.kind != DR_KEPT && it.kind != DR_NEW) return fail("item of a bad kind", shape, j);
        if (it.dst + it.n > want.size()) return fail("item past the output", shape, j);
        for (uint32_t e = 0; e < it.n; ++e) {
            const Src &w = want[it.dst + e];
            if (covered[it.dst + e]++) return fail("output position covered twice", shape, it.dst + e);
            if (w.kind != it.kind || w.pos != it.src + e) return fail("wrong source", shape, it.dst + e);
        }
    }
    for (size_t p = 0; p < want.size(); ++p)
        if (!covered[p]) return fail("output position not covered", shape, p);
}

int main() {
    size_t shape = 0;
    const uint64_t edge[] = {0, 1, 2047, 2048, 2049, 4097};
    // kept entries and new runs of every edge length against each other, at an even and an odd first offset
    for (uint64_t first : {0ull, 3ull}) {
        std::vector<uint64_t> lens, drains;
        std::vector<uint32_t> counts;
        for (uint64_t kept : edge)
            for (uint64_t add : edge) {
                const uint64_t d = (kept + add) % 5;
                lens.push_back(kept + d);
                drains.push_back(d);
                counts.push_back((uint32_t)add);
            }
        check(shape++, first, lens, drains, counts);
        check(shape++, first, lens, {}, counts);        // drain == NULL
        check(shape++, first, lens, drains, {});        // an empty batch: the drain alone
        check(shape++, first, lens, lens, counts);      // drain equal to the segment
        check(shape++, first, lens, lens, {});          // nothing left at all
        check(shape++, first, std::vector<uint64_t>(7, 0), {}, {});   // empty flows only
    }
    check(shape++, 0, {}, {}, {});   // no flow
    // refusals
    {
        const uint64_t dec[3] = {0, 5, 4}, ok[3] = {0, 5, 9}, dr[2] = {6, 0};
        uint64_t kept;
        size_t ki;
        if (sl_check(dec, nullptr, 2, &kept, &ki)) fail("decreasing offsets accepted", shape, 0);
        if (sl_check(ok, dr, 2, &kept, &ki)) fail("over-long drain accepted", shape, 0);
        if (!sl_check(ok, nullptr, 2, &kept, &ki) || kept != 9 || ki != 2) fail("valid offsets refused", shape, 0);
    }
    {
        uint32_t a[3] = {0, 5, 3}, b[3] = {1, SL_NONE, 4}, c[3] = {0, SL_NONE, 9}, d[2] = {SL_NONE, SL_NONE};
        if (sl_counts_from_starts(a, 3, 9)) fail("descending starts accepted", shape, 0);
        if (sl_counts_from_starts(b, 3, 9)) fail("starts that leave out position 0 accepted", shape, 0);
        if (sl_counts_from_starts(c, 3, 9)) fail("a start at the batch's end accepted", shape, 0);
        if (sl_counts_from_starts(d, 2, 4)) fail("no start for a batch with entries accepted", shape, 0);
    }
    {
        const char buf[64] = {0};
        const char *p = buf;
        if (ranges_overlap(p, 16, p + 32, 16)) fail("disjoint ranges overlap", shape, 0);
        if (ranges_overlap(p, 16, p + 16, 16) || ranges_overlap(p + 16, 16, p, 16))
            fail("touching ranges overlap", shape, 0);
        if (!ranges_overlap(p, 17, p + 16, 16) || !ranges_overlap(p + 16, 16, p, 17))
            fail("ranges sharing one byte do not overlap", shape, 0);
        if (!ranges_overlap(p, 64, p + 8, 4) || !ranges_overlap(p + 8, 4, p, 64)) fail("nested ranges do not overlap", shape, 0);
        if (!ranges_overlap(p, 8, p, 8)) fail("equal ranges do not overlap", shape, 0);
        if (ranges_overlap(nullptr, 8, p, 8) || ranges_overlap(p, 8, nullptr, 8)) fail("a null range overlaps", shape, 0);
        if (ranges_overlap(p + 4, 0, p, 8) || ranges_overlap(p, 8, p + 4, 0)) fail("an empty range overlaps", shape, 0);
    }
    std::mt19937_64 rng(0x5E4DE7106ull);
    for (int r = 0; r < 300; ++r) {
        const size_t nseg = 1 + rng() % 40;
        std::vector<uint64_t> lens(nseg), drains(nseg);
        std::vector<uint32_t> counts(nseg);
        for (size_t g = 0; g < nseg; ++g) {
            const uint64_t big = rng() % 8 == 0 ? 5000 : 70;
            lens[g] = rng() % 4 == 0 ? 0 : rng() % big;
            drains[g] = rng() % 3 == 0 ? lens[g] : rng() % (lens[g] + 1);
            counts[g] = rng() % 4 == 0 ? 0 : (uint32_t)(rng() % big);
        }
        check(shape++, rng() % 9, lens, rng() % 5 == 0 ? std::vector<uint64_t>{} : drains,
              rng() % 7 == 0 ? std::vector<uint32_t>{} : counts);
    }
    if (fails) {
        printf("senderlog_plan_check: FAIL (%d)\n", fails);
        return 1;
    }
    printf("senderlog_plan_check: ok %zu shapes\n", shape);
    return 0;
}
