// snapshot_plan_check — the host plan of the per-flow quACK snapshots
// (sidekick_amd/csrc/snapshots.h) against a literal per-packet loop.
//
// 1. sn_ncuts / sn_cut_pos against a loop that counts every packet of a flow
//    in a wrapping u32 and tests count % f == 0 (sidekick_multi.rs:271-280),
//    base counts on both sides of the 2^32 wrap.
// 2. The kernel chain of snapshots.hip restated on the host over the plan
//    (sn_plan_counts, sn_plan_items): a walk per item of SN_ITEM positions, the
//    chains, the carry-in pass, the empty flows.  Every access is bounds-checked
//    against the sizes the entry point allocates, no scratch row is read before
//    it is written, every snapshot row and final record is written exactly
//    where the per-flow model puts it, and a flow's carry never reaches the
//    next flow.  Two powers (x, x^2) stand for the threshold.
//
//   snapshot_plan_check          edge shapes, then 300 random shapes
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "../../sidekick_amd/csrc/snapshots.h"

using namespace qk;

static int fails = 0;
static void fail(const char *what, size_t shape, uint64_t at) {
    if (fails++ < 10) printf("snapshot_plan_check: %s (shape %zu, at %llu)\n", what, shape, (unsigned long long)at);
}

constexpr uint32_t T = 2;
struct Row {
    uint32_t count = 0, last = 0, s[T] = {0, 0};
    uint32_t seg = 0;
    uint64_t pos = 0;
    int written = 0;
};
struct Sum {
    uint32_t s[T] = {0, 0};
    int written = 0;
};

static void add_id(uint32_t (&s)[T], uint32_t id) {
    const uint32_t x = canon32(id);
    s[0] = add32(s[0], x);
    s[1] = add32(s[1], mul32(x, x));
}

static void check_cuts(size_t shape, uint32_t c0, uint32_t f, uint64_t len) {
    uint32_t c = c0;
    uint64_t r = 0;
    for (uint64_t j = 0; j < len; ++j) {
        if (sn_ncuts(c0, f, j) != r) return fail("sn_ncuts", shape, j);
        ++c;   // wrapping
        if (c % f == 0) {
            if (sn_cut_pos(c0, f, r) != j) return fail("sn_cut_pos", shape, j);
            ++r;
        }
    }
    if (sn_ncuts(c0, f, len) != r) return fail("sn_ncuts at the end", shape, len);
    if (sn_cut_pos(c0, f, r) < len) return fail("a cut past the last one lies inside", shape, r);
}

static void check(size_t shape, uint64_t first, const std::vector<uint64_t> &lens, const std::vector<uint32_t> &c0s,
                  uint32_t f, uint32_t seed) {
    const size_t nseg = lens.size();
    std::vector<uint64_t> offs(nseg + 1);
    offs[0] = first;
    for (size_t g = 0; g < nseg; ++g) offs[g + 1] = offs[g] + lens[g];
    if (!sn_check(offs.data(), nseg)) return fail("valid shape refused", shape, 0);
    std::mt19937 rng(seed);
    std::vector<uint32_t> ids(offs[nseg] + 2);
    for (auto &v : ids) v = rng() | (rng() % 7 == 0 ? 0xFFFFFFF0u : 0u);
    std::vector<Sum> base(nseg);
    for (auto &b : base) b.s[0] = rng() % P32, b.s[1] = rng() % 3 ? rng() % P32 : P32 - 1;

    // the model
    std::vector<Row> want;
    std::vector<Row> want_fin(nseg);
    std::vector<uint64_t> want_offs(nseg + 1, 0);
    for (size_t g = 0; g < nseg; ++g) {
        Row q;
        q.count = c0s[g], q.s[0] = base[g].s[0], q.s[1] = base[g].s[1];
        for (uint64_t p = offs[g]; p < offs[g + 1]; ++p) {
            add_id(q.s, ids[p]);
            ++q.count;
            q.last = ids[p];
            if (q.count % f == 0) {
                q.seg = (uint32_t)g, q.pos = p;
                want.push_back(q);
            }
        }
        want_fin[g] = q;
        want_offs[g + 1] = want.size();
    }

    // the plan
    std::vector<uint64_t> snoff(nseg + 1, ~0ull);
    const uint64_t total = sn_plan_counts(offs.data(), c0s.data(), nseg, f, snoff.data());
    if (total != want.size() || snoff != want_offs) return fail("snap_offsets", shape, total);
    const size_t ni = sn_items(offs.data(), nseg);
    std::vector<uint32_t> g0(ni, ~0u);
    std::vector<SnChain> chains(std::min(nseg, ni) + 1);
    const size_t nc = ni ? sn_plan_items(offs.data(), nseg, g0.data(), chains.data()) : 0;
    if (nc > std::min(nseg, ni)) return fail("more chains than the bound", shape, nc);
    const uint64_t end = offs[nseg];

    std::vector<Row> snap(total), fin(nseg);
    std::vector<Sum> carry(ni + 1), part(ni);
    // the walk (k_sn_walk), item by item
    for (size_t item = 0; item < ni; ++item) {
        const uint64_t lo = offs[0] + (uint64_t)item * SN_ITEM, hi = lo + SN_ITEM < end ? lo + SN_ITEM : end;
        uint32_t g = g0.at(item);
        if (g >= nseg || !(offs[g] <= lo && lo < offs[g + 1])) return fail("g0 does not hold the item's start", shape, item);
        uint64_t fb = offs[g], fe = offs[g + 1];
        bool whole = fb >= lo;
        uint32_t c0 = c0s[g];
        uint64_t r = sn_ncuts(c0, f, lo > fb ? lo - fb : 0), cut = fb + sn_cut_pos(c0, f, r);
        uint32_t run[T] = {whole ? base[g].s[0] : 0u, whole ? base[g].s[1] : 0u};
        auto finish = [&]() {
            if (whole) {
                Row &o = fin.at(g);
                o.s[0] = run[0], o.s[1] = run[1], o.count = c0 + (uint32_t)(fe - fb), o.last = ids.at(fe - 1);
                ++o.written;
            } else {
                part.at(item).s[0] = run[0], part.at(item).s[1] = run[1], ++part.at(item).written;
            }
        };
        for (uint64_t pos = lo; pos < hi; ++pos) {
            if (pos == fe) {
                finish();
                uint32_t q = g + 1;
                while (q < nseg && !(offs[q + 1] > pos)) ++q;
                if (q >= nseg) return fail("no flow holds a position of the item", shape, pos);
                g = q, fb = offs[g], fe = offs[g + 1], whole = true, c0 = c0s[g], r = 0;
                if (fb != pos) return fail("the next flow does not begin where the last ended", shape, pos);
                cut = fb + sn_cut_pos(c0, f, 0);
                run[0] = base[g].s[0], run[1] = base[g].s[1];
            }
            add_id(run, ids.at(pos));
            if (pos == cut) {
                Row &o = snap.at(snoff[g] + r);
                if (snoff[g] + r >= snoff[g + 1]) return fail("a row outside its flow's rows", shape, pos);
                o.s[0] = run[0], o.s[1] = run[1], o.count = c0 + (uint32_t)(pos - fb) + 1u, o.last = ids[pos];
                o.seg = g, o.pos = pos, ++o.written;
                ++r;
                cut = fb + sn_cut_pos(c0, f, r);
            }
        }
        if (fe == hi) finish();
        else if (whole) carry.at(item + 1).s[0] = run[0], carry.at(item + 1).s[1] = run[1], ++carry.at(item + 1).written;
        else part.at(item).s[0] = run[0], part.at(item).s[1] = run[1], ++part.at(item).written;
    }
    // k_sn_chain
    for (size_t c = 0; c < nc; ++c) {
        const SnChain ch = chains[c];
        if (!carry.at(ch.first).written) return fail("a chain starts from an unwritten carry", shape, ch.first);
        Sum v = carry[ch.first];
        for (uint32_t i = 0; i < ch.count; ++i) {
            if (!part.at(ch.first + i).written) return fail("a chain reads an unwritten part", shape, ch.first + i);
            for (uint32_t k = 0; k < T; ++k) v.s[k] = add32(v.s[k], part[ch.first + i].s[k]);
            Sum &o = carry.at(ch.first + i + 1);
            o.s[0] = v.s[0], o.s[1] = v.s[1], ++o.written;
        }
    }
    // k_sn_carry
    for (size_t item = 1; item < ni; ++item) {
        const uint64_t lo = offs[0] + (uint64_t)item * SN_ITEM, hi = lo + SN_ITEM < end ? lo + SN_ITEM : end;
        const uint32_t g = g0[item];
        const uint64_t fb = offs[g], fe = offs[g + 1];
        if (fb >= lo) continue;
        if (carry.at(item).written != 1) return fail("carry-in not written exactly once", shape, item);
        const uint64_t e = fe < hi ? fe : hi;
        const uint64_t r0 = snoff[g] + sn_ncuts(c0s[g], f, lo - fb), r1 = snoff[g] + sn_ncuts(c0s[g], f, e - fb);
        if (r1 - r0 > SN_ITEM) return fail("more rows than positions", shape, item);
        for (uint64_t row = r0; row < r1; ++row)
            for (uint32_t k = 0; k < T; ++k) snap.at(row).s[k] = add32(snap[row].s[k], carry[item].s[k]);
        if (fe <= hi) {
            if (part.at(item).written != 1) return fail("part not written exactly once", shape, item);
            Row &o = fin.at(g);
            for (uint32_t k = 0; k < T; ++k) o.s[k] = add32(carry[item].s[k], part[item].s[k]);
            o.count = c0s[g] + (uint32_t)(fe - fb), o.last = ids.at(fe - 1);
            ++o.written;
        }
    }
    // k_sn_empty
    for (size_t g = 0; g < nseg; ++g)
        if (offs[g] == offs[g + 1]) {
            fin[g].s[0] = base[g].s[0], fin[g].s[1] = base[g].s[1], fin[g].count = c0s[g];
            ++fin[g].written;
        }

    for (size_t i = 0; i < total; ++i) {
        const Row &a = snap[i], &b = want[i];
        if (a.written != 1) return fail("a snapshot row not written exactly once", shape, i);
        if (a.count != b.count || a.last != b.last || a.seg != b.seg || a.pos != b.pos || a.s[0] != b.s[0] || a.s[1] != b.s[1])
            return fail("snapshot row", shape, i);
    }
    for (size_t g = 0; g < nseg; ++g) {
        const Row &a = fin[g], &b = want_fin[g];
        if (a.written != 1) return fail("a final record not written exactly once", shape, g);
        if (a.count != b.count || (lens[g] && a.last != b.last) || a.s[0] != b.s[0] || a.s[1] != b.s[1])
            return fail("final record", shape, g);
    }
}

int main() {
    size_t shape = 0;
    const uint32_t c0s[] = {0, 1, 4, 5, 63, 64, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFF0u, 0xFFFFFFFDu, 0xFFFFFFFEu, 0xFFFFFFFFu};
    const uint32_t fs[] = {1, 2, 3, 5, 7, 8, 64, 65, 0x80000000u, 0xFFFFFFFFu, 0xFFFFFFFBu};
    for (uint32_t c0 : c0s)
        for (uint32_t f : fs) check_cuts(shape++, c0, f, 200);
    // far cuts: the r-th cut and the count of cuts invert each other on both sides of the wrap
    for (uint32_t c0 : c0s)
        for (uint32_t f : fs)
            for (uint64_t r : {0ull, 1ull, 1000ull, 1ull << 20}) {
                const uint64_t p = sn_cut_pos(c0, f, r);
                if (p + 1 < SN_WRAP && (sn_ncuts(c0, f, p) != r || sn_ncuts(c0, f, p + 1) != r + 1)) fail("inverse", shape, r);
                ++shape;
            }

    const uint64_t I = SN_ITEM;
    const uint32_t W3 = 0xFFFFFFFDu;
    check(shape++, 0, {}, {}, 2, 1);
    check(shape++, 5, {0, 0, 0}, {1, 2, 3}, 2, 2);
    check(shape++, 0, {0, 7, 0, 2, 12, 1, 11, 0}, {3, 5, 9, 6, 9, 4, 0, 2}, 5, 3);
    for (uint32_t f : {1u, 3u, 5u, 0x80000000u}) check(shape++, 0, {8, 5, 8}, {W3, 2, W3}, f, 4);
    for (uint32_t f : {1u, 2u, 7u})
        for (uint64_t n : {I - 1, I, I + 1, 2 * I - 2, 2 * I, 2 * I + 2, 3 * I + 17, 6 * I + 34}) {
            check(shape++, 0, {3, n, 5}, {4, 11, 8}, f, 5);
            check(shape++, 3, {n}, {10}, f, 6);
            check(shape++, 0, {n, n, 0, n}, {1, W3, 5, 0}, f, 7);
            check(shape++, 1, {I - 1, 0, 0, I, 1, 3 * I, I - 1}, {0, 1, 2, 3, 4, 5, 6}, f, 8);
        }
    check(shape++, 0, {4, 2400, 9}, {1, 2, 3}, 1000, 9);
    check(shape++, 0, {4, 2400, 9}, {1, 2, 3}, 100000, 10);
    {
        std::vector<uint64_t> lens = {3};
        lens.insert(lens.end(), 200, 0);
        lens.push_back(I + 5);
        lens.insert(lens.end(), 70, 0);
        lens.push_back(4);
        lens.insert(lens.end(), 65, 0);
        std::vector<uint32_t> c(lens.size());
        for (size_t i = 0; i < c.size(); ++i) c[i] = (uint32_t)(i * 3);
        check(shape++, 2, lens, c, 2, 11);
    }
    std::mt19937_64 rng(12345);
    for (int it = 0; it < 300; ++it) {
        const size_t nseg = 1 + rng() % 40;
        std::vector<uint64_t> lens(nseg);
        std::vector<uint32_t> c(nseg);
        for (size_t g = 0; g < nseg; ++g) {
            const uint64_t k = rng() % 10;
            lens[g] = k < 3 ? 0 : k < 7 ? rng() % 9 : k < 9 ? rng() % 700 : rng() % (4 * I);
            c[g] = rng() % 4 == 0 ? (uint32_t)(0u - (uint32_t)(rng() % 3000)) : (uint32_t)rng();
        }
        const uint32_t f = rng() % 3 == 0 ? 1 + (uint32_t)(rng() % 3) : 1 + (uint32_t)(rng() % 300);
        check(shape++, rng() % 5, lens, c, f, (uint32_t)rng());
    }
    if (fails) {
        printf("snapshot_plan_check: %d failures\n", fails);
        return 1;
    }
    printf("snapshot_plan_check: ok %zu shapes\n", shape);
    return 0;
}
