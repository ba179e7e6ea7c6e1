// sender_steps_plan_check — the host side of the queued sender step and of
// the ingest that feeds it (sidekick_amd/csrc/sendersteps.h, sendersteps.hip)
// against a per-packet model.
//
// 1. The queue: wq_offsets over the per-flow counts, and the stable sort by
//    (flow of an accepted datagram | nseg) restated, against per-flow lists
//    filled in arrival order; the sort regions' sizes.
// 2. The step: sq_check, the work items (segdecode.hip sd_items restated), the
//    carved buffers and the LDS sizes of sq_lds, and the kernel chain of
//    sendersteps.hip restated on the host round by round over the items —
//    find, prefix, classify, Newton, root test, remove, finish, then the item
//    counts, the scan and the hit write.  Every access is bounds-checked
//    against the sizes the entry point allocates (LDS arrays included), and
//    every output is compared with a per-flow list model that handles one quACK
//    per loop turn on a list it really drains (media_client.rs:223-323).
//    Threshold 2: the powers x and x^2, Newton of degree <= 2.
//
//   sender_steps_plan_check      edge shapes, then random shapes
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../include/quack_hip.h"
#include "../../sidekick_amd/csrc/field.h"
#include "../../sidekick_amd/csrc/sendersteps.h"

using namespace qk;

static int fails = 0;
static size_t checks = 0;
static void fail(const char *what, size_t shape, uint64_t at) {
    if (fails++ < 10) printf("sender_steps_plan_check: %s (shape %zu, at %llu)\n", what, shape, (unsigned long long)at);
}

constexpr uint32_t T = 2;
constexpr uint32_t ITEM = QK_SEG_DECODE_ITEM, WORDS = ITEM / 64;
constexpr uint64_t NONE = ~0ull;
constexpr uint32_t INV2 = (uint32_t)(((uint64_t)P32 + 1) / 2);

// a buffer of the size the entry point allocates; every access is checked
template <typename V> struct Buf {
    std::vector<V> v;
    const char *name;
    Buf(const char *n, size_t size, V init = V()) : v(size, init), name(n) {}
    V &operator[](uint64_t i) {
        ++checks;
        if (i >= v.size()) {
            fail(name, 0, i);
            static V sink;
            return sink;
        }
        return v[i];
    }
};

struct Rec {
    uint32_t count = 0, has = 0, last = 0, s[T] = {0, 0};
    bool operator==(const Rec &o) const {
        return count == o.count && has == o.has && last == o.last && s[0] == o.s[0] && s[1] == o.s[1];
    }
};
static void rec_insert(Rec &r, uint32_t id) {
    const uint32_t x = canon32(id);
    r.s[0] = add32(r.s[0], x), r.s[1] = add32(r.s[1], mul32(x, x));
    ++r.count, r.has = 1, r.last = id;
}
static void rec_remove(Rec &r, uint32_t id) {
    const uint32_t x = canon32(id);
    r.s[0] = sub32(r.s[0], x), r.s[1] = sub32(r.s[1], mul32(x, x));
    --r.count;
}
// the monic polynomial of a diff of d <= 2 ids from its power sums (Newton), evaluated at x
static bool is_root(const uint32_t *s, uint32_t d, uint32_t id) {
    const uint32_t x = canon32(id);
    const uint32_t c0 = neg32(s[0]);
    if (d == 1) return add32(x, c0) == 0;
    const uint32_t c1 = mul32(neg32(add32(s[1], mul32(s[0], c0))), INV2);
    return add32(mul32(add32(x, c0), x), c1) == 0;
}

struct Item {
    uint64_t lo;
    uint32_t n, seg0, nseg;
};
// segdecode.hip sd_items
static std::vector<Item> items_of(const std::vector<uint64_t> &offs, uint32_t maxseg) {
    std::vector<Item> items;
    const size_t nseg = offs.size() - 1;
    size_t g = 0;
    while (g < nseg) {
        const uint64_t len = offs[g + 1] - offs[g];
        if (len > ITEM) {
            for (uint64_t lo = offs[g]; lo < offs[g + 1]; lo += ITEM)
                items.push_back({lo, (uint32_t)std::min<uint64_t>(ITEM, offs[g + 1] - lo), (uint32_t)g, 1u});
            ++g;
            continue;
        }
        const size_t g0 = g;
        uint64_t tot = 0;
        while (g < nseg && g - g0 < maxseg && offs[g + 1] - offs[g] <= ITEM - tot) tot += offs[g + 1] - offs[g], ++g;
        if (tot) items.push_back({offs[g0], (uint32_t)tot, (uint32_t)g0, (uint32_t)(g - g0)});
    }
    return items;
}

enum { IDLE = 0, ADVANCED = 1, REORDERED = 2, RETX = 4, EXCEEDS = 8, UNSTEPPED = 16 };

struct Shape {
    std::vector<uint64_t> offs, qoffs;
    std::vector<uint32_t> log;
    std::vector<Rec> mine, queue;
};

struct Result {
    std::vector<Rec> mine_out;
    std::vector<uint8_t> q_action;
    std::vector<uint64_t> q_drain, drain, hits, hit_offsets;
    std::vector<uint32_t> stepped;
};

// ---- the model: per flow a list that is really drained, one quACK per turn
static Result model(const Shape &sh) {
    const size_t nseg = sh.offs.size() - 1, nq = sh.queue.size();
    Result r;
    r.mine_out.resize(nseg), r.q_action.assign(nq, UNSTEPPED), r.q_drain.assign(nq, 0), r.drain.assign(nseg, 0);
    r.stepped.assign(nseg, 0), r.hit_offsets.assign(nq + 1, 0);
    std::vector<std::vector<uint64_t>> qhits(nq);
    for (size_t g = 0; g < nseg; ++g) {
        std::vector<uint32_t> list(sh.log.begin() + sh.offs[g], sh.log.begin() + sh.offs[g + 1]);
        uint64_t gone = 0;   // entries drained: a list position + gone + offs[g] is the global position
        Rec m = sh.mine[g];
        for (uint64_t q = sh.qoffs[g]; q < sh.qoffs[g + 1]; ++q) {
            const Rec &p = sh.queue[q];
            r.stepped[g]++;
            if (p.has == m.has && (!p.has || p.last == m.last)) {
                r.q_action[q] = IDLE;
                continue;
            }
            size_t idx = list.size();
            if (p.has)
                for (size_t i = 0; i < list.size(); ++i)
                    if (list[i] == p.last) {
                        idx = i;
                        break;
                    }
            const bool found = idx < list.size();
            if (found)
                for (size_t i = 0; i <= idx; ++i) rec_insert(m, list[i]);
            uint8_t bits = 0;
            if (!found) bits |= REORDERED;
            if (m.count < p.count) bits |= RETX;
            if (m.count > (uint32_t)(p.count + T)) bits |= EXCEEDS;
            if (bits) {
                r.q_action[q] = bits;
                break;
            }
            r.q_action[q] = ADVANCED;
            r.q_drain[q] = idx + 1;
            const uint32_t d = m.count - p.count;
            uint32_t s[T] = {sub32(m.s[0], p.s[0]), sub32(m.s[1], p.s[1])};
            std::vector<uint32_t> miss;
            if (d)
                for (size_t i = 0; i < list.size(); ++i) {
                    if (list[i] == m.last) break;
                    if (is_root(s, d, list[i])) {
                        miss.push_back(list[i]);
                        qhits[q].push_back(sh.offs[g] + gone + i);
                    }
                }
            list.erase(list.begin(), list.begin() + idx + 1);
            gone += idx + 1;
            for (uint32_t id : miss) rec_remove(m, id);
        }
        r.mine_out[g] = m;
        r.drain[g] = gone;
    }
    for (size_t q = 0; q < nq; ++q) {
        r.hit_offsets[q + 1] = r.hit_offsets[q] + qhits[q].size();
        r.hits.insert(r.hits.end(), qhits[q].begin(), qhits[q].end());
    }
    return r;
}

// ---- the kernel chain of sendersteps.hip on the host
static uint32_t clamp_to(const Item &it, uint64_t a) {
    return a <= it.lo ? 0u : a - it.lo >= it.n ? it.n : (uint32_t)(a - it.lo);
}

static Result chain(size_t shape, const Shape &sh, uint32_t maxseg_limit) {
    const size_t nseg = sh.offs.size() - 1;
    uint64_t rounds = 0;
    Result r;
    if (!sq_check(sh.offs.data(), sh.qoffs.data(), nseg, &rounds)) {
        fail("valid shape refused", shape, 0);
        return r;
    }
    const size_t nq = sh.qoffs[nseg];
    const std::vector<Item> items = items_of(sh.offs, maxseg_limit);
    const size_t ni = items.size();
    uint32_t ms = 1;
    for (const Item &it : items) ms = std::max(ms, it.nseg);
    const SqLds lds = sq_lds(ms, T, std::min<uint32_t>(ms * T, 4096));
    // the buffers as sq_carve / sd_carve_plan size them
    Buf<uint64_t> fstop("fstop", nseg), acc("acc", nseg * T), begin("begin", nseg), rdrain("rdrain", nseg),
        q_drain("q_drain", nq), mask("mask", ni * WORDS), base("base", ni), d_hit("hit", sh.log.size());
    Buf<uint32_t> deg("deg", nseg), rcnt("segcnt", nseg), stepped("stepped", nseg), qcnt("qcnt", nq), icnt("icnt", ni);
    Buf<uint8_t> alive("alive", nseg, 1), q_action("q_action", nq, UNSTEPPED);
    Buf<Rec> mo("mine_out", nseg), diff("diff", nseg);
    for (size_t g = 0; g < nseg; ++g) mo[g] = sh.mine[g];
    auto turn = [&](uint64_t g, uint32_t j) { return alive[g] && j < sh.qoffs[g + 1] - sh.qoffs[g]; };
    auto first = [&](uint64_t g) { return sh.offs[g] + begin[g]; };
    auto seg_of = [&](const Item &it, uint32_t i) {   // sd_segment_of over the clamped offsets
        uint32_t lo = 0, hi = it.nseg;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) / 2;
            if (clamp_to(it, sh.offs[it.seg0 + mid]) <= i) lo = mid;
            else hi = mid;
        }
        return lo;
    };
    for (uint32_t j = 0; j < rounds; ++j) {
        for (size_t g = 0; g < nseg; ++g) fstop[g] = NONE, acc[g * T] = 0, acc[g * T + 1] = 0;
        // find
        for (const Item &it : items) {
            if (it.nseg == 1 && (!turn(it.seg0, j) || first(it.seg0) >= it.lo + it.n)) continue;
            Buf<uint32_t> lds_find("find LDS", lds.find / 4);
            for (uint32_t k = 0; k < it.nseg; ++k) {
                const uint64_t g = it.seg0 + k;
                uint32_t use = 0, val = 0, beg = 0;
                if (turn(g, j)) {
                    const Rec &hp = sh.queue[sh.qoffs[g] + j];
                    const Rec &hm = mo[g];
                    use = hp.has && !(hp.has == hm.has && (!hp.has || hp.last == hm.last));
                    val = hp.last, beg = clamp_to(it, first(g));
                }
                lds_find[it.nseg + 1 + k] = use, lds_find[2 * it.nseg + 1 + k] = val, lds_find[3 * it.nseg + 1 + k] = beg;
                (void)lds_find[(uint64_t)ms + 1 + k], (void)lds_find[(uint64_t)3 * ms + 1 + k];   // at the launch's strides
            }
            for (uint32_t i = 0; i < it.n; ++i) {
                const uint32_t rr = it.nseg > 1 ? seg_of(it, i) : 0u;
                if (lds_find[it.nseg + 1 + rr] && i >= lds_find[3 * it.nseg + 1 + rr] &&
                    sh.log[it.lo + i] == lds_find[2 * it.nseg + 1 + rr])
                    fstop[it.seg0 + rr] = std::min<uint64_t>(fstop[it.seg0 + rr], it.lo + i);
            }
        }
        // prefix
        for (const Item &it : items) {
            if (it.nseg == 1) {
                const uint64_t st = fstop[it.seg0];
                if (st == NONE || st < it.lo || first(it.seg0) >= it.lo + it.n) continue;
            }
            for (uint32_t k = 0; k < it.nseg; ++k) {
                const uint64_t g = it.seg0 + k, st = fstop[g];
                uint32_t b = clamp_to(it, sh.offs[g]), e = clamp_to(it, sh.offs[g + 1]);
                if (st == NONE || st < it.lo + b || b == e) continue;
                b = std::max(b, clamp_to(it, first(g)));
                if (st - it.lo < e) e = (uint32_t)(st - it.lo) + 1;
                for (uint32_t i = b; i < e; ++i) {
                    const uint32_t x = canon32(sh.log[it.lo + i]);
                    acc[g * T] += x, acc[g * T + 1] += mul32(x, x);
                }
            }
        }
        // classify
        for (size_t g = 0; g < nseg; ++g) {
            rcnt[g] = 0;
            if (!turn(g, j)) {
                diff[g] = Rec(), rdrain[g] = 0;
                continue;
            }
            const uint64_t q = sh.qoffs[g] + j;
            const Rec &hp = sh.queue[q];
            Rec m = mo[g];
            const bool active = !(hp.has == m.has && (!hp.has || hp.last == m.last));
            const uint64_t st = active ? fstop[g] : NONE;
            const bool found = st != NONE;
            uint64_t idx = 0;
            if (found) {
                if (st < first(g) || st >= sh.offs[g + 1]) fail("a stop outside the flow's interval", shape, g);
                idx = st - first(g);
                m.count += (uint32_t)(idx + 1), m.has = 1, m.last = sh.log[st];
                for (uint32_t k = 0; k < T; ++k) m.s[k] = add32(m.s[k], canon32(fold64_32(acc[g * T + k])));
            }
            uint8_t bits = 0;
            if (active) {
                if (!found) bits |= REORDERED;
                if (m.count < hp.count) bits |= RETX;
                if (m.count > (uint32_t)(hp.count + T)) bits |= EXCEEDS;
            }
            const bool decode = active && !bits;
            Rec df;
            if (decode) {
                df.count = m.count - hp.count, df.has = 1;
                for (uint32_t k = 0; k < T; ++k) df.s[k] = sub32(m.s[k], hp.s[k]), acc[g * T + k] = m.s[k];
            }
            df.last = m.last;
            mo[g] = m, diff[g] = df;
            q_action[q] = !active ? IDLE : bits ? bits : ADVANCED;
            q_drain[q] = rdrain[g] = decode ? idx + 1 : 0;
            stepped[g] = j + 1;
            if (bits) alive[g] = 0;
        }
        // Newton: the degree (the coefficients are is_root's)
        for (size_t g = 0; g < nseg; ++g) deg[g] = diff[g].count > T ? 0u : diff[g].count;
        // root test
        for (size_t w = 0; w < ni; ++w) {
            const Item &it = items[w];
            if (it.nseg == 1) {
                const uint64_t st = fstop[it.seg0];
                if (deg[it.seg0] == 0 || st == NONE || st <= it.lo || first(it.seg0) >= it.lo + it.n) continue;
            }
            Buf<uint32_t> lds_root("root LDS", lds.root / 4);
            (void)lds_root[(uint64_t)4 * ms + (uint64_t)(it.nseg - 1) * (T + 1) + T - 1];   // the last coefficient staged
            for (uint32_t i = 0; i < it.n; ++i) {
                const uint32_t rr = it.nseg > 1 ? seg_of(it, i) : 0u;
                const uint64_t g = it.seg0 + rr, st = fstop[g];
                const bool use = deg[g] != 0 && st != NONE;
                if (!use || i < clamp_to(it, first(g)) || i >= clamp_to(it, st)) continue;
                if (is_root(diff[g].s, deg[g], sh.log[it.lo + i])) {
                    if (mask[w * WORDS + i / 64] >> (i & 63) & 1) fail("a hit bit set twice", shape, it.lo + i);
                    mask[w * WORDS + i / 64] |= 1ull << (i & 63);
                    rcnt[g]++;
                }
            }
        }
        // remove
        for (size_t w = 0; w < ni; ++w) {
            const Item &it = items[w];
            if (it.nseg == 1) {
                const uint64_t st = fstop[it.seg0];
                if (rcnt[it.seg0] == 0 || st == NONE || st <= it.lo || first(it.seg0) >= it.lo + it.n) continue;
            }
            Buf<uint64_t> lds_rem("remove LDS", lds.remove / 8 + 1);
            const uint32_t words = it.nseg * T;
            if (words <= lds.rows) (void)lds_rem[words - 1];
            (void)lds_rem[((uint64_t)lds.rows * 8 + ((uint64_t)3 * ms + 1) * 4 - 1) / 8];
            for (uint32_t i = 0; i < it.n; ++i) {
                if (!(mask[w * WORDS + i / 64] >> (i & 63) & 1)) continue;
                const uint32_t rr = it.nseg > 1 ? seg_of(it, i) : 0u;
                const uint64_t g = it.seg0 + rr, st = fstop[g];
                const bool use = rcnt[g] != 0 && st != NONE;
                if (!use || i < clamp_to(it, first(g)) || i >= clamp_to(it, st)) continue;
                const uint32_t x = canon32(sh.log[it.lo + i]);
                acc[g * T] += P32 - x, acc[g * T + 1] += P32 - mul32(x, x);
            }
        }
        // finish
        for (size_t g = 0; g < nseg; ++g) {
            const uint32_t c = rcnt[g];
            if (c) {
                Rec m = mo[g];
                m.count -= c;
                for (uint32_t k = 0; k < T; ++k) m.s[k] = canon32(fold64_32(acc[g * T + k]));
                mo[g] = m;
                qcnt[sh.qoffs[g] + j] = c;
            }
            begin[g] += rdrain[g];
        }
    }
    // item counts, scan, hit write
    uint64_t total = 0;
    for (size_t w = 0; w < ni; ++w) {
        uint32_t c = 0;
        for (uint32_t l = 0; l < WORDS; ++l) c += (uint32_t)__builtin_popcountll(mask[w * WORDS + l]);
        icnt[w] = c, base[w] = total, total += c;
    }
    for (size_t w = 0; w < ni; ++w) {
        uint64_t rank = base[w];
        for (uint32_t i = 0; i < items[w].n; ++i)
            if (mask[w * WORDS + i / 64] >> (i & 63) & 1) d_hit[rank++] = items[w].lo + i;
    }
    r.mine_out = mo.v, r.q_action = q_action.v, r.q_drain = q_drain.v, r.drain = begin.v, r.stepped = stepped.v;
    r.hit_offsets.assign(nq + 1, 0);
    for (size_t q = 0; q < nq; ++q) r.hit_offsets[q + 1] = r.hit_offsets[q] + qcnt[q];
    if (r.hit_offsets[nq] != total) fail("the two hit counts differ", shape, total);
    r.hits.assign(d_hit.v.begin(), d_hit.v.begin() + total);
    return r;
}

static size_t seen[32], hits_seen;   // what the shapes exercised

static void check(size_t shape, const Shape &sh, uint32_t maxseg_limit) {
    const Result want = model(sh), got = chain(shape, sh, maxseg_limit);
    for (uint8_t a : want.q_action) seen[a & 31]++;
    hits_seen += want.hits.size();
    if (!(got.mine_out == want.mine_out)) fail("mine_out", shape, 0);
    if (got.q_action != want.q_action) fail("q_action", shape, 0);
    if (got.q_drain != want.q_drain) fail("q_drain", shape, 0);
    if (got.drain != want.drain) fail("drain", shape, 0);
    if (got.stepped != want.stepped) fail("stepped", shape, 0);
    if (got.hit_offsets != want.hit_offsets) fail("hit_offsets", shape, 0);
    if (got.hits != want.hits) fail("hits", shape, 0);
    for (size_t i = 1; i < got.hits.size(); ++i)
        if (got.hits[i] <= got.hits[i - 1]) fail("hits not ascending", shape, i);
}

// a flow of `len` entries whose proxy sent a quACK after each of `stops`, having lost `lost`
static void add_flow(Shape &sh, std::mt19937 &rng, uint64_t len, std::vector<uint64_t> stops, const std::vector<uint64_t> &lost,
                     int dup_ids, uint32_t count0) {
    const uint64_t o = sh.offs.back();
    for (uint64_t i = 0; i < len; ++i) {
        uint32_t v = rng() | (rng() % 9 == 0 ? 0xFFFFFFF0u : 0u);   // unreduced ids among them
        if (dup_ids && i && rng() % (uint32_t)dup_ids == 0) v = sh.log[o + rng() % i];
        sh.log.push_back(v);
    }
    Rec m;
    m.count = count0;
    sh.mine.push_back(m);
    for (uint64_t s : stops) {
        Rec p;
        p.count = count0;
        if (s < len)
            for (uint64_t i = 0; i <= s; ++i)
                if (std::find(lost.begin(), lost.end(), i) == lost.end()) rec_insert(p, sh.log[o + i]);
        if (s == len + 1) rec_insert(p, 0xDEADBEEF);   // a last value the log does not hold
        sh.queue.push_back(p);                       // s == len: a quACK without a last value
    }
    sh.offs.push_back(o + len);
    sh.qoffs.push_back(sh.queue.size());
}

static Shape empty_shape(uint64_t first) {
    Shape sh;
    sh.offs.push_back(first), sh.qoffs.push_back(0);
    sh.log.assign(first, 0x12345678u);
    return sh;
}

static void check_queue(size_t shape, std::mt19937 &rng, size_t n, size_t nseg) {
    std::vector<uint32_t> flow(n), ok(n), counts(nseg, 0);
    std::vector<std::vector<uint32_t>> lists(nseg);
    for (size_t i = 0; i < n; ++i) {
        flow[i] = rng() % nseg, ok[i] = rng() % 4 != 0;
        if (ok[i]) lists[flow[i]].push_back((uint32_t)i), counts[flow[i]]++;
    }
    std::vector<uint64_t> qoffs(nseg + 1, 77);
    const uint64_t m = wq_offsets(counts.data(), nseg, qoffs.data());
    // the sort of (key, i) by key, stable, over region X of wq_region_words(n) words
    Buf<uint32_t> x("sort region", wq_region_words(n));
    for (size_t i = 0; i < n; ++i) x[i] = ok[i] ? flow[i] : (uint32_t)nseg, x[n + i] = (uint32_t)i;
    std::vector<uint32_t> perm(n);
    for (size_t i = 0; i < n; ++i) perm[i] = x[n + i];
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return x[a] < x[b]; });
    if (qoffs[0] != 0 || qoffs[nseg] != m) fail("queue offsets", shape, m);
    for (size_t g = 0; g < nseg; ++g) {
        if (qoffs[g + 1] - qoffs[g] != lists[g].size()) return fail("queue count", shape, g);
        for (size_t k = 0; k < lists[g].size(); ++k)
            if (perm[qoffs[g] + k] != lists[g][k]) return fail("queue placement", shape, g);
    }
}

int main() {
    std::mt19937 rng(20261021);
    size_t shape = 0;
    // edge shapes: interval ends on both sides of the item boundaries, b inside an item and the stop in a later one
    for (uint32_t maxseg : {256u, 3u}) {
        Shape sh = empty_shape(5);
        add_flow(sh, rng, 0, {}, {}, 0, 0);
        add_flow(sh, rng, 0, {1}, {}, 0, 0);                                        // no log, a quACK: REORDERED
        add_flow(sh, rng, 4097 + 600, {0, 63, 64, 2047, 2048, 2049, 4103}, {5, 70, 2040, 2051, 4097, 4100}, 0, 7);
        add_flow(sh, rng, 4097 + 600, {2047, 2047, 4096}, {2046, 2048, 4095}, 0, 0xFFFFFFFEu);   // a duplicate: IDLE; the count wraps
        add_flow(sh, rng, 50, {9, 19, 29, 39}, {3, 4, 12, 13, 14, 25}, 0, 0);       // three losses > T: EXCEEDS, then UNSTEPPED
        add_flow(sh, rng, 50, {9, 51, 29}, {3}, 0, 0);                              // REORDERED in the middle
        add_flow(sh, rng, 50, {50, 9}, {3}, 0, 0);                                  // a quACK without a last value first
        add_flow(sh, rng, 50, {29, 9, 39}, {3, 35}, 0, 0);                          // out of order: the stop lies before b
        for (int i = 0; i < 300; ++i) add_flow(sh, rng, i % 4, i % 4 ? std::vector<uint64_t>{(uint64_t)(i % 4 - 1)} : std::vector<uint64_t>{}, {}, 0, 0);
        add_flow(sh, rng, 2048, {100, 2047}, {7, 2000}, 0, 0);
        add_flow(sh, rng, 2049, {2048}, {0, 2047}, 0, 0);
        check(shape++, sh, maxseg);
    }
    // decreasing indices are refused
    {
        uint64_t offs[3] = {0, 5, 4}, q[3] = {0, 1, 2}, q2[3] = {0, 2, 1}, up[3] = {0, 4, 5}, rounds = 0;
        if (sq_check(offs, q, 2, &rounds) || sq_check(up, q2, 2, &rounds) || !sq_check(up, q, 2, &rounds) || rounds != 1)
            fail("sq_check", shape, 0);
    }
    // random shapes: duplicates of ids in the logs, random stops and losses
    for (int it = 0; it < 400; ++it) {
        Shape sh = empty_shape(rng() % 3);
        const int nflows = 1 + rng() % 12;
        for (int g = 0; g < nflows; ++g) {
            const uint64_t len = rng() % 5 == 0 ? 2000 + rng() % 2500 : rng() % 40;
            std::vector<uint64_t> stops, lost;
            const int k = rng() % 5;
            for (int j = 0; j < k && len; ++j) stops.push_back(rng() % 11 == 0 ? len + rng() % 2 : rng() % len);
            if (rng() % 4) std::sort(stops.begin(), stops.end());
            for (uint64_t i = 0; i < len; ++i)
                if (rng() % 24 == 0 && std::find(stops.begin(), stops.end(), i) == stops.end()) lost.push_back(i);
            add_flow(sh, rng, len, stops, lost, rng() % 2 ? 6 : 0, rng() % 3 ? 0 : 0xFFFFFFF0u + rng() % 16);
        }
        check(shape++, sh, rng() % 2 ? 256u : 2u);
    }
    for (int it = 0; it < 200; ++it) check_queue(shape++, rng, rng() % 300, 1 + rng() % 20);
    for (int a : {IDLE, ADVANCED, REORDERED, RETX, EXCEEDS, UNSTEPPED})
        if (!seen[a]) fail("an action no shape produced", shape, a);
    if (hits_seen < 500) fail("too few hits", shape, hits_seen);
    if (fails) {
        printf("sender_steps_plan_check: %d failures\n", fails);
        return 1;
    }
    printf("sender_steps_plan_check: ok %zu shapes, %zu checked accesses\n", shape, checks);
    return 0;
}
