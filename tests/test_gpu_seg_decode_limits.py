"""Batched per-flow decode at its packing limits: runs of short segments that
end on the segment cut (QK_SEG_DECODE_MAXSEG, QK_SEG_DECODE_COEF_WORDS /
threshold), more than 1024 work items (k_seg_scan with several items per
thread), and Newton's identities at the group-width boundaries and at
t = 1024.

Expected hits are exact and independent of the kernels: a record that holds
the power sums of known dropped ids has exactly those ids' residues as roots,
so the hits are the positions congruent mod p to a dropped id (numpy, on
canonical residues), cut at the first entry equal to last_value under
stop_at_last.  The oracle (Python-integer Newton + evaluation) runs on top of
that wherever it is affordable, and on every record that is not built from
known ids.  Each test asserts that its shape passes the limit it is aimed at,
with the packing rule restated from the header's three constants."""
import os
import re

import numpy as np
import pytest

import sidekick_amd as sk
from oracle import coracle, quack_oracle as qo
from sidekick_amd._lib import QK_E_UNDECODABLE, QK_OK
from test_gpu_seg_decode import (item_len, oracle_segment, quack, raw_decode, records, short_segments, to_dev)

pytestmark = pytest.mark.gpu

P = qo.P32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_THREADS = 1024          # k_seg_scan: one workgroup, each thread a contiguous run of items


def header_const(name):
    hdr = open(os.path.join(ROOT, "include", "quack_hip.h")).read()
    return int(re.search(rf"#define {name} (\d+)u", hdr).group(1))


ITEM = item_len()
MAXSEG = header_const("QK_SEG_DECODE_MAXSEG")
COEF_WORDS = header_const("QK_SEG_DECODE_COEF_WORDS")


def max_segments(t):
    """Segments per packed work item at threshold t, as the header states the rule."""
    return max(1, min(MAXSEG, COEF_WORDS // t))


def work_items(offs, t):
    """The packing rule restated: (first segment, segments, entries) per run.  A
    segment longer than ITEM is cut into slices; whole shorter segments are
    packed while the run holds <= ITEM entries and <= max_segments(t)
    segments.  A run of 0 entries launches no work item."""
    out, g, nseg, most = [], 0, len(offs) - 1, max_segments(t)
    lens = np.diff(np.asarray(offs).astype(np.int64)).tolist()
    while g < nseg:
        if lens[g] > ITEM:
            out += [(g, 1, min(ITEM, lens[g] - lo)) for lo in range(0, lens[g], ITEM)]
            g += 1
            continue
        g0, tot = g, 0
        while g < nseg and g - g0 < most and lens[g] <= ITEM - tot:
            tot += lens[g]
            g += 1
        out.append((g0, g - g0, tot))
    return out


# --------------------------------------------------------- segments by construction
class Seg:
    """One segment: its record, its log, and (when the record is the power sums
    of known ids) those ids."""

    def __init__(self, t, log, ids=None, last=None, count=None, sums=None):
        self.log = np.array(log, dtype=np.uint32)
        self.ids = [int(v) for v in ids] if sums is None and count is None else None
        self.last = last
        self.q = quack(t, [] if ids is None else ids, count=count, last=last, sums=sums)

    def by_construction(self, stop):
        """Positions congruent mod p to a dropped id, cut at the first entry equal to last_value."""
        assert self.ids is not None
        res = self.log.astype(np.uint64) % np.uint64(P)
        hit = np.isin(res, np.array(self.ids, dtype=np.uint64) % np.uint64(P))
        if stop and self.last is not None:
            at = np.nonzero(self.log == np.uint32(self.last))[0]
            if len(at):
                hit[at[0]:] = False
        return np.nonzero(hit)[0].tolist()


def odd(rng, n):
    """n distinct odd values in (10, p - 10): log entries."""
    return (rng.choice(2**31 - 16, size=n, replace=False).astype(np.uint32) + 6) * 2 + 1


def even(rng, n):
    """n distinct even values in (10, p - 10): dropped ids that no log entry equals or is congruent to."""
    return (rng.choice(2**31 - 16, size=n, replace=False).astype(np.uint32) + 6) * 2


def small_segment(rng, t, nmin, nmax, dmax):
    """nmin..nmax odd entries; 0..dmax dropped ids, some of them in the log."""
    n = int(rng.integers(nmin, nmax + 1))
    log = odd(rng, n)
    k = int(rng.integers(0, min(n, dmax) + 1))
    extra = int(rng.integers(0, dmax - k + 1)) if rng.random() < 0.5 else 0
    ids = [int(v) for v in log[rng.choice(n, size=k, replace=False)]] + [int(v) for v in even(rng, extra)]
    last = int(log[int(rng.integers(n))]) if n and rng.random() < 0.6 else None
    return Seg(t, log, ids, last=last)


def empty_segment(rng, t, deg):
    """No log entries; a record of degree deg all the same (its row is still staged)."""
    return Seg(t, [], even(rng, deg), last=7 if deg % 2 else None)


def batch_of(segs):
    offs = np.concatenate([[0], np.cumsum([len(s.log) for s in segs])]).astype(np.uint64)
    return [s.q for s in segs], np.concatenate([s.log for s in segs]).astype(np.uint32), offs


def check(segs, qs, d_log, offs, stop, oracle):
    """One device pass against the construction (every segment with known ids)
    and against the oracle's lists (every segment of `oracle`)."""
    got, status = sk.decode_segments(qs, d_log, offs, stop_at_last=stop)
    assert len(got) == len(status) == len(segs)
    for g, s in enumerate(segs):
        und = s.q.count() > s.q.threshold()
        assert status[g] == (QK_E_UNDECODABLE if und else QK_OK), g
        if s.ids is not None:
            assert got[g] == s.by_construction(stop), (g, stop)
        else:
            assert g in oracle, g
    for g, want in oracle.items():
        assert got[g] == want[int(stop)], (g, stop)
    return got


def oracle_lists(segs, which):
    """{g: (hits without the stop rule, hits with it)} by the oracle."""
    return {g: (oracle_segment(segs[g].q, segs[g].log, False)[0], oracle_segment(segs[g].q, segs[g].log, True)[0])
            for g in which}


# ----------------------------------------------------- a. the segment cut, T <= 32
def cut_batch(t, seed):
    rng = np.random.default_rng(seed)
    M = max_segments(t)
    segs = [small_segment(rng, t, 0, 6, t) for _ in range(5 * M + 20)]

    def stop_special():
        # last_value is the segment's own first entry, itself a root: cut before anything
        log = odd(rng, 3)
        return Seg(t, log, [int(log[0]), int(log[1])], last=int(log[0]))

    # runs are [0, M), [M, 2M), ...: an empty segment ends run 0, another opens run 1
    segs[M - 2] = small_segment(rng, t, 3, 6, t)
    segs[M - 1] = empty_segment(rng, t, min(t, 3))
    segs[M] = empty_segment(rng, t, 0)
    segs[M + 1] = small_segment(rng, t, 3, 6, t)
    segs[2 * M - 1] = stop_special()                         # ends run 1
    # run 2: M one-entry segments, degrees 0, 1, ..., t, 0, ...; every third entry is a root
    for j in range(M):
        deg = j % (t + 1)
        ids = [int(v) for v in even(rng, deg)]
        root = j % 3 == 0 and deg > 0
        entry = ids[j % deg] if root else int(odd(rng, 1)[0])
        segs[2 * M + j] = Seg(t, [entry], ids, last=entry if j % 4 == 1 else None)
    # M + 3 empty segments: run 3 holds no entry at all, run 4 opens with three empty ones
    for j in range(M + 3):
        segs[3 * M + j] = empty_segment(rng, t, j % (t + 1))
    segs[4 * M + 3] = stop_special()                         # first entry of run 4
    x, y = (int(v) for v in odd(rng, 2))
    segs[4 * M + 10] = Seg(t, [x, y, x, x], [x])             # the dropped id several times in the log
    segs[4 * M + 11] = Seg(t, [x, y, y], [y, y])             # and dropped twice: a double root
    # the dropped ids are 3 and 0: 3, p + 3, 0 and p are hits, p - 1 and 2^32 - 1 are not
    segs[4 * M + 12] = Seg(t, [3, P + 3, P - 1, 0, P, 2**32 - 1], [3, 0], last=P)
    segs[5 * M - 1] = stop_special()                         # ends run 4
    segs[5 * M] = stop_special()                             # opens the last run
    return segs


@pytest.fixture(scope="module", params=[4, 32])
def cut(request):
    t = request.param
    segs = cut_batch(t, seed=9000 + t)
    qs, log, offs = batch_of(segs)
    return t, segs, qs, log, offs, oracle_lists(segs, range(len(segs)))


def test_segment_cut_shape(cut):
    t, segs, qs, log, offs, _ = cut
    M = max_segments(t)
    assert M == MAXSEG and len(segs) >= 3 * MAXSEG + 17
    runs = work_items(offs, t)
    assert len(runs) >= 4 and all(n == M for _, n, _ in runs[:-1])          # every run ends on the segment cut
    assert all(tot <= 6 * M < ITEM for _, _, tot in runs)                   # never on the entry limit
    assert sum(tot == 0 for _, _, tot in runs) == 1                         # one run launches no item
    lens = np.diff(offs.astype(np.int64))
    run_of_empty = max(len(r) for r in "".join("e" if n == 0 else " " for n in lens).split())
    assert run_of_empty >= MAXSEG + 3
    assert lens[M - 1] == 0 and lens[M] == 0 and lens[M - 2] > 0 and lens[M + 1] > 0
    assert (2 * M, M, M) in runs and M >= 64                                # a wave of 64 segments, LDS at the maximum
    degs = [s.q.count() for s in segs[2 * M:3 * M]]
    assert degs[:t + 2] == list(range(t + 1)) + [0]
    hits = [len(s.by_construction(False)) for s in segs[2 * M:3 * M]]
    assert hits == [int(j % 3 == 0 and degs[j] > 0) for j in range(M)]
    for g in (2 * M - 1, 4 * M + 3, 5 * M - 1, 5 * M):                      # own first entry cuts, beside a cut
        assert segs[g].by_construction(True) == [] and segs[g].by_construction(False) == [0, 1]
    assert segs[4 * M + 10].by_construction(False) == [0, 2, 3]
    assert segs[4 * M + 11].by_construction(False) == [1, 2] and segs[4 * M + 11].q.count() == 2
    assert segs[4 * M + 12].by_construction(False) == [0, 1, 3, 4] and segs[4 * M + 12].by_construction(True) == [0, 1, 3]


@pytest.mark.parametrize("where", ["host records", "device records"])
@pytest.mark.parametrize("stop", [False, True])
def test_segment_cut(cut, stop, where):
    t, segs, qs, log, offs, oracle = cut
    runs = work_items(offs, t)
    assert all(n == MAXSEG for _, n, _ in runs[:-1]) and len(runs) >= 4      # the runs end on the segment cut
    diffs = qs if where == "host records" else to_dev(records(qs))
    got = check(segs, diffs, to_dev(log), offs, stop, oracle)
    assert sum(len(h) for h in got) > 500


# ------------------------------------------------------ b. the coefficient-budget cut
def budget_batch(t, seed):
    rng = np.random.default_rng(seed)
    m = COEF_WORDS // t
    segs = [small_segment(rng, t, 1, 5, 3) for _ in range(3 * m + 5)]
    full = [m - 1, m, 2 * m + m // 2, 3 * m + 2]          # ends run 0, opens run 1, inside run 2, in the last run
    for i, g in enumerate(full):
        ids = even(rng, t)                                # count == t, of which 1..3 are in the log
        k = 1 + i % 3
        log = np.concatenate([odd(rng, 2), ids[[0, t // 2, t - 1][:k]]])
        segs[g] = Seg(t, log[rng.permutation(len(log))], ids, last=int(log[0]) if i % 2 else None)
    arbitrary = rng.integers(0, P, size=t, dtype=np.uint64)
    arbitrary[::3] = 0
    arbitrary[1::7] = P - 1
    segs[1] = Seg(t, odd(rng, 4), count=2, sums=arbitrary)          # not the power sums of known ids
    segs[2] = Seg(t, odd(rng, 4), count=t + 1, sums=arbitrary)      # undecodable
    segs[3] = Seg(t, odd(rng, 4), count=2**32 - 1, sums=arbitrary)
    return segs, full


@pytest.mark.parametrize("t", [33, 100, 129, 1024])
def test_coefficient_budget_cut(t):
    segs, full = budget_batch(t, seed=9100 + t)
    m = COEF_WORDS // t
    assert m < MAXSEG and max_segments(t) == m and len(segs) == 3 * m + 5
    qs, log, offs = batch_of(segs)
    runs = work_items(offs, t)
    assert [r[:2] for r in runs] == [(0, m), (m, m), (2 * m, m), (3 * m, 5)]    # three runs end on the budget cut
    assert all(tot <= 5 * m < ITEM for _, _, tot in runs)
    assert 1 <= len(full) <= 4 and all(segs[g].q.count() == t for g in full)
    assert all(1 <= len(segs[g].by_construction(False)) <= 3 for g in full)
    assert [segs[g].ids is None for g in (1, 2, 3)] == [True] * 3
    oracle = oracle_lists(segs, range(len(segs)))
    d_log = to_dev(log)
    for stop in (False, True):
        got = check(segs, qs, d_log, offs, stop, oracle)
    assert got[2] == got[3] == []
    check(segs, to_dev(records(qs)), d_log, offs, True, oracle)


# ------------------------------------------------- c. more than 1024 work items
def test_scan_past_one_item_per_thread_long_segment():
    t = 8
    n_long = (SCAN_THREADS + 1) * ITEM + 3
    rng = np.random.default_rng(9200)
    pre = short_segments(5, t, seed=41)
    post = short_segments(6, t, seed=42)
    long_log = rng.integers(0, 2**31, size=n_long).astype(np.uint32) * 2          # even: apart from the shorts
    missing = [int(v) for v in long_log[rng.choice(n_long, size=t, replace=False)]]
    offs = np.concatenate([pre[2], pre[2][-1] + n_long + post[2]]).astype(np.uint64)
    g_long = len(pre[0])
    runs = work_items(offs, t)
    launched = [r for r in runs if r[2]]
    nitems = len(launched)
    assert nitems > SCAN_THREADS
    per = -(-nitems // SCAN_THREADS)
    assert per >= 2
    # the scan thread that holds the final non-empty run, and its first and last item
    last_thread = (nitems - 1) // per
    first_item, last_item = last_thread * per, min(last_thread * per + per, nitems) - 1
    starts = np.concatenate([[0], np.cumsum([r[2] for r in launched])])           # log position of each item
    lo_long = int(offs[g_long])
    edge = [0, n_long - 1]
    for b in range(64 * ITEM, n_long, 64 * ITEM):                                 # both sides of every 64th boundary
        edge += [b - 1, b]
    for it in (first_item, last_item):                                            # where the item lies in the long segment
        if launched[it][0] == g_long:
            edge.append(int(starts[it]) - lo_long)
    edge += rng.choice(n_long, size=3000, replace=False).tolist()                 # and spread over the items between
    for j, pos in enumerate(edge):
        long_log[pos] = missing[j % t]
    stop_pos = 900 * ITEM + 5
    long_q = quack(t, missing, last=int(long_log[stop_pos]))
    qs = pre[0] + [long_q] + post[0]
    log = np.concatenate([pre[1], long_log, post[1]])
    want_long = qo.root_test_u32_np(qo.newton_coeffs(long_q.power_sums()[:t], P), long_log)
    assert set(edge) <= set(want_long.tolist())
    first_stop = int(np.nonzero(long_log == long_log[stop_pos])[0][0])
    assert first_stop > 64 * ITEM
    want_short = {g: (oracle_segment(q, log[offs[g]:offs[g + 1]], False)[0],
                      oracle_segment(q, log[offs[g]:offs[g + 1]], True)[0]) for g, q in enumerate(qs) if g != g_long}
    # both items of the final thread hold hits, so its run start and its second base are both used
    flat = np.concatenate([np.array(want_short[g][0], dtype=np.int64) + int(offs[g]) if g != g_long
                           else want_long + lo_long for g in range(len(qs))])
    for it in (first_item, last_item):
        assert ((flat >= starts[it]) & (flat < starts[it + 1])).any(), it
    d_log = to_dev(log)
    for stop in (False, True):
        got, status = sk.decode_segments(qs, d_log, offs, stop_at_last=stop)
        assert status == [QK_OK] * len(qs)
        assert np.array_equal(np.array(got[g_long], dtype=np.int64),
                              want_long[want_long < first_stop] if stop else want_long)
        for g in want_short:
            assert got[g] == want_short[g][int(stop)], g


def power_sums_np(ids, deg, t):
    """[n, t] power sums mod p of the first deg[g] ids of every row (numpy, 64-bit exact)."""
    p = np.uint64(P)
    x = ids.astype(np.uint64) % p
    mask = (np.arange(ids.shape[1])[None, :] < deg[:, None]).astype(np.uint64)
    y, out = x.copy(), np.zeros((len(ids), t), dtype=np.uint64)
    for k in range(t):
        out[:, k] = (y * mask).sum(axis=1, dtype=np.uint64) % p
        y = (y * x) % p
    return out.astype(np.uint32)


def test_scan_past_one_item_per_thread_segment_cut(ctx):
    """More than 1024 work items by the segment cut alone: one-entry segments at t = 4."""
    t = 4
    M = max_segments(t)
    nseg = (SCAN_THREADS + 2) * M + 5
    rng = np.random.default_rng(9300)
    g = np.arange(nseg)
    deg = (g % (t + 1)).astype(np.int64)
    ids = rng.integers(6, 2**31 - 10, size=(nseg, t)).astype(np.uint32) * 2            # even, canonical
    root = (g % 3 == 0) & (deg > 0)
    entry = np.where(root, ids[g, g % np.maximum(deg, 1)], rng.integers(6, 2**31 - 10, size=nseg).astype(np.uint32) * 2 + 1)
    has_last = g % 4 == 1
    rec = np.zeros((nseg, 4 + t), dtype=np.uint32)
    rec[:, 0], rec[:, 1], rec[:, 2] = t, deg, has_last
    rec[:, 3] = np.where(has_last, entry, 0)                 # its own entry: cut before anything under the stop rule
    rec[:, 4:] = power_sums_np(ids, deg, t)
    for k in rng.integers(0, nseg, size=40):                 # the numpy sums are the C oracle's
        assert rec[k, 4:].tolist() == (coracle.encode_u32(ids[k, :deg[k]], t) if deg[k] else [0] * t)
    offs = np.arange(nseg + 1, dtype=np.uint64)
    runs = work_items(offs, t)
    assert len(runs) > SCAN_THREADS and all(r[1:] == (M, M) for r in runs[:-1]) and runs[-1][1:] == (5, 5)
    assert -(-len(runs) // SCAN_THREADS) >= 2
    d_log = to_dev(entry)
    for stop in (False, True):
        hit = root & ~has_last if stop else root
        want = np.nonzero(hit)[0].astype(np.uint64)
        assert len(want) > 50_000
        rc, hits, hoffs, nh = raw_decode(ctx, rec, d_log, offs, nseg, t, stop, len(want))
        assert rc == QK_OK and nh == len(want)
        assert np.array_equal(hoffs, np.concatenate([[0], np.cumsum(hit)]).astype(np.uint64))
        assert np.array_equal(hits[:nh], want)
    # the oracle on the segments of the first item, of the two around the scan's
    # first thread boundary, and of the last two items
    per = -(-len(runs) // SCAN_THREADS)
    for g0 in (0, (per - 1) * M, per * M, (len(runs) - 2) * M):
        for k in range(g0, min(g0 + M + 5, nseg)):
            q = quack(t, ids[k, :deg[k]], last=int(entry[k]) if has_last[k] else None)
            assert records([q])[0].tolist() == rec[k].tolist()
            for stop in (False, True):
                assert oracle_segment(q, entry[k:k + 1], stop)[0] == ([0] if root[k] and not (stop and has_last[k]) else [])


# ------------------------------------------------ d. Newton at the group boundaries
@pytest.mark.parametrize("t,nseg", [(32, 77), (33, 77), (128, 45), (129, 45), (1024, 13)])
def test_newton_group_boundaries(t, nseg):
    """Groups of 8 lanes (32 segments per workgroup) up to t = 32, of 16 (16)
    up to 128, of 64 (4) above; nseg is no multiple of any of them."""
    assert nseg % (32 if t <= 32 else 16 if t <= 128 else 4) != 0 and (t < 129 or nseg % 4 == 1)
    rng = np.random.default_rng(9400 + t)
    counts = [t, t, t - 1, t + 1, 0, t, 1, 2**32 - 1, t, t - 1]
    qs = []
    for g in range(nseg):
        cnt = counts[g % len(counts)]
        if g % 3 != 2 and cnt <= t + 1:          # a real diff: the power sums of cnt ids
            qs.append(quack(t, rng.integers(0, 2**32, size=cnt, dtype=np.uint64).astype(np.uint32)))
        else:                                    # arbitrary canonical sums, 0 and p - 1 among them
            s = rng.integers(0, P, size=t, dtype=np.uint64)
            s[rng.random(t) < 0.15] = 0
            s[rng.random(t) < 0.15] = P - 1
            qs.append(quack(t, count=cnt, sums=s))
    want_status = [QK_OK if q.count() <= t else QK_E_UNDECODABLE for q in qs]
    full = [g for g, q in enumerate(qs) if q.count() == t]
    assert len(full) >= 4 and QK_E_UNDECODABLE in want_status
    assert any(q.count() == t and 0 in q.power_sums() and P - 1 in q.power_sums() for q in qs)
    # Python integers: every segment up to t = 129; at 1024 the first four of full degree and the short ones
    by_python = [g for g, q in enumerate(qs) if q.count() <= t and (t <= 129 or g in full[:4] or q.count() <= 1)]
    want = {g: qo.newton_coeffs(qs[g].power_sums()[:qs[g].count()], P) for g in by_python}
    assert sum(qs[g].count() == t for g in by_python) >= 4
    for diffs in (qs, to_dev(records(qs))):
        got, status = sk.to_coeffs_segments(diffs, t)
        assert status == want_status
        for g, q in enumerate(qs):
            assert len(got[g]) == (q.count() if q.count() <= t else 0), g
            if g in want:
                assert list(got[g]) == want[g], g
    for g, q in enumerate(qs):                   # second witness: the host to_coeffs, on every decodable segment
        if q.count() <= t:
            assert list(q.to_coeffs()) == list(got[g]), g
