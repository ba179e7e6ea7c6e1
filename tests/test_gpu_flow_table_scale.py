"""Device-resident flow table past 1024 join tiles (k_ft_scan with several
tiles per thread): a 1.2·10⁶-key table merged with, and diffed against, a
10⁶-key batch, and a lookup of 10⁵ keys in it.

Expected values come from a vectorised numpy model of merge and diff: keys
compared as three big-endian words, header and sum rules those of the dict
model of test_gpu_flow_table.py (the host merge / sub_assign).  The numpy
model is first held to that dict model on every join shape, in a test of its
own; the scale tests then rely on it."""
import numpy as np
import pytest

import sidekick_amd as sk
from oracle import quack_oracle as qo
from sidekick_amd._lib import FLOW_JOIN_TILE, QK_OK, lib
from test_gpu_flow_table import dev, host, model_diff, model_merge, rand_recs, shapes

pytestmark = pytest.mark.gpu

P = qo.P32
SCAN_THREADS = 1024          # k_ft_scan: one workgroup, each thread a contiguous run of tiles
NA, NB, SHARED = 1_200_000, 1_000_000, 300_000


# -------------------------------------------------------------- the numpy model
def key_words(keys):
    """uint8 [n, 12] keys as uint64 [n, 3]: three big-endian words, so that
    comparing them most significant first is memcmp on the 12 bytes."""
    return np.ascontiguousarray(keys).view(">u4").reshape(len(keys), 3).astype(np.uint64)


def np_join(ka, kb):
    """The union of two ascending key arrays: (ia, ib), per output key in
    ascending order its index in a and in b, -1 where the key is not there."""
    wa, wb = key_words(ka), key_words(kb)
    w = np.concatenate([wa, wb])
    src = np.concatenate([np.zeros(len(wa), np.uint64), np.ones(len(wb), np.uint64)])
    idx = np.concatenate([np.arange(len(wa)), np.arange(len(wb))])
    # two 64-bit sort keys: words 0 and 1, then word 2 with a before b on a tie
    order = np.lexsort(((w[:, 2] << np.uint64(1)) | src, (w[:, 0] << np.uint64(32)) | w[:, 1]))
    w, src, idx = w[order], src[order], idx[order]
    first = np.ones(len(w), bool)
    first[1:] = (w[1:] != w[:-1]).any(axis=1)
    out = np.cumsum(first) - 1
    n = int(first.sum())
    ia, ib = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    ia[out[src == 0]] = idx[src == 0]
    ib[out[src == 1]] = idx[src == 1]
    return ia, ib


def np_combine(a, b, diff):
    """qk_u32_merge(a, b) / qk_u32_sub_assign(a, b) on rows of records: the
    threshold is a's, counts add / subtract mod 2^32, sums add / subtract mod
    p; a merge takes has_last and last_value from b when b has one, a diff
    keeps a's."""
    a64, b64 = a.astype(np.uint64), b.astype(np.uint64)
    r = a.copy()
    if diff:
        r[:, 1] = ((a64[:, 1] + np.uint64(2**32) - b64[:, 1]) % np.uint64(2**32)).astype(np.uint32)
        r[:, 4:] = ((a64[:, 4:] + np.uint64(P) - b64[:, 4:]) % np.uint64(P)).astype(np.uint32)
    else:
        r[:, 1] = ((a64[:, 1] + b64[:, 1]) % np.uint64(2**32)).astype(np.uint32)
        r[:, 4:] = ((a64[:, 4:] + b64[:, 4:]) % np.uint64(P)).astype(np.uint32)
        later = b[:, 2] != 0
        r[later, 2] = 1
        r[later, 3] = b[later, 3]
    return r


def np_merge(ka, ra, kb, rb, f=0, join=None):
    """(keys, records, due) of table ∪ batch."""
    ia, ib = join if join is not None else np_join(ka, kb)
    ina, inb = ia >= 0, ib >= 0
    keys = np.zeros((len(ia), 12), dtype=np.uint8)
    keys[ina] = ka[ia[ina]]
    keys[~ina] = kb[ib[~ina]]
    recs = np.zeros((len(ia), ra.shape[1]), dtype=np.uint32)
    recs[ina] = ra[ia[ina]]
    recs[~ina] = rb[ib[~ina]]
    both = ina & inb
    recs[both] = np_combine(ra[ia[both]], rb[ib[both]], diff=False)
    before = np.zeros(len(ia), dtype=np.uint64)
    before[ina] = ra[ia[ina], 1]
    after = before.copy()
    after[inb] += rb[ib[inb], 1].astype(np.uint64)
    due = np.zeros(len(ia), dtype=np.uint8)
    if f > 0:
        due = (inb & (after // np.uint64(f) > before // np.uint64(f))).astype(np.uint8)
    return keys, recs, due


def np_diff(ka, ra, kb, rb, join=None):
    """(records in a's order, matches): a[i] minus its b record where the key is in b."""
    ia, ib = join if join is not None else np_join(ka, kb)
    both = (ia >= 0) & (ib >= 0)
    out = ra.copy()
    out[ia[both]] = np_combine(ra[ia[both]], rb[ib[both]], diff=True)
    return out, int(both.sum())


@pytest.mark.parametrize("t", [1, 4])
def test_numpy_model_is_the_dict_model(t):
    rng = np.random.default_rng(4300 + t)
    seen = 0
    for i, (name, ka, kb) in enumerate(shapes(rng)):
        ra, rb = rand_recs(rng, len(ka), t), rand_recs(rng, len(kb), t)
        for f in (0, (1, 3, 1000)[i % 3]):
            for got, want in zip(np_merge(ka, ra, kb, rb, f), model_merge(ka, ra, kb, rb, t, f)):
                assert got.shape == want.shape and np.array_equal(got, want), (name, f)
        got, m = np_diff(ka, ra, kb, rb)
        want, wm = model_diff(ka, ra, kb, rb, t)
        assert m == wm and np.array_equal(got, want.reshape(got.shape)), name
        seen += m
    assert seen > 3 * FLOW_JOIN_TILE


def test_numpy_model_count_edges():
    """The rules the random records seldom reach: a count that wraps, `due`
    evaluated in 64 bits, sums that meet p."""
    t = 2
    keys = np.arange(4 * 12, dtype=np.uint8).reshape(4, 12)
    ra = np.array([[t, 0xFFFFFFFE, 0, 0, P - 1, 0], [t, 0xFFFFFFFF, 1, 9, 5, P - 5],
                   [t, 5, 1, 7, 0, 1], [t, 2, 0, 0, 3, 3]], dtype=np.uint32)
    rb = np.array([[t, 5, 1, 8, 1, 0], [t, 0xFFFFFFFF, 0, 0, P - 5, 5],
                   [t, 7, 0, 0, P - 1, P - 1], [t, 2, 1, 0, 3, 3]], dtype=np.uint32)
    for f in (1, 3, 1000):
        for got, want in zip(np_merge(keys, ra, keys, rb, f), model_merge(keys, ra, keys, rb, t, f)):
            assert np.array_equal(got, want), f
    got, m = np_diff(keys, ra, keys, rb)
    assert m == 4 and np.array_equal(got, model_diff(keys, ra, keys, rb, t)[0])
    assert got[:, 1].tolist() == [0xFFFFFFF9, 0, 0xFFFFFFFE, 0] and got[:, 4:].tolist() == [[P - 2, 0], [10, P - 10], [1, 2], [0, 0]]


# ------------------------------------------------------------------ scale inputs
def keys_from_integers(rng, n):
    """n distinct ascending keys from sorted distinct integers.  Words 0 and 1
    are a 64-bit integer v (some of them consecutive: keys that differ in the
    low bits of word 1 only); a twentieth of the v's stand five times, told
    apart by the top byte of word 2 alone; its other three bytes are random."""
    nv = n - 4 * (n // 20)
    base = rng.integers(2**24, 2**64 - 2**24, size=nv, dtype=np.uint64)
    near = (base[:nv // 50, None] + np.arange(1, 4, dtype=np.uint64)[None, :]).reshape(-1)
    v = np.unique(np.concatenate([base, near]))
    assert len(v) >= nv
    v = np.sort(v[rng.permutation(len(v))[:nv]])
    reps = np.ones(nv, dtype=np.int64)
    reps[rng.permutation(nv)[:n // 20]] = 5
    start = np.cumsum(reps) - reps
    c = (np.arange(n) - np.repeat(start, reps)).astype(np.uint64)       # 0, or 0..4 within a repeated v
    v = np.repeat(v, reps)
    w = np.stack([v >> np.uint64(32), v & np.uint64(0xFFFFFFFF),
                  (c * np.uint64(50) << np.uint64(24)) | rng.integers(0, 2**24, size=n, dtype=np.uint64)], axis=1)
    return w.astype(">u4").view(np.uint8).reshape(n, 12)


class Scale:
    pass


@pytest.fixture(scope="module")
def scale():
    rng = np.random.default_rng(4400)
    s = Scale()
    u = keys_from_integers(rng, NA + NB - SHARED)
    role = np.repeat(np.array([0, 1, 2], np.uint8), [NA - SHARED, NB - SHARED, SHARED])   # a only, b only, shared
    role = role[rng.permutation(len(role))]
    s.ka, s.kb = u[role != 1], u[role != 0]
    assert len(s.ka) == NA and len(s.kb) == NB
    s.join = np_join(s.ka, s.kb)
    s.d_ka, s.d_kb = dev(s.ka), dev(s.kb)
    return s


def assert_past_one_tile_per_thread():
    ntiles = -(-(NA + NB) // FLOW_JOIN_TILE)
    assert ntiles > SCAN_THREADS and -(-ntiles // SCAN_THREADS) >= 2


def test_scale_shape(scale):
    assert_past_one_tile_per_thread()
    ia, ib = scale.join
    both = (ia >= 0) & (ib >= 0)
    assert both.sum() == SHARED and 0.25 < SHARED / NB < 0.35 and len(ia) == NA + NB - SHARED
    # ascending in memcmp order, and neighbours that differ in the last word only
    w = key_words(np.concatenate([scale.ka[:200_000], scale.kb[:200_000]]))
    for k in (w[:200_000], w[200_000:]):
        hi = (k[:, 0] << np.uint64(32)) | k[:, 1]
        assert ((hi[1:] > hi[:-1]) | ((hi[1:] == hi[:-1]) & (k[1:, 2] > k[:-1, 2]))).all()
        assert (hi[1:] == hi[:-1]).sum() > 1000
    # as little-endian words the keys are not ascending: a kernel that compared those would refuse them
    le = np.ascontiguousarray(scale.ka[:1000]).view("<u4").reshape(-1, 3)[:, 0]
    assert (le[1:] < le[:-1]).any()


@pytest.mark.parametrize("t", [1, 4])
def test_merge_past_1024_tiles(scale, t):
    """t = 1: 20-byte records on the dword path; t = 4: the 16-byte vector path."""
    assert_past_one_tile_per_thread()
    rng = np.random.default_rng(4500 + t)
    ra, rb = rand_recs(rng, NA, t), rand_recs(rng, NB, t)
    wk, ws, wd = np_merge(scale.ka, ra, scale.kb, rb, 3, scale.join)
    k, s, d = sk.flows_merge(scale.d_ka, dev(ra), scale.d_kb, dev(rb), frequency_pkts=3)
    assert k.shape == wk.shape and s.shape == ws.shape and d.shape == wd.shape
    assert np.array_equal(host(k), wk)
    assert np.array_equal(host(s), ws)
    assert np.array_equal(host(d), wd)
    assert 0 < wd.sum() < len(wd)


@pytest.mark.parametrize("t", [1, 4])
def test_diff_past_1024_tiles(scale, t):
    assert_past_one_tile_per_thread()
    rng = np.random.default_rng(4600 + t)
    ra, rb = rand_recs(rng, NA, t), rand_recs(rng, NB, t)
    want, wm = np_diff(scale.ka, ra, scale.kb, rb, scale.join)
    got, m = sk.flows_diff(scale.d_ka, dev(ra), scale.d_kb, dev(rb))
    assert m == wm == SHARED
    assert np.array_equal(host(got), want)


def test_lookup_in_a_large_table(scale, ctx):
    t, nk = 4, 100_000
    rng = np.random.default_rng(4700)
    recs = rand_recs(rng, NA, t)
    ia, ib = scale.join
    b_only = scale.kb[ib[ia < 0]]                                       # absent from the table, spread between its keys
    below = np.zeros((50, 12), np.uint8)
    below[:, 11] = np.arange(50)                                        # below the first key (word 0 is 0)
    above = np.full((50, 12), 0xFF, np.uint8)
    above[:, 11] = np.arange(50)                                        # above the last one
    present = np.concatenate([[0, NA - 1], rng.integers(0, NA, size=nk // 2 - 2)])
    query = np.concatenate([scale.ka[present], below, above,
                            b_only[rng.integers(0, len(b_only), size=nk // 2 - 100)]])
    query = np.ascontiguousarray(query[rng.permutation(nk)])
    # numpy searchsorted on the keys as records of three big-endian words
    dt = np.dtype([("w0", ">u4"), ("w1", ">u4"), ("w2", ">u4")])
    table, q = np.ascontiguousarray(scale.ka).view(dt).reshape(-1), query.view(dt).reshape(-1)
    pos = np.searchsorted(table, q)
    found = (pos < NA) & (table[np.minimum(pos, NA - 1)] == q)
    assert found.sum() == nk // 2 and (pos == 0).sum() >= 51 and (pos == NA).sum() == 50
    fresh = np.zeros(4 + t, dtype=np.uint32)
    fresh[0] = t                                                        # qk_u32_init's record
    want = np.where(found[:, None], recs[np.minimum(pos, NA - 1)], fresh[None, :])
    out = np.full((nk, 4 + t), 0xEEEEEEEE, dtype=np.uint32)
    got_found = np.full(nk, 0xEE, dtype=np.uint8)
    d_recs = dev(recs)
    rc = lib().qk_u32_flows_lookup_device(ctx.handle, scale.d_ka.data_ptr(), d_recs.data_ptr(), NA, t,
                                          query.ctypes.data, nk, out.ctypes.data, got_found.ctypes.data, None)
    assert rc == QK_OK
    assert np.array_equal(got_found, found.astype(np.uint8))
    assert np.array_equal(out, want)
    # and through the wrapper, on a slice
    some = sk.flows_lookup(scale.d_ka, d_recs, [k.tobytes() for k in query[:300]])
    assert [None if x is None else x._buf.raw for x in some] == \
        [want[i].tobytes() if found[i] else None for i in range(300)]
