"""Device-resident flow table (qk_u32_flows_merge_device / _diff_device /
_lookup_device, DeviceFlowQuacks) on the GPU.  Expected values come from a
Python dict over keys with the host PowerSumQuackU32.merge / sub_assign, from
coracle.encode_u32, and from qo.sniff_multi_batch with its table kept across
batches — never from the code under test."""
import ctypes as C

import numpy as np
import pytest

import sidekick_amd as sk
from oracle import coracle, quack_oracle as qo
from sidekick_amd._lib import (FLOW_JOIN_TILE, QK_E_CAPACITY, QK_E_INVAL, QK_E_MISMATCH, QK_E_UNDECODABLE, QK_OK,
                               lib)

pytestmark = pytest.mark.gpu

P = qo.P32
T = FLOW_JOIN_TILE
MY_ADDR = (10, 0, 2, 1, 0x1F, 0x90)
META_DT = np.dtype([("pkttype", "u1"), ("reserved", "u1"), ("protocol_be", "<u2"), ("len", "<u4")])


# ----------------------------------------------------------------- plumbing
def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def host(tensor):
    a = tensor.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def hq(raw: bytes, t: int):
    """A host PowerSumQuackU32 holding the record `raw`."""
    q = sk.PowerSumQuackU32(t)
    assert len(raw) == len(q._buf)
    C.memmove(q._buf, raw, len(raw))
    return q


def sort_keys(keys):
    """Rows of a uint8 [n, 12] array in memcmp order."""
    return keys[np.lexsort(keys.T[::-1])] if len(keys) else keys


def rand_keys(rng, n):
    """n distinct random AddrKeys, ascending."""
    keys = np.unique(rng.integers(0, 256, size=(n + 16, 12), dtype=np.uint8), axis=0)
    assert len(keys) >= n
    return sort_keys(keys[rng.permutation(len(keys))[:n]])


def rand_recs(rng, n, t):
    r = rng.integers(0, P, size=(n, 4 + t), dtype=np.uint32)
    r[:, 0] = t
    r[:, 1] = rng.integers(0, 2**32, size=n, dtype=np.uint32)
    r[:, 2] = rng.integers(0, 2, size=n)
    r[:, 3] = np.where(r[:, 2] != 0, rng.integers(0, 2**32, size=n, dtype=np.uint32), 0)
    return r


def count_of(raw: bytes) -> int:
    return int.from_bytes(raw[4:8], "little")


# ------------------------------------------------------------------- models
def as_dict(keys, recs):
    return {keys[i].tobytes(): recs[i].tobytes() for i in range(len(keys))}


def model_merge(ka, ra, kb, rb, t, f=0):
    """(keys, records, due) of table ∪ batch by a dict and the host merge."""
    A, B = as_dict(ka, ra), as_dict(kb, rb)
    out, due = dict(A), {}
    for k, rec in B.items():
        before = count_of(A[k]) if k in A else 0
        if k in A:
            q = hq(A[k], t)
            q.merge(hq(rec, t))
            out[k] = q._buf.raw
        else:
            out[k] = rec
        due[k] = int(f > 0 and (before + count_of(rec)) // f > before // f)
    ks = sorted(out)
    keys = np.frombuffer(b"".join(ks), dtype=np.uint8).reshape(len(ks), 12)
    recs = np.frombuffer(b"".join(out[k] for k in ks), dtype=np.uint32).reshape(len(ks), 4 + t)
    return keys, recs, np.array([due.get(k, 0) for k in ks], dtype=np.uint8)


def model_diff(ka, ra, kb, rb, t):
    """(records in a's order, matches) by the host clone() + sub_assign."""
    B = as_dict(kb, rb)
    rows, matched = [], 0
    for i in range(len(ka)):
        raw, k = ra[i].tobytes(), ka[i].tobytes()
        if k in B:
            q = hq(raw, t).clone()
            q.sub_assign(hq(B[k], t))
            raw = q._buf.raw
            matched += 1
        rows.append(raw)
    return np.frombuffer(b"".join(rows), dtype=np.uint32).reshape(len(ka), 4 + t), matched


def run_merge(ka, ra, kb, rb, f=0, ctx=None):
    k, s, d = sk.flows_merge(dev(ka), dev(ra), dev(kb), dev(rb), frequency_pkts=f, ctx=ctx)
    return host(k), host(s), host(d)


def check_merge(ka, ra, kb, rb, t, f=0, ctx=None):
    gk, gs, gd = run_merge(ka, ra, kb, rb, f, ctx)
    wk, ws, wd = model_merge(ka, ra, kb, rb, t, f)
    assert gk.shape == wk.shape and np.array_equal(gk, wk)
    assert np.array_equal(gs, ws)
    assert np.array_equal(gd, wd)
    return gk, gs, gd


def check_diff(ka, ra, kb, rb, t):
    d, m = sk.flows_diff(dev(ka), dev(ra), dev(kb), dev(rb))
    want, wm = model_diff(ka, ra, kb, rb, t)
    assert m == wm
    assert np.array_equal(host(d).reshape(len(ka), 4 + t), want)


# ------------------------------------------------------------------- shapes
def split(universe, in_a, in_b):
    return universe[np.asarray(in_a, bool)], universe[np.asarray(in_b, bool)]


def shapes(rng, small=False):
    """(name, keys_a, keys_b) of the join shapes; small: every array <= 64 keys."""
    U = 12 if small else T
    out = [("empty", rand_keys(rng, 0), rand_keys(rng, 0)),
           ("a empty", rand_keys(rng, 0), rand_keys(rng, 7)),
           ("b empty", rand_keys(rng, 7), rand_keys(rng, 0))]
    k = rand_keys(rng, 1)
    out.append(("one shared key", k, k.copy()))
    k = rand_keys(rng, 3 * U)
    out.append(("identical sets: every diagonal lands on a pair", k, k.copy()))
    u = rand_keys(rng, 5 * U)                                  # disjoint, interleaved: 3U+1 and 2U-1
    ina = np.ones(5 * U, bool)
    ina[1:2 * (2 * U - 1):2] = False
    assert ina.sum() == 3 * U + 1
    out.append(("disjoint interleaved",) + split(u, ina, ~ina))
    u = rand_keys(rng, 2 * U + U // 2 + 3)                     # all of a below all of b, and the reverse
    lowa = np.arange(len(u)) < U + U // 2
    out.append(("a below b",) + split(u, lowa, ~lowa))
    out.append(("b below a",) + split(u, ~lowa, lowa))
    u = rand_keys(rng, 7 * U + U // 2)                         # 5U and 5U, half of each shared
    role = rng.permutation(np.repeat([0, 1, 2], [2 * U + U // 2] * 3))
    out.append(("half shared",) + split(u, role != 1, role != 0))
    if not small:
        # the only shared keys sit at merged positions (T-1, T) and (2T-1, 2T):
        # universe index T-1 is merged positions T-1, T; index 2T-2 is 2T-1, 2T
        u = rand_keys(rng, 2 * T + 500)
        ina = rng.integers(0, 2, size=len(u)).astype(bool)
        inb = ~ina
        ina[[T - 1, 2 * T - 2]] = True
        inb[[T - 1, 2 * T - 2]] = True
        out.append(("pairs on the diagonals",) + split(u, ina, inb))
    return out


@pytest.mark.parametrize("t", [1, 5, 32, 80, 1024])
def test_merge_and_diff_against_dict_model(t):
    """t = 1: 20-byte records on the dword path; 32 and 80: the vector path;
    1024 with n <= 64."""
    rng = np.random.default_rng(4100 + t)
    for name, ka, kb in shapes(rng, small=t == 1024):
        ra, rb = rand_recs(rng, len(ka), t), rand_recs(rng, len(kb), t)
        f = int(rng.choice([0, 1, 3, 1000]))
        try:
            check_merge(ka, ra, kb, rb, t, f)
            check_diff(ka, ra, kb, rb, t)
        except AssertionError as e:
            raise AssertionError(f"shape {name!r}, t={t}, f={f}: {e}") from e


def test_diff_ignores_b_keys_outside_a():
    t = 8
    rng = np.random.default_rng(77)
    u = rand_keys(rng, 3 * T)
    ina = np.arange(len(u)) % 3 == 0
    ka, kb_extra = split(u, ina, ~ina)
    shared = ka[::2]
    ra = rand_recs(rng, len(ka), t)
    rs = rand_recs(rng, len(shared), t)
    d1, m1 = sk.flows_diff(dev(ka), dev(ra), dev(shared), dev(rs))
    kb = sort_keys(np.concatenate([shared, kb_extra]))
    B = as_dict(shared, rs)
    B.update(as_dict(kb_extra, rand_recs(rng, len(kb_extra), t)))
    rb = np.frombuffer(b"".join(B[k.tobytes()] for k in kb), dtype=np.uint32).reshape(len(kb), 4 + t)
    d2, m2 = sk.flows_diff(dev(ka), dev(ra), dev(kb), dev(rb))
    assert m1 == m2 == len(shared)
    assert np.array_equal(host(d1), host(d2))
    check_diff(ka, ra, kb, rb, t)


# ---------------------------------------------------------------- key order
def test_key_order_is_memcmp():
    t = 4
    rng = np.random.default_rng(5)
    z = [0] * 12
    keys = []
    for v in (1, 2, 0x80, 0xFF):
        keys.append(bytes([v] + z[1:]))          # differ only in byte 0
        keys.append(bytes(z[:11] + [v]))         # differ only in byte 11
    # as little-endian words 0x02000001 > 0x01000002, but memcmp puts the first one first
    keys += [bytes([0x01, 0, 0, 0x02] + z[4:]), bytes([0x02, 0, 0, 0x01] + z[4:]),
             bytes(z[:4] + [0x01, 0, 0, 0x02] + z[8:]), bytes(z[:4] + [0x02, 0, 0, 0x01] + z[8:]),
             bytes(z[:8] + [0x01, 0, 0, 0x02]), bytes(z[:8] + [0x02, 0, 0, 0x01])]
    keys = sorted(set(keys))
    u = np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(len(keys), 12)
    assert np.array_equal(u, sort_keys(u))
    for trial in range(6):
        role = rng.integers(0, 3, size=len(u))
        ka, kb = split(u, role != 1, role != 0)
        ra, rb = rand_recs(rng, len(ka), t), rand_recs(rng, len(kb), t)
        check_merge(ka, ra, kb, rb, t)
        check_diff(ka, ra, kb, rb, t)
    recs = rand_recs(rng, len(u), t)
    got = sk.flows_lookup(dev(u), dev(recs), keys)
    assert [q._buf.raw for q in got] == [recs[i].tobytes() for i in range(len(u))]


# ---------------------------------------------------------- arithmetic edges
@pytest.mark.parametrize("t", [4, 5])
def test_arithmetic_edges(t):
    """Hand-built records, every key shared: t = 4 takes the vector path, 5 the dword path."""
    def rec(sums, count, last):
        r = np.zeros(4 + t, dtype=np.uint32)
        r[0], r[1], r[2], r[3] = t, count, int(last is not None), last or 0
        r[4:] = sums
        return r
    cases = [  # (a sums, a count, a last), (b ...), merged (sum, count, last), diff (sum, count, last)
        ((P - 1, 0xFFFFFFFF, None), (P - 1, 2, None), (P - 2, 1, None), (0, 0xFFFFFFFD, None)),
        ((0, 1, 7), (P - 1, 2, None), (P - 1, 3, 7), (1, 0xFFFFFFFF, 7)),
        ((123456, 5, None), (123456, 5, 9), (246912, 10, 9), (0, 0, None)),
        ((P - 1, 0, 11), (1, 0, 12), (0, 0, 12), (P - 2, 0, 11)),
        ((5, 9, 0xFFFFFFFF), (P - 5, 4, 0), (0, 13, 0), (10, 5, 0xFFFFFFFF)),
    ]
    keys = rand_keys(np.random.default_rng(9), len(cases))
    ra = np.stack([rec([c[0][0]] * t, c[0][1], c[0][2]) for c in cases])
    rb = np.stack([rec([c[1][0]] * t, c[1][1], c[1][2]) for c in cases])
    _, gs, _ = check_merge(keys, ra, keys, rb, t)
    check_diff(keys, ra, keys, rb, t)
    gd = host(sk.flows_diff(dev(keys), dev(ra), dev(keys), dev(rb))[0])
    for i, c in enumerate(cases):
        for got, (s, cnt, last) in ((gs[i], c[2]), (gd[i], c[3])):
            assert got[0] == t and got[1] == cnt, (i, got[:4])
            assert got[2] == int(last is not None) and got[3] == (last or 0), (i, got[:4])
            assert got[4:].tolist() == [s] * t, (i, got[4:])


# ----------------------------------------------------------------- alignment
def test_record_array_off_the_vector_alignment():
    import torch
    t = 32
    rng = np.random.default_rng(32)
    u = rand_keys(rng, 3 * T)
    role = rng.integers(0, 3, size=len(u))
    ka, kb = split(u, role != 1, role != 0)
    ra, rb = rand_recs(rng, len(ka), t), rand_recs(rng, len(kb), t)

    def shifted(r):
        big = torch.zeros(r.size + 8, dtype=torch.int32, device="cuda")
        v = big[1:1 + r.size].view(r.shape)
        v.copy_(dev(r))
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    want = check_merge(ka, ra, kb, rb, t, 3)
    wd, wm = sk.flows_diff(dev(ka), dev(ra), dev(kb), dev(rb))
    for sa, sb in ((shifted(ra), dev(rb)), (dev(ra), shifted(rb)), (shifted(ra), shifted(rb))):
        k, s, d = sk.flows_merge(dev(ka), sa, dev(kb), sb, frequency_pkts=3)
        assert np.array_equal(host(k), want[0]) and np.array_equal(host(s), want[1])
        assert np.array_equal(host(d), want[2])
        gd, gm = sk.flows_diff(dev(ka), sa, dev(kb), sb)
        assert gm == wm and torch.equal(gd, wd)


# -------------------------------------------------------------------- errors
def raw_merge(ctx, ka, ra, kb, rb, t, ko, so, do, cap, f=0):
    n = C.c_size_t(12345)
    p = lambda x: x if isinstance(x, int) or x is None else x.data_ptr()   # noqa: E731
    rc = lib().qk_u32_flows_merge_device(ctx.handle, p(ka), p(ra), len(ka), p(kb), p(rb), len(kb), t, f, p(ko), p(so),
                                         p(do), cap, C.byref(n), None)
    return rc, n.value


def raw_diff(ctx, ka, ra, kb, rb, t, out):
    m = C.c_size_t()
    p = lambda x: x if isinstance(x, int) or x is None else x.data_ptr()   # noqa: E731
    return lib().qk_u32_flows_diff_device(ctx.handle, p(ka), p(ra), len(ka), p(kb), p(rb), len(kb), t, p(out),
                                          C.byref(m), None)


def outputs(cap, t, fill=0x5A):
    import torch
    return (torch.full((cap, 12), fill, dtype=torch.uint8, device="cuda"),
            torch.full((cap, 4 + t), 0x5A5A5A5A, dtype=torch.int32, device="cuda"),
            torch.full((cap,), fill, dtype=torch.uint8, device="cuda"))


def test_capacity_is_decided_before_any_write(ctx):
    import torch
    t = 8
    rng = np.random.default_rng(11)
    u = rand_keys(rng, 3 * T)
    role = rng.integers(0, 3, size=len(u))
    ka, kb = split(u, role != 1, role != 0)
    ra, rb = rand_recs(rng, len(ka), t), rand_recs(rng, len(kb), t)
    n_out = len(u)
    ko, so, do = outputs(n_out, t)
    rc, n = raw_merge(ctx, dev(ka), dev(ra), dev(kb), dev(rb), t, ko, so, do, n_out - 1)
    assert rc == QK_E_CAPACITY and n == n_out
    torch.cuda.synchronize()
    assert bool((ko == 0x5A).all()) and bool((so == 0x5A5A5A5A).all()) and bool((do == 0x5A).all())
    rc, n = raw_merge(ctx, dev(ka), dev(ra), dev(kb), dev(rb), t, ko, so, do, n_out)
    assert rc == QK_OK and n == n_out
    wk, ws, _ = model_merge(ka, ra, kb, rb, t)
    assert np.array_equal(host(ko), wk) and np.array_equal(host(so), ws)


@pytest.mark.parametrize("where", ["a in a tile", "b in a tile", "a across tiles", "b across tiles"])
@pytest.mark.parametrize("fault", ["swapped", "duplicated"])
def test_input_out_of_order_is_invalid(ctx, where, fault):
    t = 4
    rng = np.random.default_rng(13)
    across = "across" in where
    bad = rand_keys(rng, 2 * T + 100)
    good = rand_keys(rng, 0 if across else T + 50)   # alone, the bad array is cut at multiples of T
    pos = T - 1 if across else 700
    if fault == "swapped":
        bad[[pos, pos + 1]] = bad[[pos + 1, pos]]
    else:
        bad[pos + 1] = bad[pos]
    ka, kb = (bad, good) if where.startswith("a") else (good, bad)
    ra, rb = rand_recs(rng, len(ka), t), rand_recs(rng, len(kb), t)
    ko, so, do = outputs(len(ka) + len(kb), t)
    rc, _ = raw_merge(ctx, dev(ka), dev(ra), dev(kb), dev(rb), t, ko, so, do, len(ka) + len(kb))
    assert rc == QK_E_INVAL
    assert raw_diff(ctx, dev(ka), dev(ra), dev(kb), dev(rb), t, outputs(max(len(ka), 1), t)[1]) == QK_E_INVAL


def test_threshold_field_mismatch(ctx):
    t = 8
    rng = np.random.default_rng(17)
    u = rand_keys(rng, 2 * T)
    ka, kb = u[::2], u[1::3]
    for which in ("a", "b"):
        ra, rb = rand_recs(rng, len(ka), t), rand_recs(rng, len(kb), t)
        (ra if which == "a" else rb)[333, 0] = t + 1
        ko, so, do = outputs(len(u), t)
        rc, _ = raw_merge(ctx, dev(ka), dev(ra), dev(kb), dev(rb), t, ko, so, do, len(u))
        assert rc == QK_E_MISMATCH, which
    # in a diff only a record that is read can be found: a's, or a matched b's
    ra, rb = rand_recs(rng, len(ka), t), rand_recs(rng, len(ka), t)
    rb[100, 0] = t - 1
    assert raw_diff(ctx, dev(ka), dev(ra), dev(ka), dev(rb), t, outputs(len(ka), t)[1]) == QK_E_MISMATCH
    ra[5, 0] = 0
    assert raw_diff(ctx, dev(ka), dev(ra), dev(kb), dev(rand_recs(rng, len(kb), t)), t,
                    outputs(len(ka), t)[1]) == QK_E_MISMATCH
    with pytest.raises(sk.QuackError) as e:
        sk.flows_lookup(dev(ka), dev(ra), [ka[5].tobytes()])
    assert e.value.code == QK_E_MISMATCH


def test_overlap_and_host_pointers_are_invalid(ctx):
    t = 8
    rng = np.random.default_rng(19)
    ka, kb = rand_keys(rng, 40), rand_keys(rng, 30)
    ra, rb = rand_recs(rng, 40, t), rand_recs(rng, 30, t)
    dka, dra, dkb, drb = dev(ka), dev(ra), dev(kb), dev(rb)
    ko, so, do = outputs(70, t)
    assert raw_merge(ctx, dka, dra, dkb, drb, t, ko, so, do, 70)[0] == QK_OK
    # an output over an input
    assert raw_merge(ctx, dka, dra, dkb, drb, t, ko, dra, do, 40)[0] == QK_E_INVAL
    assert raw_merge(ctx, dka, dra, dkb, drb, t, dkb, so, do, 30)[0] == QK_E_INVAL
    big = outputs(200, t)[1]
    inner = big.view(-1)[100:]                       # a record array inside a larger one
    assert raw_merge(ctx, dka, dra, dkb, drb, t, ko, inner, do, 70)[0] == QK_OK
    inner[:30 * (4 + t)].copy_(drb.view(-1))
    assert raw_merge(ctx, dka, dra, dkb, inner, t, ko, so, do, 70)[0] == QK_OK
    assert raw_merge(ctx, dka, dra, dkb, inner, t, ko, big, do, 70)[0] == QK_E_INVAL
    assert raw_diff(ctx, dka, dra, dkb, drb, t, dra) == QK_E_INVAL
    assert raw_diff(ctx, dka, dra, dkb, drb, t, drb) == QK_E_INVAL
    # a host pointer where a device array is required
    hk, hr = np.ascontiguousarray(ka), np.ascontiguousarray(ra)
    n = C.c_size_t()
    args = [dka.data_ptr(), dra.data_ptr(), 40, dkb.data_ptr(), drb.data_ptr(), 30, t, 0, ko.data_ptr(),
            so.data_ptr(), do.data_ptr(), 70, C.byref(n), None]
    for slot, hostp in ((0, hk.ctypes.data), (1, hr.ctypes.data), (3, hk.ctypes.data), (4, hr.ctypes.data),
                        (8, hk.ctypes.data), (9, hr.ctypes.data)):
        bad = list(args)
        bad[slot] = hostp
        assert lib().qk_u32_flows_merge_device(ctx.handle, *bad) == QK_E_INVAL, slot
    out = outputs(40, t)[1]
    m = C.c_size_t()
    assert lib().qk_u32_flows_diff_device(ctx.handle, hk.ctypes.data, dra.data_ptr(), 40, dkb.data_ptr(),
                                          drb.data_ptr(), 30, t, out.data_ptr(), C.byref(m), None) == QK_E_INVAL
    assert lib().qk_u32_flows_diff_device(ctx.handle, dka.data_ptr(), dra.data_ptr(), 40, dkb.data_ptr(),
                                          drb.data_ptr(), 30, t, hr.ctypes.data, C.byref(m), None) == QK_E_INVAL
    # a misaligned array
    assert raw_merge(ctx, dka, dra.data_ptr() + 2, dkb, drb, t, ko, so, do, 70)[0] == QK_E_INVAL
    found = C.create_string_buffer(1)
    rec = C.create_string_buffer(lib().qk_u32_size(t))
    assert lib().qk_u32_flows_lookup_device(ctx.handle, hk.ctypes.data, dra.data_ptr(), 40, t, hk.ctypes.data, 1, rec,
                                            found, None) == QK_E_INVAL
    assert lib().qk_u32_flows_lookup_device(ctx.handle, dka.data_ptr(), dra.data_ptr(), 40, t, dka.data_ptr(), 1, rec,
                                            found, None) == QK_E_INVAL


# -------------------------------------------------------------------- lookup
def test_lookup(ctx):
    t = 8
    rng = np.random.default_rng(23)
    u = rand_keys(rng, 3 * T + 1 + 50)
    absent = np.zeros(len(u), bool)
    absent[rng.permutation(len(u))[:50]] = True
    absent[[0, len(u) - 1]] = False
    keys, gone = u[~absent], u[absent]
    recs = rand_recs(rng, len(keys), t)
    table = as_dict(keys, recs)
    query = [keys[0].tobytes(), keys[-1].tobytes(), gone[3].tobytes(), keys[T].tobytes(), keys[T].tobytes(),
             b"\x00" * 12, b"\xff" * 12, keys[0].tobytes()]
    query += [k.tobytes() for k in gone[:20]] + [keys[i].tobytes() for i in rng.integers(0, len(keys), size=200)]
    dk, dr = dev(keys), dev(recs)
    got = sk.flows_lookup(dk, dr, query)
    assert len(got) == len(query)
    for k, q in zip(query, got):
        if k in table:
            assert q is not None and q._buf.raw == table[k] and q.threshold() == t, k.hex()
        else:
            assert q is None, k.hex()
    assert sk.flows_lookup(dk, dr, []) == []
    # the records of the C call itself: a flow's own, or qk_u32_init's
    nk, rec = len(query), lib().qk_u32_size(t)
    hk = C.create_string_buffer(b"".join(query), nk * 12)
    out = C.create_string_buffer(b"\xEE" * (nk * rec), nk * rec)
    found = C.create_string_buffer(b"\xEE" * nk, nk)
    assert lib().qk_u32_flows_lookup_device(ctx.handle, dk.data_ptr(), dr.data_ptr(), len(keys), t, hk, nk, out, found,
                                            None) == QK_OK
    fresh = sk.PowerSumQuackU32(t)._buf.raw
    for i, k in enumerate(query):
        assert found.raw[i] == int(k in table)
        assert out.raw[i * rec:(i + 1) * rec] == table.get(k, fresh)
    # an empty table finds nothing
    ek, er = dev(np.zeros((0, 12), np.uint8)), dev(np.zeros((0, 4 + t), np.uint32))
    assert sk.flows_lookup(ek, er, query[:5]) == [None] * 5
    empty = sk.DeviceFlowQuacks(t)
    assert len(empty) == 0 and empty.quack(query[0]) is None and empty.senders() == {}


# ----------------------------------------------------------------------- due
@pytest.mark.parametrize("f", [1, 3, 1000])
def test_due_against_python_integers(f):
    t = 4
    rng = np.random.default_rng(29 + f)
    u = rand_keys(rng, 2 * T + 77)
    role = rng.integers(0, 3, size=len(u))
    role[:4] = 2                                     # shared, for the hand-set counts below
    ka, kb = split(u, role != 1, role != 0)
    ra, rb = rand_recs(rng, len(ka), t), rand_recs(rng, len(kb), t)
    ra[:, 1] = rng.integers(0, 3000, size=len(ka))
    rb[:, 1] = rng.integers(0, 5, size=len(kb))      # b.count 0: never due
    ra[0, 1], rb[0, 1] = 0xFFFFFFFE, 5               # the rule is evaluated in 64 bits
    ra[1, 1], rb[1, 1] = 0xFFFFFFFF, 0xFFFFFFFF
    ra[2, 1], rb[2, 1] = 2 * f - 1, 1
    ra[3, 1], rb[3, 1] = 2 * f, max(f - 1, 0)
    gk, _, gd = check_merge(ka, ra, kb, rb, t, f)
    A, B = as_dict(ka, ra), as_dict(kb, rb)
    for i in range(len(gk)):
        k = gk[i].tobytes()
        before = count_of(A[k]) if k in A else 0
        want = k in B and (before + count_of(B[k])) // f > before // f
        assert gd[i] == int(want), (k.hex(), before, f)
    k0 = ka[0].tobytes()
    assert gd[[g.tobytes() for g in gk].index(k0)] == int((0xFFFFFFFE + 5) // f > 0xFFFFFFFE // f)
    # frequency 0: no flow is ever due
    assert not run_merge(ka, ra, kb, rb, 0)[2].any()


# -------------------------------------------------------------- packet batches
def packets(flows, f, ids, seed=0):
    """One full-length incoming UDP record per entry: flow flows[f[i]], identifier ids[i]."""
    rng = np.random.default_rng(seed)
    n = len(f)
    bufs = rng.integers(0, 256, size=(n, 67), dtype=np.uint8)
    bufs[:, 23] = 17
    key = flows[f]
    bufs[:, 26:30] = key[:, 0:4]
    bufs[:, 34:36] = key[:, 4:6]
    bufs[:, 30:34] = key[:, 6:10]
    bufs[:, 36:38] = key[:, 10:12]
    ids = np.asarray(ids, dtype=np.uint32)
    for b in range(4):
        bufs[:, 63 + b] = (ids >> (24 - 8 * b)) & 0xFF
    meta = np.zeros(n, dtype=META_DT)
    meta["protocol_be"] = 0x0008
    meta["len"] = 67
    return bufs, meta


def make_flows(n, nflows, seed, stride=67, p_filter=0.1, p_reset=0.01, flows=None, reset_until=0.5):
    """tests/test_flows.py make_flows: n records over the AddrKeys `flows`, some
    filtered, resets (packets to MY_ADDR) only in the first reset_until fraction."""
    rng = np.random.default_rng(seed)
    bufs = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
    bufs[:, 23] = 17
    if flows is None:
        flows = rng.integers(0, 256, size=(nflows, 12), dtype=np.uint8)
        flows[:, 6:12] = (192, 168, 0, 9, 0x11, 0x5C)
        flows[: nflows // 2, 9] = rng.integers(0, 256, size=nflows // 2)
    f = rng.integers(0, len(flows), size=n)
    key = flows[f]
    bufs[:, 26:30] = key[:, 0:4]
    bufs[:, 34:36] = key[:, 4:6]
    bufs[:, 30:34] = key[:, 6:10]
    bufs[:, 36:38] = key[:, 10:12]
    r = rng.random(n)
    rs = (r < p_reset) & (np.arange(n) < int(reset_until * n))
    bufs[rs, 30:34] = MY_ADDR[:4]
    bufs[rs, 36:38] = MY_ADDR[4:]
    meta = np.zeros(n, dtype=META_DT)
    meta["protocol_be"] = 0x0008
    meta["len"] = 67
    k = (r >= p_reset) & (r < p_reset + p_filter)
    kind = rng.integers(0, 4, size=n)
    meta["pkttype"][k & (kind == 0)] = 4
    meta["protocol_be"][k & (kind == 1)] = 0xDD86
    bufs[k & (kind == 2), 23] = 6
    meta["len"][k & (kind == 3)] = 40
    return bufs, meta, flows


def vector_flows(bufs, meta, my_addr=MY_ADDR):
    """tests/test_flows.py vector_flows: {key: ids in packet order after the last reset}."""
    inc = (meta["pkttype"] == 0) | (meta["pkttype"] == 3)
    ok = inc & (meta["protocol_be"] == 0x0008) & (bufs[:, 23] == 17)
    keys = np.concatenate([bufs[:, 26:30], bufs[:, 34:36], bufs[:, 30:34], bufs[:, 36:38]], axis=1)
    rst = ok & np.all(keys[:, 6:12] == np.array(my_addr, dtype=np.uint8), axis=1)
    ins = ok & ~rst & (meta["len"] == 67)
    last_reset = int(np.nonzero(rst)[0][-1]) if rst.any() else -1
    idb = bufs[:, 63:67].astype(np.uint32)
    ids = (idb[:, 0] << 24) | (idb[:, 1] << 16) | (idb[:, 2] << 8) | idb[:, 3]
    out = {}
    for i in np.nonzero(ins[last_reset + 1:])[0] + last_reset + 1:
        out.setdefault(bytes(keys[i]), []).append(int(ids[i]))
    return out


def dev_batch(bufs, meta):
    import torch
    return (torch.from_numpy(bufs.reshape(-1).copy()).cuda(), torch.from_numpy(meta.view(np.int64).copy()).cuda())


def test_due_literally_against_the_sniff_loop():
    """400 packets, 5 flows, f = 3: the flows whose count hit a multiple of 3
    after an insert (start_sidekick_multi_frequency_pkts) are stats["due"]."""
    t, f = 8, 3
    bufs, meta, _ = make_flows(400, 5, seed=31, p_reset=0.0, p_filter=0.1)
    table, due = {}, set()
    for i in range(len(bufs)):
        _, st = qo.sniff_multi_batch(table, t, bufs[i:i + 1], meta["pkttype"][i:i + 1], meta["protocol_be"][i:i + 1],
                                     meta["len"][i:i + 1], MY_ADDR)
        if st["inserted"]:
            k = qo.addr_key(bufs[i])
            if table[k].count % f == 0:
                due.add(k)
    dt = sk.DeviceFlowQuacks(t)
    b, m = dev_batch(bufs, meta)
    stats = dt.insert_packets(b, 67, m, MY_ADDR, frequency_pkts=f)
    assert set(stats["due"]) == due and len(stats["due"]) == len(due) and due
    # a second batch of one packet per flow: due exactly where the count reaches a multiple of 3
    flows = np.frombuffer(b"".join(sorted(table)), dtype=np.uint8).reshape(-1, 12)
    bufs2, meta2 = packets(flows, np.arange(len(flows)), np.arange(len(flows)) + 9000)
    before = {k: q.count for k, q in table.items()}
    b2, m2 = dev_batch(bufs2, meta2)
    stats = dt.insert_packets(b2, 67, m2, MY_ADDR, frequency_pkts=f)
    assert set(stats["due"]) == {k for k, c in before.items() if (c + 1) % f == 0}
    assert dt.insert_packets(b, 67, m, MY_ADDR)["due"] == []


def assert_table_equals_oracle(got: dict, want: dict):
    assert set(got) == set(want)
    for k, w in want.items():
        q = got[k]
        assert q.power_sums() == w.power_sums, k.hex()
        assert q.count() == w.count and q.last_value() == w.last_value, k.hex()


def test_table_across_batches_equals_the_oracle():
    """Four batches of 5 000 records over 300 flows, the third with resets up
    to its midpoint: after each, the device table is the oracle's and FlowQuacks'."""
    t = 16
    _, _, flows = make_flows(10, 300, seed=40)
    oracle, dt, ht = {}, sk.DeviceFlowQuacks(t), sk.FlowQuacks(t)
    for b in range(4):
        bufs, meta, _ = make_flows(5000, 300, seed=41 + b, flows=flows, p_reset=0.01 if b == 2 else 0.0,
                                   reset_until=0.5)
        oracle, ost = qo.sniff_multi_batch(oracle, t, bufs, meta["pkttype"], meta["protocol_be"], meta["len"], MY_ADDR)
        assert (ost["resets"] > 0) == (b == 2)
        db, dm = dev_batch(bufs, meta)
        st = dt.insert_packets(db, 67, dm, MY_ADDR)
        hst = ht.insert_packets(db, 67, dm, MY_ADDR)
        assert {k: st[k] for k in ost} == ost == hst
        got = dt.senders()
        assert len(dt) == len(oracle) == len(got)
        assert_table_equals_oracle(got, oracle)
        assert got == ht.senders()
        assert list(got) == sorted(got) and dt.keys.shape == (len(got), 12)
        some = sorted(oracle)[::37] + [b"\x07" * 12]
        for k, q in zip(some, dt.quacks(some)):
            assert (q is None) == (k not in oracle) and (q is None or q == got[k])


def test_table_spanning_several_tiles():
    """60 000 records over 3T flows in two batches, against vector_flows + coracle.encode_u32."""
    t = 8
    _, _, flows = make_flows(10, 3 * T, seed=50)
    dt = sk.DeviceFlowQuacks(t)
    parts = [make_flows(30_000, 3 * T, seed=51 + b, flows=flows, p_reset=0.0)[:2] for b in range(2)]
    for bufs, meta in parts:
        db, dm = dev_batch(bufs, meta)
        dt.insert_packets(db, 67, dm, MY_ADDR)
    want = vector_flows(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
    got = dt.senders()
    assert len(want) > 2 * T and set(got) == set(want)
    for k, ids in want.items():
        q = got[k]
        assert q.power_sums() == coracle.encode_u32(np.array(ids, dtype=np.uint32), t), k.hex()
        assert q.count() == len(ids) and q.last_value() == ids[-1]


def test_end_to_end_on_the_device():
    """sender table - proxy table -> decode_segments, the diffs never leaving
    the device: the positions are the dropped positions per flow."""
    import torch
    t, n, nflows = 8, 20_000, 300
    rng = np.random.default_rng(60)
    flows = rand_keys(rng, nflows)
    flows[:, 6:12] = (192, 168, 0, 9, 0x11, 0x5C)
    flows = np.unique(flows, axis=0)
    nflows = len(flows)
    f = np.concatenate([np.zeros(3, np.int64), rng.integers(1, nflows, size=n - 3)])
    f = f[rng.permutation(n)]
    ids = rng.permutation(1 << 24)[:n].astype(np.uint32) + 1000   # distinct: a hit can only be a drop
    bufs, meta = packets(flows, f, ids, seed=61)
    drop = np.zeros(n, bool)
    big = int(np.argmax(np.bincount(f, minlength=nflows)[1:])) + 1
    for g in range(nflows):
        idx = np.nonzero(f == g)[0]
        k = len(idx) if g == 0 else 9 if g == big else int(rng.integers(0, 9))
        drop[rng.permutation(idx)[:min(k, len(idx))]] = True
    assert (f[drop] == 0).sum() == 3 and (f[drop] == big).sum() == 9
    sender, proxy = sk.DeviceFlowQuacks(t), sk.DeviceFlowQuacks(t)
    for table, keep in ((sender, np.ones(n, bool)), (proxy, ~drop)):
        db, dm = dev_batch(bufs[keep], meta[keep])
        table.insert_packets(db, 67, dm, MY_ADDR)
    assert len(sender) == len(np.unique(f)) and len(proxy) == len(sender) - 1
    diffs = sender.diff(proxy)
    assert isinstance(diffs, torch.Tensor) and diffs.is_cuda and diffs.shape == (len(sender), 4 + t)
    # the sender's log, grouped by flow in key order
    order = [int(g) for g in np.lexsort(flows.T[::-1]) if (f == g).any()]
    assert [flows[g].tobytes() for g in order] == [bytes(k) for k in host(sender.keys)]
    log, offs, want = [], [0], []
    for g in order:
        idx = np.nonzero(f == g)[0]
        log.append(ids[idx])
        offs.append(offs[-1] + len(idx))
        want.append(np.nonzero(drop[idx])[0].tolist())
    d_log = torch.from_numpy(np.concatenate(log).view(np.int32)).cuda()
    pos, status = sk.decode_segments(diffs, d_log, offs, stop_at_last=False)
    for j, g in enumerate(order):
        if g == big:
            assert status[j] == QK_E_UNDECODABLE and pos[j] == []
        else:
            assert status[j] == QK_OK and pos[j] == want[j], (g, pos[j], want[j])
    assert pos[order.index(0)] == [0, 1, 2]


# ------------------------------------------------------------ growth hygiene
def test_scratch_growth_does_not_change_the_result():
    t = 1
    rng = np.random.default_rng(70)
    u = rand_keys(rng, 150_000)
    role = rng.integers(0, 8, size=len(u))
    ka, kb = split(u, (role < 4) | (role == 7), role >= 4)   # an eighth of the keys shared
    ra, rb = rand_recs(rng, len(ka), t), rand_recs(rng, len(kb), t)
    fresh = sk.Context(0)
    try:
        small = rand_keys(rng, 40)
        check_merge(small[::2], rand_recs(rng, 20, t), small[1::2], rand_recs(rng, 20, t), t, ctx=fresh)
        grown = run_merge(ka, ra, kb, rb, 3, ctx=fresh)     # > 1 MiB of index arrays: the scratch grows
        again = run_merge(ka, ra, kb, rb, 3, ctx=fresh)     # and now it does not
        d1 = sk.flows_diff(dev(ka), dev(ra), dev(kb), dev(rb), ctx=fresh)
    finally:
        fresh.close()
    want = model_merge(ka, ra, kb, rb, t, 3)
    for got in (grown, again):
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    wd, wm = model_diff(ka, ra, kb, rb, t)
    assert d1[1] == wm and np.array_equal(host(d1[0]), wd)
