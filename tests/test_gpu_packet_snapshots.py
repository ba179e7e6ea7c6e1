"""The proxy loop on captured packets on the device
(qk_u32_snapshot_flows_device, sk.snapshot_flows,
DeviceFlowQuacks.insert_packets(every=True)) against the literal per-packet
loop of packet_snapshot_model.py, bit for bit: the emitted quACKs, their keys
and packet indices in send order, the table after the batch and the statistics.

The shapes are the smallest at which each piece can go wrong: the thresholds
where the walk changes its column passes, frequencies from every packet to
never, batch sizes around a record tile, flow counts on both sides of the key
ranking's and the grouping's switches, a flow that spans three work items of
the walk, a table join of more than one tile with untouched rows, the u32
count wrap, and Resets at every awkward place."""
import ctypes as C

import numpy as np
import pytest

from oracle.quack_oracle import P32
from packet_snapshot_model import META_DT, make_packets, packet_loop, sent_arrays, set_reset, table_arrays
from snapshot_model import base_quack, serialize

gpu = pytest.mark.gpu

MY_ADDR = (10, 0, 2, 1, 0x1F, 0x90)


def flow_keys(nf, seed):
    """nf distinct AddrKeys, none addressed to MY_ADDR."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 256, size=(nf, 12), dtype=np.uint8)
    k[:, 6:10] = (192, 168, 0, 9)
    k[:, 0:4] = (np.arange(nf, dtype=np.uint32)[:, None] >> np.array([24, 16, 8, 0], dtype=np.uint32)) & 0xFF   # distinct
    return k


def random_table(keys, t, seed):
    """{key: quACK} with random sums, counts of random phase and a last value."""
    rng = np.random.default_rng(seed)
    return {k.tobytes(): base_quack(t, count=int(rng.integers(0, 1000)), sums=rng.integers(0, P32, size=t).tolist(),
                                    last=int(rng.integers(0, 1 << 32))) for k in keys}


def clone_table(table):
    return {k: q.clone() for k, q in table.items()}


def u32(x):
    return x.cpu().numpy().view(np.uint32) if x.element_size() == 4 else x.cpu().numpy()


def upload(bufs, meta, table, t, use_meta=True):
    import torch
    d_bufs = torch.from_numpy(np.ascontiguousarray(bufs).reshape(-1)).cuda()
    d_meta = torch.from_numpy(meta.view(np.uint8).copy()).cuda() if use_meta and meta is not None else None
    tk, tr = table_arrays(table, t)
    d_k = torch.from_numpy(tk).cuda() if len(tk) else None
    d_r = torch.from_numpy(tr.view(np.int32)).cuda() if len(tk) else None
    return d_bufs, d_meta, d_k, d_r


def check(bufs, meta, table, t, f, my_addr=MY_ADDR, use_meta=True, stride=67):
    """One batch through the device and through the model; everything equal."""
    import sidekick_amd as sk
    sent, after, stats = packet_loop(clone_table(table), t, f, bufs, meta if use_meta else None, my_addr)
    d_bufs, d_meta, d_k, d_r = upload(bufs, meta, table, t, use_meta)
    s = sk.snapshot_flows(d_bufs, t, f, d_k, d_r, stride=stride, meta=d_meta, my_addr=my_addr)
    rec, keys, index = sent_arrays(sent, t)
    assert s.stats == stats
    assert s.records.shape[0] == len(sent)
    assert np.array_equal(u32(s.index), index)
    assert np.array_equal(u32(s.keys), keys)
    assert np.array_equal(u32(s.records), rec)
    tk, tr = table_arrays(after, t)
    assert np.array_equal(u32(s.table_keys), tk)
    assert np.array_equal(u32(s.table_sketches), tr)
    return s, sent, after, stats


def batch(n, nf, seed, t, table_share=0.5, stride=67):
    """n Inserts spread over nf flows, and a table that holds a share of those
    flows plus a run of flows without traffic in front and behind."""
    rng = np.random.default_rng(seed)
    keys = flow_keys(nf + 8, seed)
    flow = rng.integers(0, nf, size=n)
    ids = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    bufs, meta = make_packets(keys[4:4 + nf], flow, ids, stride=stride, seed=seed)
    held = [k for j, k in enumerate(keys[4:4 + nf]) if j < nf * table_share] + list(keys[:4]) + list(keys[4 + nf:])
    return bufs, meta, random_table(held, t, seed + 1)


# ------------------------------------------------------------ walk and frequency
@gpu
@pytest.mark.parametrize("t", [1, 32, 33, 65])
@pytest.mark.parametrize("f", [1, 2, 7, 1 << 20])
def test_thresholds_and_frequencies(t, f):
    bufs, meta, table = batch(1500, 3, seed=t * 31 + (f & 0xFF), t=t)
    s, sent, after, _ = check(bufs, meta, table, t, f)
    if f == 1 << 20:
        assert len(sent) == 0 and len(after) == len(table) + 1    # no quACK is due, the table is still updated
    if f == 1:
        assert len(sent) == 1500


@gpu
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 5000])
def test_batch_sizes_around_a_record_tile(n):
    bufs, meta, table = batch(n, 3, seed=n + 5, t=4)
    check(bufs, meta, table, 4, 2)


@gpu
@pytest.mark.parametrize("nf,n", [(1, 2000), (3, 2000), (300, 5000), (3000, 20000), (20000, 200000)])
def test_flow_counts(nf, n):
    """1 and 3 flows; ~300; ~3000 (above KR_MAX: the radix key ranking, two
    join tiles); ~20000 flows over 200 000 packets (three-digit grouping)."""
    bufs, meta, table = batch(n, nf, seed=nf, t=4)
    check(bufs, meta, table, 4, 2)


@gpu
@pytest.mark.parametrize("t", [4, 33])
def test_one_long_flow_among_short_ones(t):
    """A flow of 7000 packets spans three SN_ITEM work items (the chain
    kernel), between flows of a few packets each."""
    rng = np.random.default_rng(7)
    keys = flow_keys(40, 3)
    flow = np.concatenate([np.full(7000, 17), rng.integers(0, 40, size=300)])
    rng.shuffle(flow)
    ids = rng.integers(0, 1 << 32, size=len(flow), dtype=np.uint64).astype(np.uint32)
    bufs, meta = make_packets(keys, flow, ids, seed=3)
    check(bufs, meta, random_table(keys[10:30], t, 9), t, 3)


# ------------------------------------------------------------------- table join
@gpu
@pytest.mark.parametrize("empty_table", [False, True])
def test_table_join_spans_tiles_and_copies_untouched_rows(empty_table):
    """A table of 3000 keys; the batch touches 1500 of them and brings 1500 new
    keys, interleaved in key order: 6000 keys through the join, three tiles."""
    t = 4
    keys = flow_keys(4500, 11)               # ascending in their first four bytes
    in_table = keys[np.arange(4500) % 3 != 2]                      # 3000 of them
    touched = np.concatenate([np.nonzero(np.arange(4500) % 3 == 0)[0], np.nonzero(np.arange(4500) % 3 == 2)[0]])
    rng = np.random.default_rng(12)
    flow = np.concatenate([touched, touched[::2]])
    rng.shuffle(flow)
    ids = rng.integers(0, 1 << 32, size=len(flow), dtype=np.uint64).astype(np.uint32)
    bufs, meta = make_packets(keys, flow, ids, seed=13)
    table = {} if empty_table else random_table(in_table, t, 14)
    s, sent, after, _ = check(bufs, meta, table, t, 2)
    assert len(after) == (3000 if empty_table else 4500)
    if not empty_table:
        tk, tr = table_arrays(table, t)
        untouched = {k.tobytes() for k in keys[np.arange(4500) % 3 == 1]}
        got = {bytes(k): r for k, r in zip(u32(s.table_keys), u32(s.table_sketches))}
        for k, r in zip(tk, tr):
            if k.tobytes() in untouched:
                assert np.array_equal(got[k.tobytes()], r)


@gpu
def test_count_wrapping_to_zero_emits():
    keys = flow_keys(1, 1)
    table = {keys[0].tobytes(): base_quack(2, count=(1 << 32) - 3, sums=[5, 6], last=9)}
    bufs, meta = make_packets(keys, [0] * 8, list(range(1, 9)))
    s, sent, _, _ = check(bufs, meta, table, 2, 5)
    assert [q.count for _, _, q in sent] == [(1 << 32) - 1, 0, 5]
    assert u32(s.records)[:, 1].tolist() == [(1 << 32) - 1, 0, 5]


# ----------------------------------------------------------------------- Resets
def reset_batch(n, seed, resets, short=(), filtered=0.0):
    rng = np.random.default_rng(seed)
    keys = flow_keys(5, seed)
    bufs, meta = make_packets(keys, rng.integers(0, 5, size=n), rng.integers(0, 1 << 32, size=n, dtype=np.uint64), seed=seed)
    for i in resets:
        set_reset(bufs, i, MY_ADDR)
    for i in short:
        meta["len"][i] = 40
    kind = rng.integers(0, 4, size=n)
    hit = rng.random(n) < filtered
    meta["pkttype"][hit & (kind == 0)] = 4
    meta["protocol_be"][hit & (kind == 1)] = 0xDD86
    bufs[hit & (kind == 2), 23] = 6
    meta["len"][hit & (kind == 3)] = 40
    return bufs, meta, random_table(keys[:3], 4, seed + 1)


RESETS = {
    "none": dict(resets=()),
    "first": dict(resets=(0,)),
    "last": dict(resets=(599,)),
    "two_in_a_row": dict(resets=(300, 301)),
    "first_and_last": dict(resets=(0, 599)),
    "several": dict(resets=(5, 6, 7, 250, 598)),
    "short_reset": dict(resets=(200,), short=(200,)),
    "filtered_between": dict(resets=(100, 400), filtered=0.3),
}


@gpu
@pytest.mark.parametrize("case", sorted(RESETS))
@pytest.mark.parametrize("f", [1, 3])
def test_resets(case, f):
    bufs, meta, table = reset_batch(600, seed=len(case), **RESETS[case])
    s, sent, after, stats = check(bufs, meta, table, 4, f)
    assert stats["resets"] == len(RESETS[case]["resets"])
    if f == 1:
        assert s.records.shape[0] == stats["inserted"] + stats["discarded"]
    if case == "last":
        assert after == {} and s.table_keys.shape[0] == 0


@gpu
def test_reset_between_two_crossings_of_one_flow():
    keys = flow_keys(1, 2)
    bufs, meta = make_packets(keys, [0] * 6, [1, 2, 3, 0, 4, 5])
    set_reset(bufs, 3, MY_ADDR)
    s, sent, after, stats = check(bufs, meta, {}, 4, 2)
    assert u32(s.records).tolist() == [[4, 2, 1, 2, 3, 5, 9, 17], [4, 2, 1, 5, 9, 41, 189, 881]]
    assert u32(s.index).tolist() == [1, 5] and stats["discarded"] == 3
    assert u32(s.table_sketches).tolist() == [[4, 2, 1, 5, 9, 41, 189, 881]]


@gpu
def test_no_own_address_means_no_reset():
    bufs, meta, table = reset_batch(600, seed=3, resets=(100,))
    _, _, _, stats = check(bufs, meta, table, 4, 2, my_addr=None)
    assert stats["resets"] == 0


# -------------------------------------------------------------- strides and meta
@gpu
@pytest.mark.parametrize("stride", [67, 96])
@pytest.mark.parametrize("use_meta", [False, True])
def test_strides_and_meta(stride, use_meta):
    bufs, meta, table = batch(1025, 7, seed=stride, t=4, stride=stride)
    set_reset(bufs, 500, MY_ADDR)
    if use_meta:
        meta["pkttype"][::17] = 4
        meta["len"][5::29] = 40
    check(bufs, meta, table, 4, 2, use_meta=use_meta, stride=stride)


# ------------------------------------------------- against what the library has
@gpu
def test_final_table_equals_the_end_of_batch_path():
    import sidekick_amd as sk
    import torch
    bufs, meta, _ = batch(5000, 300, seed=21, t=8)
    d_bufs = torch.from_numpy(bufs.reshape(-1)).cuda()
    first, second = d_bufs[:2500 * 67], d_bufs[2500 * 67:]
    a, b = sk.DeviceFlowQuacks(8), sk.DeviceFlowQuacks(8)
    for part in (first, second):
        a.insert_packets(part, my_addr=MY_ADDR, frequency_pkts=4)
        b.insert_packets(part, my_addr=MY_ADDR, frequency_pkts=4, every=True)
        assert torch.equal(a.keys, b.keys) and torch.equal(a.sketches, b.sketches)


@gpu
def test_snapshot_stream_equals_device_flow_snapshots():
    """DeviceFlowSnapshots.insert fed the same packets, the flows numbered by key rank."""
    import sidekick_amd as sk
    import torch
    t, f, nf = 8, 3, 50
    rng = np.random.default_rng(5)
    keys = flow_keys(nf, 5)                  # ascending: flow j has key rank j
    flow = rng.integers(0, nf, size=4000)
    ids = rng.integers(0, 1 << 32, size=4000, dtype=np.uint64).astype(np.uint32)
    bufs, _ = make_packets(keys, flow, ids, seed=5)
    s = sk.snapshot_flows(torch.from_numpy(bufs.reshape(-1)).cuda(), t, f, my_addr=MY_ADDR)
    ref = sk.DeviceFlowSnapshots(t, nf, f)
    seg, wire, lens, recs = ref.insert(flow.astype(np.uint32), ids)
    assert torch.equal(recs, s.records)
    rank = {k.tobytes(): j for j, k in enumerate(keys)}
    assert [rank[bytes(k)] for k in u32(s.keys)] == seg.cpu().tolist()
    assert torch.equal(s.table_sketches, ref.records)


# ----------------------------------------------------------------------- errors
def raw(ctx, d_bufs, n, t, f, d_k, d_r, nt, ko, so, tcap, rec, sk_, si, scap, stride=67):
    from sidekick_amd._lib import lib
    from sidekick_amd.quack import PktStats
    ntab, m, st = C.c_size_t(), C.c_size_t(), PktStats()
    p = lambda x: x.data_ptr() if hasattr(x, "data_ptr") else x   # noqa: E731
    rc = lib().qk_u32_snapshot_flows_device(ctx.handle, p(d_bufs), n, stride, None, (C.c_uint8 * 6)(*MY_ADDR), t, f,
                                            p(d_k), p(d_r), nt, p(ko), p(so), tcap, C.byref(ntab), p(rec), p(sk_), p(si),
                                            scap, C.byref(m), C.byref(st), None)
    return rc, ntab.value, m.value, st


@gpu
def test_errors_and_capacity():
    import sidekick_amd as sk
    import torch
    from sidekick_amd._lib import QK_E_CAPACITY, QK_E_INVAL, QK_E_MISMATCH, QK_E_THRESHOLD
    t, f, n = 4, 2, 600
    bufs, meta, table = reset_batch(n, seed=8, resets=(250,))
    quiet, qmeta, _ = reset_batch(n, seed=8, resets=())
    ctx = sk.get_context(0)
    d_bufs, _, d_k, d_r = upload(bufs, meta, table, t, use_meta=False)
    d_quiet = torch.from_numpy(quiet.reshape(-1)).cuda()
    nt = d_k.shape[0]
    dev = d_bufs.device
    out = lambda rows, cols, dt: torch.full((rows, cols), -1, dtype=dt, device=dev)   # noqa: E731
    ko, so, rec, sk_, si = out(64, 12, torch.uint8), out(64, 8, torch.int32), out(n, 8, torch.int32), \
        out(n, 12, torch.uint8), out(n, 1, torch.int32)
    torch.cuda.synchronize()
    full = raw(ctx, d_bufs, n, t, f, d_k, d_r, nt, ko, so, 64, rec, sk_, si, n)
    assert full[0] == 0
    want = (ko.clone(), so.clone(), rec.clone(), sk_.clone(), si.clone())
    sent, after, stats = packet_loop(clone_table(table), t, f, bufs, None, MY_ADDR)
    assert (full[1], full[2]) == (len(after), len(sent)) and np.array_equal(u32(rec)[:len(sent)], sent_arrays(sent, t)[0])
    # each cap too small, with and without a Reset in the batch: the sizes and the statistics, nothing written
    for b in (d_bufs, d_quiet):
        ok = raw(ctx, b, n, t, f, d_k, d_r, nt, ko, so, 64, rec, sk_, si, n)
        assert ok[0] == 0
        keep = (ko.clone(), so.clone(), rec.clone(), sk_.clone(), si.clone())
        for tcap, scap in ((ok[1] - 1, n), (64, ok[2] - 1), (0, 0)):
            for x in (ko, so, rec, sk_, si):
                x.fill_(-1)
            rc, ntab, m, st = raw(ctx, b, n, t, f, d_k, d_r, nt, ko, so, tcap, rec, sk_, si, scap)
            torch.cuda.synchronize()
            assert rc == QK_E_CAPACITY and (ntab, m) == (ok[1], ok[2])
            assert (st.inserted, st.discarded, st.resets) == (ok[3].inserted, ok[3].discarded, ok[3].resets)
            assert all(bool((x == (255 if x.dtype == torch.uint8 else -1)).all()) for x in (ko, so, rec, sk_, si))
        # the repeat with the reported sizes gives the same result
        rc, ntab, m, _ = raw(ctx, b, n, t, f, d_k, d_r, nt, ko, so, ok[1], rec, sk_, si, ok[2])
        assert rc == 0 and (ntab, m) == (ok[1], ok[2])
        for x, y, rows in zip((ko, so, rec, sk_, si), keep, (ntab, ntab, m, m, m)):
            assert torch.equal(x[:rows], y[:rows])
    call = lambda **kw: raw(**{**dict(ctx=ctx, d_bufs=d_bufs, n=n, t=t, f=f, d_k=d_k, d_r=d_r, nt=nt, ko=ko, so=so, tcap=64,   # noqa: E731
                                      rec=rec, sk_=sk_, si=si, scap=n), **kw})[0]
    assert call(f=0) == QK_E_INVAL
    assert call(t=0) == QK_E_THRESHOLD and call(t=1025) == QK_E_THRESHOLD
    assert call(stride=66) == QK_E_INVAL and call(stride=513) == QK_E_INVAL
    # input keys out of order (found on the device), with and without traffic for them
    swapped = d_k.clone()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert call(d_k=swapped) == QK_E_INVAL
    assert call(d_k=swapped, n=0) == QK_E_INVAL
    dup = d_k.clone()
    dup[1] = dup[0]
    assert call(d_k=dup) == QK_E_INVAL
    # a table record of another threshold
    other = d_r.clone()
    other[nt - 1, 0] = t + 1
    assert call(d_r=other) == QK_E_MISMATCH
    # outputs overlapping an input or each other
    assert call(so=d_r) == QK_E_INVAL and call(ko=d_k) == QK_E_INVAL
    assert call(rec=so) == QK_E_INVAL and call(sk_=ko) == QK_E_INVAL
    assert call(si=d_bufs[:4 * n].view(torch.int32)) == QK_E_INVAL
    # a host pointer where a device pointer is required, a misaligned array
    host = np.zeros(n * 8, dtype=np.int32)
    assert call(rec=host.ctypes.data) == QK_E_INVAL
    assert call(d_bufs=bufs.ctypes.data) == QK_E_INVAL
    assert call(d_k=table_arrays(table, t)[0].ctypes.data) == QK_E_INVAL
    odd = torch.empty(n * 32 + 8, dtype=torch.uint8, device=dev)
    assert call(rec=odd.data_ptr() + 2) == QK_E_INVAL
    # and after all that the call still answers as before
    rc, ntab, m, _ = raw(ctx, d_bufs, n, t, f, d_k, d_r, nt, ko, so, 64, rec, sk_, si, n)
    assert rc == 0 and (ntab, m) == (full[1], full[2])
    for x, y, rows in zip((ko, so, rec, sk_, si), want, (ntab, ntab, m, m, m)):
        assert torch.equal(x[:rows], y[:rows])


@gpu
def test_wrapper_retries_on_capacity():
    import sidekick_amd as sk
    import torch
    bufs, meta, table = batch(3000, 2000, seed=4, t=4, table_share=0.0)
    sent, after, stats = packet_loop(clone_table(table), 4, 1, bufs, None, MY_ADDR)
    d_bufs, _, d_k, d_r = upload(bufs, meta, table, 4, use_meta=False)
    s = sk.snapshot_flows(d_bufs, 4, 1, d_k, d_r, my_addr=MY_ADDR, snap_cap=10)     # both caps too small at first
    assert s.records.shape[0] == 3000 and np.array_equal(u32(s.records), sent_arrays(sent, 4)[0])
    assert np.array_equal(u32(s.table_sketches), table_arrays(after, 4)[1])


# ------------------------------------------------ DeviceFlowQuacks(every=True)
@gpu
def test_insert_packets_every_wire_images_over_two_batches():
    import sidekick_amd as sk
    import torch
    t, f = 4, 3
    one, meta1, _ = reset_batch(700, seed=30, resets=())
    two, meta2, _ = reset_batch(700, seed=31, resets=(350,), filtered=0.1)
    table = sk.DeviceFlowQuacks(t)
    model, images, got = {}, [], []
    for bufs, meta in ((one, meta1), (two, meta2)):
        sent, model, stats = packet_loop(model, t, f, bufs, meta, MY_ADDR)
        images += [serialize(q) for _, _, q in sent]
        st = table.insert_packets(torch.from_numpy(bufs.reshape(-1)).cuda(),
                                  meta=torch.from_numpy(meta.view(np.uint8).copy()).cuda(), my_addr=MY_ADDR,
                                  frequency_pkts=f, every=True)
        keys, index, wire, lens, records = st["wire"]
        assert {k: st[k] for k in stats} == stats and st["due"] == []
        assert u32(index).tolist() == [i for i, _, _ in sent]
        assert [bytes(k) for k in u32(keys)] == [k for _, k, _ in sent]
        w, ln = wire.cpu().numpy(), lens.cpu().tolist()
        got += [w[r, :ln[r]].tobytes() for r in range(len(ln))]
        tk, tr = table_arrays(model, t)
        assert np.array_equal(u32(table.keys), tk) and np.array_equal(u32(table.sketches), tr)
    assert got == images and len(images) > 300
