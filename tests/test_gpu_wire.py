"""Device wire leg on the GPU (qk_u32_flows_emit_device,
qk_u32_wire_ingest_device, emit_wire / ingest_wire).  Expected images come from
a literal packer of the bincode layout (struct.pack), cross-checked against the
host qk_u32_serialize; expected statuses from the host qk_u32_deserialize on
the same bytes.  Nothing is derived from the code under test."""
import ctypes as C
import struct

import numpy as np
import pytest

import sidekick_amd as sk
from sidekick_amd._lib import (P32, QK_E_CAPACITY, QK_E_FORMAT, QK_E_INVAL, QK_E_MISMATCH, QK_E_THRESHOLD,
                               QK_WIRE_SUPERSEDED, lib)
from sidekick_amd.quack import _quack_from_bytes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 64


def pack(threshold, sums, tag, last, count, with_last=None):
    """The layout, literally: u64 threshold | u32 sums | u8 tag | u32 last (tag 1) | u32 count."""
    with_last = bool(tag) if with_last is None else with_last
    out = struct.pack("<Q", threshold) + b"".join(struct.pack("<I", s) for s in sums) + struct.pack("<B", tag)
    if with_last:
        out += struct.pack("<I", last)
    return out + struct.pack("<I", count)


def records(t, n, seed):
    """n qk_u32 records [n, 4 + t]: has_last 0 and 1, counts 0 and 2^32 - 1, sums 0 and p - 1 among random ones."""
    rng = np.random.default_rng(seed)
    r = np.zeros((n, 4 + t), dtype=np.uint32)
    r[:, 0] = t
    r[:, 1] = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    r[:, 2] = rng.integers(0, 2, size=n)
    r[:, 3] = rng.integers(0, 1 << 32, size=n, dtype=np.uint64) * r[:, 2]
    r[:, 4:] = rng.integers(0, P32, size=(n, t), dtype=np.uint64)
    if n:
        r[0::5, 1] = 0
        r[1::5, 1] = 0xFFFFFFFF
        r[0::3, 4] = 0
        r[1::3, 4 + t - 1] = P32 - 1
        r[2::7, 4:] = P32 - 1
        r[3::7, 4:] = 0
    return r


def image(rec):
    t = int(rec[0])
    return pack(t, rec[4:].tolist(), int(rec[2]), int(rec[3]), int(rec[1]))


def keys_for(n, seed=3):
    k = np.random.default_rng(seed).integers(0, 256, size=(n, 12), dtype=np.uint8)
    return k


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


class Emit:
    """One raw emit call into a guarded buffer: GUARD bytes of 0xA5 before the
    first slot and after the last, the first slot `off` bytes past a 256-byte
    boundary."""

    def __init__(self, recs, t, select=None, stride=None, off=0, cap=None, keys=True, rows=True):
        self.ctx = sk.get_context(0)
        n = recs.shape[0]
        self.n, self.t, self.recs = n, t, recs
        self.stride = sk.wire_max(t) if stride is None else stride
        self.cap = n if cap is None else cap
        self.d_recs = dev(recs) if n else torch.empty((0, 4 + t), dtype=torch.int32, device="cuda")
        self.keys = keys_for(n)
        self.d_keys = dev(self.keys) if keys else None
        self.d_sel = None if select is None else dev(np.asarray(select, dtype=np.uint8))
        self.off = off
        self.buf = torch.full((GUARD + off + self.cap * self.stride + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.keys_out = torch.full((max(self.cap, 1), 12), 0x5A, dtype=torch.uint8, device="cuda") if keys else None
        self.rows = torch.full((max(self.cap, 1),), -5, dtype=torch.int32, device="cuda") if rows else None
        self.lens = torch.full((max(self.cap, 1),), -6, dtype=torch.int32, device="cuda")
        self.m = C.c_size_t(12345)

    def call(self, **kw):
        a = dict(keys=self.d_keys.data_ptr() if self.d_keys is not None and self.n else None,
                 sk=self.d_recs.data_ptr() if self.n else None, n=self.n, t=self.t,
                 select=self.d_sel.data_ptr() if self.d_sel is not None and self.n else None, stride=self.stride,
                 keys_out=self.keys_out.data_ptr() if self.keys_out is not None else None,
                 rows=self.rows.data_ptr() if self.rows is not None else None,
                 wire=self.buf.data_ptr() + GUARD + self.off, lens=self.lens.data_ptr(), cap=self.cap)
        a.update(kw)
        return lib().qk_u32_flows_emit_device(self.ctx.handle, a["keys"], a["sk"], a["n"], a["t"], a["select"],
                                              a["stride"], a["keys_out"], a["rows"], a["wire"], a["lens"], a["cap"],
                                              C.byref(self.m), None)

    def untouched(self):
        torch.cuda.synchronize()
        ok = bool((self.buf == 0xA5).all()) and bool((self.lens == -6).all())
        if self.rows is not None:
            ok = ok and bool((self.rows == -5).all())
        if self.keys_out is not None:
            ok = ok and bool((self.keys_out == 0x5A).all())
        return ok

    def check(self, serialize_sample=64):
        """Everything the call wrote against the packer: images, lengths, rows, keys, guards."""
        want_rows = np.arange(self.n) if self.d_sel is None else np.flatnonzero(self.d_sel.cpu().numpy())
        m = self.m.value
        assert m == len(want_rows)
        host = self.buf.cpu().numpy()
        lo, hi = GUARD + self.off, GUARD + self.off + m * self.stride
        assert (host[:lo] == 0xA5).all() and (host[hi:] == 0xA5).all(), "guard bytes"
        slots = host[lo:hi].reshape(m, self.stride) if m else np.zeros((0, self.stride), dtype=np.uint8)
        lens = self.lens.cpu().numpy()[:m]
        if self.rows is not None:
            assert np.array_equal(self.rows.cpu().numpy()[:m], want_rows)
        if self.keys_out is not None:
            assert np.array_equal(self.keys_out.cpu().numpy()[:m], self.keys[want_rows])
        # the packer's images side by side, compared in one go
        want = np.zeros((m, self.stride), dtype=np.uint8)
        want_len = np.zeros(m, dtype=np.int32)
        for r, i in enumerate(want_rows.tolist()):
            img = image(self.recs[i])
            want_len[r] = len(img)
            want[r, :len(img)] = np.frombuffer(img, dtype=np.uint8)
        assert np.array_equal(lens, want_len)
        inside = np.arange(self.stride)[None, :] < want_len[:, None]
        assert np.array_equal(slots[inside], want[inside]), "image bytes"
        # the packer itself against the host serializer
        step = max(1, m // serialize_sample)
        for r in range(0, m, step):
            q = _quack_from_bytes(self.recs[want_rows[r]].tobytes(), self.t)
            assert q.serialize() == slots[r, :lens[r]].tobytes()
        return slots, lens


# -------------------------------------------------------------------- emit
@pytest.mark.parametrize("layout", ("dense", "pad16", "offset1"))
@pytest.mark.parametrize("t", (1, 7, 32, 1024))
def test_emit_images_equal_the_packer(t, layout):
    n = 37 if t == 1024 else 301
    stride = sk.wire_max(t)
    assert stride % 2 == 1
    if layout == "pad16":
        stride = (stride + 15) // 16 * 16
    e = Emit(records(t, n, t), t, stride=stride, off=1 if layout == "offset1" else 0)
    assert e.call() == 0
    _, lens = e.check(serialize_sample=n)
    assert set(lens.tolist()) == {4 * t + 13, 4 * t + 17}


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 2048, 2049, 70_001))
def test_emit_sizes_at_wave_tile_and_multi_tile_boundaries(n):
    rng = np.random.default_rng(n)
    recs = records(2, n, n + 1)
    for select in (None, rng.random(n) < 0.5):
        e = Emit(recs, 2, select=select, off=1)
        assert e.call() == 0
        e.check()


@pytest.mark.parametrize("which", ("none", "zeros", "ones", "tenth", "last", "first"))
def test_emit_selections(which):
    n = 5000
    rng = np.random.default_rng(8)
    sel = {"none": None, "zeros": np.zeros(n), "ones": np.ones(n), "tenth": rng.random(n) < 0.1,
           "last": np.arange(n) == n - 1, "first": np.arange(n) == 0}[which]
    if which == "tenth":
        sel = sel * 7          # any non-zero byte selects
    e = Emit(records(7, n, 5), 7, select=sel)
    assert e.call() == 0
    e.check()
    assert e.m.value == {"none": n, "zeros": 0, "ones": n, "last": 1, "first": 1}.get(which, e.m.value)


def test_emit_without_keys_and_rows():
    rng = np.random.default_rng(2)
    e = Emit(records(7, 300, 6), 7, select=rng.random(300) < 0.3, keys=False, rows=False)
    assert e.call() == 0
    e.check()


def test_emit_capacity_then_success():
    n = 3000
    sel = np.random.default_rng(4).random(n) < 0.4
    m = int(sel.sum())
    for select, want in ((sel, m), (None, n)):
        e = Emit(records(2, n, 9), 2, select=select, cap=want - 1)
        assert e.call() == QK_E_CAPACITY and e.m.value == want
        assert e.untouched()
        e = Emit(records(2, n, 9), 2, select=select, cap=want)
        assert e.call() == 0 and e.m.value == want
        e.check()


def test_emit_threshold_mismatch_only_when_selected():
    recs = records(7, 200, 1)
    recs[150, 0] = 8
    sel = np.ones(200)
    assert Emit(recs, 7, select=sel).call() == QK_E_MISMATCH
    assert Emit(recs, 7).call() == QK_E_MISMATCH
    sel[150] = 0
    e = Emit(recs, 7, select=sel)
    assert e.call() == 0
    e.check()


def test_emit_argument_errors():
    recs = records(7, 100, 1)
    e = Emit(recs, 7, select=np.ones(100))
    wm = sk.wire_max(7)
    assert e.call(t=0) == QK_E_THRESHOLD and e.call(t=1025) == QK_E_THRESHOLD
    assert e.call(stride=wm - 1) == QK_E_INVAL
    assert e.call(n=1 << 32) == QK_E_INVAL
    h = np.zeros(100 * wm, dtype=np.uint8)
    assert e.call(sk=h.ctypes.data) == QK_E_INVAL                    # host pointers
    assert e.call(select=h.ctypes.data) == QK_E_INVAL
    assert e.call(wire=h.ctypes.data) == QK_E_INVAL
    assert e.call(lens=h.ctypes.data) == QK_E_INVAL
    assert e.call(rows=h.ctypes.data) == QK_E_INVAL
    assert e.call(keys_out=h.ctypes.data) == QK_E_INVAL
    assert e.call(keys=h.ctypes.data) == QK_E_INVAL
    assert e.call(lens=e.lens.data_ptr() + 2) == QK_E_INVAL          # misaligned words
    assert e.call(wire=e.d_recs.data_ptr() + 40) == QK_E_INVAL       # output inside an input
    assert e.call(lens=e.d_sel.data_ptr()) == QK_E_INVAL
    assert e.call(rows=e.lens.data_ptr()) == QK_E_INVAL              # two outputs on one range
    assert e.call(wire=e.keys_out.data_ptr()) == QK_E_INVAL
    assert e.untouched()
    assert e.call() == 0
    e.check()


def test_emit_twice_gives_equal_bytes_and_wrapper_shapes():
    recs = records(32, 700, 3)
    sel = np.random.default_rng(6).random(700) < 0.5
    a, b = Emit(recs, 32, select=sel, off=1), Emit(recs, 32, select=sel, off=1)
    assert a.call() == 0 and b.call() == 0
    sa, la = a.check()
    sb, lb = b.check()
    assert np.array_equal(la, lb)
    inside = np.arange(a.stride)[None, :] < la[:, None]
    assert np.array_equal(sa[inside], sb[inside])
    # the wrapper: same images as views of CUDA tensors
    keys, rows, wire, lens = sk.emit_wire(a.d_keys, a.d_recs, a.d_sel.bool())
    assert wire.shape == (a.m.value, sk.wire_max(32)) and wire.dtype == torch.uint8 and wire.is_cuda
    assert np.array_equal(lens.cpu().numpy(), la) and np.array_equal(rows.cpu().numpy(), np.flatnonzero(sel))
    assert np.array_equal(keys.cpu().numpy(), a.keys[sel])
    assert np.array_equal(wire.cpu().numpy()[inside], sa[inside])
    k2, r2, w2, l2 = sk.emit_wire(None, a.d_recs, stride=160)
    assert k2 is None and w2.shape == (700, 160) and r2.tolist() == list(range(700))


# ------------------------------------------------------------------ ingest
SENTINEL = 0x5EED5EED


def host_status(data, t):
    """qk_u32_deserialize of these bytes into a sketch initialised for t."""
    q = sk.PowerSumQuackU32(t)
    src = (C.c_uint8 * max(len(data), 1))()
    C.memmove(src, data, len(data))
    return lib().qk_u32_deserialize(src, len(data), q._buf, None), q


class Ingest:
    """One raw ingest call: datagram i at `stride` bytes from datagram i - 1, the
    buffer ending with the last datagram's last byte, its start `off` bytes past
    a 256-byte boundary; d_peer pre-filled with a sentinel, d_present with 9."""

    def __init__(self, images, lens, flows, t, nseg, stride=None, off=0):
        self.ctx = sk.get_context(0)
        n = len(images)
        self.n, self.t, self.nseg = n, t, nseg
        self.stride = stride if stride is not None else max([len(b) for b in images] + [1])
        size = (n - 1) * self.stride + len(images[-1]) if n else 0
        host = np.full(off + max(size, 1), 0xEE, dtype=np.uint8)
        for i, b in enumerate(images):
            assert len(b) <= self.stride
            host[off + i * self.stride: off + i * self.stride + len(b)] = np.frombuffer(b, dtype=np.uint8)
        self.buf = torch.from_numpy(host).cuda()
        assert self.buf.data_ptr() % 256 == 0
        self.wire = self.buf.data_ptr() + off
        self.d_len = dev(np.asarray(lens, dtype=np.uint32)) if n else None
        self.d_flow = dev(np.asarray(flows, dtype=np.uint32)) if n else None
        self.peer = torch.full((max(nseg, 1), 4 + t), SENTINEL, dtype=torch.int32, device="cuda")
        self.present = torch.full((max(nseg, 1),), 9, dtype=torch.uint8, device="cuda")
        self.status = np.full(max(n, 1), 99, dtype=np.int32)
        self.acc = C.c_size_t(4242)

    def call(self, **kw):
        a = dict(wire=self.wire if self.n else None, stride=self.stride,
                 len=self.d_len.data_ptr() if self.n else None, flow=self.d_flow.data_ptr() if self.n else None,
                 n=self.n, t=self.t, nseg=self.nseg, peer=self.peer.data_ptr(), present=self.present.data_ptr(),
                 status=self.status.ctypes.data_as(C.POINTER(C.c_int32)))
        a.update(kw)
        return lib().qk_u32_wire_ingest_device(self.ctx.handle, a["wire"], a["stride"], a["len"], a["flow"], a["n"],
                                               a["t"], a["nseg"], a["peer"], a["present"], a["status"],
                                               C.byref(self.acc), None)

    def rows(self):
        torch.cuda.synchronize()
        return self.peer.cpu().numpy().view(np.uint32), self.present.cpu().numpy()


def test_round_trip_of_a_random_selection():
    t, n = 32, 3001
    recs = records(t, n, 11)
    sel = np.random.default_rng(12).random(n) < 0.3
    d_recs = dev(recs)
    _, rows, wire, lens = sk.emit_wire(None, d_recs, dev(sel.astype(np.uint8)))
    peer = torch.full((n, 4 + t), SENTINEL, dtype=torch.int32, device="cuda")
    peer2, present, status, acc = sk.ingest_wire(wire, lens, rows, n, t, peer=peer)
    assert peer2 is peer and acc == int(sel.sum()) and (status == 0).all() and len(status) == acc
    got = peer.cpu().numpy().view(np.uint32)
    assert np.array_equal(present.cpu().numpy(), sel.astype(np.uint8))
    assert np.array_equal(got[sel], recs[sel])
    assert (got[~sel] == SENTINEL).all()
    # a fresh peer: the rows of flows without a datagram are empty quACKs
    fresh, present, _, _ = sk.ingest_wire(wire, lens, rows, n, t)
    got = fresh.cpu().numpy().view(np.uint32)
    empty = np.frombuffer(sk.PowerSumQuackU32(t)._buf, dtype=np.uint32)
    assert np.array_equal(got[sel], recs[sel]) and (got[~sel] == empty).all()


def table_images(t):
    """(what, bytes in the slot, claimed length) of the per-image table."""
    rng = np.random.default_rng(t)
    ok = rng.integers(0, P32, size=t, dtype=np.uint64).tolist()
    v1, v0 = pack(t, ok, 1, 0xDEADBEEF, 7), pack(t, ok, 0, 0, 0xFFFFFFFF)
    out = [("valid tag 1", v1), ("valid tag 0", v0), ("len 0", b""), ("len 7", v1[:7]), ("len 8", v1[:8]),
           ("len 4t + 12", v0[:4 * t + 12]), ("tag 2", pack(t, ok, 2, 5, 6, True)),
           ("tag 0 at the tag-1 length", pack(t, ok, 0, 5, 6, True)),
           ("tag 1 at the tag-0 length", pack(t, ok, 1, 5, 6, False)),
           ("trailing byte", v1 + b"\0"), ("trailing byte, tag 0", v0 + b"\0"),
           ("threshold t + 1", pack(t + 1, [3] * (t + 1), 1, 5, 6)),
           ("threshold t - 1", pack(t - 1, [3] * (t - 1), 0, 0, 6)),
           ("threshold 2^32 - 1", pack((1 << 32) - 1, ok, 1, 5, 6)),
           ("threshold 2^32", pack(1 << 32, ok, 1, 5, 6)),
           ("sum == p", pack(t, ok[:-1] + [P32], 1, 5, 6)),
           ("sum == 2^32 - 1", pack(t, [0xFFFFFFFF] + ok[1:], 0, 0, 6)),
           ("sums == p - 1", pack(t, [P32 - 1] * t, 1, 5, 6)),
           ("threshold 2^63", pack(1 << 63, ok, 1, 5, 6))]        # last: the buffer ends with its last byte
    return out


@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("t", (1, 32))
def test_ingest_statuses_equal_the_host_deserializer(t, off):
    tab = table_images(t)
    images = [b for _, b in tab]
    n = len(images)
    stride = max(len(b) for b in images) | 1          # odd
    g = Ingest(images, [len(b) for b in images], list(range(n)), t, n, stride=stride, off=off)
    assert g.call() == 0
    peer, present = g.rows()
    n_ok = 0
    for i, (what, b) in enumerate(tab):
        want, q = host_status(b, t)
        assert g.status[i] == want, (what, g.status[i], want)
        if want == 0:
            n_ok += 1
            assert present[i] == 1 and np.array_equal(peer[i], np.frombuffer(q._buf, dtype=np.uint32)), what
        else:
            assert present[i] == 0 and (peer[i] == SENTINEL).all(), what
    assert n_ok == 3 and g.acc.value == 3
    codes = [int(s) for s in g.status[:n]]
    assert codes.count(QK_E_MISMATCH) == 2 and codes.count(QK_E_FORMAT) == n - 5


def test_ingest_length_beyond_the_stride_is_malformed():
    t = 7
    v1 = pack(t, [5] * t, 1, 9, 3)
    g = Ingest([v1, v1, v1], [len(v1), len(v1), len(v1) + 1], [0, 1, 2], t, 3, stride=len(v1))
    assert g.call() == 0 and g.status[:3].tolist() == [0, 0, QK_E_FORMAT] and g.acc.value == 2
    # at stride 20 every claimed length exceeds its slot, whatever the bytes hold
    assert g.call(stride=20) == 0 and g.status[:3].tolist() == [QK_E_FORMAT] * 3 and g.acc.value == 0


def test_ingest_duplicates_last_accepted_wins():
    t = 7
    a, b = pack(t, [1] * t, 1, 11, 1), pack(t, [2] * t, 1, 22, 2)
    bad = b[:-1]
    other = pack(t, [3] * t, 0, 0, 3)
    g = Ingest([a, other, b, bad], [len(a), len(other), len(b), len(bad)], [1, 0, 1, 1], t, 2)
    assert g.call() == 0
    assert g.status[:4].tolist() == [QK_WIRE_SUPERSEDED, 0, 0, QK_E_FORMAT] and g.acc.value == 2
    peer, present = g.rows()
    assert present.tolist() == [1, 1]
    assert np.array_equal(peer[1], np.frombuffer(host_status(b, t)[1]._buf, dtype=np.uint32))
    assert np.array_equal(peer[0], np.frombuffer(host_status(other, t)[1]._buf, dtype=np.uint32))


def test_ingest_ten_thousand_datagrams_of_one_flow():
    t, n = 2, 10_000
    images = [pack(t, [i, i + 1], 1, i, i) for i in range(n)]
    g = Ingest(images, [len(b) for b in images], [0] * n, t, 3)
    assert g.call() == 0 and g.acc.value == 1
    assert (g.status[:n - 1] == QK_WIRE_SUPERSEDED).all() and g.status[n - 1] == 0
    peer, present = g.rows()
    assert present[:3].tolist() == [1, 0, 0]
    assert peer[0].tolist() == [t, n - 1, 1, n - 1, n - 1, n] and (peer[1:] == SENTINEL).all()


def test_ingest_flow_index_out_of_range_writes_nothing():
    t, n, nseg = 2, 5000, 40
    rng = np.random.default_rng(5)
    images = [pack(t, [i, 7], 0, 0, i) for i in range(n)]
    flows = rng.integers(0, nseg, size=n)
    flows[3210] = nseg
    g = Ingest(images, [len(b) for b in images], flows, t, nseg)
    assert g.call() == QK_E_INVAL
    peer, present = g.rows()
    assert (peer == SENTINEL).all() and (present == 9).all()
    flows[3210] = 0xFFFFFFFF
    g = Ingest(images, [len(b) for b in images], flows, t, nseg)
    assert g.call() == QK_E_INVAL
    peer, present = g.rows()
    assert (peer == SENTINEL).all() and (present == 9).all()


@pytest.mark.parametrize("n", (2047, 2048, 2049))
def test_ingest_sizes_and_odd_stride_off_by_one_base(n):
    t, nseg = 7, 300
    rng = np.random.default_rng(n)
    recs = records(t, n, n)
    images = [image(r) for r in recs]
    for i in range(0, n, 17):
        images[i] = images[i][:-2]                     # malformed now and then
    flows = rng.integers(0, nseg, size=n)
    g = Ingest(images, [len(b) for b in images], flows, t, nseg, stride=sk.wire_max(t) + 2, off=1)
    assert g.stride % 2 == 1 and g.call() == 0
    want_status = np.array([host_status(b, t)[0] for b in images])
    winner = {}
    for i in range(n):
        if want_status[i] == 0:
            winner[int(flows[i])] = i
    for i in range(n):
        if want_status[i] == 0 and winner[int(flows[i])] != i:
            want_status[i] = QK_WIRE_SUPERSEDED
    assert np.array_equal(g.status[:n], want_status) and g.acc.value == len(winner)
    peer, present = g.rows()
    for f in range(nseg):
        if f in winner:
            assert present[f] == 1 and np.array_equal(peer[f], recs[winner[f]]), f
        else:
            assert present[f] == 0 and (peer[f] == SENTINEL).all(), f


def test_ingest_empty_batch_no_flows_and_argument_errors():
    t = 7
    v = pack(t, [5] * t, 1, 9, 3)
    g = Ingest([], [], [], t, 5, stride=64)
    assert g.call() == 0 and g.acc.value == 0
    peer, present = g.rows()
    assert (present == 0).all() and (peer == SENTINEL).all()
    g = Ingest([v, v], [len(v)] * 2, [0, 1], t, 2)
    assert g.call(nseg=0) == QK_E_INVAL
    assert g.call(stride=0) == QK_E_INVAL
    assert g.call(t=0) == QK_E_THRESHOLD and g.call(t=1025) == QK_E_THRESHOLD
    assert g.call(n=1 << 32) == QK_E_INVAL and g.call(nseg=1 << 32) == QK_E_INVAL
    h = np.zeros(4096, dtype=np.uint8)
    assert g.call(wire=h.ctypes.data) == QK_E_INVAL                               # host pointers
    assert g.call(len=h.ctypes.data) == QK_E_INVAL
    assert g.call(flow=h.ctypes.data) == QK_E_INVAL
    assert g.call(peer=h.ctypes.data) == QK_E_INVAL
    assert g.call(present=h.ctypes.data) == QK_E_INVAL
    d_status = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert g.call(status=C.cast(d_status.data_ptr(), C.POINTER(C.c_int32))) == QK_E_INVAL   # a device status
    assert g.call(peer=g.peer.data_ptr() + 2) == QK_E_INVAL                       # misaligned words
    assert g.call(present=g.wire + 3) == QK_E_INVAL                               # output inside an input
    assert g.call(peer=g.d_flow.data_ptr()) == QK_E_INVAL
    assert g.call(present=g.peer.data_ptr() + 8) == QK_E_INVAL                    # the outputs on one range
    peer, present = g.rows()
    assert (peer == SENTINEL).all() and (present == 9).all()
    assert g.call() == 0 and g.status[:2].tolist() == [0, 0]


# ------------------------------------------------------- the table's surface
META_DT = np.dtype([("pkttype", "u1"), ("reserved", "u1"), ("protocol_be", "<u2"), ("len", "<u4")])


def packet_batch(flows, f, ids, seed=0):
    """One full-length incoming UDP record per entry: AddrKey flows[f[i]], identifier ids[i]."""
    rng = np.random.default_rng(seed)
    n = len(f)
    bufs = rng.integers(0, 256, size=(n, 67), dtype=np.uint8)
    bufs[:, 23] = 17
    key = flows[f]
    bufs[:, 26:30], bufs[:, 34:36], bufs[:, 30:34], bufs[:, 36:38] = key[:, 0:4], key[:, 4:6], key[:, 6:10], key[:, 10:12]
    ids = np.asarray(ids, dtype=np.uint32)
    for b in range(4):
        bufs[:, 63 + b] = (ids >> (24 - 8 * b)) & 0xFF
    meta = np.zeros(n, dtype=META_DT)
    meta["protocol_be"] = 0x0008
    meta["len"] = 67
    return torch.from_numpy(bufs.reshape(-1).copy()).cuda(), torch.from_numpy(meta.view(np.int64).copy()).cuda()


def test_flow_table_emits_its_due_flows():
    """insert_packets(emit=True) hands back the images of exactly the flows
    stats["due"] names, each equal to serialize() of the table's quACK."""
    t, f, nflows = 8, 5, 40
    rng = np.random.default_rng(21)
    flows = rng.integers(0, 256, size=(nflows, 12), dtype=np.uint8)
    listed, emitting = sk.DeviceFlowQuacks(t), sk.DeviceFlowQuacks(t)
    seen_due = 0
    for rnd in range(3):
        which = rng.integers(0, nflows, size=150)
        b, m = packet_batch(flows, which, rng.integers(0, 1 << 32, size=150, dtype=np.uint64), seed=rnd)
        due = listed.insert_packets(b, 67, m, None, frequency_pkts=f)["due"]
        stats = emitting.insert_packets(b, 67, m, None, frequency_pkts=f, emit=True)
        keys, rows, wire, lens = stats["wire"]
        got_keys = [bytes(k) for k in keys.cpu().numpy()]
        assert got_keys == sorted(due) and stats["due"] == []
        wire, lens = wire.cpu().numpy(), lens.cpu().numpy()
        table_keys = emitting.keys.cpu().numpy()
        for r, k in enumerate(got_keys):
            assert wire[r, :lens[r]].tobytes() == listed.quack(k).serialize()
            assert table_keys[int(rows[r])].tobytes() == k
        seen_due += len(due)
    assert seen_due > 20
    # emit() of the whole table, at a stride of the caller's
    keys, rows, wire, lens = emitting.emit(stride=64)
    assert wire.shape == (len(emitting), 64) and rows.tolist() == list(range(len(emitting)))
    want = listed.senders()
    wire, lens = wire.cpu().numpy(), lens.cpu().numpy()
    for r, k in enumerate(keys.cpu().numpy()):
        assert wire[r, :lens[r]].tobytes() == want[k.tobytes()].serialize()
    assert emitting.insert_packets(b, 67, m, None, emit=True)["wire"][2].shape[0] == 0   # frequency 0: none due
