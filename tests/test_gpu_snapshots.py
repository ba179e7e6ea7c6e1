"""Per-flow quACK snapshots (qk_u32_snapshot_segments_device, snapshot_segments,
DeviceFlowSnapshots) on the GPU against the reference loop over the oracle
(snapshot_model.py): one insert per packet, a clone whenever the count reached
is a multiple of frequency_pkts.  Every comparison is bit for bit.  The shapes
are the smallest at which the kernels can go wrong: every threshold at which
the walk changes shape, flows across work-item boundaries (SN_ITEM = 2048
positions), the u32 wrap of the count, empty flows, special ids."""
import ctypes as C

import numpy as np
import pytest

import sidekick_amd as sk
from sidekick_amd.quack import encode_segments
from sidekick_amd._lib import (QK_E_CAPACITY, QK_E_INVAL, QK_E_MISMATCH, QK_E_THRESHOLD, P32, lib)
from snapshot_model import (FREQUENCIES, LOSS_F, LOSS_LOST, LOSS_T, THRESHOLDS, base_quack, loss_case_ids,
                            per_packet_states, record, reference_loop, run_loss_case, serialize)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ITEM = 2048
NAME = "qk_u32_snapshot_segments_device"
SENTINEL = 0x5A5A5A5A


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint32)


class Case:
    """A grouped batch with its base records, and the model's state of every
    flow after each of its packets (computed once, whatever the frequency)."""

    def __init__(self, t, lens, counts, seed=1, first=0, sums="rand", ids=None):
        rng = np.random.default_rng(seed)
        self.t, self.nseg = t, len(lens)
        self.offs = np.zeros(self.nseg + 1, dtype=np.uint64)
        self.offs[0] = first
        self.offs[1:] = first + np.cumsum(np.asarray(lens, dtype=np.uint64))
        n = int(self.offs[-1]) + 3
        self.ids = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        if ids is not None:
            self.ids[first:first + len(ids)] = np.asarray(ids, dtype=np.uint32)
        self.arrival = rng.permutation(n).astype(np.uint32) + np.uint32(7)
        self.base = np.zeros((self.nseg, 4 + t), dtype=np.uint32)
        self.base[:, 0] = t
        for g, c in enumerate(counts):
            if c is None:          # a flow the table has not seen: a qk_u32_init row
                continue
            self.base[g, 1] = c
            self.base[g, 2] = 1
            self.base[g, 3] = rng.integers(0, 1 << 32)
            self.base[g, 4:] = P32 - 1 if sums == "pm1" else rng.integers(0, P32, size=t, dtype=np.uint64)
        self.sums, self.counts = [], []
        self.final = self.base.copy()
        for g in range(self.nseg):
            b = self.base[g]
            q = base_quack(t, b[1], b[4:], b[3] if b[2] else None)
            s, c = per_packet_states(q, self.ids[int(self.offs[g]):int(self.offs[g + 1])].tolist())
            self.sums.append(s)
            self.counts.append(c)
            self.final[g] = record(q)

    def expect(self, f):
        """(records, seg, pos, snap_offsets) of the reference at frequency f."""
        recs, seg, pos, snoffs = [], [], [], [0]
        for g in range(self.nseg):
            hit = np.flatnonzero(self.counts[g].astype(np.uint64) % np.uint64(f) == 0)
            p = hit + int(self.offs[g])
            r = np.zeros((len(hit), 4 + self.t), dtype=np.uint32)
            r[:, 0], r[:, 1], r[:, 2], r[:, 3] = self.t, self.counts[g][hit], 1, self.ids[p]
            r[:, 4:] = self.sums[g][hit]
            recs.append(r)
            seg.append(np.full(len(hit), g, dtype=np.uint32))
            pos.append(p.astype(np.int64))
            snoffs.append(snoffs[-1] + len(hit))
        return np.concatenate(recs), np.concatenate(seg), np.concatenate(pos), np.asarray(snoffs, dtype=np.uint64)

    def check(self, f, arrival=True, final=True):
        s = sk.snapshot_segments(dev(self.base).view(self.nseg, 4 + self.t), dev(self.ids), self.offs, f,
                                 arrival=dev(self.arrival) if arrival else None, final=final)
        recs, seg, pos, snoffs = self.expect(f)
        assert np.array_equal(s.offsets, snoffs)
        assert s.records.shape == (len(recs), 4 + self.t)
        got = host(s.records).reshape(len(recs), 4 + self.t)
        assert np.array_equal(got[:, :4], recs[:, :4])
        assert np.array_equal(got, recs)
        assert np.array_equal(host(s.seg), seg)
        assert np.array_equal(s.pos.cpu().numpy(), pos)
        if arrival:
            assert np.array_equal(host(s.arrival), self.arrival[pos])
        else:
            assert s.arrival is None
        if final:
            assert np.array_equal(host(s.final).reshape(self.nseg, 4 + self.t), self.final)
        else:
            assert s.final is None
        return s


_cases = {}


def case(*args, **kw):
    """Case(...), built once per session and left unchanged."""
    key = (args, tuple(sorted((k, tuple(v) if isinstance(v, (list, np.ndarray)) else v) for k, v in kw.items())))
    key = repr(key)
    if key not in _cases:
        _cases[key] = Case(*args, **kw)
    return _cases[key]


# ----------------------------------------------------------------- thresholds
@pytest.mark.parametrize("t", THRESHOLDS)
def test_every_threshold_shape_at_every_frequency(t):
    """5 flows of a few hundred ids (two work items, one flow across the
    boundary, one empty), base counts of every phase."""
    c = case(t, [700, 0, 900, 1300, 130], [5, 9, None, 64 * 65 * 21 - 1, 1000003], seed=t)
    for f in FREQUENCIES:
        c.check(f)


# ---------------------------------------------------------------------- phase
@pytest.mark.parametrize("t", [4, 33])
def test_phase_and_empty_segments(t):
    f = 5
    # c0 % f = 0, 1, f - 1; a first snapshot at position 0 (c0 % f == f - 1); a
    # segment shorter than the distance to the next multiple; empty segments
    # first, in the middle and last
    c = case(t, [0, 7, 0, 2, 12, 1, 11, 0], [3, 5, 9, 6, 9, 4, None, 2], seed=3)
    s = c.check(f)
    assert s.offsets.tolist() == [0, 0, 1, 1, 1, 4, 5, 7, 7]
    assert host(s.pos.to(torch.int32)).tolist()[1] == 9       # flow 4's first packet
    c.check(f, arrival=False, final=False)
    c.check(1)


def test_no_segments_and_all_segments_empty(ctx):
    s = sk.snapshot_segments(torch.empty((0, 8), dtype=torch.int32, device="cuda"), dev([1, 2, 3]), [0], 2, final=True)
    assert s.records.shape == (0, 8) and s.offsets.tolist() == [0] and s.final.shape == (0, 8)
    c = case(4, [0, 0, 0], [7, None, 1 << 31], seed=4)
    s = c.check(2)
    assert s.records.shape[0] == 0
    c.check(2, arrival=False, final=False)


# ------------------------------------------------------------------- the wrap
@pytest.mark.parametrize("f", [1, 3, 5, 1 << 31])
def test_count_wrapping_to_zero_triggers(f):
    w = (1 << 32) - 3
    c = case(4, [8, 5, 8], [w, 2, w], seed=5)
    s = c.check(f)
    counts = host(s.records).reshape(-1, 8)[:, 1].tolist()
    first = counts[:int(s.offsets[1])]
    assert 0 in first                                      # a count of 0 triggers
    assert all(v < 6 for v in first[first.index(0):])      # and the counts after it are small
    want = [v & 0xFFFFFFFF for v in range(w + 1, w + 9) if (v & 0xFFFFFFFF) % f == 0]
    assert first == want


# ------------------------------------------------- across work-item boundaries
@pytest.mark.parametrize("t", [4, 32])
@pytest.mark.parametrize("f,c0,lengths", [(1, 10, (ITEM - 1, ITEM, ITEM + 1, 3 * ITEM + 17)),
                                         (2, 11, (2 * ITEM - 2, 2 * ITEM, 2 * ITEM + 2, 6 * ITEM + 34))])
def test_one_long_flow_past_item_boundaries(t, f, c0, lengths):
    """The long flow between two short ones, so that a carry that leaks from
    one flow into the next shows; alone as well, where it starts on an item
    boundary."""
    for n in lengths:
        case(t, [3, n, 5], [4, c0, 8], seed=n).check(f)
    case(t, [lengths[3]], [c0], seed=6).check(f)
    case(t, [lengths[1], lengths[1]], [c0, None], seed=7).check(f)   # a flow that ends on a boundary


def test_many_short_flows_packed_into_items():
    rng = np.random.default_rng(8)
    lens = rng.integers(0, 6, size=1000)
    counts = [None if v % 7 == 0 else int(v) for v in rng.integers(0, 1 << 32, size=1000)]
    case(8, lens.tolist(), counts, seed=8).check(2)


def test_long_runs_of_empty_flows_between_flows():
    """More empty flows in a row than the walk's search takes at once (64)."""
    lens = [3] + [0] * 200 + [ITEM + 5] + [0] * 70 + [4] + [0] * 65
    case(5, lens, [i * 3 for i in range(len(lens))], seed=9).check(2)


def test_long_intervals():
    # about 2.4 f ids, f beyond anything a lane would take; and f larger than the whole batch
    case(5, [4, 2400, 9], [1, 2, 3], seed=10).check(1000)
    s = case(5, [4, 2400, 9], [1, 2, 3], seed=10).check(100000)
    assert s.records.shape[0] == 0
    s = case(5, [4, 2400, 9], [1, 99999, 3], seed=11).check(100000)
    assert s.offsets.tolist() == [0, 0, 1, 1]


# ---------------------------------------------------------------- special ids
@pytest.mark.parametrize("t", [4, 33])
def test_special_ids_inside_an_interval_and_as_the_trigger(t, golden):
    wraps = sorted({v for ids in golden["bsgs_wrap_ids"].values() for v in ids})
    pool = [0, P32 - 1, P32, P32 + 1, P32 + 2, P32 + 3, P32 + 4] + wraps
    if len(pool) % 2 == 0:
        pool.append(1)
    ids = pool + pool        # an odd pool: every id once at an even and once at an odd position
    c = case(t, [len(ids), 3], [0, 1], seed=12, ids=ids)
    s = c.check(2)
    trig = set(host(s.records).reshape(-1, 4 + t)[:int(s.offsets[1]), 3].tolist())
    assert trig == set(pool)                       # each one triggers, last_value raw (ids >= p unreduced)
    c.check(3)


# ----------------------------------------------------------------------- base
def test_fresh_base_and_base_sums_that_wrap():
    case(9, [300, 40, 0], [None, None, None], seed=13).check(4)
    # every sum p - 1: each add wraps mod p
    case(9, [300, 40, 0, ITEM + 3], [1, 2, 3, 5], seed=14, sums="pm1").check(4)


# ------------------------------------------------------------------ alignment
@pytest.mark.parametrize("first", [0, 1, 2, 3])
@pytest.mark.parametrize("t", [5, 7])
def test_ids_at_every_word_offset_and_odd_record_rows(first, t):
    case(t, [130, 67, ITEM], [3, None, 6], seed=15 + first, first=first).check(3)


# ------------------------------------------------- the C ABI: capacity, errors
class Raw:
    """The entry point called as C calls it, every output filled with a sentinel."""

    def __init__(self, ctx, c, cap, with_final=True, with_arrival=True):
        self.ctx, self.c, self.cap = ctx, c, cap
        W = 4 + c.t
        fill = lambda n, dt: torch.full((max(n, 1),), SENTINEL, dtype=dt, device="cuda")   # noqa: E731
        self.base, self.ids, self.arrival = dev(c.base), dev(c.ids), dev(c.arrival) if with_arrival else None
        self.snap, self.seg, self.pos = fill(cap * W, torch.int32), fill(cap, torch.int32), fill(cap, torch.int64)
        self.arr = fill(cap, torch.int32) if with_arrival else None
        self.fin = fill(c.nseg * W, torch.int32) if with_final else None
        self.snoffs = np.full(c.nseg + 1, 99, dtype=np.uint64)
        self.m = C.c_size_t(12345)
        self.t, self.f, self.nseg, self.offs = c.t, 2, c.nseg, c.offs.copy()

    def args(self):
        p = lambda x: x.data_ptr() if x is not None else None   # noqa: E731
        return dict(ctx=self.ctx.handle, base=p(self.base), ids=p(self.ids), arrival=p(self.arrival),
                    offs=self.offs.ctypes.data_as(C.POINTER(C.c_uint64)), nseg=self.nseg, t=self.t, f=self.f,
                    snap=p(self.snap), seg=p(self.seg), pos=p(self.pos), arr=p(self.arr), cap=self.cap,
                    snoffs=self.snoffs.ctypes.data_as(C.POINTER(C.c_uint64)), m=C.byref(self.m), fin=p(self.fin),
                    stream=None)

    def call(self, **over):
        a = self.args()
        a.update(over)
        rc = getattr(lib(), NAME)(*a.values())
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        outs = [self.snap, self.seg, self.arr, self.fin]
        return (all(bool((o == SENTINEL).all()) for o in outs if o is not None)
                and bool((self.pos == SENTINEL).all()))


def test_capacity(ctx):
    c = case(6, [40, 0, 25, 9], [1, 2, None, 4], seed=20)
    recs, seg, pos, snoffs = c.expect(2)
    m = len(recs)
    r = Raw(ctx, c, m - 1)
    assert r.call() == QK_E_CAPACITY
    assert r.m.value == m and np.array_equal(r.snoffs, snoffs)
    assert r.untouched()
    r = Raw(ctx, c, m)
    assert r.call() == 0
    assert r.m.value == m and np.array_equal(r.snoffs, snoffs)
    assert np.array_equal(host(r.snap).reshape(m, 10), recs)
    assert np.array_equal(host(r.seg), seg) and np.array_equal(r.pos.cpu().numpy(), pos)
    assert np.array_equal(host(r.arr), c.arrival[pos])
    assert np.array_equal(host(r.fin).reshape(c.nseg, 10), c.final)
    # no snapshot at all: a capacity of 0 is enough
    c0 = case(6, [3, 0, 2], [0, 5, 8], seed=21)
    r = Raw(ctx, c0, 0)
    r.f = 1000
    assert r.call(snap=None, seg=None, pos=None, arr=None, arrival=None) == 0
    assert r.m.value == 0 and r.snoffs.tolist() == [0, 0, 0, 0]
    assert np.array_equal(host(r.fin).reshape(3, 10), c0.final)


def test_every_error(ctx):
    c = case(6, [40, 0, 25, 9], [1, 2, None, 4], seed=20)
    m = len(c.expect(2)[0])

    def bad(want, **over):
        r = Raw(ctx, c, m)
        for k in [k for k in over if k in ("t", "f", "nseg", "offs_np")]:
            v = over.pop(k)
            if k == "offs_np":
                r.offs = v
            else:
                setattr(r, k, v)
        assert r.call(**over) == want, over
        assert r.untouched()
        return r

    bad(QK_E_THRESHOLD, t=0)
    bad(QK_E_THRESHOLD, t=1025)
    bad(QK_E_INVAL, f=0)
    dec = c.offs.copy()
    dec[2] = dec[1] - 1
    bad(QK_E_INVAL, offs_np=dec)
    bad(QK_E_INVAL, nseg=1 << 32)
    # a host pointer where a device one is required, and the reverse
    hostbuf = np.zeros(4096, dtype=np.uint32)
    hp = hostbuf.ctypes.data
    for k in ("base", "ids", "snap", "seg", "pos", "fin"):
        bad(QK_E_INVAL, **{k: hp})
    d64 = torch.zeros(16, dtype=torch.int64, device="cuda")
    bad(QK_E_INVAL, offs=C.cast(d64.data_ptr(), C.POINTER(C.c_uint64)))
    bad(QK_E_INVAL, snoffs=C.cast(d64.data_ptr(), C.POINTER(C.c_uint64)))
    # one arrival pointer without the other
    bad(QK_E_INVAL, arrival=None)
    bad(QK_E_INVAL, arr=None)
    # an output over an input, or over another output
    r = Raw(ctx, c, m)
    assert r.call(fin=r.base.data_ptr()) == QK_E_INVAL
    assert np.array_equal(host(r.base).reshape(c.nseg, 10), c.base) and bool((r.snap == SENTINEL).all())
    r = Raw(ctx, c, m)
    assert r.call(snap=r.ids.data_ptr()) == QK_E_INVAL and np.array_equal(host(r.ids), c.ids)
    r = Raw(ctx, c, m)
    assert r.call(seg=r.snap.data_ptr() + 8) == QK_E_INVAL and r.untouched()
    r = Raw(ctx, c, m)
    assert r.call(pos=r.fin.data_ptr()) == QK_E_INVAL and r.untouched()
    # a base record of another threshold, found on the device (outputs unspecified)
    r = Raw(ctx, c, m)
    r.base.view(-1)[2 * 10] = 5
    assert r.call() == QK_E_MISMATCH
    # the wrapper: a final that is the base
    b = dev(c.base).view(c.nseg, 10)
    with pytest.raises(sk.QuackError) as e:
        sk.snapshot_segments(b, dev(c.ids), c.offs, 2, final=b)
    assert e.value.code == QK_E_INVAL


# ------------------------------------- cross-checks against existing entry points
@pytest.mark.parametrize("t", [8, 33])
def test_final_is_merge_of_base_and_encode_segments(t):
    c = case(t, [700, 0, 900, 1300, 130], [5, 9, None, 64 * 65 * 21 - 1, 1000003], seed=t)
    s = c.check(7)
    enc = encode_segments(dev(c.ids), c.offs, t)
    fin = host(s.final).reshape(c.nseg, 4 + t)
    for g in range(c.nseg):
        q = sk.PowerSumQuackU32._from_record(c.base[g].tobytes(), t)
        q.merge(enc[g])
        assert q._buf.raw == fin[g].tobytes(), g


@pytest.mark.parametrize("t", [5, 32])
def test_emitted_images_equal_the_model_serialization(t):
    c = case(t, [130, 67, ITEM], [3, None, 6], seed=15, first=0)
    s = c.check(3)
    _, rows, wire, lens = sk.emit_wire(None, s.records)
    assert host(rows).tolist() == list(range(s.records.shape[0]))
    wire, lens = wire.cpu().numpy(), host(lens)
    table = {g: base_quack(t, c.base[g, 1], c.base[g, 4:], c.base[g, 3] if c.base[g, 2] else None)
             for g in range(c.nseg)}
    r = 0
    for g in range(c.nseg):                      # ordered by flow, then by position
        for _, q in reference_loop(table, [g] * int(c.offs[g + 1] - c.offs[g]),
                                   c.ids[int(c.offs[g]):int(c.offs[g + 1])].tolist(), 3):
            assert wire[r, :lens[r]].tobytes() == serialize(q), r
            r += 1
    assert r == s.records.shape[0]


# -------------------------------------------------------- DeviceFlowSnapshots
def test_device_flow_snapshots_sends_the_reference_datagrams_in_order():
    t, f = 8, 4
    rng = np.random.default_rng(30)
    tab = sk.DeviceFlowSnapshots(t, 48, f)
    model = {g: base_quack(t) for g in range(48)}
    for rnd in range(5):
        if rnd == 2:                              # flows added mid-way
            tab.add_flows(16)
            model.update({g: base_quack(t) for g in range(48, 64)})
        nf = tab.nflows
        n = 500 + 37 * rnd
        flows = rng.integers(0, nf, size=n).astype(np.uint32)
        flows[rng.integers(0, n, size=n // 3)] = 5          # one busy flow: several datagrams per batch
        ids = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        want = reference_loop(model, flows.tolist(), ids.tolist(), f)
        fl, wire, lens, recs = tab.insert(flows, ids if rnd % 2 else dev(ids))
        wire, lens = wire.cpu().numpy(), host(lens)
        assert host(fl).tolist() == [g for g, _ in want]
        assert [wire[r, :lens[r]].tobytes() for r in range(len(want))] == [serialize(q) for _, q in want]
        assert np.array_equal(host(recs).reshape(len(want), 4 + t), np.array([record(q) for _, q in want]))
        assert np.array_equal(host(tab.records).reshape(nf, 4 + t), np.array([record(model[g]) for g in range(nf)]))
    # a batch without a datagram
    fl, wire, lens, recs = sk.DeviceFlowSnapshots(t, 3, 1000).insert([0, 1, 1], [7, 8, 9])
    assert fl.numel() == 0 and wire.shape[0] == 0 and lens.numel() == 0 and recs.shape == (0, 4 + t)


def test_device_snapshots_recover_the_loss_case():
    ids = loss_case_ids()
    received = np.array([v for s, v in enumerate(ids.tolist()) if s not in LOSS_LOST], dtype=np.uint32)
    tab = sk.DeviceFlowSnapshots(LOSS_T, 1, LOSS_F)
    fl, wire, lens, recs = tab.insert(np.zeros(len(received), dtype=np.uint32), received)
    assert recs.shape[0] == 6
    rows = host(recs).reshape(6, 4 + LOSS_T)
    quacks = [sk.PowerSumQuackU32._from_record(rows[r].tobytes(), LOSS_T) for r in range(6)]
    retx, resets = run_loss_case(quacks)
    assert resets == 0 and retx == LOSS_LOST
    # the table's end-of-batch quACK alone: the sender resets
    end = sk.PowerSumQuackU32._from_record(host(tab.records).tobytes(), LOSS_T)
    retx, resets = run_loss_case([end])
    assert resets == 1 and retx == []
