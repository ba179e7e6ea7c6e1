"""Every queued quACK of a flow stepped in one call
(qk_u32_sender_steps_segments_device) and the ingest that keeps every accepted
datagram (qk_u32_wire_ingest_queue_device) on the GPU, bit for bit against
sender_steps_model.py: every word of mine_out, q_action, q_drain, stepped,
drain, hit_offsets and the hits; the queue's placement against a numpy stable
grouping; and DeviceSenderLog.on_wire(every=True) in a closed loop with
DeviceFlowSnapshots against one QuackReceiver per flow fed one quACK at a time."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import sidekick_amd as sk
from sidekick_amd._lib import (QK_E_CAPACITY, QK_E_FORMAT, QK_E_INVAL, QK_E_MISMATCH, QK_E_THRESHOLD,
                               QK_WIRE_SUPERSEDED, lib)
from sidekick_amd.receiver import QuackReceiver
from oracle import quack_oracle as qo
import sender_steps_model as sm
from snapshot_model import serialize

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

P = qo.P32
M32 = 0xFFFFFFFF
THRESHOLDS = (1, 8, 32, 33, 129)
RESET = sm.SND_RESET_REORDERED | sm.SND_RESET_RETX | sm.SND_RESET_EXCEEDS


def dev(a):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint8): np.uint8}[a.dtype]
    return torch.from_numpy(a.view(view).copy()).to("cuda:0")


def host(tensor, dtype=np.uint32):
    return tensor.cpu().numpy().view(dtype)


# ------------------------------------------------------------------ the call
class Out:
    pass


def call_steps(ctx, mine, queue, q_offsets, log, offsets, t, cap, d_mine_out=None):
    """The raw call on host arrays: (rc, Out) with every output as a numpy array."""
    nseg, nq = len(offsets) - 1, int(q_offsets[-1]) if len(q_offsets) else 0
    o = Out()
    o.d_mine, o.d_queue, o.d_log = dev(mine.reshape(-1)), dev(queue.reshape(-1)), dev(log)
    o.d_out = torch.full((max(nseg, 1) * (4 + t),), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    o.q_action = np.full(max(nq, 1), 0xEE, dtype=np.uint8)
    o.q_drain = np.full(max(nq, 1), 0xEEEE, dtype=np.uint64)
    o.stepped = np.full(max(nseg, 1), 0xEEEE, dtype=np.uint32)
    o.drain = np.full(max(nseg, 1), 0xEEEE, dtype=np.uint64)
    o.hits = np.full(max(cap, 1), 0xEEEE, dtype=np.uint64)
    o.hit_offsets = np.full(nq + 1, 0xEEEE, dtype=np.uint64)
    nh = C.c_size_t(12345)
    offs, qoffs = np.ascontiguousarray(offsets, dtype=np.uint64), np.ascontiguousarray(q_offsets, dtype=np.uint64)
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))  # noqa: E731
    rc = lib().qk_u32_sender_steps_segments_device(
        ctx.handle, o.d_mine.data_ptr(), o.d_queue.data_ptr() if nq else None, p64(qoffs),
        o.d_log.data_ptr() if len(log) else None, p64(offs), nseg, t,
        (d_mine_out if d_mine_out is not None else o.d_out).data_ptr(), o.q_action.ctypes.data_as(C.POINTER(C.c_uint8)),
        p64(o.q_drain), o.stepped.ctypes.data_as(C.POINTER(C.c_uint32)), p64(o.drain), p64(o.hits), cap,
        p64(o.hit_offsets), C.byref(nh), None)
    o.n_hits = nh.value
    o.mine_out = host(o.d_out).reshape(max(nseg, 1), 4 + t)[:nseg]
    o.q_action, o.q_drain, o.stepped, o.drain = o.q_action[:nq], o.q_drain[:nq], o.stepped[:nseg], o.drain[:nseg]
    return rc, o


def assert_equal(o, want, hits=True):
    assert np.array_equal(o.q_action, want["q_action"]), np.flatnonzero(o.q_action != want["q_action"])[:8]
    assert np.array_equal(o.q_drain, want["q_drain"])
    assert np.array_equal(o.stepped, want["stepped"])
    assert np.array_equal(o.drain, want["drain"])
    assert np.array_equal(o.hit_offsets, want["hit_offsets"])
    assert o.n_hits == len(want["hits"])
    if hits:
        assert np.array_equal(o.hits[:o.n_hits], want["hits"])
    bad = np.flatnonzero((o.mine_out != want["mine_out"]).any(axis=1))
    assert bad.size == 0, (bad[:8], o.mine_out[bad[:1]], want["mine_out"][bad[:1]])


# --------------------------------------------------------------- scenarios
def ids(rng, n):
    return [rng.randrange(1 << 8, P - (1 << 8)) for _ in range(n)]


def build_flows(t, seed):
    rng = random.Random(seed)
    flows = []
    # k_g = 0, 1, 2, 5 in one call, a loss in every interval
    for k in (0, 1, 2, 5):
        stops = [10 * (j + 1) for j in range(k)]
        flows.append(sm.queued_flow(rng, t, 60, stops, [s - 3 for s in stops]))
    # interval ends at 0, 63, 64, 2047, 2048, 2049 and in the third 2048-slice: b inside a slice, the
    # stop in a later one; hits in the slice of b and in the slice of the stop
    stops = [0, 63, 64, 2047, 2048, 2049, 4096 + 7]
    for lost in ([], [5, 70, 2051, 4100], [5, 6, 70, 2040, 2051, 2052, 4097, 4100]):
        per = {}
        keep = []
        for p in lost:                      # at most t per interval
            j = next(i for i, s in enumerate(stops) if p <= s)
            if per.get(j, 0) < t:
                per[j] = per.get(j, 0) + 1
                keep.append(p)
        flows.append(sm.queued_flow(rng, t, 4097 + 600, stops, keep))
    # more short flows in a row than one packed work item holds (256, or 8192 / T)
    for i in range(300):
        n = i % 4
        stops = sorted(rng.sample(range(n), rng.randrange(0, n + 1))) if n else []
        lost = [p for p in range(n) if p not in stops and rng.random() < 0.3][:t]
        flows.append(sm.queued_flow(rng, t, n, stops, lost))
    # 0, 1, t and t + 1 losses per interval; t + 1 in the middle: EXCEEDS there, UNSTEPPED behind it
    w = t + 4
    for k in (0, 1, t, t + 1):
        stops = [w - 1, 2 * w - 1, 3 * w - 1]
        lost = [s - 1 - i for s in stops for i in range(k)]
        flows.append(sm.queued_flow(rng, t, 3 * w + 5, stops, lost))
        lost = [stops[1] - 1 - i for i in range(k)]                       # the middle interval only
        flows.append(sm.queued_flow(rng, t, 3 * w + 5, stops, lost))
    if t != 8:
        return flows
    # a duplicate datagram: last_value unchanged, IDLE in the middle of a queue
    f = sm.queued_flow(rng, t, 40, [9, 19, 29], [3, 14, 25])
    f.queue.insert(2, f.queue[1].clone())
    flows.append(f)
    # the last_value of quACK j + 1 before and after stop j: the search starts at b
    seg = ids(rng, 30)
    seg[12] = seg[2]
    flows.append(sm.queued_flow(rng, t, 30, [5, 12, 20], [4, 8, 15], seg=seg))
    # a missing id twice in one interval, and once in each of two intervals
    seg = ids(rng, 40)
    seg[6] = seg[3]
    flows.append(sm.queued_flow(rng, t, 40, [10, 30], [3, 6, 20], seg=seg))
    seg = ids(rng, 40)
    seg[20] = seg[3]
    flows.append(sm.queued_flow(rng, t, 40, [10, 30], [3, 20], seg=seg))
    # unreduced ids: raw equality for the stop, id mod p for the hits
    seg = ids(rng, 30)
    seg[4], seg[9], seg[14] = 2, P + 2, P + 3            # 2 and p + 2 are equal mod p, not as raw ids
    seg[7], seg[17] = P + 4, 0xFFFFFFFF
    flows.append(sm.queued_flow(rng, t, 30, [9, 14, 25], [7, 11, 17], seg=seg))
    flows.append(sm.queued_flow(rng, t, 30, [4, 9], [3], seg=seg))
    # a last_value that is not in the rest of the log: REORDERED, then UNSTEPPED
    f = sm.queued_flow(rng, t, 40, [9, 19, 29], [3, 14, 25])
    f.queue[1].insert(0xDEADBEEF)
    flows.append(f)
    f = sm.queued_flow(rng, t, 40, [19, 9, 29], [3])     # quACKs out of order: the second one's stop lies before b
    flows.append(f)
    # RETX in the middle of a queue: the peer counts ids of its own
    f = sm.queued_flow(rng, t, 40, [9, 19, 29], [3, 14, 25])
    q = f.queue[1]
    for v in ids(rng, 3):
        q.insert(v)
    q.last_value = f.seg[19]
    flows.append(f)
    # mine.count wraps across a step
    f = sm.queued_flow(rng, t, 40, [9, 19, 29], [3, 14, 25], history=0)
    f.mine.count = M32 - 12
    for q in f.queue:
        q.count = (q.count + M32 - 12) & M32
    flows.append(f)
    # a peer without a last_value: mine with one (REORDERED), mine without (IDLE, then stepped on)
    f = sm.queued_flow(rng, t, 20, [9], [3])
    f.queue.insert(0, qo.OracleQuack(t))
    flows.append(f)
    f = sm.queued_flow(rng, t, 20, [9], [3], history=0)
    f.queue.insert(0, qo.OracleQuack(t))
    flows.append(f)
    return flows


@functools.lru_cache(maxsize=None)
def scenario(t):
    """The flows of threshold t, their arrays and the model's answer, computed once."""
    flows = build_flows(t, 1000 + t)
    return flows, sm.layout(flows, t), sm.steps(flows, t)


@pytest.mark.parametrize("t", THRESHOLDS)
def test_bit_for_bit_against_the_model(ctx, t):
    flows, (mine, queue, qoffs, log, offsets), want = scenario(t)
    rc, o = call_steps(ctx, mine, queue, qoffs, log, offsets, t, len(log))
    assert rc == 0
    assert_equal(o, want)
    # the scenario holds what it is meant to hold
    acts = set(want["q_action"].tolist())
    assert {sm.SND_ADVANCED, sm.SND_RESET_EXCEEDS, sm.SND_UNSTEPPED} <= acts
    if t == 8:
        assert sm.SND_IDLE in acts
        for bit in (sm.SND_RESET_REORDERED, sm.SND_RESET_RETX):
            assert any(a & bit for a in acts)
    k = (qoffs[1:] - qoffs[:-1]).tolist()
    assert {0, 1, 2, 5} <= set(k)
    assert len(want["hits"]) > 0 and np.all(np.diff(want["hits"].astype(np.int64)) > 0)   # ascending over the call


def test_wrapper_returns_the_model_answer(ctx):
    t = 8
    flows, (mine, queue, qoffs, log, offsets), want = scenario(t)
    res = sk.sender_steps(dev(mine.reshape(-1)).view(len(flows), 4 + t), dev(queue.reshape(-1)).view(-1, 4 + t), qoffs,
                          log, offsets, ctx=ctx)
    assert np.array_equal(host(res.mine_out).reshape(len(flows), 4 + t), want["mine_out"])
    assert np.array_equal(res.q_action, want["q_action"]) and np.array_equal(res.q_drain, want["q_drain"])
    assert np.array_equal(res.stepped, want["stepped"]) and np.array_equal(res.drain, want["drain"])
    flow_of = np.repeat(np.arange(len(flows)), (qoffs[1:] - qoffs[:-1]).astype(np.int64))
    got = [p + int(offsets[flow_of[q]]) for q, m in enumerate(res.missing) for p in m]
    assert got == want["hits"].tolist()
    assert [len(m) for m in res.missing] == np.diff(want["hit_offsets"].astype(np.int64)).tolist()
    # sketches on the host are uploaded
    f = flows[1]
    res = sk.sender_steps([sk.PowerSumQuackU32._from_record(sm.record(f.mine).tobytes(), t)],
                          [sk.PowerSumQuackU32._from_record(sm.record(q).tobytes(), t) for q in f.queue],
                          [0, len(f.queue)], np.array(f.seg, dtype=np.uint32), [0, len(f.seg)], ctx=ctx)
    w = sm.steps([f], t)
    assert np.array_equal(host(res.mine_out).reshape(1, 4 + t), w["mine_out"]) and res.drain.tolist() == w["drain"].tolist()


def test_at_most_one_quack_per_flow_equals_the_single_step(ctx):
    t = 8
    rng = random.Random(5)
    flows = [sm.queued_flow(rng, t, 50 + i, [20 + i] if i % 3 else [], [4, 9][: i % 3]) for i in range(40)]
    f = sm.queued_flow(rng, t, 30, [9], [3])
    f.queue[0].insert(0xDEADBEEF)
    flows.append(f)
    mine, queue, qoffs, log, offsets = sm.layout(flows, t)
    rc, o = call_steps(ctx, mine, queue, qoffs, log, offsets, t, len(log))
    assert rc == 0
    present = (qoffs[1:] > qoffs[:-1])
    peer = np.zeros_like(mine)
    peer[:, 0] = t
    peer[present] = queue
    one = sk.sender_step(dev(mine.reshape(-1)).view(len(flows), 4 + t), dev(peer.reshape(-1)).view(len(flows), 4 + t),
                         log, offsets, present=present, ctx=ctx)
    assert np.array_equal(host(one.mine_out).reshape(len(flows), 4 + t), o.mine_out)
    assert np.array_equal(one.action[present], o.q_action) and np.all(one.action[~present] == sm.SND_IDLE)
    assert np.array_equal(one.drain, o.drain) and np.array_equal(one.drain[present], o.q_drain)
    assert [p + int(offsets[g]) for g, m in enumerate(one.missing) for p in m] == o.hits[:o.n_hits].tolist()


def test_empty_queues_and_no_flows(ctx):
    t = 8
    rng = random.Random(6)
    flows = [sm.queued_flow(rng, t, n, [], []) for n in (0, 5, 3000)]
    mine, queue, qoffs, log, offsets = sm.layout(flows, t)
    rc, o = call_steps(ctx, mine, queue, qoffs, log, offsets, t, 16)
    assert rc == 0 and o.n_hits == 0 and o.hit_offsets.tolist() == [0]
    assert np.array_equal(o.mine_out, mine) and o.stepped.tolist() == [0, 0, 0] and o.drain.tolist() == [0, 0, 0]
    # flows without a log entry at all, with quACKs: REORDERED
    flows = [sm.queued_flow(rng, t, 0, [], []) for _ in range(3)]
    flows[1].queue = [sm.peer_after([], [77], t), sm.peer_after([], [77, 78], t)]
    mine, queue, qoffs, log, offsets = sm.layout(flows, t)
    rc, o = call_steps(ctx, mine, queue, qoffs, log, offsets, t, 0)
    assert rc == 0
    assert_equal(o, sm.steps(flows, t))
    assert o.q_action.tolist() == [sm.SND_RESET_REORDERED, sm.SND_UNSTEPPED]    # mine counts its history of 3: no RETX
    # nseg == 0
    hoffs = np.full(1, 7, dtype=np.uint64)
    nh = C.c_size_t(9)
    z = np.zeros(1, dtype=np.uint64)
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))  # noqa: E731
    assert lib().qk_u32_sender_steps_segments_device(ctx.handle, None, None, p64(z), None, p64(z), 0, t, None, None, None,
                                                     None, None, None, 0, p64(hoffs), C.byref(nh), None) == 0
    assert hoffs[0] == 0 and nh.value == 0


def test_capacity(ctx):
    t = 8
    flows, (mine, queue, qoffs, log, offsets), want = scenario(t)
    total = len(want["hits"])
    for cap in (0, 1, total - 1):
        rc, o = call_steps(ctx, mine, queue, qoffs, log, offsets, t, cap)
        assert rc == QK_E_CAPACITY and o.n_hits == total
        assert_equal(o, want, hits=False)
        assert np.all(o.hits == 0xEEEE)
    rc, o = call_steps(ctx, mine, queue, qoffs, log, offsets, t, total)
    assert rc == 0
    assert_equal(o, want)


def test_every_error(ctx):
    t = 8
    rng = random.Random(7)
    flows = [sm.queued_flow(rng, t, 30, [9, 19], [3, 14]) for _ in range(3)]
    mine, queue, qoffs, log, offsets = sm.layout(flows, t)
    f = lib().qk_u32_sender_steps_segments_device
    rc, o = call_steps(ctx, mine, queue, qoffs, log, offsets, t, 64)
    assert rc == 0
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))  # noqa: E731
    offs = np.ascontiguousarray(offsets)
    act, qd = np.zeros(6, dtype=np.uint8), np.zeros(6, dtype=np.uint64)
    st, dr = np.zeros(3, dtype=np.uint32), np.zeros(3, dtype=np.uint64)
    hits, hoffs, nh = np.zeros(64, dtype=np.uint64), np.zeros(7, dtype=np.uint64), C.c_size_t()
    d_host = torch.zeros(8, dtype=torch.int64, device="cuda:0")   # device memory where host memory is required

    def call(**over):
        a = dict(ctx=ctx.handle, mine=o.d_mine.data_ptr(), queue=o.d_queue.data_ptr(), qoffs=p64(qoffs), log=o.d_log.data_ptr(),
                 offs=p64(offs), nseg=3, t=t, out=o.d_out.data_ptr(), act=act.ctypes.data_as(C.POINTER(C.c_uint8)), qd=p64(qd),
                 st=st.ctypes.data_as(C.POINTER(C.c_uint32)), dr=p64(dr), hits=p64(hits), cap=64, hoffs=p64(hoffs),
                 nh=C.byref(nh))
        a.update(over)
        return f(*a.values(), None)
    assert call() == 0
    assert call(ctx=None) == QK_E_INVAL and call(ctx=None, t=0) == QK_E_INVAL       # NULL ctx first
    assert call(t=0) == QK_E_THRESHOLD and call(t=1025) == QK_E_THRESHOLD
    host_rec = np.zeros(3 * (4 + t), dtype=np.uint32)
    for name in ("mine", "queue", "log", "out"):                                      # host where device is required
        assert call(**{name: host_rec.ctypes.data_as(C.c_void_p)}) == QK_E_INVAL, name
        assert call(**{name: None}) == QK_E_INVAL, name
    kinds = dict(act=C.c_uint8, qd=C.c_uint64, st=C.c_uint32, dr=C.c_uint64, hits=C.c_uint64, hoffs=C.c_uint64,
                 qoffs=C.c_uint64, offs=C.c_uint64)
    for name, kind in kinds.items():                                                  # device where host is required
        assert call(**{name: C.cast(d_host.data_ptr(), C.POINTER(kind))}) == QK_E_INVAL, name
    for name in ("qoffs", "offs", "st", "dr", "hoffs", "nh", "act", "qd", "hits"):
        assert call(**{name: None}) == QK_E_INVAL, name
    bad = offs.copy()
    bad[1], bad[2] = bad[2], bad[1]
    assert call(offs=p64(bad)) == QK_E_INVAL                                          # decreasing offsets
    bad = qoffs.copy()
    bad[1], bad[2] = bad[2], bad[1]
    assert call(qoffs=p64(bad)) == QK_E_INVAL                                         # decreasing q_offsets
    for name in ("mine", "queue", "log"):                                             # mine_out over an input
        assert call(out=getattr(o, "d_" + name).data_ptr()) == QK_E_INVAL, name
    other = queue.copy()
    other[3, 0] = t + 1                                                               # a queue record of another threshold
    assert call(queue=dev(other.reshape(-1)).data_ptr()) == QK_E_MISMATCH
    other = mine.copy()
    other[2, 0] = t - 1
    assert call(mine=dev(other.reshape(-1)).data_ptr()) == QK_E_MISMATCH
    assert call(cap=1) == QK_E_CAPACITY and nh.value == 6


# -------------------------------------------------------------- ingest queue
def make_batch(t, n, nflows, seed, stride=None, bad=True):
    """n datagrams over nflows flows: (wire [n, stride] uint8, lens, flow, the expected status, the quACKs)."""
    rng = np.random.default_rng(seed)
    stride = sk.wire_max(t) if stride is None else stride
    wire = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)      # noise behind every image
    lens = np.zeros(n, dtype=np.uint32)
    flow = rng.integers(0, nflows, size=n).astype(np.uint32)
    status = np.zeros(n, dtype=np.int32)
    recs = np.zeros((n, 4 + t), dtype=np.uint32)
    for i in range(n):
        q = qo.OracleQuack(t)
        q.power_sums = rng.integers(0, P, size=t, dtype=np.uint64).astype(np.uint32).tolist()
        q.count = int(rng.integers(0, 1 << 32))
        q.last_value = None if i % 7 == 3 else int(rng.integers(0, 1 << 32))
        img = bytearray(serialize(q))
        kind = int(rng.integers(0, 12)) if bad else 99
        if kind == 0:
            img = img[:-1]                                              # truncated
            status[i] = QK_E_FORMAT
        elif kind == 1:
            img[8 + 4 * t] = 2                                          # a tag above 1
            status[i] = QK_E_FORMAT
        elif kind == 2:
            img[8:12] = (P + 1).to_bytes(4, "little")                   # a sum that is not canonical
            status[i] = QK_E_FORMAT
        elif kind == 3 and t > 1:
            o = qo.OracleQuack(t - 1)
            img = bytearray(serialize(o))                               # a well-formed image of another threshold
            status[i] = QK_E_MISMATCH
        wire[i, :len(img)] = np.frombuffer(bytes(img), dtype=np.uint8)
        lens[i] = len(img)
        if kind == 4:
            lens[i] = stride + 1                                        # d_len > stride
            status[i] = QK_E_FORMAT
        recs[i] = sm.record(q, t)
    return wire, lens, flow, status, recs


@pytest.mark.parametrize("n", [0, 1, 64, 65, 4097])
@pytest.mark.parametrize("t,extra", [(8, 0), (5, 3), (33, 1)])
def test_ingest_queue_places_every_accepted_datagram(ctx, t, extra, n):
    nflows = 37
    stride = sk.wire_max(t) + extra                                     # the minimum, and odd strides
    wire, lens, flow, status, recs = make_batch(t, n, nflows, 100 * t + n, stride)
    d_wire = dev(wire.reshape(-1)).view(n, stride)
    queue, qoffs, st, m = sk.ingest_wire_queue(d_wire, lens, flow, nflows, t, ctx=ctx)
    assert np.array_equal(st, status)
    ok = np.flatnonzero(status == 0)
    order = ok[np.argsort(flow[ok], kind="stable")]                     # by flow, ascending i within a flow
    assert m == len(ok) and queue.shape == (len(ok), 4 + t)
    assert np.array_equal(host(queue).reshape(len(ok), 4 + t), recs[order])
    assert np.array_equal(qoffs, np.concatenate([[0], np.cumsum(np.bincount(flow[ok], minlength=nflows))]).astype(np.uint64))
    # the statuses of the newest-only ingest, none superseded
    _, present, st1, acc = sk.ingest_wire(d_wire, lens, flow, nflows, t, ctx=ctx)
    assert np.array_equal(np.where(st1 == QK_WIRE_SUPERSEDED, 0, st1), st)
    assert acc == int((qoffs[1:] > qoffs[:-1]).sum())


def test_ingest_queue_errors_and_capacity(ctx):
    t, n, nflows = 8, 100, 9
    wire, lens, flow, status, recs = make_batch(t, n, nflows, 77)
    stride = wire.shape[1]
    d_wire, d_len, d_flow = dev(wire.reshape(-1)), dev(lens), dev(flow)
    f = lib().qk_u32_wire_ingest_queue_device
    acc = int((status == 0).sum())
    qoffs = np.full(nflows + 1, 0xEEEE, dtype=np.uint64)
    st = np.full(n, 0x7777, dtype=np.int32)
    m = C.c_size_t()
    d_q = torch.full((n * (4 + t),), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")

    def call(**over):
        a = dict(ctx=ctx.handle, wire=d_wire.data_ptr(), stride=stride, len=d_len.data_ptr(), flow=d_flow.data_ptr(), n=n, t=t,
                 nseg=nflows, q=d_q.data_ptr(), cap=n, qoffs=qoffs.ctypes.data_as(C.POINTER(C.c_uint64)),
                 st=st.ctypes.data_as(C.POINTER(C.c_int32)), m=C.byref(m))
        a.update(over)
        return f(*a.values(), None)
    # capacity: q_offsets, status and n_accepted written, the queue untouched
    assert call(cap=acc - 1) == QK_E_CAPACITY and m.value == acc
    assert np.array_equal(st, status) and qoffs[-1] == acc and qoffs[0] == 0
    assert np.all(host(d_q) == 0x5A5A5A5A)
    assert call(cap=acc) == 0 and m.value == acc
    first = host(d_q)[: acc * (4 + t)].copy()
    assert np.all(host(d_q)[acc * (4 + t):] == 0x5A5A5A5A)
    assert call() == 0 and np.array_equal(host(d_q)[: acc * (4 + t)], first)
    # a flow index out of range: before any output array is written
    far = flow.copy()
    far[n // 2] = nflows
    qoffs[:], st[:] = 0xEEEE, 0x7777
    d_q.fill_(0x5A5A5A5A)
    assert call(flow=dev(far).data_ptr()) == QK_E_INVAL
    assert np.all(qoffs == 0xEEEE) and np.all(st == 0x7777) and np.all(host(d_q) == 0x5A5A5A5A)
    assert call(ctx=None, t=0) == QK_E_INVAL and call(t=0) == QK_E_THRESHOLD and call(t=1025) == QK_E_THRESHOLD
    assert call(stride=0) == QK_E_INVAL and call(nseg=0) == QK_E_INVAL
    assert call(q=d_wire.data_ptr()) == QK_E_INVAL                     # the queue over an input
    for name in ("wire", "len", "flow", "q", "qoffs", "st", "m"):
        assert call(**{name: None}) == QK_E_INVAL, name
    assert call(q=st.ctypes.data_as(C.c_void_p)) == QK_E_INVAL          # host where device is required
    assert call(st=C.cast(d_len.data_ptr(), C.POINTER(C.c_int32))) == QK_E_INVAL     # device where host is required
    assert call(qoffs=C.cast(d_len.data_ptr(), C.POINTER(C.c_uint64))) == QK_E_INVAL
    assert call(n=0, wire=None, len=None, flow=None, nseg=0) == 0 and qoffs[0] == 0


# --------------------------------------------------------------- closed loop
def closed_loop(every, debounce=0.1, force_reset_at=None, seed=11):
    """64 flows, t = 8, f = 8: the proxy's DeviceFlowSnapshots emits each batch's
    datagrams, the sender's DeviceSenderLog takes them by on_wire; beside it one
    QuackReceiver per flow is fed the same quACKs one at a time.  Returns
    (resets fired on the device side, resets fired in the model, flows with
    more than t losses in one batch)."""
    t, f, nf, per = 8, 8, 64, 40
    rng = np.random.default_rng(seed)
    proxy = sk.DeviceFlowSnapshots(t, nf, f)
    snd = sk.DeviceSenderLog(t, nf, reset_debounce_s=debounce)
    rxs = [QuackReceiver(t, debounce) for _ in range(nf)]
    seq = 0
    dev_resets = model_resets = many = 0
    for rnd in range(4):
        n = nf * per
        flow = np.tile(np.arange(nf, dtype=np.uint32), per)            # round robin: position k of a flow is packet k
        idv = rng.integers(1 << 8, P - (1 << 8), size=n, dtype=np.uint64).astype(np.uint32)
        seqno = np.arange(seq, seq + n, dtype=np.uint32)
        seq += n
        snd.send(flow, seqno, idv)
        for g, s, v in zip(flow.tolist(), seqno.tolist(), idv.tolist()):
            rxs[g].on_send(s, v)
        # the drop: in every run of 8 packets of a flow at most 2 lost, never the run's last two.  An
        # interval of 8 received packets touches at most three runs (a run holds >= 6 received): <= 6 <= t
        # losses per interval, and up to 10 > t per batch of 40 packets
        k = np.arange(n) // nf
        lost = (rng.random(n) < 0.3) & (k % 8 < 6)
        run = (k // 8) * nf + flow
        for r in np.unique(run[lost]):
            idx = np.flatnonzero(lost & (run == r))
            lost[idx[2:]] = False
        if rnd == 0:
            lost[flow % 5 == 0] = False                                 # some flows without a loss
        many += int((np.bincount(flow[lost], minlength=nf) > t).sum())
        keep = ~lost
        fl, wire, lens, recs = proxy.insert(flow[keep], idv[keep])
        if force_reset_at is not None and rnd == force_reset_at:
            # a quACK whose last_value the sender never sent, in the middle of flow 3's queue
            rows = torch.nonzero(fl == 3).flatten().tolist()
            r = rows[len(rows) // 2]
            q = sk.PowerSumQuackU32._from_record(host(recs).reshape(-1, 4 + t)[r].tobytes(), t)
            q.insert(0xDEADBEEF)
            img = np.frombuffer(q.serialize(), dtype=np.uint8)
            wire[r, :len(img)] = torch.from_numpy(img.copy()).to(wire.device)
            recs[r] = torch.from_numpy(q._record_i32().copy()).to(recs.device)
        now = 1.0 + rnd
        step, status = snd.on_wire(wire, lens, fl, now=now, every=every)
        assert np.all((status == 0) | (status == QK_WIRE_SUPERSEDED))
        dev_resets += int(step.send_reset.sum())
        # the model: every datagram in arrival order (every), or each flow's newest
        rows = host(recs).reshape(-1, 4 + t)
        flh = host(fl).tolist()
        want = [[] for _ in range(nf)]
        newest = {g: r for r, g in enumerate(flh)}
        for r, g in enumerate(flh):
            if every or newest[g] == r:
                act = rxs[g].on_quack(sk.PowerSumQuackU32._from_record(rows[r].tobytes(), t), now)
                want[g] += act.retransmit
                model_resets += act.send_reset
        assert step.retransmit == want
        snd.flush()
        mine = host(snd.mine).reshape(nf, 4 + t)
        log, sq = host(snd.log), host(snd.seqnos)
        for g in range(nf):
            a, b = int(snd.offsets[g]), int(snd.offsets[g + 1])
            assert list(zip(sq[a:b].tolist(), log[a:b].tolist())) == rxs[g].seqno_ids, g
            assert mine[g].tobytes() == rxs[g].my_quack._buf.raw, g
            lr = rxs[g].last_quack_reset
            assert (np.isnan(snd.last_quack_reset[g]) and lr is None) or snd.last_quack_reset[g] == lr, g
    return dev_resets, model_resets, many


def test_closed_loop_every_quack_recovers_all_losses():
    dev_resets, model_resets, many = closed_loop(True)
    assert dev_resets == 0 and model_resets == 0 and many > 0


def test_closed_loop_newest_only_resets_on_the_same_traffic():
    dev_resets, model_resets, many = closed_loop(False)
    assert many > 0 and model_resets > 0 and dev_resets == model_resets


def test_closed_loop_held_back_reset_steps_the_tail():
    """The forced reset fires in round 1 (nothing is debounced yet) and is held
    back in round 2 by a large debounce: the flow's tail goes through a second
    step, from the quACK the prefix insert left."""
    for force_at in (1,):
        dev_resets, model_resets, _ = closed_loop(True, debounce=100.0, force_reset_at=force_at)
        assert dev_resets == model_resets == 1
    # held back: a receiver that has reset before, inside the debounce
    t = 8
    rng = random.Random(3)
    f = sm.queued_flow(rng, t, 40, [9, 19, 29], [3, 14, 25], history=0)
    f.queue[0].insert(0xDEADBEEF)              # the flow's first quACK: no ADVANCED before it clears the debounce
    snd = sk.DeviceSenderLog(t, 2, reset_debounce_s=100.0)
    snd.send(np.ones(40, dtype=np.uint32), np.arange(40, dtype=np.uint32), np.array(f.seg, dtype=np.uint32))
    snd.last_quack_reset[1] = 0.5
    sends = list(enumerate(f.seg))
    rx = QuackReceiver(t, 100.0)
    for s, v in sends:
        rx.on_send(s, v)
    rx.last_quack_reset = 0.5
    want, fired = [], 0
    for q in f.queue:
        act = rx.on_quack(sk.PowerSumQuackU32._from_record(sm.record(q).tobytes(), t), 1.0)
        want += act.retransmit
        fired += act.send_reset
    assert fired == 0 and len(want) == 3       # held back; the tail recovers positions 3, 14 and 25
    queue = [sk.PowerSumQuackU32._from_record(sm.record(q).tobytes(), t) for q in f.queue]
    step = snd.on_quack_queue(queue, [0, 0, 3], now=1.0)
    assert step.retransmit == [[], want] and want and not step.send_reset.any() and step.reset_reason[1]
    snd.flush()
    a, b = int(snd.offsets[1]), int(snd.offsets[2])
    assert list(zip(host(snd.seqnos)[a:b].tolist(), host(snd.log)[a:b].tolist())) == rx.seqno_ids
    assert host(snd.mine).reshape(2, 4 + t)[1].tobytes() == rx.my_quack._buf.raw
    assert (np.isnan(snd.last_quack_reset[1]) and rx.last_quack_reset is None) or snd.last_quack_reset[1] == rx.last_quack_reset
