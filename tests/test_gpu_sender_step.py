"""Batched sender step (qk_u32_sender_step_segments_device) and log drain
(qk_u32_log_drain_segments_device) on the GPU, bit for bit against a per-flow
restatement of media_client.rs:233-322 on the oracle's arithmetic: action,
drain, the missing positions and every word of mine_out.  The oracle's reset
debounce is held shut, so a reset keeps the prefix insert (mine1)."""
import ctypes as C
import random

import numpy as np
import pytest

import sidekick_amd as sk
from sidekick_amd import _lib
from sidekick_amd._lib import (QK_E_CAPACITY, QK_E_INVAL, QK_E_MISMATCH, SND_ADVANCED, SND_IDLE, SND_RESET_EXCEEDS,
                               SND_RESET_REORDERED, SND_RESET_RETX, lib)
from sidekick_amd.receiver import QuackReceiver
from oracle import quack_oracle as qo

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

P = qo.P32
M32 = 0xFFFFFFFF
THRESHOLDS = (1, 8, 32, 33, 80, 129)
LENGTHS = (0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 4097)


# ------------------------------------------------------------------ oracle
def insert_all(q, ids):
    """q.insert(id) for every id (long runs through the oracle's batch encode)."""
    ids = [int(v) for v in ids]
    if len(ids) <= 32:
        for v in ids:
            q.insert(v)
        return
    s = qo.encode_u32_np(np.array(ids, dtype=np.uint32), q.threshold)
    q.power_sums = [(a + int(b)) % P for a, b in zip(q.power_sums, s)]
    q.count = (q.count + len(ids)) & M32
    q.last_value = ids[-1]


def oracle_step(mine, peer, seg, t):
    """media_client.rs:233-322 for one flow: (mine_out, action, drain, missing
    positions).  peer None: no quACK."""
    if peer is None or peer.last_value == mine.last_value:                       # :233
        return mine.clone(), SND_IDLE, 0, []
    idx = None
    if peer.last_value is not None:
        idx = next((i for i, v in enumerate(seg) if v == peer.last_value), None)  # :240-246
    m1 = mine.clone()
    if idx is not None:
        insert_all(m1, seg[: idx + 1])                                            # :247-252
    bits = 0
    if idx is None:
        bits |= SND_RESET_REORDERED                                               # :258
    if m1.count < peer.count:
        bits |= SND_RESET_RETX                                                    # :259
    if m1.count > (peer.count + t) & M32:
        bits |= SND_RESET_EXCEEDS                                                 # :260
    if bits:
        return m1, bits, 0, []
    diff = m1.clone()
    diff.sub_assign(peer)                                                         # :295-296
    if diff.count == 0:
        return m1, SND_ADVANCED, idx + 1, []
    c = diff.to_coeffs()                                                          # :304
    stop = next(i for i, v in enumerate(seg) if v == diff.last_value)             # :307-309
    miss = qo.root_test_u32_np(c, np.array(seg[:stop], dtype=np.uint32)).tolist() if stop else []
    for i in miss:
        m1.remove(seg[i])                                                         # :319
    return m1, SND_ADVANCED, idx + 1, miss


def record(q, t):
    r = np.zeros(4 + t, dtype=np.uint32)
    r[0], r[1] = t, q.count
    r[2], r[3] = (0, 0) if q.last_value is None else (1, q.last_value)
    r[4:] = q.power_sums
    return r


# --------------------------------------------------------------- scenarios
class Flow:
    def __init__(self, mine, peer, seg, present=True):
        self.mine, self.peer, self.seg, self.present = mine, peer, [int(v) for v in seg], present


def fresh_ids(rng, n):
    """n ids below p that are not tiny (0 and the values near p are placed by hand)."""
    return [rng.randrange(1 << 8, P - (1 << 8)) for _ in range(n)]


def advance_flow(rng, t, length, stop, lost, history=3, extra_peer=0, seg=None):
    """A flow whose peer received history + seg[..=stop] without the positions
    in `lost` (all < stop) plus `extra_peer` ids of its own."""
    seg = fresh_ids(rng, length) if seg is None else seg
    mine, peer = qo.OracleQuack(t), qo.OracleQuack(t)
    hist = fresh_ids(rng, history)
    insert_all(mine, hist)
    insert_all(peer, hist + fresh_ids(rng, extra_peer))
    lost = set(lost)
    insert_all(peer, [v for i, v in enumerate(seg[: stop + 1]) if i not in lost])
    return Flow(mine, peer, seg)


def pick_lost(rng, stop, k):
    return rng.sample(range(stop), k) if k <= stop else None


def build_flows(t, seed):
    rng = random.Random(seed)
    flows = []
    # every length, its stop at the last entry, with 0, 1, T and T + 1 losses where they fit
    for n in LENGTHS:
        if n == 0:
            flows.append(Flow(qo.OracleQuack(t), qo.OracleQuack(t), []))           # both empty: IDLE
            f = advance_flow(rng, t, 0, -1, [])
            f.peer.insert(rng.randrange(1 << 8, P))                                # a last value, no log: REORDERED
            flows.append(f)
            continue
        for k in (0, 1, t, t + 1):
            lost = pick_lost(rng, n - 1, k)
            if lost is not None:
                flows.append(advance_flow(rng, t, n, n - 1, lost))
    # more short segments in a row than one packed work item holds (256, or 8192 / T)
    for i in range(300):
        n = i % 4
        if n == 0:
            flows.append(Flow(qo.OracleQuack(t), qo.OracleQuack(t), []))
        else:
            stop = rng.randrange(n)
            flows.append(advance_flow(rng, t, n, stop, pick_lost(rng, stop, min(stop, t, i % 2)) or []))
    # the stop in a later 2048-slice than some hits, hits in the stop's slice too, entries after the stop
    flows.append(advance_flow(rng, t, 4097 + 600, 4096 + 7, [5, 2050, 4097, 4100][: min(t, 4)]))
    flows.append(advance_flow(rng, t, 4097, 100, [7][: min(t, 1)]))                # stop in the first slice
    flows.append(advance_flow(rng, t, 6000, 2048, [0, 2047][: min(t, 2)]))         # stop opens the second slice
    # reset bits
    flows.append(advance_flow(rng, t, 70, 50, [3], extra_peer=3))                  # peer ahead: RETX
    f = advance_flow(rng, t, 70, 50, [])
    f.peer.insert(0xDEADBEEF)                                                      # last value not in the log
    flows.append(f)                                                                #   REORDERED | RETX
    f = advance_flow(rng, t, 10, 5, [], history=t + 5)
    f.peer = qo.OracleQuack(t)
    f.peer.insert(0xDEADBEEF)
    flows.append(f)                                                                # REORDERED | EXCEEDS
    hist = fresh_ids(rng, 3)
    f = Flow(qo.OracleQuack(t), qo.OracleQuack(t), fresh_ids(rng, 10))
    insert_all(f.mine, hist)
    insert_all(f.peer, hist[:2])
    flows.append(f)                                                                # REORDERED alone
    # a peer without a last value: mine with one -> REORDERED, without -> IDLE
    f = advance_flow(rng, t, 10, 5, [])
    f.peer = qo.OracleQuack(t)
    flows.append(f)
    flows.append(Flow(qo.OracleQuack(t), qo.OracleQuack(t), fresh_ids(rng, 10)))
    # no-ops: absent, unchanged last value
    f = advance_flow(rng, t, 40, 20, [4])
    f.present = False
    flows.append(f)
    f = advance_flow(rng, t, 40, 20, [])
    f.peer = f.mine.clone()
    flows.append(f)
    # duplicates: a missing id twice in the prefix; the last value again after the stop
    seg = fresh_ids(rng, 60)
    seg[9] = seg[4]
    flows.append(advance_flow(rng, t, 60, 40, [4, 9], seg=seg))
    seg = fresh_ids(rng, 60)
    seg[55] = seg[40]
    flows.append(advance_flow(rng, t, 60, 40, [6], seg=seg))
    # unreduced ids: raw equality (3 is not p + 3), hits on id mod p (1 and p + 1), 0 and p together
    seg = fresh_ids(rng, 50)
    seg[2], seg[5], seg[8], seg[12], seg[20], seg[30], seg[31] = 3, 1, P + 1, 0, P, P + 3, 3
    flows.append(advance_flow(rng, t, 50, 30, [8], seg=seg))
    flows.append(advance_flow(rng, t, 50, 30, [12], seg=list(seg)))
    seg = list(seg)
    seg[2] = fresh_ids(rng, 1)[0]                                                  # the first raw 3 is now at 31
    flows.append(advance_flow(rng, t, 50, 31, [5, 20][: min(t, 2)], seg=seg))
    return flows


def run_step(flows, t):
    """(step result, log tensor, offsets) of one sender_step call over `flows`."""
    offs = np.zeros(len(flows) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(f.seg) for f in flows])
    log = np.array([v for f in flows for v in f.seg], dtype=np.uint32)
    d_log = torch.from_numpy(log.view(np.int32)).cuda()
    mine = torch.from_numpy(np.stack([record(f.mine, t) for f in flows]).view(np.int32)).cuda()
    peer = torch.from_numpy(np.stack([record(f.peer, t) for f in flows]).view(np.int32)).cuda()
    present = None if all(f.present for f in flows) else [f.present for f in flows]
    return sk.sender_step(mine, peer, d_log, offs, present=present), d_log, offs


def check_against_oracle(flows, t, res):
    got = res.mine_out.cpu().numpy().view(np.uint32)
    seen = set()
    for g, f in enumerate(flows):
        m, act, dr, miss = oracle_step(f.mine, f.peer if f.present else None, f.seg, t)
        assert int(res.action[g]) == act, (g, int(res.action[g]), act)
        assert int(res.drain[g]) == dr, g
        assert res.missing[g] == miss, g
        assert np.array_equal(got[g], record(m, t)), g
        seen.add(act)
    return seen


# ------------------------------------------------------------------- tests
@pytest.mark.parametrize("t", THRESHOLDS)
def test_matches_the_per_flow_oracle(t):
    flows = build_flows(t, 0x5E9D0000 + t)
    res, _, _ = run_step(flows, t)
    seen = check_against_oracle(flows, t, res)
    assert {SND_IDLE, SND_ADVANCED, SND_RESET_REORDERED, SND_RESET_RETX, SND_RESET_EXCEEDS,
            SND_RESET_REORDERED | SND_RESET_RETX, SND_RESET_REORDERED | SND_RESET_EXCEEDS} <= seen
    assert sum(len(m) for m in res.missing) > 0


def test_duplicates_and_unreduced_ids_are_what_the_scenarios_say():
    """The scenarios of build_flows do exercise what their comments claim."""
    t = 8
    flows = build_flows(t, 0x5E9D0000 + t)
    res, _, _ = run_step(flows, t)
    dup, dup_last, raw, zero_p, both = res.missing[-5:]
    assert dup == [4, 9]                  # two hits, two removes
    assert dup_last == [6] and int(res.drain[-4]) == 41
    assert raw == [5, 8] and int(res.drain[-3]) == 31      # stop at p + 3, not at the 3 before it
    assert zero_p == [12, 20]
    assert int(res.drain[-1]) == 32 and both == [5, 8, 12, 20]


def test_count_wrap():
    """peer.count = 2^32 - 3 with T = 8: peer.count + T wraps, so RESET_EXCEEDS, as
    receiver.py:85 gives on the CPU; counts carried over near 2^32 elsewhere."""
    t, rng = 8, random.Random(77)
    flows = []
    for peer_count in (M32 - 2, M32 - 2 - t, M32 - 8, 5):
        for lost in ([], [3, 9]):
            f = advance_flow(rng, t, 30, 20, lost)
            shift = (peer_count - f.peer.count) & M32
            f.peer.count = peer_count
            f.mine.count = (f.mine.count + shift) & M32
            flows.append(f)
    f = advance_flow(rng, t, 30, 20, [])           # mine1.count wraps past 2^32, the peer's does not: RETX
    f.mine.count, f.peer.count = M32 - 10, M32 - 20
    flows.append(f)
    res, _, _ = run_step(flows, t)
    check_against_oracle(flows, t, res)
    assert int(res.action[0]) == SND_RESET_EXCEEDS and int(res.action[1]) == SND_RESET_EXCEEDS
    assert int(res.action[2]) == SND_ADVANCED and res.missing[3] == [3, 9]
    assert int(res.action[-1]) == SND_RESET_RETX


def raw_step(ctx, mine, peer, d_log, offs, t, cap, mine_out=None, action=None):
    nseg = len(offs) - 1
    mine_out = torch.empty_like(peer) if mine_out is None else mine_out
    act = np.zeros(max(nseg, 1), dtype=np.uint8)
    drain = np.zeros(max(nseg, 1), dtype=np.uint64)
    hits = np.full(max(cap, 1), M32, dtype=np.uint64)
    hoffs = np.full(nseg + 1, 99, dtype=np.uint64)
    nh = C.c_size_t(12345)
    u64 = C.POINTER(C.c_uint64)
    rc = lib().qk_u32_sender_step_segments_device(
        ctx.handle, mine if isinstance(mine, int) else mine.data_ptr(), peer.data_ptr(), None, d_log.data_ptr(),
        offs.ctypes.data_as(u64), nseg, t, mine_out if isinstance(mine_out, int) else mine_out.data_ptr(),
        C.cast(action, C.POINTER(C.c_uint8)) if action is not None else act.ctypes.data_as(C.POINTER(C.c_uint8)),
        drain.ctypes.data_as(u64), hits.ctypes.data_as(u64), cap, hoffs.ctypes.data_as(u64), C.byref(nh),
        torch.cuda.current_stream().cuda_stream)
    return rc, mine_out, act, drain, hits, hoffs, nh.value


def small_batch(t=8):
    rng = random.Random(5)
    flows = [advance_flow(rng, t, 40 + i, 30, rng.sample(range(30), i % 4)) for i in range(12)]
    offs = np.zeros(len(flows) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(f.seg) for f in flows])
    d_log = torch.from_numpy(np.array([v for f in flows for v in f.seg], dtype=np.uint32).view(np.int32)).cuda()
    mine = torch.from_numpy(np.stack([record(f.mine, t) for f in flows]).view(np.int32)).cuda()
    peer = torch.from_numpy(np.stack([record(f.peer, t) for f in flows]).view(np.int32)).cuda()
    return flows, mine, peer, d_log, offs


def test_capacity_reports_the_total_and_leaves_the_other_outputs_valid():
    t = 8
    ctx = sk.get_context(0)
    flows, mine, peer, d_log, offs = small_batch(t)
    rc, mo, act, drain, hits, hoffs, total = raw_step(ctx, mine, peer, d_log, offs, t, 1024)
    assert rc == 0 and total == sum(i % 4 for i in range(12)) == int(hoffs[-1])
    for cap in (0, total - 1):
        rc2, mo2, act2, drain2, _, hoffs2, nh2 = raw_step(ctx, mine, peer, d_log, offs, t, cap)
        assert rc2 == QK_E_CAPACITY and nh2 == total
        assert torch.equal(mo2, mo) and np.array_equal(act2, act) and np.array_equal(drain2, drain)
        assert np.array_equal(hoffs2, hoffs)
    rc3, mo3, act3, drain3, hits3, hoffs3, nh3 = raw_step(ctx, mine, peer, d_log, offs, t, total)
    assert rc3 == 0 and nh3 == total and torch.equal(mo3, mo) and np.array_equal(hits3[:total], hits[:total])
    assert np.array_equal(act3, act) and np.array_equal(drain3, drain) and np.array_equal(hoffs3, hoffs)


def test_argument_errors():
    t = 8
    ctx = sk.get_context(0)
    flows, mine, peer, d_log, offs = small_batch(t)
    # nseg == 0
    rc, _, _, _, _, hoffs, nh = raw_step(ctx, mine, peer, d_log, offs[:1], t, 4)
    assert rc == 0 and int(hoffs[0]) == 0 and nh == 0
    # thresholds
    assert raw_step(ctx, mine, peer, d_log, offs, 0, 4)[0] == _lib.QK_E_THRESHOLD
    assert raw_step(ctx, mine, peer, d_log, offs, 1025, 4)[0] == _lib.QK_E_THRESHOLD
    # a host pointer where a device one is required, and the reverse
    host = np.ascontiguousarray(mine.cpu().numpy())
    assert raw_step(ctx, host.ctypes.data, peer, d_log, offs, t, 4)[0] == QK_E_INVAL
    assert raw_step(ctx, mine, peer, d_log, offs, t, 4, mine_out=host.ctypes.data)[0] == QK_E_INVAL
    d_act = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert raw_step(ctx, mine, peer, d_log, offs, t, 4, action=d_act.data_ptr())[0] == QK_E_INVAL
    # decreasing offsets
    bad = offs.copy()
    bad[3] = bad[2] - 1
    assert raw_step(ctx, mine, peer, d_log, bad, t, 4)[0] == QK_E_INVAL
    # mine_out overlapping an input
    assert raw_step(ctx, mine, peer, d_log, offs, t, 4, mine_out=mine)[0] == QK_E_INVAL
    assert raw_step(ctx, mine, peer, d_log, offs, t, 4, mine_out=peer)[0] == QK_E_INVAL
    # a record with a foreign threshold
    for which in (0, 1):
        pair = [mine.clone(), peer.clone()]
        pair[which][5, 0] = t + 1
        assert raw_step(ctx, pair[0], pair[1], d_log, offs, t, 1024)[0] == QK_E_MISMATCH
    # the wrapper takes host sketches too
    q_mine = [sk.PowerSumQuackU32(t) for _ in flows]
    q_peer = [sk.PowerSumQuackU32(t) for _ in flows]
    for f, a, b in zip(flows, q_mine, q_peer):
        np.frombuffer(a._buf, dtype=np.uint32)[:] = record(f.mine, t)
        np.frombuffer(b._buf, dtype=np.uint32)[:] = record(f.peer, t)
    res = sk.sender_step(q_mine, q_peer, d_log.cpu().numpy().view(np.uint32), offs)
    check_against_oracle(flows, t, res)


# ------------------------------------------------------------------- drain
def drain_case(lens, first, drains, with_aux, seed):
    rng = np.random.default_rng(seed)
    offs = np.zeros(len(lens) + 1, dtype=np.uint64)
    offs[0] = first
    offs[1:] = first + np.cumsum(lens)
    n = int(offs[-1]) + 5
    log = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    aux = np.arange(n, dtype=np.uint32) * 3 + 1
    d_log = torch.from_numpy(log.view(np.int32)).cuda()
    d_aux = torch.from_numpy(aux.view(np.int32)).cuda()
    out = sk.drain_segments(d_log, offs, drains, aux=d_aux if with_aux else None)
    tails = [np.arange(int(offs[g]) + int(drains[g]), int(offs[g + 1])) for g in range(len(lens))]
    idx = np.concatenate(tails) if tails else np.zeros(0, dtype=np.int64)
    want_offs = np.concatenate([[0], np.cumsum([len(x) for x in tails])]).astype(np.uint64)
    assert np.array_equal(out[1], want_offs)
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32), log[idx])
    if with_aux:
        assert np.array_equal(out[2].cpu().numpy().view(np.uint32), aux[idx])
    else:
        assert len(out) == 2


@pytest.mark.parametrize("first", (0, 1, 3))
@pytest.mark.parametrize("with_aux", (False, True))
def test_drain_segments_equals_the_concatenated_tails(first, with_aux):
    lens = np.array([0, 1, 2, 5, 63, 64, 65, 2047, 2048, 2049, 4097, 7, 0, 4100, 3], dtype=np.uint64)
    rng = np.random.default_rng(11 + first)
    mixed = np.array([rng.integers(0, n + 1) for n in lens], dtype=np.uint64)
    for drains in (np.zeros_like(lens), lens.copy(), mixed):
        drain_case(lens, first, drains, with_aux, 3)


def test_drain_segments_errors():
    ctx = sk.get_context(0)
    d_log = torch.arange(100, dtype=torch.int32, device="cuda")
    out = torch.empty(100, dtype=torch.int32, device="cuda")
    offs = np.array([0, 40, 100], dtype=np.uint64)
    offs_out = np.zeros(3, dtype=np.uint64)
    u64 = C.POINTER(C.c_uint64)
    f = lib().qk_u32_log_drain_segments_device

    def call(drain, src=d_log.data_ptr(), dst=out.data_ptr(), cap=100, aux=None, aux_out=None):
        dr = np.array(drain, dtype=np.uint64)
        return f(ctx.handle, src, aux, offs.ctypes.data_as(u64), dr.ctypes.data_as(u64), 2, dst, aux_out, cap,
                 offs_out.ctypes.data_as(u64), None)

    assert call([41, 0]) == QK_E_INVAL                               # longer than the segment
    assert call([10, 20], cap=69) == QK_E_CAPACITY and offs_out.tolist() == [0, 30, 70]
    assert call([10, 20], cap=70) == 0
    assert call([10, 20], dst=d_log.data_ptr() + 4 * 50) == QK_E_INVAL   # output inside the input
    assert call([10, 20], aux=d_log.data_ptr()) == QK_E_INVAL           # aux without aux_out
    host = np.zeros(100, dtype=np.uint32)
    assert call([10, 20], dst=host.ctypes.data) == QK_E_INVAL
    assert call([10, 20], src=host.ctypes.data) == QK_E_INVAL
    assert f(ctx.handle, None, None, offs.ctypes.data_as(u64), None, 0, None, None, 0, offs_out.ctypes.data_as(u64),
             None) == 0 and offs_out[0] == 0


# -------------------------------------------------------------- closed loop
def test_closed_loop_against_one_receiver_per_flow():
    """64 flows, T = 16, 40 rounds of send -> lossy proxy (now and then a quACK
    whose last value the sender never logged) -> sender_step -> drain_segments,
    every round compared with one QuackReceiver per flow on its host path."""
    t, nflow, rounds = 16, 64, 40
    rnd = random.Random(0xC105ED)
    rx = [QuackReceiver(t, reset_debounce_s=0.1, batch_min=1 << 30) for _ in range(nflow)]
    proxy = [sk.PowerSumQuackU32(t) for _ in range(nflow)]
    ids = [[] for _ in range(nflow)]      # the device log's content per flow, as the test tracks it
    seqs = [[] for _ in range(nflow)]
    resend = [[] for _ in range(nflow)]
    mine = torch.from_numpy(np.stack([record(qo.OracleQuack(t), t)] * nflow).view(np.int32)).cuda()
    fresh = mine[0].clone()
    seq = 0
    stats = {"adv": 0, "reset": 0, "idle": 0, "retx": 0}
    for rno in range(rounds):
        now = float(rno)                  # past every debounce: a reset condition always fires
        for g in range(nflow):
            new = resend[g] + ([] if rnd.random() < 0.1 else [None] * rnd.randrange(0, 301))
            resend[g] = []
            for _ in new:
                seq += 1
                v = rnd.getrandbits(32)
                rx[g].on_send(seq, v)
                ids[g].append(v)
                seqs[g].append(seq)
                if rnd.random() >= 0.01:
                    proxy[g].insert(v)
        offs = np.zeros(nflow + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(x) for x in ids])
        d_log = torch.from_numpy(np.array(sum(ids, []), dtype=np.uint32).view(np.int32)).cuda()
        d_seq = torch.from_numpy(np.array(sum(seqs, []), dtype=np.uint32).view(np.int32)).cuda()
        present = [rnd.random() < 0.9 for _ in range(nflow)]
        quacks = []
        for g in range(nflow):
            q = proxy[g].clone()
            if rnd.random() < 0.03:
                q.insert(0xDEADBEEF)      # reordering: a last value that is not in the log
            quacks.append(q)
        res = sk.sender_step(mine, quacks, d_log, offs, present=present)
        mine = res.mine_out
        seq_host = d_seq.cpu().numpy().view(np.uint32)
        drain = res.drain.copy()
        for g in range(nflow):
            a = int(res.action[g])
            if not present[g]:
                assert a == SND_IDLE and res.missing[g] == []
                continue
            want = rx[g].on_quack(quacks[g], now)
            bits = sum(b for b, on in zip((SND_RESET_REORDERED, SND_RESET_RETX, SND_RESET_EXCEEDS),
                                          want.reset_reason or (0, 0, 0)) if on)
            assert (a & ~SND_ADVANCED) == bits, (rno, g)
            retx = [int(seq_host[int(offs[g]) + p]) for p in res.missing[g]]
            assert retx == want.retransmit, (rno, g)
            if bits:                      # the caller's part of a reset (media_client.rs:267-276)
                assert want.send_reset
                mine[g] = fresh
                drain[g] = offs[g + 1] - offs[g]
                proxy[g] = sk.PowerSumQuackU32(t)
                stats["reset"] += 1
            else:
                stats["adv" if a == SND_ADVANCED else "idle"] += 1
            resend[g] = [None] * len(retx)
            stats["retx"] += len(retx)
        d_log2, offs2, d_seq2 = sk.drain_segments(d_log, offs, drain, aux=d_seq)
        log2, seq2 = d_log2.cpu().numpy().view(np.uint32), d_seq2.cpu().numpy().view(np.uint32)
        got_mine = mine.cpu().numpy().view(np.uint32)
        for g in range(nflow):
            a, b = int(offs2[g]), int(offs2[g + 1])
            ids[g], seqs[g] = log2[a:b].tolist(), seq2[a:b].tolist()
            assert list(zip(seqs[g], ids[g])) == rx[g].seqno_ids, (rno, g)
            assert np.array_equal(got_mine[g], np.frombuffer(rx[g].my_quack._buf, dtype=np.uint32)), (rno, g)
    # the simulation itself went through every kind of round
    assert stats["adv"] > 1000 and stats["reset"] > 20 and stats["idle"] > 20 and stats["retx"] > 1000, stats
