"""The reference's sender loop over a QUEUE of quACKs per flow, on the oracle's
objects, for the tests of qk_u32_sender_steps_segments_device and
qk_u32_wire_ingest_queue_device (a helper module, as snapshot_model.py is).

media_client.rs:223-323 handles one datagram per loop turn: `step` is one turn
for one flow (the per-flow restatement the single sender step is tested
against), `steps_flow` the turns of a flow's queue one after the other on a log
that every ADVANCED turn shortens, stopping at the first reset (the debounce is
the caller's), `steps` that for a batch of flows in the layout the device call
returns.
"""
import numpy as np

from oracle import quack_oracle as qo

P = qo.P32
M32 = 0xFFFFFFFF
SND_IDLE, SND_ADVANCED, SND_RESET_REORDERED, SND_RESET_RETX, SND_RESET_EXCEEDS, SND_UNSTEPPED = 0, 1, 2, 4, 8, 16


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


def step(mine, peer, seg, t):
    """media_client.rs:233-322 for one flow and one quACK: (mine_out, action,
    drain, missing positions in seg)."""
    if peer.last_value == mine.last_value:                                        # :233
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


def steps_flow(mine, queue, seg, t):
    """The loop of the issue for one flow: (mine_out, actions, drains, hits per
    quACK as positions in seg, stepped, drain)."""
    m, b = mine.clone(), 0
    k = len(queue)
    actions, drains, hits = [SND_UNSTEPPED] * k, [0] * k, [[] for _ in range(k)]
    stepped = 0
    for j, peer in enumerate(queue):
        m, action, d, missing = step(m, peer, seg[b:], t)
        actions[j], drains[j], hits[j] = action, d, [p + b for p in missing]
        stepped = j + 1
        if action & (SND_RESET_REORDERED | SND_RESET_RETX | SND_RESET_EXCEEDS):
            break
        b += d
    return m, actions, drains, hits, stepped, b


def record(q, t=None):
    t = q.threshold if t is None else t
    r = np.zeros(4 + t, dtype=np.uint32)
    r[0], r[1] = t, q.count
    r[2], r[3] = (0, 0) if q.last_value is None else (1, q.last_value)
    r[4:] = q.power_sums
    return r


class Flow:
    """A flow of a scenario: my quACK, the queued quACKs in arrival order, the log."""
    def __init__(self, mine, queue, seg):
        self.mine, self.queue, self.seg = mine, list(queue), [int(v) for v in seg]


def steps(flows, t):
    """The device call's outputs for a batch of flows, as numpy arrays: mine_out
    [nseg, 4 + t], q_action, q_drain, stepped, drain, hit_offsets [nq + 1],
    hits (global positions into the concatenated log)."""
    mine_out, q_action, q_drain, stepped, drain, counts, hits = [], [], [], [], [], [], []
    at = 0
    for f in flows:
        m, a, d, h, s, b = steps_flow(f.mine, f.queue, f.seg, t)
        mine_out.append(record(m, t))
        q_action += a
        q_drain += d
        stepped.append(s)
        drain.append(b)
        for hq in h:
            counts.append(len(hq))
            hits += [p + at for p in hq]
        at += len(f.seg)
    return dict(mine_out=np.array(mine_out, dtype=np.uint32).reshape(len(flows), 4 + t),
                q_action=np.array(q_action, dtype=np.uint8), q_drain=np.array(q_drain, dtype=np.uint64),
                stepped=np.array(stepped, dtype=np.uint32), drain=np.array(drain, dtype=np.uint64),
                hit_offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64),
                hits=np.array(hits, dtype=np.uint64))


def layout(flows, t):
    """(mine [nseg, 4 + t], queue [nq, 4 + t], q_offsets, log, offsets) of a batch of flows."""
    mine = np.array([record(f.mine, t) for f in flows], dtype=np.uint32).reshape(len(flows), 4 + t)
    queue = np.array([record(q, t) for f in flows for q in f.queue], dtype=np.uint32).reshape(-1, 4 + t)
    q_offsets = np.concatenate([[0], np.cumsum([len(f.queue) for f in flows])]).astype(np.uint64)
    log = np.array([v for f in flows for v in f.seg], dtype=np.uint32)
    offsets = np.concatenate([[0], np.cumsum([len(f.seg) for f in flows])]).astype(np.uint64)
    return mine, queue, q_offsets, log, offsets


def peer_after(history, received, t):
    """The proxy's quACK after `history` and then `received`, in order."""
    q = qo.OracleQuack(t)
    insert_all(q, history)
    insert_all(q, received)
    return q


def queued_flow(rng, t, length, stops, lost, history=3, seg=None):
    """A flow whose proxy emitted a quACK after each position in `stops`
    (ascending), having received history + the log up to there without the
    positions in `lost`."""
    seg = [rng.randrange(1 << 8, P - (1 << 8)) for _ in range(length)] if seg is None else list(seg)
    hist = [rng.randrange(1 << 8, P - (1 << 8)) for _ in range(history)]
    mine = qo.OracleQuack(t)
    insert_all(mine, hist)
    lost = set(lost)
    queue = [peer_after(hist, [v for i, v in enumerate(seg[: s + 1]) if i not in lost], t) for s in stops]
    return Flow(mine, queue, seg)


# ---- the protocol case: 64 packets, t = 8, f = 8, 16 losses, at most 8 per
# interval of 8 received packets, never the packet that triggers a quACK
CASE_T, CASE_F, CASE_N = 8, 8, 64
CASE_LOST = [1, 2, 3, 12, 13, 22, 23, 24, 33, 34, 43, 44, 45, 54, 55, 56]


def case_ids():
    return ((np.arange(CASE_N, dtype=np.uint64) * 2654435761 % (1 << 32) + 17).astype(np.uint32) | np.uint32(1)).tolist()


def case_quacks():
    """The quACKs the proxy sends at f = 8 for the case's received packets, and the end-of-batch one."""
    q = qo.OracleQuack(CASE_T)
    sent = []
    for s, v in enumerate(case_ids()):
        if s in CASE_LOST:
            continue
        q.insert(int(v))
        if q.count % CASE_F == 0:
            sent.append(q.clone())
    return sent, q.clone()


def run_case(queue):
    """steps_flow on the case's log for `queue`: (lost positions found, resets)."""
    _, actions, _, hits, _, _ = steps_flow(qo.OracleQuack(CASE_T), queue, case_ids(), CASE_T)
    resets = sum(1 for a in actions if a & (SND_RESET_REORDERED | SND_RESET_RETX | SND_RESET_EXCEEDS))
    return [p for h in hits for p in h], resets


def receiver_run(threshold, debounce, sends, queue, now):
    """A QuackReceiver given `sends` [(seqno, id)] and then the quACKs of
    `queue` (oracle objects) one after the other with the same `now`: (receiver,
    retransmitted seqnos, resets fired, reasons seen)."""
    from sidekick_amd import PowerSumQuackU32
    from sidekick_amd.receiver import QuackReceiver
    rx = QuackReceiver(threshold, debounce)
    for s, v in sends:
        rx.on_send(s, v)
    retx, fired, reasons = [], 0, 0
    for q in queue:
        act = rx.on_quack(PowerSumQuackU32._from_record(record(q).tobytes(), threshold), now)
        retx += act.retransmit
        fired += act.send_reset
        reasons += bool(act.reset_reason)
    return rx, retx, fired, reasons
