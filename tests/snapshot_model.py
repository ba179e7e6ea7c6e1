"""The reference's per-flow snapshot loop over the oracle, for the snapshot
tests (a helper module, as u64_rare.py is).

sidekick_multi.rs:271-283 restated literally: one insert per packet in arrival
order, and a clone of the flow's quACK whenever the count it reaches is a
multiple of frequency_pkts:

    let quack = sc.insert(addr_key, id);
    if quack.count() % frequency_pkts == 0 { bincode::serialize(&quack) ... }

The count is the reference's wrapping u32, so a count that wraps to 0 triggers.
"""
import struct

import numpy as np

from oracle.quack_oracle import OracleQuack


def base_quack(t, count=0, sums=None, last=None):
    """A flow's quACK before the batch: OracleQuack(t) with the given fields."""
    q = OracleQuack(t)
    q.count = int(count) & 0xFFFFFFFF
    if sums is not None:
        q.power_sums = [int(v) for v in sums]
    q.last_value = None if last is None else int(last)
    return q


def reference_loop(table, flows, ids, frequency_pkts):
    """The reference loop over an ungrouped batch: table[flow] is inserted into
    (mutated), in arrival order.  Returns [(flow, clone)] in the order the
    datagrams would have been sent."""
    sent = []
    for g, ident in zip(flows, ids):
        q = table[int(g)]
        q.insert(int(ident))
        if q.count % frequency_pkts == 0:
            sent.append((int(g), q.clone()))
    return sent


def per_packet_states(q, ids):
    """q after each of ids, inserted in order (q is mutated): the power sums
    [n, t] and the counts [n].  A snapshot at any frequency is a row of these."""
    sums = np.zeros((len(ids), q.threshold), dtype=np.uint32)
    counts = np.zeros(len(ids), dtype=np.uint32)
    for j, ident in enumerate(ids):
        q.insert(int(ident))
        sums[j] = q.power_sums
        counts[j] = q.count
    return sums, counts


def record(q):
    """The qk_u32 record of an oracle quACK: np.uint32 [4 + t]."""
    has = q.last_value is not None
    return np.array([q.threshold, q.count, int(has), q.last_value if has else 0] + list(q.power_sums), dtype=np.uint32)


def serialize(q):
    """bincode 1.3 of {power_sums: Vec<u32>, last_value: Option<u32>, count: u32}."""
    out = struct.pack("<Q", q.threshold) + np.asarray(q.power_sums, dtype="<u4").tobytes()
    out += b"\x00" if q.last_value is None else b"\x01" + struct.pack("<I", q.last_value)
    return out + struct.pack("<I", q.count)


def to_sketch(q):
    """The PowerSumQuackU32 with the oracle quACK's state."""
    from sidekick_amd import PowerSumQuackU32
    return PowerSumQuackU32._from_record(record(q).tobytes(), q.threshold)


# The loss case of the protocol property.  t = 4, f = 8: 64 packets sent, 2 lost in every block of 8, never a block's last
LOSS_T, LOSS_F, LOSS_N = 4, 8, 64
LOSS_LOST = [b * 8 + o for b in range(8) for o in (2, 5)]


def loss_case_ids():
    return (np.arange(LOSS_N, dtype=np.uint64) * 2654435761 % (1 << 32) + 17).astype(np.uint32) | np.uint32(1)


def run_loss_case(quacks):
    """A QuackReceiver (the sender's loop, media_client.rs:233-322) that sent
    the 64 packets is given `quacks` one at a time.  Returns (retransmitted
    seqnos, resets)."""
    ids = loss_case_ids()
    assert len(set(ids.tolist())) == LOSS_N
    from sidekick_amd.receiver import QuackReceiver
    rx = QuackReceiver(LOSS_T)
    for s, v in enumerate(ids.tolist()):
        rx.on_send(s, v)
    retx, resets = [], 0
    for q in quacks:
        act = rx.on_quack(q, now=1.0)
        retx += act.retransmit
        resets += bool(act.reset_reason)
    return retx, resets


# Every threshold at which the snapshot kernels or their dispatch change shape
# (test_snapshots_abi.py restates the rule from snapshots.h and checks this
# list against it), crossed with these frequencies.
THRESHOLDS = (1, 4, 5, 8, 9, 16, 17, 24, 25, 31, 32, 33, 64, 65, 80, 81, 128, 129, 1024)
FREQUENCIES = (1, 2, 3, 7, 64, 65)
