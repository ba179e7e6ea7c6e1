"""The proxy's frequency loop over captured packets, restated over the oracle,
for the packet snapshot tests (a helper module, as snapshot_model.py is).

start_sidekick_multi_frequency_pkts (sidekick_multi.rs:240-287), literally,
one packet at a time in capture order:

    match process_one_packet(n, &buf, &addr, my_addr) {          (:101-143)
        Skip => continue,
        Reset { .. } => { sc = SidekickMulti::new(threshold); }   (:263-266)
        Insert { addr_key, id } => {
            let quack = sc.insert(addr_key, id);                  (:65-90)
            if quack.count() % frequency_pkts == 0 { send(bincode::serialize(&quack)) }   (:271-283)
        }
    }

The filters come in process_one_packet's order: direction, protocol and
not-UDP skip; then a packet to my own address is a Reset, whatever its length;
then a capture length other than BUFFER_SIZE skips.  The count is the
reference's wrapping u32, so a count that wraps to 0 sends.  Nothing here
touches sidekick_amd.
"""
import numpy as np

from oracle.quack_oracle import (BUFFER_SIZE, ETH_P_IP_BE, ID_OFFSET, IPPROTO_UDP, PACKET_HOST, PACKET_OTHERHOST,
                                 OracleQuack, addr_key)
from snapshot_model import record

META_DT = np.dtype([("pkttype", "u1"), ("reserved", "u1"), ("protocol_be", "<u2"), ("len", "<u4")])


def packet_loop(table, threshold, frequency_pkts, bufs, meta=None, my_addr=None):
    """The loop over records bufs[i] (uint8 rows; meta: None or a META_DT
    array).  table: {AddrKey: OracleQuack} before the batch, consumed.
    Returns (sent, table, stats): sent = [(i, key, clone)] in send order, the
    table after the last packet (a new dict after a Reset), and the
    qk_pkt_stats of the batch."""
    stats = {"inserted": 0, "discarded": 0, "resets": 0, "filtered": 0, "last_reset_index": -1}
    sent = []
    head = np.ascontiguousarray(bufs[:, :38]).tolist() if len(bufs) else []
    tail = np.ascontiguousarray(bufs[:, ID_OFFSET:ID_OFFSET + 4]).tolist() if len(bufs) else []
    for i in range(len(bufs)):
        buf = head[i]
        pt = PACKET_HOST if meta is None else int(meta["pkttype"][i])
        proto = ETH_P_IP_BE if meta is None else int(meta["protocol_be"][i])
        ln = BUFFER_SIZE if meta is None else int(meta["len"][i])
        if pt not in (PACKET_HOST, PACKET_OTHERHOST) or proto != ETH_P_IP_BE or buf[23] != IPPROTO_UDP:
            stats["filtered"] += 1
            continue
        key = addr_key(buf)
        if my_addr is not None and list(key[6:12]) == list(my_addr):
            stats["resets"] += 1
            stats["discarded"] += stats["inserted"]
            stats["inserted"] = 0
            stats["last_reset_index"] = i
            table = {}
            continue
        if ln != BUFFER_SIZE:
            stats["filtered"] += 1
            continue
        ident = int.from_bytes(bytes(tail[i]), "big")
        q = table.get(key)
        if q is None:
            q = table[key] = OracleQuack(threshold)
        q.insert(ident)
        stats["inserted"] += 1
        if q.count % frequency_pkts == 0:
            sent.append((i, key, q.clone()))
    return sent, table, stats


def table_arrays(table, threshold):
    """A table as a flow array: (keys uint8 [n, 12] ascending, records uint32 [n, 4 + t])."""
    keys = sorted(table)
    k = np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(len(keys), 12).copy() if keys else \
        np.zeros((0, 12), dtype=np.uint8)
    r = np.stack([record(table[key]) for key in keys]) if keys else np.zeros((0, 4 + threshold), dtype=np.uint32)
    return k, r


def sent_arrays(sent, threshold):
    """The sent list as the call's three outputs: (records [m, 4 + t], keys [m, 12], index [m])."""
    if not sent:
        return (np.zeros((0, 4 + threshold), dtype=np.uint32), np.zeros((0, 12), dtype=np.uint8),
                np.zeros(0, dtype=np.uint32))
    return (np.stack([record(q) for _, _, q in sent]),
            np.frombuffer(b"".join(k for _, k, _ in sent), dtype=np.uint8).reshape(len(sent), 12).copy(),
            np.array([i for i, _, _ in sent], dtype=np.uint32))


def make_packets(keys, flow, ids, stride=67, seed=0):
    """Records for Inserts of ids[i] into flow keys[flow[i]] (keys: uint8 [nf,
    12] AddrKeys), every other byte random: (bufs uint8 [n, stride], meta all
    incoming IPv4 of full length)."""
    rng = np.random.default_rng(seed)
    n = len(ids)
    bufs = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
    bufs[:, 23] = IPPROTO_UDP
    key = np.asarray(keys, dtype=np.uint8)[np.asarray(flow, dtype=np.int64)] if n else np.zeros((0, 12), dtype=np.uint8)
    bufs[:, 26:30] = key[:, 0:4]
    bufs[:, 34:36] = key[:, 4:6]
    bufs[:, 30:34] = key[:, 6:10]
    bufs[:, 36:38] = key[:, 10:12]
    v = np.asarray(ids, dtype=np.uint32)
    for b in range(4):
        bufs[:, ID_OFFSET + b] = (v >> np.uint32(24 - 8 * b)) & np.uint32(0xFF)
    meta = np.zeros(n, dtype=META_DT)
    meta["protocol_be"] = ETH_P_IP_BE
    meta["len"] = BUFFER_SIZE
    return bufs, meta


def set_reset(bufs, i, my_addr):
    """Record i becomes a packet to the proxy's own address: a Reset."""
    bufs[i, 30:34] = my_addr[:4]
    bufs[i, 36:38] = my_addr[4:]
