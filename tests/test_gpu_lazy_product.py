"""GPU parity of the kernels that share the lazy product (field.h
mulfold32_min as three multiply-adds, and bsgs.h's fused power chain over a
fixed register window): the plain baby-step/giant-step kernels with four-,
six- and eight-wide baby chains, the t = 80 kernel, a multi-pass threshold
(pass 0 writes the x^80 cache, an offset pass reads it), the packet kernel
and the per-flow kernels.  Small shapes: a few workgroups, unaligned head,
tail, and the wrap ids that force the exact recompute.  All against the
oracle, bit-exact."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import sidekick_amd as sk
from oracle import coracle

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
P32 = 4294967291
N = 4096 + 3

# threshold -> golden wrap-id lists whose chains are part of the kernel's
# (encode.hip enc32): 32 -> (8,4); 24 -> (4,6), whose three babies and first
# two giants are the 4x4 chain (6x4 is what the suite's sweep places there);
# 30 -> (6,5), the two-wide leftovers, containing the 6x4 chain; 80 -> (8,10);
# 96 -> pass 0 is (8,10) with the x^80 cache, then an offset pass reads it
WRAP_KEYS = {32: ("8x4",), 24: ("4x4", "6x4"), 30: ("6x4",), 80: ("8x10",), 96: ("8x10",)}
TS = sorted(WRAP_KEYS)


def load(name):
    spec = importlib.util.spec_from_file_location(f"_lp_{name}", os.path.join(HERE, f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to("cuda:0")


def encode(d, t):
    q = sk.PowerSumQuackU32(t)
    q.insert_batch(d)
    return q


@pytest.mark.parametrize("t", TS)
def test_unaligned_head_and_tail(t):
    """4096 + 3 ids starting 4 bytes past a 16-byte boundary (a head of three
    ids, 1024 full groups) and 8 bytes past it (a head of two, a tail of one)."""
    ids = coracle.splitmix_u32(0x1A2F + t, N + 2)
    d = dev_u32(ids)
    for off in (1, 2):
        sub = ids[off:off + N]
        q = encode(d[off:off + N], t)
        assert q.power_sums() == coracle.encode_u32(sub, t), (t, off)
        assert q.count() == N and q.last_value() == int(sub[-1])


@pytest.mark.parametrize("t", TS)
def test_wrap_ids_among_edge_ids(golden, t):
    """Wrap ids in one lane of a full 16-byte group, four in one lane's group,
    in the head and in the tail, among the edge ids 0, 1, p-1, p, 2^32-1."""
    wraps = np.concatenate([np.array(golden["bsgs_wrap_ids"][k], dtype=np.uint32) for k in WRAP_KEYS[t]])
    edge = np.array([0, 1, P32 - 1, P32, 2**32 - 1], dtype=np.uint32)
    for off, head in ((1, 3), (2, 2)):
        ids = coracle.splitmix_u32(0x2B3E + t, N + 2)
        sub = ids[off:off + N]                       # a view: the writes below land in ids
        sub[5::37] = np.resize(edge, len(sub[5::37]))
        sub[0] = wraps[-1]                           # head
        sub[head + 4 * 100 + 2] = wraps[0]           # one lane, one id of its group
        sub[head + 4 * 200:head + 4 * 200 + 4] = wraps[:4]   # one lane's whole group
        sub[head + 4 * 300 + 1] = wraps[len(wraps) // 2]
        sub[-1] = wraps[1]                           # tail (off 2); last full group (off 1)
        q = encode(dev_u32(ids)[off:off + N], t)
        assert q.power_sums() == coracle.encode_u32(sub, t), (t, off)
        assert q.last_value() == int(sub[-1])


def test_packet_batch(golden):
    """1024 records, t = 32, no reset: the fused packet kernel."""
    from sidekick_amd.quack import encode_packets
    tp = load("test_packets")
    n = 1024
    bufs, meta = tp.make_batch(n, seed=0x9AC, p_filter=0.05)
    for j, w in enumerate(golden["bsgs_wrap_ids"]["8x4"]):
        bufs[40 + 97 * j, 63:67] = np.frombuffer(int(w).to_bytes(4, "big"), dtype=np.uint8)
    q = sk.PowerSumQuackU32(32)
    st = encode_packets(q, torch.from_numpy(bufs.reshape(-1).copy()).cuda(), stride=67,
                        meta=torch.from_numpy(meta.view(np.int64).copy()).cuda(), my_ipv4=tp.MY_IP)
    ids, last = tp.vector_sniff(bufs, meta)
    assert last == -1 and len(ids) > 900
    assert q.power_sums() == coracle.encode_u32(ids, 32)
    assert q.count() == len(ids) and st["inserted"] == len(ids) and q.last_value() == int(ids[-1])


def test_flow_batch(golden):
    """1024 records over 8 flows, t = 32: the per-flow kernels."""
    tf = load("test_flows")
    n = 1024
    bufs, meta = tf.make_flows(n, 8, seed=0xF70, p_reset=0.0, p_filter=0.05)
    for j, w in enumerate(golden["bsgs_wrap_ids"]["8x4"]):
        bufs[40 + 97 * j, 63:67] = np.frombuffer(int(w).to_bytes(4, "big"), dtype=np.uint8)
    flows, nres, last_reset = tf.vector_flows(bufs, meta)
    assert nres == 0 and len(flows) == 8
    table = sk.FlowQuacks(32)
    st = table.insert_packets(torch.from_numpy(bufs.reshape(-1).copy()).cuda(), stride=67,
                              meta=torch.from_numpy(meta.view(np.int64).copy()).cuda(), my_addr=tf.MY_ADDR)
    assert st["resets"] == 0 and st["inserted"] == sum(len(v) for v in flows.values())
    assert set(table.senders()) == set(flows)
    for k, v in flows.items():
        q = table.senders()[k]
        assert q.power_sums() == coracle.encode_u32(np.array(v, dtype=np.uint32), 32), k.hex()
        assert q.count() == len(v) and q.last_value() == v[-1]
