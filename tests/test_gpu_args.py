"""The capacity retries of the per-flow wrappers on the GPU: a batch whose
result is larger than the size a wrapper first allocates for it runs the
library call a second time with the reported size, and gives what a call that
never retried gives.  (root_test's retry: test_gpu_decode.py,
test_many_hits_capacity_growth.)"""
import numpy as np
import pytest

import sidekick_amd as sk
from sidekick_amd._lib import P32, QK_OK, SND_ADVANCED
from sidekick_amd.receiver import QuackReceiver

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NSEG, LEN, T, LOST = 64, 40, 32, 20      # 1280 hits: above the first capacity, max(1024, 4 * NSEG)


@pytest.fixture(scope="module")
def batch():
    """(log, offsets, device log, lost): 64 segments of 40 distinct ids; lost[g] the
    20 positions of segment g that the peer never got, none of them the last."""
    rng = np.random.default_rng(0xA295)
    ids = np.unique(rng.integers(1 << 8, P32 - (1 << 8), size=2 * NSEG * LEN, dtype=np.uint64))
    log = rng.permutation(ids)[:NSEG * LEN].astype(np.uint32)
    assert len(log) == NSEG * LEN
    offs = np.arange(NSEG + 1, dtype=np.uint64) * LEN
    lost = [sorted(rng.choice(LEN - 1, size=LOST, replace=False).tolist()) for _ in range(NSEG)]
    assert NSEG * LOST > max(1024, 4 * NSEG)
    return log, offs, torch.from_numpy(log.view(np.int32)).cuda(), lost


def sketch(ids):
    q = sk.PowerSumQuackU32(T)
    for v in ids:
        q.insert(int(v))
    return q


def test_decode_segments_with_more_hits_than_first_allocated(batch):
    log, offs, d_log, lost = batch
    diffs = [sketch(log[g * LEN:(g + 1) * LEN][lost[g]]) for g in range(NSEG)]
    got, status = sk.decode_segments(diffs, d_log, offs)
    assert status == [QK_OK] * NSEG and sum(len(p) for p in got) == NSEG * LOST
    for g in range(NSEG):
        assert got[g] == diffs[g].decode_host(log[g * LEN:(g + 1) * LEN]) == lost[g], g


def test_sender_step_with_more_hits_than_first_allocated(batch):
    """Against one QuackReceiver per flow, as tests/test_gpu_sender_step.py models a flow."""
    log, offs, d_log, lost = batch
    rx, peers = [], []
    for g in range(NSEG):
        seg = log[g * LEN:(g + 1) * LEN]
        r = QuackReceiver(T, batch_min=1 << 30)
        for p, v in enumerate(seg.tolist()):
            r.on_send(1000 * g + p, v)
        rx.append(r)
        peers.append(sketch(np.delete(seg, lost[g])))
    res = sk.sender_step([sk.PowerSumQuackU32(T) for _ in range(NSEG)], peers, d_log, offs)
    assert sum(len(m) for m in res.missing) == NSEG * LOST
    mine = res.mine_out.cpu().numpy().view(np.uint32)
    for g in range(NSEG):
        want = rx[g].on_quack(peers[g], 0.0)
        assert not want.reset_reason and int(res.action[g]) == SND_ADVANCED and int(res.drain[g]) == LEN, g
        assert res.missing[g] == lost[g] and [1000 * g + p for p in res.missing[g]] == want.retransmit, g
        assert np.array_equal(mine[g], np.frombuffer(rx[g].my_quack._buf, dtype=np.uint32)), g


@pytest.mark.parametrize("device_out", (False, True))
def test_encode_flows_sized_for_one_flow_equals_the_roomy_call(device_out):
    """cap=1 on a batch of three flows: the second run has the reported size."""
    rng = np.random.default_rng(3)
    n = 50
    bufs = rng.integers(0, 256, size=(n, 67), dtype=np.uint8)
    bufs[:, 23] = 17                                        # UDP
    bufs[:, 26:38] = rng.integers(0, 256, size=(3, 12), dtype=np.uint8)[rng.integers(0, 3, size=n)]
    meta = np.zeros(n, dtype=np.dtype([("pkttype", "u1"), ("reserved", "u1"), ("protocol_be", "<u2"), ("len", "<u4")]))
    meta["protocol_be"], meta["len"] = 0x0008, 67
    d_bufs, d_meta = torch.from_numpy(bufs.reshape(-1)).cuda(), torch.from_numpy(meta.view(np.int64)).cuda()
    out = [sk.quack.encode_flows(d_bufs, 8, 67, d_meta, device_out=device_out, cap=cap) for cap in (1, 1024)]
    (k1, q1, s1), (k2, q2, s2) = out
    assert s1 == s2 and s1["inserted"] == n and len(k1) == len(k2) == 3
    if device_out:
        assert torch.equal(k1, k2) and torch.equal(q1, q2)
    else:
        assert k1 == k2 and q1 == q2 and sum(q.count() for q in q1) == n
