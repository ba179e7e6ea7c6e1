"""The closed loop of tests/test_gpu_sender_log.py through the wire: 64 flows,
T = 16, 40 rounds, the same debounce timing.  Each round the proxy's flow array
goes through emit_wire with select = present; the images cross to the host,
where about 2 % are corrupted (truncated, or a bad tag), about 5 % are preceded
by the previous round's image of the same flow, and the order is shuffled
across flows (per-flow order kept); then they come back through
DeviceSenderLog.on_wire.  The model is 64 QuackReceivers, each fed
PowerSumQuackU32.deserialize of its flow's last surviving datagram."""
import ctypes as C
import random

import numpy as np
import pytest

import sidekick_amd as sk
from sidekick_amd._lib import QK_WIRE_SUPERSEDED, SND_ADVANCED, SND_IDLE, lib
from sidekick_amd.receiver import QuackReceiver

pytestmark = pytest.mark.gpu

# chosen by running the host model alone (wire_loop(seed, None)): the seed must
# exercise every path, see the assertion at the end
LOOP_SEED = 0xC105ED


def host(t):
    return t.cpu().numpy().view(np.uint32)


def deserialize_status(data, t):
    q = sk.PowerSumQuackU32(t)
    src = (C.c_uint8 * max(len(data), 1))()
    C.memmove(src, data, len(data))
    return lib().qk_u32_deserialize(src, len(data), q._buf, None)


def wire_loop(seed, device_log):
    """With device_log None only the QuackReceivers run, on images the host
    serializer makes (the host model alone, to see what the seed exercises)."""
    t, nflow, rounds = 16, 64, 40
    rnd = random.Random(seed)
    rx = [QuackReceiver(t, reset_debounce_s=0.1, batch_min=1 << 30) for _ in range(nflow)]
    proxy = [sk.PowerSumQuackU32(t) for _ in range(nflow)]
    resend = [0] * nflow
    previous = [None] * nflow          # the image of the flow's last round, as sent
    seq = 0
    stats = {"adv": 0, "fired": 0, "held": 0, "idle": 0, "retx": 0, "superseded": 0, "malformed": 0}
    d = device_log
    if d is not None:
        import torch
    stride = sk.wire_max(t) if d is not None else 4 * t + 17

    def compare_logs(where):
        log, seqs = host(d.log), host(d.seqnos)
        for g in range(nflow):
            a, b = int(d.offsets[g]), int(d.offsets[g + 1])
            assert list(zip(seqs[a:b].tolist(), log[a:b].tolist())) == rx[g].seqno_ids, (where, g)

    def compare_mine(where):
        got = host(d.mine)
        for g in range(nflow):
            assert np.array_equal(got[g], np.frombuffer(rx[g].my_quack._buf, dtype=np.uint32)), (where, g)

    for rno in range(rounds):
        now = 0.04 * rno
        batch = []
        for g in range(nflow):
            k = resend[g] + (0 if rnd.random() < 0.1 else rnd.randrange(0, 301))
            batch += [g] * k
            resend[g] = 0
        rnd.shuffle(batch)
        seqnos, ids = [], []
        for g in batch:
            seq += 1
            v = rnd.getrandbits(32)
            rx[g].on_send(seq, v)
            seqnos.append(seq)
            ids.append(v)
            if rnd.random() >= 0.01:
                proxy[g].insert(v)
        if d is not None:
            d.send(np.array(batch, dtype=np.uint32), np.array(seqnos, dtype=np.uint32), np.array(ids, dtype=np.uint32))
            compare_logs(("send", rno))
        present = [rnd.random() < 0.9 for _ in range(nflow)]
        quacks = []
        for g in range(nflow):
            q = proxy[g].clone()
            if rnd.random() < 0.03:
                q.insert(0xDEADBEEF)          # reordering: a last value that is not in the log
            quacks.append(q)
        # 1. the proxy's flow array -> wire images of the present flows
        sent = [g for g in range(nflow) if present[g]]
        if d is not None:
            recs = np.stack([np.frombuffer(q._buf, dtype=np.int32) for q in quacks])
            _, rows, wire, lens = sk.emit_wire(None, torch.from_numpy(recs).cuda(),
                                               torch.tensor(present, dtype=torch.uint8).cuda())
            assert rows.tolist() == sent
            wire, lens = wire.cpu().numpy(), lens.cpu().numpy()
            images = [wire[r, :lens[r]].tobytes() for r in range(len(sent))]
        else:
            images = [quacks[g].serialize() for g in sent]
        # 2. the host leg: corruption, duplicates, reordering across flows
        queues = {}
        for g, img in zip(sent, images):
            fresh = img
            if rnd.random() < 0.02:
                if rnd.random() < 0.5:
                    fresh = img[:len(img) - rnd.randrange(1, 6)]
                else:
                    fresh = img[:8 + 4 * t] + b"\x02" + img[9 + 4 * t:]
            queues[g] = [fresh]
            if previous[g] is not None and rnd.random() < 0.05:
                queues[g].insert(0, previous[g])
            previous[g] = img
        order = [g for g, q in queues.items() for _ in q]
        rnd.shuffle(order)
        at = {g: 0 for g in queues}
        datagrams, flows = [], []
        for g in order:
            datagrams.append(queues[g][at[g]])
            flows.append(g)
            at[g] += 1
        # the model: the last surviving datagram of every flow
        want_status = [deserialize_status(b, t) for b in datagrams]
        survivor = {}
        for i, g in enumerate(flows):
            if want_status[i] == 0:
                survivor[g] = i
        for i, g in enumerate(flows):
            if want_status[i] == 0 and survivor[g] != i:
                want_status[i] = QK_WIRE_SUPERSEDED
        stats["superseded"] += want_status.count(QK_WIRE_SUPERSEDED)
        stats["malformed"] += sum(1 for s in want_status if s < 0)
        # 3. back through the device
        step = None
        if d is not None:
            buf = np.zeros((len(datagrams), stride), dtype=np.uint8)
            for i, b in enumerate(datagrams):
                buf[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
            step, status = d.on_wire(torch.from_numpy(buf).cuda(), np.array([len(b) for b in datagrams], dtype=np.uint32),
                                     np.array(flows, dtype=np.uint32), now=now)
            assert status.tolist() == want_status, rno
        for g in range(nflow):
            if g not in survivor:
                if d is not None:
                    assert step.action[g] == SND_IDLE and step.retransmit[g] == [] and not step.send_reset[g]
                continue
            quack = sk.PowerSumQuackU32.deserialize(datagrams[survivor[g]])
            idle = quack.last_value() == rx[g].my_quack.last_value()
            want = rx[g].on_quack(quack, now)
            if d is not None:
                assert (step.action[g] == SND_IDLE) == idle, (rno, g)
                assert step.reset_reason[g] == want.reset_reason, (rno, g)
                assert bool(step.send_reset[g]) == want.send_reset, (rno, g)
                assert step.retransmit[g] == want.retransmit, (rno, g)
                assert (step.action[g] == SND_ADVANCED) == (not idle and not want.reset_reason), (rno, g)
            if want.reset_reason:
                stats["fired" if want.send_reset else "held"] += 1
                if want.send_reset:           # the proxy's part of a reset
                    proxy[g] = sk.PowerSumQuackU32(t)
            elif idle:
                stats["idle"] += 1
            else:
                stats["adv"] += 1
            resend[g] = len(want.retransmit)
            stats["retx"] += len(want.retransmit)
        if d is not None:
            compare_mine(rno)
            if rno % 2:
                d.flush()
                compare_logs(("flush", rno))
    if d is not None:
        d.flush()
        compare_logs("end")
    return stats


def test_closed_loop_through_the_wire():
    pytest.importorskip("torch")
    d = sk.DeviceSenderLog(16, 60)
    d.add_flows(4)
    stats = wire_loop(LOOP_SEED, d)
    # a condition on the seed, not a tolerance: it exercised every path
    assert stats["adv"] > 1000 and stats["fired"] > 20 and stats["superseded"] > 50 and stats["malformed"] > 20, stats
