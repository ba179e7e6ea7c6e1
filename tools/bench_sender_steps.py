#!/usr/bin/env python3
"""Every queued quACK of a flow stepped in one call, against the same outputs
from the calls that existed before.  One process, warmed, the two arms
alternated; one JSON line (median, min, max of --rounds calls per arm).

  queued    qk_u32_wire_ingest_queue_device on the batch's F * K datagrams, then
            qk_u32_sender_steps_segments_device: --flows flows of --len log
            entries, T = --t, --k quACKs per flow, one every len / k entries,
            each entry before a stop lost with probability --loss
  rounds    K rounds, each qk_u32_wire_ingest_device on that round's F
            datagrams, qk_u32_sender_step_segments_device and
            qk_u32_log_drain_segments_device (the log moves every round)
  Both through the C ABI with preallocated outputs.  After the timing the
  outputs of the two arms are compared bit for bit (mine_out, every action,
  every drain, every hit as a position in the undrained log).

    python tools/bench_sender_steps.py [--flows 100000] [--len 1000] [--t 32] [--k 8] [--loss 0.01] [--rounds 10]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P = 4294967291
U64P, U8P, U32P, I32P = (C.POINTER(c) for c in (C.c_uint64, C.c_uint8, C.c_uint32, C.c_int32))


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs),
            "samples": [round(float(x), 4) for x in xs]}


def make_inputs(torch, sk, lib, ctx, a):
    """The log [F * L], and the batch's F * K datagrams in arrival order: round j's F datagrams, flow by flow."""
    dev, F, L, K, t = "cuda:0", a.flows, a.len, a.k, a.t
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5E9E)
    log = torch.randint(0, 1 << 32, (F, L), device=dev, generator=gen, dtype=torch.int64).to(torch.int32).contiguous()
    got = torch.rand((F, L), device=dev, generator=gen) >= a.loss
    w = L // K
    got[:, w - 1::w] = True                                   # the entries that trigger a quACK arrive
    counts = got.view(F, K, w).sum(dim=2).reshape(-1).cpu().numpy().astype(np.uint64)
    roffs = np.zeros(F * K + 1, dtype=np.uint64)
    roffs[1:] = np.cumsum(counts)
    received = log[got].contiguous()
    torch.cuda.synchronize()
    part = np.zeros((F * K, 4 + t), dtype=np.uint32)          # the quACK of each interval's received entries alone
    rc = lib.qk_u32_encode_segments_device(ctx.handle, received.data_ptr(), roffs.ctypes.data_as(U64P), F * K, t,
                                           part.ctypes.data, None)
    assert rc == 0, rc
    part = part.reshape(F, K, 4 + t)
    recs = part.copy()                                         # cumulative: what the proxy holds at each crossing
    recs[:, :, 4:] = (np.cumsum(part[:, :, 4:].astype(np.uint64), axis=1) % P).astype(np.uint32)
    recs[:, :, 1] = np.cumsum(part[:, :, 1].astype(np.uint64), axis=1).astype(np.uint32)
    arrival = np.ascontiguousarray(recs.transpose(1, 0, 2)).reshape(K * F, 4 + t)
    d_recs = torch.from_numpy(arrival.view(np.int32)).to(dev)
    _, _, wire, lens = sk.emit_wire(None, d_recs, ctx=ctx)
    flow = torch.arange(F, dtype=torch.int32, device=dev).repeat(K).contiguous()
    mine = np.zeros((F, 4 + t), dtype=np.uint32)
    mine[:, 0] = t
    offs = np.arange(F + 1, dtype=np.uint64) * np.uint64(L)
    lost = int(F * L - counts.sum())
    return log.view(-1), offs, torch.from_numpy(mine.view(np.int32)).to(dev), wire, lens, flow, lost


class Queued:
    """The new ingest and the new step."""

    def __init__(self, torch, lib, ctx, d_log, offs, mine, wire, lens, flow, t, K, cap):
        self.lib, self.ctx, self.t, self.cap = lib, ctx, t, cap
        self.d_log, self.offs, self.mine, self.wire, self.lens, self.flow = d_log, offs, mine, wire, lens, flow
        F, n = len(offs) - 1, wire.shape[0]
        self.queue = torch.empty((n, 4 + t), dtype=torch.int32, device=wire.device)
        self.qoffs = np.zeros(F + 1, dtype=np.uint64)
        self.status = np.zeros(n, dtype=np.int32)
        self.mine_out = torch.empty_like(mine)
        self.q_action, self.q_drain = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint64)
        self.stepped, self.drain = np.zeros(F, dtype=np.uint32), np.zeros(F, dtype=np.uint64)
        self.hits, self.hoffs = np.zeros(cap, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
        self.m, self.nh = C.c_size_t(), C.c_size_t()

    def __call__(self):
        n, F = self.wire.shape[0], len(self.offs) - 1
        rc = self.lib.qk_u32_wire_ingest_queue_device(
            self.ctx.handle, self.wire.data_ptr(), self.wire.shape[1], self.lens.data_ptr(), self.flow.data_ptr(), n,
            self.t, F, self.queue.data_ptr(), n, self.qoffs.ctypes.data_as(U64P), self.status.ctypes.data_as(I32P),
            C.byref(self.m), None)
        assert rc == 0 and self.m.value == n, (rc, self.m.value)
        rc = self.lib.qk_u32_sender_steps_segments_device(
            self.ctx.handle, self.mine.data_ptr(), self.queue.data_ptr(), self.qoffs.ctypes.data_as(U64P),
            self.d_log.data_ptr(), self.offs.ctypes.data_as(U64P), F, self.t, self.mine_out.data_ptr(),
            self.q_action.ctypes.data_as(U8P), self.q_drain.ctypes.data_as(U64P), self.stepped.ctypes.data_as(U32P),
            self.drain.ctypes.data_as(U64P), self.hits.ctypes.data_as(U64P), self.cap, self.hoffs.ctypes.data_as(U64P),
            C.byref(self.nh), None)
        assert rc == 0, rc


class Rounds:
    """The same outputs from what existed before: K rounds of ingest, step and drain."""

    def __init__(self, torch, lib, ctx, d_log, offs, mine, wire, lens, flow, t, K, cap):
        self.lib, self.ctx, self.t, self.K, self.cap = lib, ctx, t, K, cap
        self.d_log, self.offs, self.mine0, self.wire, self.lens, self.flow = d_log, offs, mine, wire, lens, flow
        F = len(offs) - 1
        dev = wire.device
        self.peer = torch.zeros_like(mine)
        self.present = torch.empty((F,), dtype=torch.uint8, device=dev)
        self.status = np.zeros(F, dtype=np.int32)
        self.mines = [torch.empty_like(mine), torch.empty_like(mine)]
        self.logs = [torch.empty_like(d_log), torch.empty_like(d_log)]
        self.action = [np.zeros(F, dtype=np.uint8) for _ in range(K)]
        self.drain = [np.zeros(F, dtype=np.uint64) for _ in range(K)]
        self.hits = [np.zeros(cap, dtype=np.uint64) for _ in range(K)]
        self.hoffs = [np.zeros(F + 1, dtype=np.uint64) for _ in range(K)]
        self.offs_in = [np.zeros(F + 1, dtype=np.uint64) for _ in range(K + 1)]
        self.nh = [C.c_size_t() for _ in range(K)]
        self.acc = C.c_size_t()

    def __call__(self):
        lib, h, t, F = self.lib, self.ctx.handle, self.t, len(self.offs) - 1
        stride = self.wire.shape[1]
        log, mine = self.d_log, self.mine0
        self.offs_in[0][:] = self.offs
        for j in range(self.K):
            offs = self.offs_in[j]
            rc = lib.qk_u32_wire_ingest_device(h, self.wire.data_ptr() + j * F * stride, stride,
                                               self.lens.data_ptr() + 4 * j * F, self.flow.data_ptr() + 4 * j * F, F, t, F,
                                               self.peer.data_ptr(), self.present.data_ptr(), self.status.ctypes.data_as(I32P),
                                               C.byref(self.acc), None)
            assert rc == 0, rc
            out = self.mines[j % 2]
            rc = lib.qk_u32_sender_step_segments_device(
                h, mine.data_ptr(), self.peer.data_ptr(), self.present.data_ptr(), log.data_ptr(), offs.ctypes.data_as(U64P),
                F, t, out.data_ptr(), self.action[j].ctypes.data_as(U8P), self.drain[j].ctypes.data_as(U64P),
                self.hits[j].ctypes.data_as(U64P), self.cap, self.hoffs[j].ctypes.data_as(U64P), C.byref(self.nh[j]), None)
            assert rc == 0, rc
            mine = out
            nxt = self.logs[j % 2]
            left = int(offs[-1] - offs[0] - self.drain[j].sum())
            rc = lib.qk_u32_log_drain_segments_device(h, log.data_ptr(), None, offs.ctypes.data_as(U64P),
                                                      self.drain[j].ctypes.data_as(U64P), F, nxt.data_ptr(), None, left,
                                                      self.offs_in[j + 1].ctypes.data_as(U64P), None)
            assert rc == 0, rc
            log = nxt
        self.mine_out = mine

    def in_queue_layout(self):
        """(q_action, q_drain, hits as positions in the undrained log), flow by flow as the queued arm orders them."""
        F = len(self.offs) - 1
        q_action = np.stack(self.action, axis=1).reshape(-1)
        q_drain = np.stack(self.drain, axis=1).reshape(-1)
        gone = np.zeros(F, dtype=np.uint64)
        pos = []
        for j in range(self.K):
            counts = (self.hoffs[j][1:] - self.hoffs[j][:-1]).astype(np.int64)
            g = np.repeat(np.arange(F), counts)
            hj = self.hits[j][:self.nh[j].value]
            pos.append(hj - self.offs_in[j][g] + gone[g] + self.offs[g])
            gone += self.drain[j]
        return q_action, q_drain, np.sort(np.concatenate(pos))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=float, default=1e5)
    ap.add_argument("--len", type=int, default=1000)
    ap.add_argument("--t", type=int, default=32)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--loss", type=float, default=0.01)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--only-queued", action="store_true", help="time the new calls alone (e.g. under a profiler)")
    a = ap.parse_args()
    a.flows = int(a.flows)
    if a.len % a.k:
        ap.error("--len must be a multiple of --k")
    import torch
    import sidekick_amd as sk
    from sidekick_amd._lib import lib as load
    lib, ctx = load(), sk.get_context(0)
    d_log, offs, mine, wire, lens, flow, lost = make_inputs(torch, sk, lib, ctx, a)
    cap = 2 * lost + 1024
    args = (torch, lib, ctx, d_log, offs, mine, wire, lens, flow, a.t, a.k, cap)
    arms = {"queued": Queued(*args)}
    if not a.only_queued:
        arms["rounds"] = Rounds(*args)
    times = {k: [] for k in arms}
    for r in range(a.rounds + 2):            # two warm calls: the arenas reach their size
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
    q = arms["queued"]
    nh = q.nh.value
    out = {"what": "sender_steps", "flows": a.flows, "log_entries_per_flow": a.len, "log_bytes": int(d_log.numel()) * 4,
           "t": a.t, "k": a.k, "datagrams": int(wire.shape[0]), "lost_ids": lost, "hits": int(nh),
           "actions": {int(k): int(v) for k, v in zip(*np.unique(q.q_action, return_counts=True))},
           "wall_ms": {k: spread(v) for k, v in times.items()}}
    if not a.only_queued:
        b = arms["rounds"]
        q_action, q_drain, pos = b.in_queue_layout()
        out["arms_agree"] = bool(np.array_equal(q.q_action, q_action) and np.array_equal(q.q_drain, q_drain)
                                 and np.array_equal(q.hits[:nh], pos)
                                 and np.array_equal(q.drain, np.sum(b.drain, axis=0))
                                 and torch.equal(q.mine_out, b.mine_out))
        ma, mb = out["wall_ms"]["queued"], out["wall_ms"]["rounds"]
        out["queued_faster_beyond_spreads"] = bool(mb["median"] - ma["median"] > (ma["max"] - ma["min"]) + (mb["max"] - mb["min"]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
