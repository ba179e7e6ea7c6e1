#!/usr/bin/env python3
"""Batched sender step: what one step over many device-resident logs costs,
against what a caller could compose for the same inputs and outputs before the
step existed.  One process, warmed, the two arms alternated; one JSON line per
measurement (median, min, max of --rounds calls).

  step      qk_u32_sender_step_segments_device through the C ABI with
            preallocated outputs: --flows flows of --len log entries, T = --t,
            every flow's quACK covering all but its last --tail entries, each
            entry before the stop lost with probability --loss
  composed  the same outputs from the older entry points:
              the log copied to the host
              numpy finds each flow's first entry equal to the peer's last value
              the prefixes packed, uploaded, qk_u32_encode_segments_device
              numpy: mine + prefix, the reset test, mine1 - peer
              qk_u32_decode_segments_device (host diffs, the device log)
              the hits' ids gathered, uploaded, encoded per flow and subtracted
            (the removes through the segmented encode, not one host call per
            hit: the cheapest composition, not the most obvious one)
  With --profile the context's kernel events are on during extra step calls:
  the summed time of the bracketed kernels (find, prefix, Newton, root test).

    python tools/bench_sender_step.py [--flows 100000] [--len 1000] [--t 32] [--loss 0.01] [--rounds 10]
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
U64P = C.POINTER(C.c_uint64)


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs),
            "samples": [round(float(x), 4) for x in xs]}


def encode_segments_raw(lib, ctx, d_ids, offs, t, stream):
    """qk_u32_encode_segments_device into a numpy record array [nseg, 4 + t]."""
    nseg = len(offs) - 1
    out = np.zeros((nseg, 4 + t), dtype=np.uint32)
    rc = lib.qk_u32_encode_segments_device(ctx.handle, d_ids.data_ptr(), offs.ctypes.data_as(U64P), nseg, t,
                                           out.ctypes.data, stream)
    assert rc == 0, rc
    return out


def make_inputs(torch, sk, lib, ctx, a):
    dev, F, L, t = "cuda:0", a.flows, a.len, a.t
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5E9D)
    log = torch.randint(0, 1 << 32, (F, L), device=dev, generator=gen, dtype=torch.int64).to(torch.int32).contiguous()
    stop = L - 1 - a.tail
    got = torch.rand((F, L), device=dev, generator=gen) >= a.loss
    got[:, stop] = True
    got[:, stop + 1:] = False
    counts = got.sum(dim=1).cpu().numpy().astype(np.uint64)
    roffs = np.zeros(F + 1, dtype=np.uint64)
    roffs[1:] = np.cumsum(counts)
    received = log[got].contiguous()
    torch.cuda.synchronize()
    peer = encode_segments_raw(lib, ctx, received, roffs, t, None)
    mine = np.zeros((F, 4 + t), dtype=np.uint32)
    mine[:, 0] = t
    offs = (np.arange(F + 1, dtype=np.uint64) * np.uint64(L))
    lost = int(F * (stop + 1) - counts.sum())
    return (log.view(-1), offs, torch.from_numpy(mine.view(np.int32)).to(dev), torch.from_numpy(peer.view(np.int32)).to(dev),
            lost)


class Step:
    """The new entry point with every output preallocated."""

    def __init__(self, torch, lib, ctx, d_log, offs, mine, peer, t, cap):
        self.torch, self.lib, self.ctx, self.t, self.cap = torch, lib, ctx, t, cap
        self.d_log, self.offs, self.mine, self.peer = d_log, offs, mine, peer
        n = len(offs) - 1
        self.mine_out = torch.empty_like(mine)
        self.action = np.zeros(n, dtype=np.uint8)
        self.drain = np.zeros(n, dtype=np.uint64)
        self.hits = np.zeros(cap, dtype=np.uint64)
        self.hoffs = np.zeros(n + 1, dtype=np.uint64)
        self.nh = C.c_size_t()

    def __call__(self):
        rc = self.lib.qk_u32_sender_step_segments_device(
            self.ctx.handle, self.mine.data_ptr(), self.peer.data_ptr(), None, self.d_log.data_ptr(),
            self.offs.ctypes.data_as(U64P), len(self.offs) - 1, self.t, self.mine_out.data_ptr(),
            self.action.ctypes.data_as(C.POINTER(C.c_uint8)), self.drain.ctypes.data_as(U64P),
            self.hits.ctypes.data_as(U64P), self.cap, self.hoffs.ctypes.data_as(U64P), C.byref(self.nh), None)
        assert rc == 0, rc


class Composed:
    """The same outputs from the entry points that existed before the step."""

    def __init__(self, torch, lib, ctx, d_log, offs, mine, peer, t, cap, L):
        self.torch, self.lib, self.ctx, self.t, self.cap, self.L = torch, lib, ctx, t, cap, L
        self.d_log, self.offs, self.mine, self.peer = d_log, offs, mine, peer
        n = len(offs) - 1
        self.hits = np.zeros(cap, dtype=np.uint64)
        self.hoffs = np.zeros(n + 1, dtype=np.uint64)
        self.status = np.zeros(n, dtype=np.int32)
        self.nh = C.c_size_t()

    def __call__(self):
        torch, lib, ctx, t, L = self.torch, self.lib, self.ctx, self.t, self.L
        F = len(self.offs) - 1
        log = self.d_log.cpu().numpy().view(np.uint32).reshape(F, L)                 # the log over PCIe
        mine = self.mine.cpu().numpy().view(np.uint32)
        peer = self.peer.cpu().numpy().view(np.uint32)
        active = (peer[:, 2] != mine[:, 2]) | ((peer[:, 2] != 0) & (peer[:, 3] != mine[:, 3]))
        eq = log == peer[:, 3:4]
        found = eq.any(axis=1) & active & (peer[:, 2] != 0)
        idx = np.where(found, eq.argmax(axis=1), 0).astype(np.uint64)
        plen = np.where(found, idx + 1, 0).astype(np.uint64)
        poffs = np.zeros(F + 1, dtype=np.uint64)
        poffs[1:] = np.cumsum(plen)
        prefix = log[np.arange(L)[None, :] < plen[:, None]]                           # packed prefixes
        d_prefix = torch.from_numpy(prefix.view(np.int32)).to(self.d_log.device)      # and back over PCIe
        pre = encode_segments_raw(lib, ctx, d_prefix, poffs, t, None)
        m1 = mine.copy()
        m1[:, 4:] = ((mine[:, 4:].astype(np.uint64) + pre[:, 4:]) % P).astype(np.uint32)
        m1[:, 1] = mine[:, 1] + plen.astype(np.uint32)
        m1[found, 2] = 1
        m1[found, 3] = log[np.arange(F), idx.astype(np.int64)][found]
        pc = peer[:, 1]
        bits = (np.where(~found, 2, 0) | np.where(m1[:, 1] < pc, 4, 0)
                | np.where(m1[:, 1] > (pc + np.uint32(t)), 8, 0)).astype(np.uint8)
        bits[~active] = 0
        decode = active & (bits == 0)
        action = np.where(decode, 1, bits).astype(np.uint8)
        drain = np.where(decode, plen, 0).astype(np.uint64)
        diff = np.zeros_like(m1)
        diff[:, 0] = t
        diff[decode, 1] = (m1[:, 1] - pc)[decode]
        diff[decode, 2] = 1
        diff[:, 3] = m1[:, 3]
        diff[decode, 4:] = ((m1[decode, 4:].astype(np.uint64) + P - peer[decode, 4:]) % P).astype(np.uint32)
        rc = lib.qk_u32_decode_segments_device(ctx.handle, diff.ctypes.data, self.d_log.data_ptr(),
                                               self.offs.ctypes.data_as(U64P), F, t, 1, self.hits.ctypes.data_as(U64P),
                                               self.cap, self.hoffs.ctypes.data_as(U64P),
                                               self.status.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(self.nh), None)
        assert rc == 0, rc
        nh = self.nh.value
        hit_ids = log.reshape(-1)[self.hits[:nh].astype(np.int64)]
        mine_out = m1
        if nh:
            d_hit = torch.from_numpy(hit_ids.view(np.int32)).to(self.d_log.device)
            rem = encode_segments_raw(lib, ctx, d_hit, self.hoffs, t, None)
            mine_out[:, 4:] = ((m1[:, 4:].astype(np.uint64) + P - rem[:, 4:]) % P).astype(np.uint32)
            mine_out[:, 1] = m1[:, 1] - rem[:, 1]
        self.action, self.drain, self.mine_out = action, drain, mine_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=float, default=1e5)
    ap.add_argument("--len", type=int, default=1000)
    ap.add_argument("--t", type=int, default=32)
    ap.add_argument("--loss", type=float, default=0.01)
    ap.add_argument("--tail", type=int, default=8, help="log entries after the peer's last value")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--no-composed", action="store_true", help="time the step alone (e.g. under a profiler)")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    a.flows = int(a.flows)
    a.rounds = max(a.rounds, 1 if a.no_composed else 10)
    import torch
    import sidekick_amd as sk
    from sidekick_amd._lib import lib as load
    lib, ctx = load(), sk.get_context(0)
    d_log, offs, mine, peer, lost = make_inputs(torch, sk, lib, ctx, a)
    cap = 2 * lost + 1024
    arms = {"step": Step(torch, lib, ctx, d_log, offs, mine, peer, a.t, cap)}
    if not a.no_composed:
        arms["composed"] = Composed(torch, lib, ctx, d_log, offs, mine, peer, a.t, cap, a.len)
    times = {k: [] for k in arms}
    for r in range(a.rounds + 2):            # two warm rounds: the arenas reach their size
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
    s = arms["step"]
    out = {"what": "sender_step", "flows": a.flows, "log_entries_per_flow": a.len, "log_bytes": int(d_log.numel()) * 4,
           "t": a.t, "lost_ids": lost, "hits": int(s.nh.value),
           "actions": {int(k): int(v) for k, v in zip(*np.unique(s.action, return_counts=True))},
           "wall_ms": {k: spread(v) for k, v in times.items()}}
    if not a.no_composed:
        c = arms["composed"]
        nh = s.nh.value
        out["arms_agree"] = bool(nh == c.nh.value and np.array_equal(s.action, c.action)
                                 and np.array_equal(s.drain, c.drain) and np.array_equal(s.hoffs, c.hoffs)
                                 and np.array_equal(s.hits[:nh], c.hits[:nh])
                                 and np.array_equal(s.mine_out.cpu().numpy().view(np.uint32), c.mine_out))
    print(json.dumps(out), flush=True)
    if a.profile:
        ctx.set_profiling(True)
        ks = []
        for _ in range(a.rounds):
            s()
            ms, launches = ctx.kernel_stats()
            ks.append(ms)
        ctx.set_profiling(False)
        print(json.dumps({"what": "sender_step_profiled_kernels", "kernels": "find + prefix + newton + root test",
                          "launches_per_call": int(launches), "ms": spread(ks)}), flush=True)


if __name__ == "__main__":
    main()
