#!/usr/bin/env python3
"""Device-resident sender log: what one round's log maintenance costs — the
drain the last quACKs allowed plus the push of the packets sent since — fused
on the device, against the drain alone and against what a caller did before the
update existed.  One process, warmed, the arms alternated; one JSON line
(median, min, max of --rounds calls per arm).

  update        qk_u32_log_update_segments_device through the C ABI with
                preallocated outputs: --flows flows of --len log entries and
                seqnos, --drain of each segment drained, --new new entries with
                shuffled flow indices, the batch already on the device
  update_h2d    the same with the batch's three arrays uploaded first
  update_empty  the same call with n_new = 0: the drain's copy and nothing else
  drain         qk_u32_log_drain_segments_device alone, the floor for the copy
  host          log and seqnos to the host, the batch grouped by a stable
                argsort, a per-flow numpy concatenation (as index arithmetic,
                the cheapest form), and the upload of both arrays

    python tools/bench_sender_log.py [--flows 100000] [--len 1000] [--new 5e7] [--rounds 10] [--no-host]
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

U64P = C.POINTER(C.c_uint64)
DR_ITEM = 2048


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs),
            "samples": [round(float(x), 4) for x in xs]}


def p64(a):
    return a.ctypes.data_as(U64P)


class Update:
    def __init__(self, torch, lib, ctx, d_log, d_seq, offs, drain, batch, total, upload=None):
        self.lib, self.ctx, self.d_log, self.d_seq, self.offs, self.drain = lib, ctx, d_log, d_seq, offs, drain
        self.batch, self.upload, self.torch = batch, upload, torch
        self.out = torch.empty(total, dtype=torch.int32, device=d_log.device)
        self.aout = torch.empty(total, dtype=torch.int32, device=d_log.device)
        self.cap = total
        self.offs_out = np.zeros(len(offs), dtype=np.uint64)

    def __call__(self):
        b = self.batch
        if self.upload is not None:
            b = [self.torch.from_numpy(x).to(self.d_log.device) for x in self.upload]
        n = int(b[0].numel()) if b is not None else 0
        ptr = [x.data_ptr() for x in b] if n else [None, None, None]
        rc = self.lib.qk_u32_log_update_segments_device(
            self.ctx.handle, self.d_log.data_ptr(), self.d_seq.data_ptr(), p64(self.offs), p64(self.drain),
            len(self.offs) - 1, ptr[0], ptr[1], ptr[2], n, self.out.data_ptr(), self.aout.data_ptr(), self.cap,
            p64(self.offs_out), None)
        assert rc == 0, rc


class Drain(Update):
    def __call__(self):
        rc = self.lib.qk_u32_log_drain_segments_device(
            self.ctx.handle, self.d_log.data_ptr(), self.d_seq.data_ptr(), p64(self.offs), p64(self.drain),
            len(self.offs) - 1, self.out.data_ptr(), self.aout.data_ptr(), self.cap, p64(self.offs_out), None)
        assert rc == 0, rc


class Host:
    """Today's path: both arrays over PCIe, regrouped on the host, and back."""

    def __init__(self, torch, d_log, d_seq, offs, drain, h_batch):
        self.torch, self.d_log, self.d_seq, self.offs, self.drain, self.h_batch = torch, d_log, d_seq, offs, drain, h_batch

    def __call__(self):
        torch = self.torch
        log, seq = self.d_log.cpu().numpy(), self.d_seq.cpu().numpy()
        flow, ids, seqs = self.h_batch
        nseg = len(self.offs) - 1
        order = np.argsort(flow, kind="stable")
        counts = np.bincount(flow, minlength=nseg).astype(np.int64)
        kept = (self.offs[1:] - self.offs[:-1] - self.drain).astype(np.int64)
        offs_out = np.zeros(nseg + 1, dtype=np.int64)
        offs_out[1:] = np.cumsum(kept + counts)
        out, aout = np.empty(int(offs_out[-1]), dtype=np.int32), np.empty(int(offs_out[-1]), dtype=np.int32)
        # flow g's kept tail, then its new entries: positions by index arithmetic
        seg = np.repeat(np.arange(nseg), kept)
        within = np.arange(int(kept.sum())) - np.repeat(np.cumsum(kept) - kept, kept)
        src = (self.offs[:-1] + self.drain).astype(np.int64)[seg] + within
        dst = offs_out[:-1][seg] + within
        out[dst], aout[dst] = log[src], seq[src]
        nseg_of = flow[order].astype(np.int64)
        within = np.arange(len(order)) - np.repeat(np.cumsum(counts) - counts, counts)
        dst = offs_out[:-1][nseg_of] + kept[nseg_of] + within
        out[dst], aout[dst] = ids[order], seqs[order]
        self.out = torch.from_numpy(out).to(self.d_log.device)
        self.aout = torch.from_numpy(aout).to(self.d_log.device)
        self.offs_out = offs_out.astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=float, default=1e5)
    ap.add_argument("--len", type=int, default=1000)
    ap.add_argument("--drain", type=float, default=0.5, help="share of every segment drained")
    ap.add_argument("--new", type=float, default=5e7)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="leave out the host arm (e.g. under a profiler)")
    ap.add_argument("--only-update", action="store_true", help="the fused update alone (kernel traces)")
    a = ap.parse_args()
    F, L, n_new = int(a.flows), a.len, int(a.new)
    import torch
    import sidekick_amd as sk
    from sidekick_amd._lib import lib as load
    lib, ctx = load(), sk.get_context(0)
    dev = "cuda:0"
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5E9D106)
    d_log = torch.randint(0, 1 << 32, (F * L,), device=dev, generator=gen, dtype=torch.int64).to(torch.int32)
    d_seq = torch.arange(F * L, device=dev, dtype=torch.int32)
    offs = np.arange(F + 1, dtype=np.uint64) * np.uint64(L)
    drain = np.full(F, int(L * a.drain), dtype=np.uint64)
    flow = torch.randint(0, F, (n_new,), device=dev, generator=gen, dtype=torch.int64).to(torch.int32)
    ids = torch.randint(0, 1 << 32, (n_new,), device=dev, generator=gen, dtype=torch.int64).to(torch.int32)
    seqs = torch.arange(F * L, F * L + n_new, device=dev, dtype=torch.int64).to(torch.int32)
    h_batch = [x.cpu().numpy() for x in (flow, ids, seqs)]
    kept = int((offs[1:] - offs[:-1] - drain).sum())
    total = kept + n_new
    torch.cuda.synchronize()
    mk = lambda cls, batch, tot, up=None: cls(torch, lib, ctx, d_log, d_seq, offs, drain, batch, tot, up)  # noqa: E731
    arms = {"update": mk(Update, [flow, ids, seqs], total)}
    if not a.only_update:
        arms["update_h2d"] = mk(Update, None, total, h_batch)
        arms["update_empty"] = mk(Update, None, kept)
        arms["drain"] = mk(Drain, None, kept)
        if not a.no_host:
            arms["host"] = Host(torch, d_log, d_seq, offs, drain, h_batch)
    times = {k: [] for k in arms}
    for r in range(a.rounds + 2):            # two warm rounds: the arenas reach their size
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
    u = arms["update"]
    counts = np.bincount(h_batch[0], minlength=F)
    items = int(np.sum((offs[1:] - offs[:-1] - drain + DR_ITEM - 1) // DR_ITEM) + np.sum((counts + DR_ITEM - 1) // DR_ITEM))
    # k_log_update's algorithmic bytes: kept entries read and written in both
    # arrays; new entries: the permutation, id and seqno read, id and seqno
    # written; one 24-byte item per wave
    move_bytes = kept * 16 + n_new * 20 + items * 24
    out = {"what": "sender_log", "flows": F, "log_entries_per_flow": L, "drained_per_flow": int(drain[0]),
           "new_entries": n_new, "entries_out": total, "move_items": items, "move_bytes": move_bytes,
           "wall_ms": {k: spread(v) for k, v in times.items()}}
    if "drain" in arms:
        e, d = out["wall_ms"]["update_empty"], out["wall_ms"]["drain"]
        out["update_empty_median_within_drain_range"] = bool(d["min"] <= e["median"] <= d["max"])
        out["empty_equals_drain"] = bool(torch.equal(arms["update_empty"].out, arms["drain"].out)
                                         and torch.equal(arms["update_empty"].aout, arms["drain"].aout)
                                         and np.array_equal(arms["update_empty"].offs_out, arms["drain"].offs_out))
    if "host" in arms:
        h = arms["host"]
        out["arms_agree"] = bool(np.array_equal(u.offs_out, h.offs_out) and torch.equal(u.out, h.out)
                                 and torch.equal(u.aout, h.aout))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
