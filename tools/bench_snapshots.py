#!/usr/bin/env python3
"""Per-flow quACK snapshots: what the quACKs of every frequency crossing of a
batch cost on the device, against the same records composed from what existed
before the call, and against a plain copy of the output bytes.  One process,
warmed, the arms alternated; one JSON line per frequency (median, min, max of
--rounds calls per arm).

  snapshot        qk_u32_snapshot_segments_device through the C ABI with
                  preallocated outputs: --flows flows of --len ids, threshold
                  --t, base counts of random phase (below 2^31: no wrap), the
                  final records written too
  copy            a device-to-device copy of the snapshot records: the yardstick
  snapshot_small  the same call over the first --composed-flows flows
  composed        those flows' records from what exists without the call: the
                  base counts read back, the cut positions on the host,
                  qk_u32_encode_segments_device over the intervals between cuts
                  (sketches to the host), the per-flow running sums in numpy

    python tools/bench_snapshots.py [--flows 100000] [--len 1000] [--t 32] [--freqs 2,32] [--rounds 10]
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
P32 = 4294967291


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs),
            "samples": [round(float(x), 4) for x in xs]}


def p64(a):
    return a.ctypes.data_as(U64P)


class Snapshot:
    def __init__(self, torch, lib, ctx, base, ids, offs, t, f, cap):
        self.lib, self.ctx, self.base, self.ids, self.offs, self.t, self.f, self.cap = lib, ctx, base, ids, offs, t, f, cap
        nseg, dev = len(offs) - 1, ids.device
        self.rec = torch.empty((cap, 4 + t), dtype=torch.int32, device=dev)
        self.seg = torch.empty((cap,), dtype=torch.int32, device=dev)
        self.pos = torch.empty((cap,), dtype=torch.int64, device=dev)
        self.fin = torch.empty((nseg, 4 + t), dtype=torch.int32, device=dev)
        self.snoffs = np.zeros(nseg + 1, dtype=np.uint64)
        self.m = C.c_size_t()

    def __call__(self):
        rc = self.lib.qk_u32_snapshot_segments_device(
            self.ctx.handle, self.base.data_ptr(), self.ids.data_ptr(), None, p64(self.offs), len(self.offs) - 1,
            self.t, self.f, self.rec.data_ptr(), self.seg.data_ptr(), self.pos.data_ptr(), None, self.cap,
            p64(self.snoffs), C.byref(self.m), self.fin.data_ptr(), None)
        assert rc == 0, rc


class Copy:
    def __init__(self, torch, src):
        self.src, self.dst = src, torch.empty_like(src)

    def __call__(self):
        self.dst.copy_(self.src)


class Composed:
    """The records without the call: counts to the host, cuts on the host, one
    segmented encode over the intervals, running sums in numpy."""

    def __init__(self, lib, ctx, base, ids, offs, t, f):
        self.lib, self.ctx, self.base, self.ids, self.offs, self.t, self.f = lib, ctx, base, ids, offs, t, f

    def __call__(self):
        t, f, W = self.t, self.f, 4 + self.t
        nseg = len(self.offs) - 1
        hb = self.base.cpu().numpy().view(np.uint32)
        c0 = hb[:, 1].astype(np.int64)
        lens = (self.offs[1:] - self.offs[:-1]).astype(np.int64)
        j0 = (-(c0 + 1)) % f                                   # the first cut of every flow
        m = np.where(j0 < lens, (lens - j0 + f - 1) // f, 0)   # its cuts
        first = np.cumsum(m) - m
        flow = np.repeat(np.arange(nseg), m)
        k = np.arange(int(m.sum())) - first[flow]
        cut = self.offs[:-1].astype(np.int64)[flow] + j0[flow] + k * f      # positions of the triggering packets
        # CSR over the intervals: every flow's start, and the position after each cut (the tails are segments too)
        bounds = np.unique(np.concatenate([self.offs.astype(np.int64), cut + 1])).astype(np.uint64)
        ns = len(bounds) - 1
        sk = np.empty((ns, W), dtype=np.uint32)
        rc = self.lib.qk_u32_encode_segments_device(self.ctx.handle, self.ids.data_ptr(), p64(bounds), ns, t,
                                                    sk.ctypes.data_as(C.POINTER(C.c_uint8)), None)
        assert rc == 0, rc
        rows = np.searchsorted(bounds, (cut + 1).astype(np.uint64)) - 1       # the interval that ends at each cut
        part = sk[rows, 4:].astype(np.uint64)
        run = np.cumsum(part, axis=0)                          # < 2^64: rows * 2^32
        start = np.zeros((nseg, t), dtype=np.uint64)
        has = m > 0
        start[has] = run[first[has]] - part[first[has]]
        sums = (run - start[flow]) % np.uint64(P32)
        sums = (sums + hb[flow, 4:].astype(np.uint64)) % np.uint64(P32)
        rec = np.empty((len(cut), W), dtype=np.uint32)
        rec[:, 0], rec[:, 1], rec[:, 2] = t, (c0[flow] + (cut - self.offs[:-1].astype(np.int64)[flow]) + 1) & 0xFFFFFFFF, 1
        rec[:, 3] = sk[rows, 3]
        rec[:, 4:] = sums
        self.rec = rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=float, default=1e5)
    ap.add_argument("--len", type=int, default=1000)
    ap.add_argument("--t", type=int, default=32)
    ap.add_argument("--freqs", default="2,32")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--composed-flows", type=float, default=2000, help="flows of the composed arm (0: leave it out)")
    ap.add_argument("--only-snapshot", action="store_true", help="the new call alone (kernel traces)")
    a = ap.parse_args()
    F, L, t, Fc = int(a.flows), a.len, a.t, min(int(a.composed_flows), int(a.flows))
    import torch
    import sidekick_amd as sk
    from sidekick_amd._lib import lib as load
    lib, ctx = load(), sk.get_context(0)
    dev = "cuda:0"
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5A4B50)
    ids = torch.randint(0, 1 << 32, (F * L,), device=dev, generator=gen, dtype=torch.int64).to(torch.int32)
    base = torch.randint(0, P32, (F, 4 + t), device=dev, generator=gen, dtype=torch.int64).to(torch.int32)
    base[:, 0], base[:, 2] = t, 1
    base[:, 1] = torch.randint(0, 1 << 31, (F,), device=dev, generator=gen, dtype=torch.int64).to(torch.int32)
    offs = np.arange(F + 1, dtype=np.uint64) * np.uint64(L)
    torch.cuda.synchronize()
    for f in [int(x) for x in a.freqs.split(",")]:
        cap = F * (L // f + 1)
        arms = {"snapshot": Snapshot(torch, lib, ctx, base, ids, offs, t, f, cap)}
        arms["snapshot"]()
        torch.cuda.synchronize()
        m = arms["snapshot"].m.value
        if not a.only_snapshot:
            arms["copy"] = Copy(torch, arms["snapshot"].rec[:m])
            if Fc:
                arms["snapshot_small"] = Snapshot(torch, lib, ctx, base[:Fc], ids, offs[:Fc + 1], t, f, Fc * (L // f + 1))
                arms["composed"] = Composed(lib, ctx, base[:Fc], ids, offs[:Fc + 1], t, f)
        times = {k: [] for k in arms}
        for r in range(a.rounds + 2):            # two warm rounds: the arenas reach their size
            for name, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r >= 2:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        W = 4 + t
        # the call's algorithmic bytes: ids read once, every record written once, seg and pos, base read, final written
        moved = F * L * 4 + m * (W * 4 + 12) + 2 * F * W * 4
        out = {"what": "snapshots", "flows": F, "ids_per_flow": L, "threshold": t, "frequency_pkts": f, "snapshots": m,
               "record_bytes": m * W * 4, "bytes_moved": moved, "wall_ms": {k: spread(v) for k, v in times.items()}}
        s = out["wall_ms"]["snapshot"]
        out["snapshot_gbps"] = round(moved / s["median"] / 1e6, 1)
        if "composed" in arms:
            small, comp = arms["snapshot_small"], arms["composed"]
            ms = small.m.value
            out["composed_flows"] = Fc
            out["arms_agree"] = bool(ms == len(comp.rec)
                                     and np.array_equal(small.rec[:ms].cpu().numpy().view(np.uint32), comp.rec))
            a_, b_ = out["wall_ms"]["snapshot_small"], out["wall_ms"]["composed"]
            out["faster_by_more_than_both_spreads"] = bool(
                b_["median"] - a_["median"] > max(a_["max"] - a_["min"], b_["max"] - b_["min"]))
        print(json.dumps(out), flush=True)
        del arms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
