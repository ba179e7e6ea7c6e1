#!/usr/bin/env python3
"""The proxy loop on captured packets: what every due quACK of a capture batch
costs on the device against the flow table held by AddrKey
(qk_u32_snapshot_flows_device), beside the calls it joins.  One process, warmed,
the arms alternated; one JSON line per frequency (median, min, max of --rounds
calls per arm).

  packets         the new call through the C ABI with preallocated outputs:
                  --records 67-byte records over --flows flows, threshold --t,
                  the table already holding the flows, base counts of random
                  phase; no Reset in the batch
  end_of_batch    (a) the path it extends: qk_u32_encode_flows_device (device
                  output) + qk_u32_flows_merge_device into the same table
  segments        (b) qk_u32_snapshot_segments_device alone on the same ids,
                  grouped by flow beforehand (outside the timing), the same base
                  records, the final records written too
  packets_small   the new call over the first --composed-records records, empty table
  composed        (c) those records through what existed before the call:
                  encode_flows for the keys, the keys and the captures to the
                  host, the flows numbered there, DeviceFlowSnapshots.insert;
                  checked to agree bit for bit with packets_small

    python tools/bench_packet_snapshots.py [--records 1e8] [--flows 1e5] [--t 32] [--freqs 2,32] [--rounds 10]
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
STRIDE = 67


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs),
            "samples": [round(float(x), 4) for x in xs]}


class Packets:
    def __init__(self, torch, sk, lib, ctx, bufs, n, t, f, keys, recs, snap_cap):
        from sidekick_amd.quack import PktStats
        self.lib, self.ctx, self.bufs, self.n, self.t, self.f, self.keys, self.recs = lib, ctx, bufs, n, t, f, keys, recs
        dev, nt = bufs.device, 0 if keys is None else keys.shape[0]
        self.nt, self.tcap, self.scap = nt, nt + min(n, 1 << 20), snap_cap
        self.ko = torch.empty((self.tcap, 12), dtype=torch.uint8, device=dev)
        self.so = torch.empty((self.tcap, 4 + t), dtype=torch.int32, device=dev)
        self.rec = torch.empty((snap_cap, 4 + t), dtype=torch.int32, device=dev)
        self.sk = torch.empty((snap_cap, 12), dtype=torch.uint8, device=dev)
        self.si = torch.empty((snap_cap,), dtype=torch.int32, device=dev)
        self.ntab, self.m, self.st = C.c_size_t(), C.c_size_t(), PktStats()

    def __call__(self):
        rc = self.lib.qk_u32_snapshot_flows_device(
            self.ctx.handle, self.bufs.data_ptr(), self.n, STRIDE, None, None, self.t, self.f,
            self.keys.data_ptr() if self.nt else None, self.recs.data_ptr() if self.nt else None, self.nt,
            self.ko.data_ptr(), self.so.data_ptr(), self.tcap, C.byref(self.ntab), self.rec.data_ptr(),
            self.sk.data_ptr(), self.si.data_ptr(), self.scap, C.byref(self.m), C.byref(self.st), None)
        assert rc == 0, rc


class EndOfBatch:
    def __init__(self, torch, sk, ctx, bufs, t, f, keys, recs, flows):
        self.sk, self.ctx, self.bufs, self.t, self.f, self.keys, self.recs, self.cap = sk, ctx, bufs, t, f, keys, recs, flows + 1024

    def __call__(self):
        k, s, _ = self.sk.quack.encode_flows(self.bufs, self.t, STRIDE, ctx=self.ctx, device_out=True, cap=self.cap)
        self.out = self.sk.flows_merge(self.keys, self.recs, k, s, self.f, ctx=self.ctx)


class Segments:
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
            self.ctx.handle, self.base.data_ptr(), self.ids.data_ptr(), None, self.offs.ctypes.data_as(U64P),
            len(self.offs) - 1, self.t, self.f, self.rec.data_ptr(), self.seg.data_ptr(), self.pos.data_ptr(), None,
            self.cap, self.snoffs.ctypes.data_as(U64P), C.byref(self.m), self.fin.data_ptr(), None)
        assert rc == 0, rc


class Composed:
    """Today's route to the same datagrams: the batch's keys from encode_flows,
    keys and captures to the host, the flows numbered there by key rank,
    DeviceFlowSnapshots.insert (its own grouping, walk and argsort)."""

    def __init__(self, sk, ctx, bufs, n, t, f):
        self.sk, self.ctx, self.bufs, self.n, self.t, self.f = sk, ctx, bufs, n, t, f

    def __call__(self):
        keys, _, _ = self.sk.quack.encode_flows(self.bufs, self.t, STRIDE, ctx=self.ctx, device_out=True, cap=1 << 17)
        hk = keys.cpu().numpy()
        raw = self.bufs.cpu().numpy().reshape(self.n, STRIDE)
        pk = np.concatenate([raw[:, 26:30], raw[:, 34:36], raw[:, 30:34], raw[:, 36:38]], axis=1)
        void = np.dtype((np.void, 12))
        flow = np.searchsorted(np.ascontiguousarray(hk).view(void).ravel(), np.ascontiguousarray(pk).view(void).ravel())
        ids = raw[:, 63:67].astype(np.uint32)
        ids = (ids[:, 0] << 24) | (ids[:, 1] << 16) | (ids[:, 2] << 8) | ids[:, 3]
        table = self.sk.DeviceFlowSnapshots(self.t, len(hk), self.f)
        self.seg, _, _, self.rec = table.insert(flow.astype(np.uint32), ids)
        self.keys = hk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=float, default=1e8)
    ap.add_argument("--flows", type=float, default=1e5)
    ap.add_argument("--t", type=int, default=32)
    ap.add_argument("--freqs", default="2,32")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--composed-records", type=float, default=2e6, help="records of the composed arm (0: leave it out)")
    ap.add_argument("--only-packets", action="store_true", help="the new call alone (kernel traces)")
    a = ap.parse_args()
    n, F, t, nc = int(a.records), int(a.flows), a.t, min(int(a.composed_records), int(a.records))
    import torch
    import sidekick_amd as sk
    from sidekick_amd._lib import lib as load
    lib, ctx = load(), sk.get_context(0)
    dev = "cuda:0"
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x504B54)
    # F distinct AddrKeys, ascending (the first four bytes count up); every record an Insert of a random id
    fk = torch.randint(0, 256, (F, 12), device=dev, generator=gen, dtype=torch.int64).to(torch.uint8)
    idx = torch.arange(F, device=dev)
    for b in range(4):
        fk[:, b] = ((idx >> (24 - 8 * b)) & 0xFF).to(torch.uint8)
    fk[:, 6:10] = torch.tensor([192, 168, 0, 9], dtype=torch.uint8, device=dev)
    flow = torch.randint(0, F, (n,), device=dev, generator=gen)
    bufs = torch.empty((n, STRIDE), dtype=torch.uint8, device=dev)
    step = 1 << 24
    for lo in range(0, n, step):          # in slices: the int64 draw of a whole batch would take 8 bytes per byte
        hi = min(n, lo + step)
        bufs[lo:hi] = torch.randint(0, 256, (hi - lo, STRIDE), device=dev, generator=gen, dtype=torch.uint8)
        k = fk[flow[lo:hi]]
        bufs[lo:hi, 26:30], bufs[lo:hi, 34:36], bufs[lo:hi, 30:34], bufs[lo:hi, 36:38] = \
            k[:, 0:4], k[:, 4:6], k[:, 6:10], k[:, 10:12]
    bufs[:, 23] = 17
    idb = bufs[:, 63:67].to(torch.int64)
    ids = ((idb[:, 0] << 24) | (idb[:, 1] << 16) | (idb[:, 2] << 8) | idb[:, 3]).to(torch.int32)
    del idb
    bufs = bufs.reshape(-1)
    # the table: every flow, random sums, base counts of random phase (below 2^31: no wrap)
    recs = torch.randint(0, P32, (F, 4 + t), device=dev, generator=gen, dtype=torch.int64).to(torch.int32)
    recs[:, 0], recs[:, 2] = t, 1
    recs[:, 1] = torch.randint(0, 1 << 31, (F,), device=dev, generator=gen, dtype=torch.int64).to(torch.int32)
    # (b)'s input: the ids grouped by flow, stably, outside the timing
    order = torch.sort(flow, stable=True).indices
    grouped = ids[order].contiguous()
    counts = torch.bincount(flow, minlength=F).cpu().numpy().astype(np.uint64)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    del order, flow
    torch.cuda.synchronize()
    for f in [int(x) for x in a.freqs.split(",")]:
        cap = n // f + F + 1024
        arms = {"packets": Packets(torch, sk, lib, ctx, bufs, n, t, f, fk, recs, cap)}
        arms["packets"]()
        torch.cuda.synchronize()
        m = arms["packets"].m.value
        if not a.only_packets:
            arms["end_of_batch"] = EndOfBatch(torch, sk, ctx, bufs, t, f, fk, recs, F)
            arms["segments"] = Segments(torch, lib, ctx, recs, grouped, offs, t, f, cap)
            if nc:
                arms["packets_small"] = Packets(torch, sk, lib, ctx, bufs[:nc * STRIDE], nc, t, f, None, None, nc // f + F + 1024)
                arms["composed"] = Composed(sk, ctx, bufs[:nc * STRIDE], nc, t, f)
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
        out = {"what": "packet_snapshots", "records": n, "flows": F, "threshold": t, "frequency_pkts": f, "snapshots": m,
               "record_bytes": n * STRIDE, "snapshot_bytes": m * (W * 4 + 16),
               "wall_ms": {k: spread(v) for k, v in times.items()}}
        if "segments" in arms:
            p, e, s = (out["wall_ms"][k]["median"] for k in ("packets", "end_of_batch", "segments"))
            out["packets_over_a_plus_b"] = round(p / (e + s), 3)
            seg = arms["segments"]
            # the two calls emit the same snapshots: as a multiset of records (theirs by flow, ours in send order)
            out["segments_snapshots"] = seg.m.value
            out["final_tables_agree"] = bool(torch.equal(seg.fin, arms["packets"].so[:arms["packets"].ntab.value]))
        if "composed" in arms:
            small, comp = arms["packets_small"], arms["composed"]
            ms = small.m.value
            out["composed_records"] = nc
            rank = {k.tobytes(): j for j, k in enumerate(comp.keys)}
            out["arms_agree"] = bool(
                ms == comp.rec.shape[0] and torch.equal(small.rec[:ms], comp.rec)
                and [rank[bytes(k)] for k in small.sk[:ms].cpu().numpy()] == comp.seg.cpu().tolist())
        print(json.dumps(out), flush=True)
        del arms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
