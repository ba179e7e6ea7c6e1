#!/usr/bin/env python3
"""Device-resident flow table: what a merge costs, and what a batch costs with
the table on the device against the host table it replaces.  One process,
warmed, the arms alternated; one JSON line per measurement (median, min, max).

  merge   qk_u32_flows_merge_device at na = nb = --flows, half of b's keys in a:
          HIP events around the call (its three launches and the one wait
          between them), the algorithmic bytes worked out from the shapes
          (keys + records read for a and b, keys + records + due written; the
          index arrays apart) and their share of the 8 TB/s HBM peak
  batch   --npkts records over --flows flows (bench.py's f1 shape):
            arm 1  steady encode_flows(device_out=True) alone
            arm 2  DeviceFlowQuacks.insert_packets (encode + device merge)
            arm 3  at --host-flows flows, FlowQuacks.insert_packets: the host
                   table (every record over PCIe, one host merge per flow);
                   arm 2 at that size beside it

    python tools/bench_flow_table.py [--flows 1000000] [--npkts 1e8] [--rounds 5] [--t 32]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8e12   # bytes/s, MI355X


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs)}


def flow_array(torch, lo, n, t, gen, dev):
    """Flows lo .. lo + n - 1: the flow number big-endian in the key's first
    four bytes (so ascending), canonical random sums, small counts."""
    idx = torch.arange(lo, lo + n, device=dev, dtype=torch.int64)
    keys = torch.zeros((n, 12), dtype=torch.uint8, device=dev)
    for k in range(4):
        keys[:, k] = ((idx >> (8 * (3 - k))) & 255).to(torch.uint8)
    keys[:, 6:12] = torch.tensor([192, 168, 0, 9, 0x11, 0x5C], dtype=torch.uint8, device=dev)
    sums = torch.randint(0, 4294967291, (n, 4 + t), device=dev, generator=gen, dtype=torch.int64)
    sums[:, 0] = t
    sums[:, 1] = torch.randint(1, 200, (n,), device=dev, generator=gen, dtype=torch.int64)
    sums[:, 2] = 1
    return keys, sums.to(torch.int32).contiguous()   # the conversion wraps like a C cast


def bench_merge(torch, sk, a):
    dev, t, n = "cuda:0", a.t, a.flows
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    ka, ra = flow_array(torch, 0, n, t, gen, dev)
    kb, rb = flow_array(torch, n // 2, n, t, gen, dev)
    rec = 4 * (4 + t)
    ev_ms, wall_ms, n_out = [], [], 0
    for r in range(a.rounds + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        keys, _, _ = sk.flows_merge(ka, ra, kb, rb, frequency_pkts=32)
        e1.record()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        n_out = keys.shape[0]
        if r >= 2:
            ev_ms.append(e0.elapsed_time(e1))
            wall_ms.append(dt * 1e3)
    from sidekick_amd._lib import FLOW_JOIN_TILE
    ntiles = (2 * n + FLOW_JOIN_TILE - 1) // FLOW_JOIN_TILE
    read = 2 * n * (12 + rec)
    written = n_out * (12 + rec + 1)
    index = ntiles * (FLOW_JOIN_TILE + 1) * 8          # written by the join, read by the move
    med = float(np.median(ev_ms)) * 1e-3
    # the events also cover the allocation of the output tensors: flows_merge is timed as a caller sees it
    print(json.dumps({"what": "merge", "na": n, "nb": n, "n_out": n_out, "t": t, "event_ms": spread(ev_ms),
                      "wall_ms": spread(wall_ms), "bytes_read": read, "bytes_written": written,
                      "index_bytes_written_then_read": index,
                      "algorithmic_bytes_per_s": (read + written) / med,
                      "share_of_8TBps_peak": (read + written) / med / HBM_PEAK}), flush=True)


def packet_batch(torch, n, nflows, gen, dev):
    """bench.py's f1 shape: n 67-byte records, src ip = flow number."""
    raw = torch.empty(n * 67, dtype=torch.uint8, device=dev)
    raw.random_(0, 256, generator=gen)
    rec = raw.view(n, 67)
    rec[:, 23] = 17
    f = torch.randint(0, nflows, (n,), device=dev, generator=gen, dtype=torch.int64)
    for k in range(4):
        rec[:, 26 + k] = ((f >> (8 * k)) & 255).to(torch.uint8)
    rec[:, 30:38] = torch.tensor([192, 168, 0, 9, 0x11, 0x5C, 0x1F, 0x90], dtype=torch.uint8, device=dev)
    return raw


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def bench_batch(torch, sk, a, nflows, host_arm):
    from sidekick_amd.quack import encode_flows
    dev, t, n = "cuda:0", a.t, int(a.npkts)
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    raw = packet_batch(torch, n, nflows, gen, dev)
    ctx = sk.get_context(0)
    table, htable = sk.DeviceFlowQuacks(t), sk.FlowQuacks(t) if host_arm else None
    cap = nflows + nflows // 8
    arms = {"encode_flows_device_out": lambda: encode_flows(raw, t, ctx=ctx, device_out=True, cap=cap),
            "DeviceFlowQuacks.insert_packets": lambda: table.insert_packets(raw)}
    if host_arm:
        arms["FlowQuacks.insert_packets"] = lambda: htable.insert_packets(raw)
    times = {k: [] for k in arms}
    for r in range(a.rounds + 2):          # two warm rounds: the table and its two buffers reach their size
        for name, fn in arms.items():
            ms, _ = timed(torch, fn)
            if r >= 2:
                times[name].append(ms)
    print(json.dumps({"what": "batch", "n_packets": n, "flows": nflows, "t": t, "table_flows": len(table),
                      "wall_ms": {k: spread(v) for k, v in times.items()}}), flush=True)
    del raw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=float, default=1e6)
    ap.add_argument("--host-flows", type=float, default=1e5)
    ap.add_argument("--npkts", type=float, default=1e8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--t", type=int, default=32)
    a = ap.parse_args()
    a.flows, a.host_flows = int(a.flows), int(a.host_flows)
    a.rounds = max(a.rounds, 5)
    import torch
    import sidekick_amd as sk
    bench_merge(torch, sk, a)
    bench_batch(torch, sk, a, a.flows, host_arm=False)
    bench_batch(torch, sk, a, a.host_flows, host_arm=True)


if __name__ == "__main__":
    main()
