#!/usr/bin/env python3
"""Device wire leg: what emitting the due flows' bincode images and ingesting a
batch of datagrams cost on the device, against the per-flow host paths they
replace and against a plain device copy of the same bytes.  One process,
warmed, the arms alternated; one JSON line per selection (median, min, max of
--rounds calls).

  emit         qk_u32_flows_emit_device through the C ABI, outputs preallocated:
               --flows flows of T = --t, a fraction --select of them selected
  ingest       qk_u32_wire_ingest_device on the images emit wrote, one per flow
  loop         emit, the images and lengths copied to the host and back, ingest
  host_emit    what the proxy could do before: flows_lookup of the selected
               keys (one PowerSumQuackU32 per flow), .serialize() per flow
  host_ingest  what the sender could do before: PowerSumQuackU32.deserialize
               per datagram, then the record tensor uploaded (Records.to_device)
  copy         the yardstick: torch copy, device to device, of the image bytes

    python tools/bench_wire.py [--flows 100000] [--t 32] [--select 0.1 1.0] [--rounds 10]
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


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs),
            "samples": [round(float(x), 4) for x in xs]}


def make_table(torch, n, t, seed):
    """A flow array: ascending 12-byte keys, random canonical records."""
    rng = np.random.default_rng(seed)
    keys = np.zeros((n, 12), dtype=np.uint8)
    keys[:, 8:] = np.arange(n, dtype=">u4").view(np.uint8).reshape(n, 4)
    recs = np.zeros((n, 4 + t), dtype=np.uint32)
    recs[:, 0] = t
    recs[:, 1] = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    recs[:, 2] = rng.random(n) < 0.9
    recs[:, 3] = rng.integers(0, 1 << 32, size=n, dtype=np.uint64) * recs[:, 2]
    recs[:, 4:] = rng.integers(0, P, size=(n, t), dtype=np.uint64)
    return keys, recs, torch.from_numpy(keys).cuda(), torch.from_numpy(recs.view(np.int32)).cuda()


def run(torch, sk, lib, ctx, a, frac):
    from sidekick_amd._args import Records
    from sidekick_amd.quack import flows_lookup
    n, t = a.flows, a.t
    stride = sk.wire_max(t)
    keys, recs, d_keys, d_recs = make_table(torch, n, t, 7)
    sel = np.random.default_rng(9).random(n) < frac if frac < 1 else np.ones(n, dtype=bool)
    m = int(sel.sum())
    d_sel = torch.from_numpy(sel.astype(np.uint8)).cuda()
    keys_out = torch.empty((m, 12), dtype=torch.uint8, device="cuda")
    rows = torch.empty((m,), dtype=torch.int32, device="cuda")
    wire = torch.empty((m, stride), dtype=torch.uint8, device="cuda")
    lens = torch.empty((m,), dtype=torch.int32, device="cuda")
    wire2, lens2 = torch.empty_like(wire), torch.empty_like(lens)
    peer = torch.empty((n, 4 + t), dtype=torch.int32, device="cuda")
    present = torch.empty((n,), dtype=torch.uint8, device="cuda")
    status = np.zeros(m, dtype=np.int32)
    copy_dst = torch.empty_like(wire)
    n_out, acc = C.c_size_t(), C.c_size_t()
    state = {}

    def emit():
        rc = lib.qk_u32_flows_emit_device(ctx.handle, d_keys.data_ptr(), d_recs.data_ptr(), n, t, d_sel.data_ptr(), stride,
                                          keys_out.data_ptr(), rows.data_ptr(), wire.data_ptr(), lens.data_ptr(), m,
                                          C.byref(n_out), None)
        assert rc == 0 and n_out.value == m, (rc, n_out.value)

    def ingest(w=wire, ln=lens):
        rc = lib.qk_u32_wire_ingest_device(ctx.handle, w.data_ptr(), stride, ln.data_ptr(), rows.data_ptr(), m, t, n,
                                           peer.data_ptr(), present.data_ptr(),
                                           status.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(acc), None)
        assert rc == 0 and acc.value == m, (rc, acc.value)

    def loop():
        emit()
        h_wire, h_lens = wire.cpu(), lens.cpu()          # the images cross to the host (the sockets' side)
        wire2.copy_(h_wire)
        lens2.copy_(h_lens)
        ingest(wire2, lens2)

    def host_emit():
        wanted = [keys[i].tobytes() for i in np.flatnonzero(sel)]
        state["images"] = [q.serialize() for q in flows_lookup(d_keys, d_recs, wanted, ctx)]

    def host_ingest():
        quacks = [sk.PowerSumQuackU32.deserialize(b) for b in state["images"]]
        state["peer"] = Records.parse(quacks, sk.PowerSumQuackU32).to_device(ctx, "peer")

    def copy():
        copy_dst.copy_(wire)

    arms = {"emit": emit, "ingest": ingest, "loop": loop, "copy": copy}
    if not a.no_host:
        arms["host_emit"] = host_emit
        arms["host_ingest"] = host_ingest
    times = {k: [] for k in arms}
    for r in range(a.rounds + 2):            # two warm rounds: the scratch reaches its size
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
    out = {"what": "wire", "flows": n, "t": t, "selected": m, "stride": stride, "image_bytes": m * stride,
           "wall_ms": {k: spread(v) for k, v in times.items()}}
    med = {k: v["median"] for k, v in out["wall_ms"].items()}
    out["emit_over_copy"] = round(med["emit"] / med["copy"], 2)
    out["ingest_over_copy"] = round(med["ingest"] / med["copy"], 2)
    # the arms agree: the round trip reproduces the selected records, and the host path the same images
    got = peer.cpu().numpy().view(np.uint32)
    want = recs[sel].copy()
    want[want[:, 2] == 0, 3] = 0
    out["round_trip_equal"] = bool(np.array_equal(got[sel], want) and np.array_equal(present.cpu().numpy(), sel))
    if not a.no_host:
        h_wire, h_lens = wire.cpu().numpy(), lens.cpu().numpy()
        out["host_images_equal"] = bool(all(h_wire[r, :h_lens[r]].tobytes() == b for r, b in enumerate(state["images"])))
        out["host_over_device"] = {"emit": round(med["host_emit"] / med["emit"], 1),
                                   "ingest": round(med["host_ingest"] / med["ingest"], 1)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=float, default=1e5)
    ap.add_argument("--t", type=int, default=32)
    ap.add_argument("--select", type=float, nargs="+", default=[0.1, 1.0])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="time the device arms alone (e.g. under a profiler)")
    a = ap.parse_args()
    a.flows = int(a.flows)
    import torch
    import sidekick_amd as sk
    from sidekick_amd._lib import lib as load
    lib, ctx = load(), sk.get_context(0)
    for frac in a.select:
        run(torch, sk, lib, ctx, a, frac)


if __name__ == "__main__":
    main()
