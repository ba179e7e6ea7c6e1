#!/usr/bin/env python3
"""What the Python layer costs per call: the per-flow wrappers of
sidekick_amd/quack.py on batches so small that the kernels are short and the
argument handling (checks, pointers, CSR offsets, the retry loop, the hit
split) is a visible share of the call.  The other bench_* tools call the C ABI
directly; this one goes through the wrappers.  One process, warmed, the arms
alternated; one JSON line (median, min, max in ms of --rounds calls per arm,
each call synchronised).

    python tools/bench_wrappers.py [--flows 64] [--len 40] [--t 32] [--rounds 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P = 4294967291


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=int, default=64)
    ap.add_argument("--len", type=int, default=40)
    ap.add_argument("--t", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=200)
    a = ap.parse_args()
    import torch
    import sidekick_amd as sk
    nf, ln, t = a.flows, a.len, a.t
    rng = np.random.default_rng(5)
    ids = np.unique(rng.integers(256, P - 256, size=2 * nf * ln, dtype=np.uint64))
    log = rng.permutation(ids)[:nf * ln].astype(np.uint32)
    offs = np.arange(nf + 1, dtype=np.uint64) * ln
    lost = [rng.choice(ln - 1, size=min(t, ln - 1) // 2, replace=False) for _ in range(nf)]

    def sketch(ids):
        q = sk.PowerSumQuackU32(t)
        for v in ids:
            q.insert(int(v))
        return q

    def tensor(qs):
        return torch.from_numpy(np.stack([np.frombuffer(q._buf, dtype=np.int32) for q in qs])).cuda()

    segs = [log[g * ln:(g + 1) * ln] for g in range(nf)]
    diffs = [sketch(s[m]) for s, m in zip(segs, lost)]
    peers = [sketch(np.delete(s, m)) for s, m in zip(segs, lost)]
    d_diffs, d_peers, d_mine = tensor(diffs), tensor(peers), tensor([sk.PowerSumQuackU32(t)] * nf)
    d_log = torch.from_numpy(log.view(np.int32)).cuda()
    drain = np.full(nf, ln // 2, dtype=np.uint64)
    new_flow = torch.arange(nf, dtype=torch.int32, device="cuda")
    keys = np.zeros((2 * nf, 12), dtype=np.uint8)
    keys[:, 8:] = np.arange(2 * nf, dtype=">u4").view(np.uint8).reshape(-1, 4)
    ka, kb = torch.from_numpy(keys[:nf + nf // 2]).cuda(), torch.from_numpy(keys[nf // 2:]).cuda()
    sa, sb = tensor((diffs + peers)[:nf + nf // 2]), tensor((peers + diffs)[nf // 2:])
    _, _, wire, lens = sk.emit_wire(None, d_peers)
    flow = torch.arange(nf, dtype=torch.int32, device="cuda")
    peer_out = d_peers.clone()
    arms = {
        "decode_segments": lambda: sk.decode_segments(d_diffs, d_log, offs),
        "decode_segments_host_list": lambda: sk.decode_segments(diffs, d_log, offs),
        "to_coeffs_segments": lambda: sk.to_coeffs_segments(d_diffs),
        "sender_step": lambda: sk.sender_step(d_mine, d_peers, d_log, offs),
        "drain_segments": lambda: sk.drain_segments(d_log, offs, drain),
        "update_segments": lambda: sk.update_segments(d_log, offs, drain, new_flow, new_flow),
        "flows_merge": lambda: sk.flows_merge(ka, sa, kb, sb),
        "flows_diff": lambda: sk.flows_diff(ka, sa, kb, sb),
        "flows_lookup": lambda: sk.flows_lookup(ka, sa, [keys[0].tobytes(), keys[nf].tobytes()]),
        "emit_wire": lambda: sk.emit_wire(ka, sa),
        "ingest_wire": lambda: sk.ingest_wire(wire, lens, flow, nf, t, peer=peer_out),
        "decode_host_x100": lambda: [diffs[g % nf].decode_host(segs[g % nf]) for g in range(100)],
        "clone_x1000": lambda: [diffs[0].clone() for _ in range(1000)],
    }
    times = {k: [] for k in arms}
    for r in range(a.rounds + 20):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= 20:
                times[name].append((time.perf_counter() - t0) * 1e3)
    out = {"what": "wrappers", "flows": nf, "len": ln, "t": t, "rounds": a.rounds,
           "wall_ms": {k: {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4),
                           "max": round(float(np.max(v)), 4)} for k, v in times.items()}}
    pos, status = sk.decode_segments(d_diffs, d_log, offs)
    out["decode_equal"] = bool(all(p == sorted(m.tolist()) for p, m in zip(pos, lost)) and not any(status))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
