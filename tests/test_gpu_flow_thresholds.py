"""Segmented encode (qk_u32_encode_segments_device) and per-flow batch
(FlowQuacks.insert_packets) at every threshold where the work-item kernel
k_seg_encode<G, K> changes shape: both ends of the range of each (G, K) that
seg_choose can produce, up to QK_MAX_THRESHOLD.  Bit for bit against the C
oracle; all arithmetic is integer.

The dispatch rule is restated here (choose) and guarded by a CPU test that
reads the constants out of segments.hip / segments.h / bsgs.h."""
import os
import re

import numpy as np
import pytest

from oracle import coracle, quack_oracle as qo
from test_flows import MY_ADDR, make_flows, vector_flows

gpu = pytest.mark.gpu

P = qo.P32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sidekick_amd", "csrc")

# ---- the rule, restated
KS = (4, 8, 16, 20, 24, 32)        # chain lengths k_seg_encode is built for
BSGS = range(5, 81)                # thresholds of the baby-step/giant-step work-item kernel
SMALL_T = 32                       # small_ok(T): the lane-per-segment kernel takes segments <= SMALL_SEG
SMALL_SEG = 4096
SEG_CHUNK = 65536
BLOCK = 256
MAX_T = 1024

# both ends of every reachable (G, K) range; 1 and 81 (the low ends of (1, 4)
# and (4, 24)) also run in test_flows.py
THRESHOLDS = (1, 2, 3, 4, 81, 82, 96, 97, 128, 129, 160, 161, 192, 193, 256, 257, 320, 321, 384, 385, 512, 513, 640, 641,
              768, 769, 1023, 1024)
FLOW_THRESHOLDS = (81, 129, 257, 513, 1024)
EDGE_IDS = (0, 1, P - 1, P, P + 1, 2**32 - 1, 2**31)


def choose(t):
    """(G, K) of k_seg_encode at threshold t: G the smallest power of two with
    ceil(t / G) <= 32, K the first supported chain length >= ceil(t / G)."""
    g = 1
    while -(-t // g) > 32:
        g *= 2
    return g, next(k for k in KS if k >= -(-t // g))


def reachable():
    """{(G, K): (lowest t, highest t)} over the thresholds that take k_seg_encode."""
    out = {}
    for t in range(1, MAX_T + 1):
        if t not in BSGS:
            lo, _ = out.get(choose(t), (t, t))
            out[choose(t)] = (lo, t)
    return out


def test_dispatch_rule_is_the_sources_and_the_list_covers_it():
    hip = open(os.path.join(CSRC, "segments.hip")).read()
    hdr = open(os.path.join(CSRC, "segments.h")).read()
    bsgs = open(os.path.join(CSRC, "bsgs.h")).read()
    api = open(os.path.join(ROOT, "include", "quack_hip.h")).read()
    ks = re.search(r"static const int ks\[\] = \{([\d, ]+)\};", hip).group(1)
    assert tuple(int(v) for v in ks.split(",")) == KS
    assert re.search(r"while \(\(T \+ G - 1\) / G > (\d+)u\) G \*= 2;", hip).group(1) == str(KS[-1])
    cases = [int(v) for v in re.findall(r"case (\d+): return seg_launch_gk<G, \d+>", hip)]
    assert cases + [32] == list(KS)                                    # every K has a kernel (32: the default)
    lo, hi = re.search(r"if \(T >= (\d+) && T <= (\d+)\) \{", hip).groups()
    assert (int(lo), int(hi)) == (BSGS[0], BSGS[-1])
    assert int(re.search(r"constexpr uint64_t SMALL_SEG = (\d+);", hdr).group(1)) == SMALL_SEG
    assert 1 << int(re.search(r"constexpr uint32_t SEG_CHUNK = 1u << (\d+);", hdr).group(1)) == SEG_CHUNK
    assert int(re.search(r"inline bool small_ok\(uint32_t T\) \{ return T <= (\d+); \}", hdr).group(1)) == SMALL_T
    assert "constexpr int SG_BLOCK = bsgs::BLOCK;" in hip
    assert int(re.search(r"constexpr int BLOCK = (\d+);", bsgs).group(1)) == BLOCK
    assert int(re.search(r"#define QK_MAX_THRESHOLD (\d+)u", api).group(1)) == MAX_T
    # the shapes the rule can produce, and both ends of each in the list
    shapes = reachable()
    assert sorted(shapes) == [(1, 4), (4, 24), (4, 32), (8, 20), (8, 24), (8, 32), (16, 20), (16, 24), (16, 32),
                              (32, 20), (32, 24), (32, 32)]
    assert all(g in (1, 4, 8, 16, 32) and g * k >= hi for (g, k), (_, hi) in shapes.items())
    for gk, (lo, hi) in shapes.items():
        assert lo in THRESHOLDS and hi in THRESHOLDS, (gk, lo, hi)
    assert all(t not in BSGS and 1 <= t <= MAX_T for t in THRESHOLDS)
    # the per-flow batch sends every flow through the work items above small_ok, at every group width
    assert all(t > SMALL_T and t not in BSGS for t in FLOW_THRESHOLDS)
    assert {choose(t)[0] for t in FLOW_THRESHOLDS} == {4, 8, 16, 32} and MAX_T in FLOW_THRESHOLDS


def segment_case(t, extra=0):
    """(ids with `extra` spare words at the end, offsets) of the grouped array at threshold t."""
    S = BLOCK // choose(t)[0]                      # ids per workgroup step
    lens = [0, 1, S - 1, S, S + 1, 4 * S + 3, 0, SEG_CHUNK, SEG_CHUNK + 1]
    if t <= 4:
        lens += [SMALL_SEG, SMALL_SEG + 1]         # the last lane-per-segment length, the first work item
    lens.append(1)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = coracle.splitmix_u32(0x7E5 + t, int(offs[-1]) + extra)
    ids[offs[2]:offs[3]] = np.resize(np.array(EDGE_IDS, dtype=np.uint32), S - 1)      # edge ids only
    where = [offs[3], offs[4] - 1, offs[4], offs[5] - 1, offs[8], offs[9] - 1]        # first / last of S, S + 1, 65537
    for j, pos in enumerate(where):
        ids[pos] = EDGE_IDS[(j + t) % len(EDGE_IDS)]
    assert offs[9] - offs[8] == SEG_CHUNK + 1 and S - 1 >= len(EDGE_IDS)
    return ids, offs


def check_segments(qs, ids, offs, t, tag=None):
    assert len(qs) == len(offs) - 1
    for g, q in enumerate(qs):
        seg = ids[offs[g]:offs[g + 1]]
        assert q.threshold() == t
        assert q.count() == len(seg) and q.last_value() == (int(seg[-1]) if len(seg) else None), (tag, g)
        want = coracle.encode_u32(seg, t)
        got = q.power_sums()
        if got != want:
            bad = [m + 1 for m in range(t) if got[m] != want[m]]
            raise AssertionError(f"t={t} (G, K)={choose(t)} {tag}: segment {g} of {len(seg)} ids, powers {bad[:8]} "
                                 f"({len(bad)} wrong)")


@gpu
@pytest.mark.parametrize("t", THRESHOLDS)
def test_gpu_encode_segments_at_threshold(t):
    import torch
    from sidekick_amd.quack import encode_segments
    ids, offs = segment_case(t)
    d = torch.from_numpy(ids.view(np.int32)).cuda()
    check_segments(encode_segments(d, offs.tolist(), t), ids, offs, t)
    if t <= 4:       # the id array 4, 8 and 12 bytes past a 16-byte boundary
        n = int(offs[-1])
        ids, offs = segment_case(t, extra=3)
        d = torch.from_numpy(ids.view(np.int32)).cuda()
        assert d.data_ptr() % 16 == 0
        for off in (1, 2, 3):
            check_segments(encode_segments(d[off:off + n], offs.tolist(), t), ids[off:off + n], offs, t, tag=off)


# ------------------------------------------------------------ per-flow batch
FLOW_CASES = {"40 flows": (20_000, 40, False, 0.3), "3000 flows, skewed": (6000, 3000, True, 0.0),
              "3000 flows": (6000, 3000, False, 0.0)}
_batches = {}


def flow_batch(case):
    """The packets of a case and what the sniff loop makes of them (threshold-independent; built once)."""
    if case not in _batches:
        n, nflows, skew, reset_until = FLOW_CASES[case]
        bufs, meta = make_flows(n, nflows, seed=n + nflows + int(skew), skew=skew, reset_until=reset_until)
        _batches[case] = (bufs, meta) + vector_flows(bufs, meta)
    return _batches[case]


@gpu
@pytest.mark.parametrize("case", list(FLOW_CASES))
@pytest.mark.parametrize("t", FLOW_THRESHOLDS)
def test_gpu_flows_at_threshold(t, case):
    import torch
    import sidekick_amd as sk
    bufs, meta, flows, nres, last_reset = flow_batch(case)
    if case == "3000 flows":
        assert len(flows) > 2000 and nres == 0       # thousands of accumulator rows, one work item each
    elif case == "40 flows":
        assert nres > 0 and len(flows) == 40
    table = sk.FlowQuacks(t)
    pre_key = sorted(flows)[0]
    table.insert(pre_key, 424242)                    # merges with the batch, or is wiped by a reset
    st = table.insert_packets(torch.from_numpy(bufs.reshape(-1).copy()).cuda(), stride=67,
                              meta=torch.from_numpy(meta.view(np.int64).copy()).cuda(), my_addr=MY_ADDR)
    assert st["resets"] == nres and st["inserted"] == sum(len(v) for v in flows.values())
    assert st["last_reset_index"] == last_reset
    assert set(table.senders()) == set(flows)
    for k, ids in flows.items():
        q = table.senders()[k]
        want_ids = ([424242] if k == pre_key and nres == 0 else []) + ids
        assert q.count() == len(want_ids) and q.last_value() == ids[-1], k.hex()
        assert q.power_sums() == coracle.encode_u32(np.array(want_ids, dtype=np.uint32), t), (k.hex(), len(ids))


@gpu
def test_gpu_flows_device_resident_output_large_threshold():
    """The records k_flow_finalize_big writes in place in HBM at t = 513 are
    the host-output path's, and the oracle's."""
    import torch
    from sidekick_amd.quack import encode_flows
    t = 513
    bufs, meta, flows, nres, _ = flow_batch("40 flows")
    d_bufs = torch.from_numpy(bufs.reshape(-1).copy()).cuda()
    d_meta = torch.from_numpy(meta.view(np.int64).copy()).cuda()
    hk, hq, hst = encode_flows(d_bufs, t, meta=d_meta, my_addr=MY_ADDR)
    dk, dq, dst = encode_flows(d_bufs, t, meta=d_meta, my_addr=MY_ADDR, device_out=True)
    torch.cuda.synchronize()
    assert hst == dst and dst["resets"] == nres
    assert hk == sorted(flows) and [bytes(r) for r in dk.cpu().numpy()] == hk
    recs = dq.cpu().numpy().view(np.uint32)
    assert recs.shape == (len(hk), 4 + t)
    for i, (k, q) in enumerate(zip(hk, hq)):
        assert bytes(q._buf.raw) == recs[i].tobytes(), k.hex()
        assert q.count() == len(flows[k]) and q.last_value() == flows[k][-1]
        assert q.power_sums() == coracle.encode_u32(np.array(flows[k], dtype=np.uint32), t), k.hex()
