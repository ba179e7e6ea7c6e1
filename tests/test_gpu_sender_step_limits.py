"""Batched sender step at the shapes its kernels switch on: every lane-group
width of k_snd_prefix<G, 32> (both ends of each threshold range up to 1024),
k_snd_remove's LDS / global-atomics boundary (nseg * T against SN_REM_ROWS),
k_snd_prefix's striped / wave-per-segment switch (nseg against SN_WAVES), and
a segment with far more hits than T.  Bit for bit against the per-flow oracle
of test_gpu_sender_step.py: action, drain, missing and every word of mine_out.

Each batch asserts the packing it is aimed at with the rule restated in
test_gpu_seg_decode_limits.py (work_items); a CPU test reads the constants
the shapes rest on out of sender.hip and segdecode.h."""
import os
import random
import re

import numpy as np
import pytest

from sidekick_amd._lib import SND_ADVANCED, SND_IDLE, SND_RESET_EXCEEDS, SND_RESET_REORDERED, SND_RESET_RETX
from test_gpu_seg_decode_limits import ITEM, max_segments, work_items
from test_gpu_sender_step import (THRESHOLDS as ELSEWHERE, advance_flow, build_flows, check_against_oracle, fresh_ids,
                                  oracle_step, run_step)

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sidekick_amd", "csrc")

# ---- restated from sender.hip / segdecode.h
LADDER = ((4, 1), (8, 1), (16, 1), (32, 1), (64, 2), (128, 4), (256, 8), (512, 16), (1024, 32))   # T <= bound: G
SN_REM_ROWS = 4096
SN_GROUP = 16
SN_WAVES = 4

GROUP_THRESHOLDS = (64, 65, 128, 256, 257, 512, 513, 1024)
REMOVE_ROWS = {32: 128, 33: 124, 129: 31, 512: 8, 1024: 4}      # T: R = SN_REM_ROWS // T
STRIPE_THRESHOLDS = (8, 64, 513)
SEPARATOR = ITEM + 1                               # longer than a work item: ends a packed run


def group_of(t):
    return next(g for bound, g in LADDER if t <= bound)


def test_restated_constants_are_the_sources():
    src = open(os.path.join(CSRC, "sender.hip")).read()
    sdh = open(os.path.join(CSRC, "segdecode.h")).read()
    assert int(re.search(r"constexpr uint32_t SN_REM_ROWS = (\d+);", src).group(1)) == SN_REM_ROWS
    assert int(re.search(r"constexpr uint32_t SN_GROUP = (\d+);", src).group(1)) == SN_GROUP
    assert "constexpr uint32_t SN_WAVES = SD_BLOCK / 64;" in src
    assert int(re.search(r"constexpr int SD_BLOCK = (\d+);", sdh).group(1)) == SN_WAVES * 64
    body = src[src.index("static void sn_prefix("):]
    body = body[:body.index("\n}\n")]
    rungs = [(int(b), int(g), int(k)) for b, g, k in re.findall(r"if \(T <= (\d+)\) sn_prefix_gk<(\d+), (\d+)>", body)]
    last = re.search(r"\n    else sn_prefix_gk<(\d+), (\d+)>", body).groups()
    assert [(b, g) for b, g, _ in rungs] + [(1024, int(last[0]))] == list(LADDER)
    assert all(g * k >= b for b, g, k in rungs) and int(last[0]) * int(last[1]) >= 1024
    # (a) with the older file's thresholds: both ends of every rung with G > 1, every G launched
    bounds = [b for b, _ in LADDER]
    for t in GROUP_THRESHOLDS:
        assert t in bounds or t - 1 in bounds, t
    ran = set(GROUP_THRESHOLDS) | set(ELSEWHERE)
    for i, (b, g) in enumerate(LADDER):
        if g > 1:
            assert bounds[i - 1] + 1 in ran and b in ran, (b, g)
    assert {group_of(t) for t in GROUP_THRESHOLDS} == {2, 4, 8, 16, 32}
    assert any(t % SN_GROUP for t in GROUP_THRESHOLDS) and any(t % SN_GROUP == 0 for t in GROUP_THRESHOLDS)
    # (b) R segments fill the LDS rows, R + 1 do not, and a packed work item can hold R + 1
    for t, r in REMOVE_ROWS.items():
        assert r == SN_REM_ROWS // t and r * t <= SN_REM_ROWS < (r + 1) * t and r + 1 <= max_segments(t)
    assert any(r * t == SN_REM_ROWS for t, r in REMOVE_ROWS.items()) and any(r * t < SN_REM_ROWS for t, r in REMOVE_ROWS.items())
    # (c) 3 segments striped, 4 a wave each, 5 a second trip of wave 0
    assert SN_WAVES == 4 and all(max_segments(t) >= SN_WAVES + 1 for t in STRIPE_THRESHOLDS)
    assert {group_of(t) for t in STRIPE_THRESHOLDS} == {1, 2, 32}
    assert SEPARATOR == 2049


# ------------------------------------------- a. the scenario set, every group width
@gpu
@pytest.mark.parametrize("t", GROUP_THRESHOLDS)
def test_scenarios_at_the_group_widths(t):
    flows = build_flows(t, 0x5E9D0000 + t)
    res, _, _ = run_step(flows, t)
    seen = check_against_oracle(flows, t, res)
    assert {SND_IDLE, SND_ADVANCED, SND_RESET_REORDERED, SND_RESET_RETX, SND_RESET_EXCEEDS,
            SND_RESET_REORDERED | SND_RESET_RETX, SND_RESET_REORDERED | SND_RESET_EXCEEDS} <= seen
    assert sum(len(m) for m in res.missing) > 0


# --------------------------------------------------- b. remove: LDS rows / global rows
def separator(rng, t):
    """A flow of ITEM + 1 entries, two work items: the stop is its last entry
    (alone in the second slice), the losses lie at both ends and inside the first."""
    return advance_flow(rng, t, SEPARATOR, SEPARATOR - 1, [0, 1000, ITEM - 1])


def short_run(rng, t, k, n=3):
    """k flows of n entries, the stop at entry 1 or 2; the first, a middle and
    the last one lose an entry before it."""
    flows = []
    for i in range(k):
        stop = 1 + (i + rng.randrange(2)) % 2
        lost = [rng.randrange(stop)] if i in (0, k // 2, k - 1) else []
        flows.append(advance_flow(rng, t, n, stop, lost))
    return flows


@gpu
@pytest.mark.parametrize("which", ["both", "R", "R + 1"])
@pytest.mark.parametrize("t", list(REMOVE_ROWS))
def test_remove_at_the_lds_boundary(t, which):
    r = REMOVE_ROWS[t]
    rng = random.Random(0xB0DE + t)
    if which == "both":       # rows = SN_REM_ROWS: R segments in LDS, R + 1 on the global rows, in one launch
        flows = [separator(rng, t)] + short_run(rng, t, r) + [separator(rng, t)] + short_run(rng, t, r + 1) + \
                [separator(rng, t)]
        runs = [(1, r), (r + 2, r + 1)]
    else:                     # alone: rows = R * T (every LDS word used), or SN_REM_ROWS < (R + 1) * T
        k = r if which == "R" else r + 1
        flows = [separator(rng, t)] + short_run(rng, t, k) + [separator(rng, t)]
        runs = [(1, k)]
    # the separators' second slices are one-entry items of one segment: not packed runs
    offs = np.concatenate([[0], np.cumsum([len(f.seg) for f in flows])]).astype(np.uint64)
    items = work_items(offs, t)
    assert [it[:2] for it in items if it[1] > 1] == runs
    assert all(it[1] == 1 and it[2] in (ITEM, 1) for it in items if it[1] == 1)
    res, _, _ = run_step(flows, t)
    check_against_oracle(flows, t, res)
    for g0, k in runs:        # the hits the removes are for: first, middle and last flow of each run
        assert [len(res.missing[g0 + i]) for i in (0, k // 2, k - 1)] == [1, 1, 1]
        assert sum(len(res.missing[g0 + i]) for i in range(k)) == len({0, k // 2, k - 1})
    assert all(res.missing[g] == [0, 1000, ITEM - 1] for g, f in enumerate(flows) if len(f.seg) == SEPARATOR)


# ------------------------------------------- c. prefix: striped / a wave per segment
@gpu
@pytest.mark.parametrize("t", STRIPE_THRESHOLDS)
def test_prefix_striped_and_wave_per_segment(t):
    rng = random.Random(0x57A1 + t)
    flows, runs = [separator(rng, t)], []
    for k in (1, 2, 3, 4, 5):
        runs.append((len(flows), k))
        for i in range(k):
            n = rng.randrange(5, 41)
            stop = rng.randrange(1, n - 1)                       # never the last entry
            lost = rng.sample(range(stop), min(stop, t, (i + k) % 3))
            flows.append(advance_flow(rng, t, n, stop, lost))
        flows.append(separator(rng, t))
    offs = np.concatenate([[0], np.cumsum([len(f.seg) for f in flows])]).astype(np.uint64)
    items = work_items(offs, t)
    short = [it[:2] for it in items if it[2] <= 5 * 40 and it[2] != 1]
    assert short == runs and [k for _, k in runs] == [SN_WAVES - 3, SN_WAVES - 2, SN_WAVES - 1, SN_WAVES, SN_WAVES + 1]
    res, _, _ = run_step(flows, t)
    check_against_oracle(flows, t, res)
    assert all(int(res.action[g]) == SND_ADVANCED and 0 < int(res.drain[g]) < len(f.seg) or len(f.seg) == SEPARATOR
               for g, f in enumerate(flows))
    assert sum(len(res.missing[g]) for g, f in enumerate(flows) if len(f.seg) != SEPARATOR) > 0


# ------------------------------------------------- d. more hits than T in a segment
@gpu
def test_one_missing_id_five_hundred_times():
    """The peer lacks ONE copy of an id the log holds 501 times before the stop:
    the diff has count 1, every copy is a root, and the reference removes the id
    once per hit (media_client.rs:319) — 501 removes on one row at T = 8."""
    t, n, stop = 8, 2600, 2550
    rng = random.Random(0xD0B1E)
    seg = fresh_ids(rng, n)
    at = rng.sample(range(2500), 501)
    x = seg[at[0]]                                               # where it already stood, and 500 more places
    for pos in at[1:]:
        seg[pos] = x
    assert seg.count(x) == 501 and seg[stop] != x and seg.index(seg[stop]) == stop
    flows = [advance_flow(rng, t, 30, 20, [7]), advance_flow(rng, t, n, stop, [at[0]], seg=seg),
             advance_flow(rng, t, 30, 20, [11])]
    offs = np.concatenate([[0], np.cumsum([len(f.seg) for f in flows])]).astype(np.uint64)
    assert [it[:2] for it in work_items(offs, t)] == [(0, 1), (1, 1), (1, 1), (2, 1)]
    want, act, drain, miss = oracle_step(flows[1].mine, flows[1].peer, seg, t)
    assert act == SND_ADVANCED and drain == stop + 1 and miss == sorted(at)
    assert sum(p < ITEM for p in miss) > t and sum(p >= ITEM for p in miss) > t       # both slices, each past T hits
    assert want.count == (3 + stop + 1 - 501) & 0xFFFFFFFF
    res, _, _ = run_step(flows, t)
    check_against_oracle(flows, t, res)
    assert int(res.action[1]) == SND_ADVANCED and int(res.drain[1]) == stop + 1 and len(res.missing[1]) == 501
    assert res.missing[0] == [7] and res.missing[2] == [11]
