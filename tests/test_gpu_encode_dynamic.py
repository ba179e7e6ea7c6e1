"""The dynamic form of the single-pass u32 baby-step/giant-step encode
(bsgs.h body_dyn, knob enc_dyn): waves claim chunks of DYN_CH x 64 16-byte
groups from a counter that is never reset, and one wave of the launch walks
what is no whole chunk (the groups past the last chunk, the unaligned head,
the tail).  Every result is compared with the oracle, for enc_dyn = 1 and for
the static form (enc_dyn = 0): chunk edges, misaligned starts, grids from one
workgroup to more workgroups than chunks, launches of alternating sizes on
one context (the counter's per-launch base), and the ids that force the
exact recompute of a lazy fold, in a claimed chunk and in the ragged rest.

t = 8, 32 and 80 are the kernels (4,2), (8,4) and (8,10)."""
import contextlib
import functools
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "sidekick_amd", "csrc", "bsgs.h")) as _f:
    DYN_CH = int(re.search(r"#define QK_DYN_CH (\d+)", _f.read()).group(1))
CHUNK = DYN_CH * 64 * 4          # ids per claim
TS = (8, 32, 80)
ROUND = 1280                     # one resident round of the t = 32 kernel on 256 CUs (5 workgroups each)
# no chunk, exactly one, one plus a ragged rest, a rest shorter than a wave,
# two and sixteen chunks plus a few ids
EDGES = (0, 1, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5, 3 * CHUNK - 1, 16 * CHUNK + 7)
WRAP_KEY = {8: "4x4", 32: "8x4", 80: "8x10"}


@contextlib.contextmanager
def setup(dyn, blocks=0):
    import sidekick_amd as sk
    ctx = sk.get_context(0)
    ctx.set_knob("enc_dyn", dyn)
    ctx.set_grid(blocks)
    try:
        yield ctx
    finally:
        ctx.set_grid(0)
        ctx.set_knob("enc_dyn", 1)


@functools.lru_cache(maxsize=None)
def stream(n):
    """n + 3 ids, on the device and on the host (slices of it start 0..3 ids
    past a 16-byte boundary)."""
    import torch
    from oracle import coracle
    ids = coracle.splitmix_u32(0xD1A + n, n + 3)
    return ids, torch.from_numpy(ids.view(np.int32)).cuda()


@functools.lru_cache(maxsize=None)
def want(n, off, t):
    from oracle import coracle
    return coracle.encode_u32(stream(n)[0][off:off + n], t)


def check(n, off, t, tag=""):
    import sidekick_amd as sk
    ids, d = stream(n)
    q = sk.PowerSumQuackU32(t)
    q.insert_batch(d[off:off + n])
    assert q.power_sums() == want(n, off, t), (tag, n, off, t)
    assert q.count() == n, (tag, n, off, t)
    if n:
        assert q.last_value() == int(ids[off + n - 1]), (tag, n, off, t)


@pytest.mark.parametrize("dyn", [1, 0])
@pytest.mark.parametrize("t", TS)
def test_chunk_edges_and_misaligned_starts(t, dyn):
    """Every edge size from an aligned start and from 1, 2 and 3 ids past a
    16-byte boundary (a head of 3, 2, 1 ids; the sizes then leave tails of
    every length)."""
    with setup(dyn):
        for n in EDGES:
            for off in (0, 1, 2, 3):
                check(n, off, t)


@pytest.mark.parametrize("dyn", [1, 0])
@pytest.mark.parametrize("blocks", [1, 2, 7, ROUND, 4096])
def test_grids(blocks, dyn):
    """One workgroup (four waves take every chunk and the rest), a few, one
    resident round and more workgroups than chunks (most claim nothing and
    store zero partials)."""
    with setup(dyn, blocks):
        for t in TS:
            for n, off in ((3 * CHUNK - 1, 1), (16 * CHUNK + 7, 0), (40 * CHUNK + 5, 3), (3, 0)):
                check(n, off, t, blocks)


@pytest.mark.parametrize("dyn", [1, 0])
def test_repeated_launches(dyn):
    """Twenty launches of alternating sizes and thresholds on one context:
    the counter keeps growing and every launch's base must be right.  The
    grid changes too (the base moves by chunks + waves)."""
    sizes = (16 * CHUNK + 7, 3, 2 * CHUNK + 5, 0, CHUNK, 40 * CHUNK + 5, CHUNK - 1)
    grids = (0, 7, 0, 4096, 1)
    for i in range(20):
        with setup(dyn, grids[i % len(grids)]):
            check(sizes[i % len(sizes)], i % 4, TS[i % 3], i)


@pytest.mark.parametrize("dyn", [1, 0])
@pytest.mark.parametrize("t", TS)
def test_two_batches_into_one_sketch(t, dyn):
    """Two insert_batch calls into one sketch, and a host array through the
    pipelined path (the kernels' accumulate form), against the oracle of the
    concatenation."""
    import sidekick_amd as sk
    from oracle import coracle
    a, da = stream(2 * CHUNK + 5)
    b, db = stream(3 * CHUNK - 1)
    both = np.concatenate([a[1:], b[:-3]])
    with setup(dyn):
        q = sk.PowerSumQuackU32(t)
        q.insert_batch(da[1:])
        q.insert_batch(db[:-3])
        h = sk.PowerSumQuackU32(t)
        h.insert_batch(both)
    exp = coracle.encode_u32(both, t)
    assert q.power_sums() == exp and q.count() == len(both) and q.last_value() == int(both[-1])
    assert h.power_sums() == exp and h.count() == len(both) and h.last_value() == int(both[-1])


@pytest.mark.parametrize("dyn", [1, 0])
@pytest.mark.parametrize("t", TS)
def test_wrap_ids_in_chunk_and_rest(golden, t, dyn):
    """The ids whose lazy folds wrap (the exact recompute), in claimed chunks
    and, separately, in the ragged rest, the head and the tail."""
    import sidekick_amd as sk
    import torch
    from oracle import coracle
    wraps = np.array(golden["bsgs_wrap_ids"][WRAP_KEY[t]], dtype=np.uint32)
    n, off = 3 * CHUNK + 300, 1               # head of 3 ids, three chunks, 74 groups of rest, a tail
    base = stream(n)[0][off:off + n]
    where = {
        "chunk": [3 + 4 * 100 + 2, 3 + CHUNK + 4 * 64 * 5 + 1, 3 + 3 * CHUNK - 1],
        "rest": [0, 3 + 3 * CHUNK, 3 + 3 * CHUNK + 4 * 70 + 3, n - 1],
    }
    for place, idx in where.items():
        ids = np.zeros(n + off, dtype=np.uint32)
        ids[off:] = base
        for j, i in enumerate(idx):
            ids[off + i] = wraps[j % len(wraps)]
        if place == "chunk":                  # one lane's whole group, and every lane of one wave
            ids[off + 3 + 4 * 200:off + 3 + 4 * 200 + 4] = np.resize(wraps, 4)
            ids[off + 3 + 2 * CHUNK:off + 3 + 2 * CHUNK + 256:4] = np.resize(wraps, 64)
        with setup(dyn):
            q = sk.PowerSumQuackU32(t)
            q.insert_batch(torch.from_numpy(ids.view(np.int32)).cuda()[off:])
        assert q.power_sums() == coracle.encode_u32(ids[off:], t), (place, t)
        assert q.count() == n and q.last_value() == int(ids[-1])
