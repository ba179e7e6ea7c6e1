"""The u32 t = 31..32 encode from the nine-power basis (basis32.h, bsgs.h
CfgBasis, knob u32_basis) against the oracle, bit-exact, with count and last
value: both thresholds, the basis and the (8,4) grid (u32_basis = 1 / 0), the
dynamic and the static form (enc_dyn = 1 / 0).

A chunk of the dynamic form is CHUNK = 4 096 ids.  Shapes: nothing but a head
(0, 1, 3 ids); about one chunk (CHUNK + 3 ids from 1 and 2 ids past a 16-byte
boundary, and CHUNK - 5, which holds no whole chunk whatever the start: only
the ragged rest, the head and the tail); five claimed chunks and a rest
(5 CHUNK + 259); the same with edge ids and with the ids whose lazy chain
wraps (tests/golden/basis_wrap_ids.json: every product of the chain) in one
lane of a full group, four in one lane's group, in the head, in the tail, in
a claimed chunk and in the ragged rest; and grids of 1 and 7 workgroups."""
import contextlib
import functools
import json
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "sidekick_amd", "csrc", "bsgs.h")) as _f:
    CHUNK = int(re.search(r"#define QK_DYN_CH (\d+)", _f.read()).group(1)) * 64 * 4   # ids per claim
with open(os.path.join(ROOT, "tests", "golden", "basis_wrap_ids.json")) as _f:
    WRAPS = json.load(_f)["wraps"]
P32 = 2**32 - 5
EDGE_IDS = (0, 1, P32 - 1, P32, 2**32 - 1)
BIG = 5 * CHUNK + 259
MODES = [(basis, dyn) for basis in (1, 0) for dyn in (1, 0)]
TS = (31, 32)


@contextlib.contextmanager
def setup(basis, dyn, blocks=0):
    import sidekick_amd as sk
    ctx = sk.get_context(0)
    ctx.set_knob("u32_basis", basis)
    ctx.set_knob("enc_dyn", dyn)
    ctx.set_grid(blocks)
    try:
        yield ctx
    finally:
        ctx.set_grid(0)
        ctx.set_knob("enc_dyn", 1)
        ctx.set_knob("u32_basis", 1)


@functools.lru_cache(maxsize=None)
def stream(kind, n, off):
    """off + n ids whose first id sits `off` ids past a 16-byte boundary on the
    device (host array, device tensor); kind "wraps": edge and wrap ids placed."""
    import torch
    from oracle import coracle
    ids = coracle.splitmix_u32(0xBA515 + 7 * n + off, off + n).copy()
    if kind == "wraps":
        assert n == BIG and off == 2           # head 2 ids, 5 chunks, 64 groups of rest, a tail of 1
        h, w = 2, [x["id"] for x in WRAPS]
        body = ids[off:]
        rng = np.random.default_rng(32)
        for e in EDGE_IDS:                     # edge ids sprinkled: chunks, rest, and next to each other
            body[rng.integers(0, n, 3)] = e
        body[h + 5 * CHUNK + 8:h + 5 * CHUNK + 8 + len(EDGE_IDS)] = EDGE_IDS
        body[h + 4 * 100 + 2] = w[0]                                   # one lane of a full group
        body[h + 4 * 200:h + 4 * 200 + 4] = [w[4], w[8], w[12], w[16]]  # four in one lane's group
        body[0], body[1] = w[20], w[27]                                # the head
        body[n - 1] = w[24]                                            # the tail
        body[h + CHUNK + 4 * 64 * 5 + 1] = w[1]                        # a claimed chunk
        body[h + 5 * CHUNK + 4 * 10 + 3] = w[5]                        # the ragged rest
        # every committed id (every product of the chain) once more: chunks 2..4 and the rest
        for j, x in enumerate(w):
            body[h + 2 * CHUNK + 4 * (97 * j + 5) + j % 4] = x
            body[h + 5 * CHUNK + 4 * (16 + j) + (j + 1) % 4] = x
    return ids, torch.from_numpy(ids.view(np.int32)).cuda()


@functools.lru_cache(maxsize=None)
def want(kind, n, off, t):
    from oracle import coracle
    return coracle.encode_u32(stream(kind, n, off)[0][off:], t)


def check(kind, n, off, t, tag=""):
    import sidekick_amd as sk
    ids, d = stream(kind, n, off)
    q = sk.PowerSumQuackU32(t)
    q.insert_batch(d[off:off + n])
    assert q.power_sums() == want(kind, n, off, t), (tag, kind, n, off, t)
    assert q.count() == n, (tag, kind, n, off, t)
    if n:
        assert q.last_value() == int(ids[off + n - 1]), (tag, kind, n, off, t)


@pytest.mark.parametrize("basis,dyn", MODES)
@pytest.mark.parametrize("t", TS)
def test_head_only(t, basis, dyn):
    with setup(basis, dyn):
        for n in (0, 1, 3):
            check("plain", n, 1, t)


@pytest.mark.parametrize("basis,dyn", MODES)
@pytest.mark.parametrize("t", TS)
def test_about_one_chunk(t, basis, dyn):
    with setup(basis, dyn):
        for off in (1, 2):
            check("plain", CHUNK + 3, off, t)
            check("plain", CHUNK - 5, off, t)


@pytest.mark.parametrize("basis,dyn", MODES)
@pytest.mark.parametrize("t", TS)
def test_claimed_chunks_then_the_rest(t, basis, dyn):
    with setup(basis, dyn):
        for off in (1, 2):
            check("plain", BIG, off, t)


@pytest.mark.parametrize("basis,dyn", MODES)
@pytest.mark.parametrize("t", TS)
def test_edge_and_wrap_ids(t, basis, dyn):
    with setup(basis, dyn):
        check("wraps", BIG, 2, t)


@pytest.mark.parametrize("blocks", [1, 7])
@pytest.mark.parametrize("basis,dyn", MODES)
@pytest.mark.parametrize("t", TS)
def test_grid_overrides(t, basis, dyn, blocks):
    with setup(basis, dyn, blocks):
        check("plain", BIG, 1, t, blocks)
        check("wraps", BIG, 2, t, blocks)
