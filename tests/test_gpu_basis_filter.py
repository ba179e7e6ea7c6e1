"""The id filter of the u32 t = 31..32 basis encode (basis_filter.h, bsgs.h
CfgBasis FILT) against the oracle, bit for bit, with count and last value:
t = 31 and 32, u32_basis = 1 (filtered), 2 (minimum tracked per product) and 0
(the (8,4) grid), enc_dyn = 1 / 0, grids of 1 and 7 workgroups.

Inputs, three groups: the 61 ids whose lazy chain is wrong and the 122 ids
that trip the minimum test although their chain is right
(tests/golden/basis_wrong_ids.json), and false positives of the filter built
here from its table (candidates that are not wrong: from slots in use and from
unused ones, at both ends of the window).  Each group is placed in claimed
chunks, in the ragged rest, in the head and the tail and four in one lane's
16-byte group; one trip of one wave holds nothing but candidates.  Sizes:
nothing but a head (3 ids), about one chunk (CHUNK + 3 and CHUNK - 5: the
latter holds no whole chunk), five chunks and a rest."""
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
with open(os.path.join(ROOT, "tests", "golden", "basis_wrong_ids.json")) as _f:
    _G = json.load(_f)
WRONG, FLAGGED = _G["wrong"], _G["flagged_right"]
with open(os.path.join(ROOT, "sidekick_amd", "csrc", "basis_filter.h")) as _f:
    _H = _f.read()
KEY_MASK = int(re.search(r"KEY_MASK = (0x[0-9A-Fa-f]+)u", _H).group(1), 16)
WINDOW = int(re.search(r"WINDOW = (0x[0-9A-Fa-f]+)u", _H).group(1), 16)
EMPTY_HIGH = int(re.search(r"EMPTY_HIGH = (0x[0-9A-Fa-f]+)u", _H).group(1), 16)
EMPTY_FLIP = int(re.search(r"EMPTY_FLIP = (0x[0-9A-Fa-f]+)u", _H).group(1), 16)


def make_table():
    """basis_filter::make_table, restated"""
    tab = [EMPTY_HIGH | ((k << 2) ^ EMPTY_FLIP) for k in range((KEY_MASK >> 2) + 1)]
    used = set()
    for i in WRONG:
        k = (i & KEY_MASK) >> 2
        tab[k] = tab[k] | i if k in used else i
        used.add(k)
    return tab, used


TABLE, USED = make_table()


def candidate(i):
    return (TABLE[(i & KEY_MASK) >> 2] ^ i) < WINDOW


def false_positives():
    """candidates that are not wrong: for three slots in use and three unused
    ones (the first, one in the middle, the last), the smallest and the largest
    differences the window admits"""
    out = []
    used = sorted(USED)
    for k in (used[0], used[len(used) // 2], used[-1]):
        for x in (0x4000, 0x1C000 | 3, 0x20000 | 3):         # key bits equal: bits 14..17 and 0..1 differ
            out.append(TABLE[k] ^ x)
    free = [k for k in range(len(TABLE)) if k not in USED]
    for k in (free[0], free[len(free) // 2], free[-1]):
        for x in (EMPTY_FLIP, EMPTY_FLIP | 0x1C000 | 3):     # the flipped key bit, alone and with the rest
            out.append(TABLE[k] ^ x)
    out = [i for i in dict.fromkeys(out) if i not in set(WRONG)]
    assert len(out) >= 8 and all(candidate(i) for i in out)
    return out


FALSE_POS = false_positives()
GROUPS = (WRONG, FLAGGED, FALSE_POS)
assert all(candidate(i) for i in WRONG) and not candidate(0)
BIG = 5 * CHUNK + 262          # from 1 id past a 16-byte boundary: head 3, 5 chunks, 64 groups of rest, tail 3
MODES = [(basis, dyn) for basis in (1, 2, 0) for dyn in (1, 0)]
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
def stream(kind, n):
    """1 + n ids whose first id sits 1 id past a 16-byte boundary on the device
    (host array, device tensor): a head of min(n, 3) ids"""
    import torch
    from oracle import coracle
    off, h = 1, min(n, 3)
    ids = coracle.splitmix_u32(0xF117E5 + 5 * n, off + n).copy()
    body = ids[off:]
    nbody = (n - h) // 4
    tail0 = h + 4 * nbody
    if kind == "head":
        assert n == 3
        body[:] = [WRONG[-1], FLAGGED[5], FALSE_POS[0]]
    elif kind == "chunk":
        # sprinkled: every id of every group once, one per 16-byte group, lanes and words varying
        every = [i for g in GROUPS for i in g]
        step = max(1, (nbody - 1) // len(every))
        for j, x in enumerate(every):
            if j * step < nbody:
                body[h + 4 * (j * step) + j % 4] = x
        for g, grp in enumerate(GROUPS):                      # the head and the tail
            if g < h:
                body[g] = grp[g]
            if tail0 + g < n:
                body[tail0 + g] = grp[-1 - g]
    elif kind == "big":
        assert n == BIG and nbody == 5 * (CHUNK // 4) + 64 and n - tail0 == 3
        every = [i for g in GROUPS for i in g]
        assert len(every) <= 256
        for j, x in enumerate(every):
            body[h + (1 + j % 4) * CHUNK + 4 * (53 * j % (CHUNK // 4)) + (j // 4) % 4] = x   # claimed chunks 1..4
            body[h + 5 * CHUNK + j] = x                                                      # the ragged rest
        for g, grp in enumerate(GROUPS):
            body[g] = grp[len(grp) // 2]                                                     # the head
            body[tail0 + g] = grp[len(grp) // 3]                                             # the tail
            body[h + 4 * (700 + g):h + 4 * (700 + g) + 4] = grp[:4]                          # four in one lane's group
            body[h + 2 * CHUNK + 4 * (900 + g):h + 2 * CHUNK + 4 * (900 + g) + 4] = grp[-4:]   # ... in a later chunk
        # one trip of one wave with nothing but candidates: 64 lanes x 4 ids of chunk 3's trip 5
        cands = WRONG + FALSE_POS
        body[h + 3 * CHUNK + 5 * 256:h + 3 * CHUNK + 6 * 256] = [cands[j % len(cands)] for j in range(256)]
    else:
        raise ValueError(kind)
    return ids, torch.from_numpy(ids.view(np.int32)).cuda()


@functools.lru_cache(maxsize=None)
def want(kind, n, t):
    from oracle import coracle
    return coracle.encode_u32(stream(kind, n)[0][1:], t)


def check(kind, n, t, tag=""):
    import sidekick_amd as sk
    ids, d = stream(kind, n)
    q = sk.PowerSumQuackU32(t)
    q.insert_batch(d[1:1 + n])
    assert q.power_sums() == want(kind, n, t), (tag, kind, n, t)
    assert q.count() == n, (tag, kind, n, t)
    assert q.last_value() == int(ids[n]), (tag, kind, n, t)


@pytest.mark.parametrize("blocks", [1, 7])
@pytest.mark.parametrize("basis,dyn", MODES)
@pytest.mark.parametrize("t", TS)
def test_head_only(t, basis, dyn, blocks):
    with setup(basis, dyn, blocks):
        check("head", 3, t, blocks)


@pytest.mark.parametrize("blocks", [1, 7])
@pytest.mark.parametrize("basis,dyn", MODES)
@pytest.mark.parametrize("t", TS)
def test_about_one_chunk(t, basis, dyn, blocks):
    with setup(basis, dyn, blocks):
        check("chunk", CHUNK + 3, t, blocks)
        check("chunk", CHUNK - 5, t, blocks)


@pytest.mark.parametrize("blocks", [1, 7])
@pytest.mark.parametrize("basis,dyn", MODES)
@pytest.mark.parametrize("t", TS)
def test_five_chunks_and_a_rest(t, basis, dyn, blocks):
    with setup(basis, dyn, blocks):
        check("big", BIG, t, blocks)
