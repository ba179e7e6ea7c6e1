"""The device wire leg (wire.hip, wire.h: qk_u32_flows_emit_device,
qk_u32_wire_ingest_device) at the shapes where its kernels change form:

  ingest  thresholds around and above one wave of sums (the second and later
          trips of the 64-lane share in k_wi_validate and k_wi_place), a bad
          sum at every position of a share, batches smaller than a workgroup's
          waves, a flow range far wider than the batch
  emit    every base alignment 0 ... 15 against every stride residue mod 16 and
          gaps of whole vectors, one flow (the byte-store path alone), every
          byte of the m * stride range written from the inputs alone, the tile
          scan at one, two and three tiles per scan thread
  both    byte offsets past 2^32

Expected images come from a literal packer of the bincode layout
(test_gpu_wire.pack, and pack_np below: the same layout written with array
slices, held to the first by a CPU test), expected statuses and placed records
from the host qk_u32_deserialize.  Nothing is derived from the code under test.

The shape lists below are restated from wire.hip and held to it by a CPU test."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import sidekick_amd as sk
from sidekick_amd._lib import P32, QK_E_CAPACITY, QK_E_FORMAT, QK_E_MISMATCH
from test_gpu_wire import GUARD, SENTINEL, Emit, Ingest, dev, host_status, image, pack, records, table_images

gpu = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- restated from wire.hip
WR_BLOCK = 256                     # threads per workgroup of every kernel but the scan
WE_IPT = 8                         # flows per thread of a tile
WE_SCAN = 1024                     # threads of the tile scan
WE_CHUNK = 16384                   # output bytes per workgroup of k_we_emit
WAVE = 64                          # lanes the sums of one datagram are shared out over
TILE = WR_BLOCK * WE_IPT
SCAN_FLOWS = TILE * WE_SCAN        # the most flows at one tile per scan thread

T_LIMITS = (63, 64, 65, 127, 128, 129, 1024)
ROUND_TRIP_T = (65, 1024)
BIG_N = (SCAN_FLOWS, SCAN_FLOWS + 1, 2 * SCAN_FLOWS + 5)
ALIGN_N = 1000
ALIGN_T = (1, 2)
SMALL_N = (1, 2, 3, 5)
FAR_STRIDE, FAR_N = 65536, 65540   # slot 65536 starts at byte 2^32


def wire_max(t):
    return 4 * t + 17


def bad_positions(t):
    """The first and last sum of a lane share's first three trips, and the image's last two."""
    return sorted({k for k in (0, 1, 62, 63, 64, 65, 126, 127, 128, 129, t - 2, t - 1) if 0 <= k < t})


def test_shape_lists_are_the_sources():
    src = open(os.path.join(ROOT, "sidekick_amd", "csrc", "wire.hip")).read()
    hdr = open(os.path.join(ROOT, "sidekick_amd", "csrc", "wire.h")).read()

    def const(name):
        return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))

    assert const("WR_BLOCK") == WR_BLOCK and const("WE_IPT") == WE_IPT
    assert const("WE_SCAN") == WE_SCAN and const("WE_CHUNK") == WE_CHUNK
    assert "constexpr uint32_t WE_TILE = WR_BLOCK * WE_IPT;" in src
    assert "const uint32_t per = (ntiles + WE_SCAN - 1) / WE_SCAN;" in src
    # the wave width of the ingest kernels, in every place it is written
    assert re.search(r"constexpr uint32_t WR_WAVES = WR_BLOCK / (\d+);", src).group(1) == str(WAVE)
    assert len(re.findall(r"blockIdx\.x \* WR_WAVES \+ \(threadIdx\.x >> (\d+)\)", src)) == 2
    assert set(re.findall(r"threadIdx\.x >> (\d+)", src)) == {str(WAVE.bit_length() - 1)}
    assert set(re.findall(r"lane = threadIdx\.x & (\d+);", src)) == {str(WAVE - 1)}
    assert re.search(r"wire_validate\(wire \+ i \* stride, len\[i\], stride, T, lane, (\d+)\)", src).group(1) == str(WAVE)
    assert re.search(r"for \(uint32_t k = lane; k < T; k \+= (\d+)\)", src).group(1) == str(WAVE)
    assert "for (uint64_t k = lane; k < t; k += nlanes)" in hdr
    # ingest thresholds: one, two and three trips of a lane's share, each edge from both sides, and the largest
    trips = {t: -(-t // WAVE) for t in T_LIMITS}
    assert {WAVE - 1, WAVE, WAVE + 1, 2 * WAVE - 1, 2 * WAVE, 2 * WAVE + 1, 1024} == set(T_LIMITS)
    assert set(trips.values()) >= {1, 2, 3, 16}
    assert all(t > WAVE for t in ROUND_TRIP_T)
    for t in T_LIMITS:
        at = bad_positions(t)
        assert {0, t - 1} <= set(at)
        for edge in (WAVE, 2 * WAVE):                   # the last sum of a trip and the first of the next
            if t > edge:
                assert {edge - 1, edge} <= set(at)
    # small batches: fewer datagrams than a workgroup has waves, and one workgroup and a wave
    waves = WR_BLOCK // WAVE
    assert set(range(1, waves)) <= set(SMALL_N) and waves + 1 in SMALL_N
    # emit: the alignment shapes end past the first chunk at their smallest, past the fourth at their largest
    for t in ALIGN_T:
        assert WE_CHUNK + 16 < ALIGN_N * wire_max(t) and ALIGN_N * (wire_max(t) + 48) > 4 * WE_CHUNK
    # the scan: exactly one tile per thread, the first shape with two, and three with most threads past the end
    ntiles = [-(-n // TILE) for n in BIG_N]
    per = [-(-k // WE_SCAN) for k in ntiles]
    assert ntiles == [WE_SCAN, WE_SCAN + 1, 2 * WE_SCAN + 1] and per == [1, 2, 3]
    assert [min(-(-k // p), WE_SCAN) for k, p in zip(ntiles, per)] == [1024, 513, 683]   # threads with a tile
    assert BIG_N[1] % TILE == 1 and BIG_N[2] % TILE == 5                                 # a ragged last tile
    # byte offsets: slots on both sides of 2^32, the last slot past it
    assert (FAR_N - 4) * FAR_STRIDE == 1 << 32 and FAR_STRIDE >= wire_max(1)


# ------------------------------------------------------------------ the packer, vectorised
def pack_np(recs, t):
    """pack() of every record at once: ([n, 4t + 17] bytes, zero past an image's end; [n] lengths)."""
    recs = np.ascontiguousarray(recs, dtype="<u4")
    n, body = recs.shape[0], 8 + 4 * t
    out = np.zeros((n, body + 9), dtype=np.uint8)
    out[:, 0:8] = np.full(n, t, dtype="<u8").view(np.uint8).reshape(n, 8)          # u64 threshold
    out[:, 8:body] = np.ascontiguousarray(recs[:, 4:]).view(np.uint8).reshape(n, 4 * t)   # u32 sums
    tag = recs[:, 2] != 0
    out[:, body] = tag                                                             # u8 tag
    last = np.ascontiguousarray(recs[:, 3]).view(np.uint8).reshape(n, 4)
    count = np.ascontiguousarray(recs[:, 1]).view(np.uint8).reshape(n, 4)
    out[:, body + 1:body + 5] = np.where(tag[:, None], last, count)                # u32 last (tag 1) | u32 count
    out[:, body + 5:body + 9] = np.where(tag[:, None], count, 0)                   # u32 count (tag 1)
    return out, (body + 5 + 4 * tag).astype(np.int32)


@pytest.mark.parametrize("t", (1, 2, 7, 65))
def test_vectorised_packer_equals_the_literal_one(t):
    recs = records(t, 300, 40 + t)
    recs[5, 2], recs[5, 3] = 1, 0x01020304
    recs[6, 2], recs[6, 3] = 0, 0
    assert set(recs[:, 2].tolist()) == {0, 1}
    img, lens = pack_np(recs, t)
    assert img.shape == (300, wire_max(t)) and set(lens.tolist()) == {4 * t + 13, 4 * t + 17}
    for i in range(300):
        want = image(recs[i])
        assert lens[i] == len(want) and img[i, :lens[i]].tobytes() == want and not img[i, lens[i]:].any(), i


# ------------------------------------------------------------------ helpers
class DeviceIngest(Ingest):
    """Ingest's call over datagrams that are in device memory already (what an emit wrote)."""

    def __init__(self, wire, stride, d_len, d_flow, n, t, nseg):
        self.ctx = sk.get_context(0)
        self.n, self.t, self.nseg, self.stride, self.wire = n, t, nseg, stride, wire
        self.d_len, self.d_flow = d_len, d_flow
        self.peer = torch.full((nseg, 4 + t), SENTINEL, dtype=torch.int32, device="cuda")
        self.present = torch.full((nseg,), 9, dtype=torch.uint8, device="cuda")
        self.status = np.full(n, 99, dtype=np.int32)
        self.acc = C.c_size_t(4242)


def record_of(q):
    return np.frombuffer(q._buf, dtype=np.uint32)


def check_np(e, want_rows):
    """Emit.check() with the vectorised packer, and nothing past slot m written in any output."""
    m = e.m.value
    assert m == len(want_rows)
    host = e.buf.cpu().numpy()
    lo, hi = GUARD + e.off, GUARD + e.off + m * e.stride
    assert (host[:lo] == 0xA5).all() and (host[hi:] == 0xA5).all(), "guard bytes"
    img, want_len = pack_np(e.recs[want_rows], e.t)
    lens, rows, keys = e.lens.cpu().numpy(), e.rows.cpu().numpy(), e.keys_out.cpu().numpy()
    assert np.array_equal(lens[:m], want_len) and (lens[m:] == -6).all()
    assert np.array_equal(rows[:m], want_rows) and (rows[m:] == -5).all()
    assert np.array_equal(keys[:m], e.keys[want_rows]) and (keys[m:] == 0x5A).all()
    slots = host[lo:hi].reshape(m, e.stride)[:, :img.shape[1]]
    inside = np.arange(img.shape[1])[None, :] < want_len[:, None]
    assert np.array_equal(slots[inside], img[inside]), "image bytes"


# ------------------------------------------------------------------ ingest above one wave of sums
@gpu
@pytest.mark.parametrize("off", (0, 3))
@pytest.mark.parametrize("t", T_LIMITS)
def test_ingest_status_table_above_a_wave(t, off):
    tab = table_images(t)
    v1 = tab[0][1]
    rows = [(what, b, len(b), None) for what, b in tab[:-1]]
    rows.append(("threshold t + 1, sums not canonical", pack(t + 1, [P32] * (t + 1), 1, 5, 6), 4 * t + 21,
                 QK_E_MISMATCH))                           # deser's order: the threshold before the sums
    rows.append(("a claimed length of 2^32 - 1", v1, 0xFFFFFFFF, QK_E_FORMAT))
    rows.append(tab[-1] + (len(tab[-1][1]), None))         # last: the buffer ends with its last byte
    n = len(rows)
    stride = max(len(b) for _, b, _, _ in rows) + 2
    assert stride % 2 == 1
    g = Ingest([b for _, b, _, _ in rows], [ln for _, _, ln, _ in rows], list(range(n)), t, n, stride=stride, off=off)
    assert g.call() == 0
    peer, present = g.rows()
    n_ok = 0
    for i, (what, b, ln, fixed) in enumerate(rows):
        if ln == len(b):
            want, q = host_status(b, t)
            assert fixed is None or want == fixed, what
        else:
            want = fixed                                   # more bytes claimed than the slot holds
        assert g.status[i] == want, (what, g.status[i], want)
        if want == 0:
            n_ok += 1
            assert present[i] == 1 and np.array_equal(peer[i], record_of(q)), what
        else:
            assert present[i] == 0 and (peer[i] == SENTINEL).all(), what
    assert n_ok == 3 and g.acc.value == 3


@gpu
@pytest.mark.parametrize("t", T_LIMITS)
def test_ingest_one_bad_sum_at_every_position_of_a_share(t):
    images, bad = [], []
    for j, k in enumerate(bad_positions(t)):
        for v, tag in ((P32, j & 1), (0xFFFFFFFF, ~j & 1), (P32 - 1, j & 1)):
            sums = [P32 - 1] * t
            sums[k] = v
            images.append(pack(t, sums, tag, 0xC0FFEE00 + k, 1000 + k))
            bad.append(v != P32 - 1)
    n = len(images)
    flows = np.random.default_rng(t).permutation(n)        # a flow of its own each: nothing is superseded
    stride = wire_max(t) + 2
    g = Ingest(images, [len(b) for b in images], flows, t, n, stride=stride, off=1)
    assert stride % 2 == 1 and g.call() == 0
    peer, present = g.rows()
    tags = set()
    for i, b in enumerate(images):
        want, q = host_status(b, t)
        f = int(flows[i])
        assert want == (QK_E_FORMAT if bad[i] else 0) and g.status[i] == want, (i, g.status[i], want)
        if bad[i]:
            tags.add(b[8 + 4 * t])
            assert present[f] == 0 and (peer[f] == SENTINEL).all(), i
        else:
            assert present[f] == 1 and np.array_equal(peer[f], record_of(q)), i
    assert tags == {0, 1} and g.acc.value == n // 3


@gpu
@pytest.mark.parametrize("t", ROUND_TRIP_T)
def test_round_trip_above_a_wave_off_alignment(t):
    n = 301
    recs = records(t, n, 70 + t)
    sel = np.random.default_rng(t).random(n) < 0.5
    e = Emit(recs, t, select=sel, stride=wire_max(t) + 2, off=1)
    assert e.call() == 0
    e.check()
    m = e.m.value
    g = DeviceIngest(e.buf.data_ptr() + GUARD + e.off, e.stride, e.lens, e.rows, m, t, n)
    assert g.call() == 0 and (g.status == 0).all() and g.acc.value == m
    peer, present = g.rows()
    assert np.array_equal(present, sel.astype(np.uint8))
    assert np.array_equal(peer[sel], recs[sel])            # all 4 + t words
    assert (peer[~sel] == SENTINEL).all()


# ------------------------------------------------------------------ emit: base alignment and stride residue
@gpu
@pytest.mark.parametrize("off", range(16))
@pytest.mark.parametrize("t", ALIGN_T)
def test_emit_every_stride_residue_at_base_offset(t, off):
    recs = records(t, ALIGN_N, 90 + t)
    sel = np.random.default_rng(t).random(ALIGN_N) < 0.5
    for d in tuple(range(17)) + (48,):
        for select in (None, sel):
            e = Emit(recs, t, select=select, stride=wire_max(t) + d, off=off)
            assert e.call() == 0, d
            e.check()


@gpu
@pytest.mark.parametrize("off", range(16))
def test_emit_one_flow_is_the_byte_store_path(off):
    """m = 1 at t = 1: 21 or 22 output bytes, the first vector holding 16 - off of them."""
    for tag in (0, 1):
        rec = np.array([[1, 0xA1B2C3D4, tag, 0x11223344 * tag, P32 - 2]], dtype=np.uint32)
        for stride in (21, 22):
            e = Emit(rec, 1, stride=stride, off=off)
            assert e.call() == 0
            _, lens = e.check()
            assert lens.tolist() == [17 + 4 * tag]
            e = Emit(np.concatenate([rec, rec, rec]), 1, select=[0, 0, 1], stride=stride, off=off)
            assert e.call() == 0 and e.m.value == 1
            e.check()


@gpu
@pytest.mark.parametrize("off", (0, 5, 10, 15))
def test_emit_threshold_1024_alignments(off):
    recs = records(1024, 37, 1024)
    for d in range(4):
        e = Emit(recs, 1024, stride=wire_max(1024) + d, off=off)
        assert e.call() == 0
        e.check(serialize_sample=37)


@gpu
def test_emit_writes_every_byte_of_the_range_from_the_inputs_alone():
    """The m * stride range holds the same bytes, gaps included, whatever the
    buffer held before and wherever its 16-byte boundaries fall; what the gap
    bytes are is left open."""
    t, n = 7, 301
    recs = records(t, n, 17)
    stride = wire_max(t) + 19
    got = []
    for fill, off in ((0xA5, 7), (0x5A, 7), (0xA5, 2)):
        e = Emit(recs, t, stride=stride, off=off)
        e.buf.fill_(fill)
        assert e.call() == 0 and e.m.value == n
        host = e.buf.cpu().numpy()
        lo, hi = GUARD + off, GUARD + off + n * stride
        assert (host[:lo] == fill).all() and (host[hi:] == fill).all(), "guard bytes"
        got.append(host[lo:hi].reshape(n, stride))
    img, lens = pack_np(recs, t)
    inside = np.arange(stride)[None, :] < lens[:, None]
    assert np.array_equal(got[0][inside], img[inside[:, :img.shape[1]]])
    assert np.array_equal(got[0], got[1]), "another fill before the call"
    assert np.array_equal(got[0], got[2]), "another base alignment"


# ------------------------------------------------------------------ emit: the tile scan past one tile per thread
@functools.lru_cache(maxsize=None)
def big_records(n):
    return records(1, n, n % 1000)


def sparse_selection(n):
    """One flow in about 4096, the array's ends, the ends of the tiles around the scan's limit, one whole tile."""
    ntiles = -(-n // TILE)
    sel = np.random.default_rng(n % 999).random(n) < 1 / 4096
    for tile in (0, 1, WE_SCAN - 1, WE_SCAN, WE_SCAN + 1, ntiles - 1):
        if tile < ntiles:
            sel[tile * TILE] = sel[min((tile + 1) * TILE, n) - 1] = True
    whole = ntiles // 2 + 1
    sel[whole * TILE:(whole + 1) * TILE] = True
    assert sel[0] and sel[n - 1] and whole < ntiles - 1
    return sel


@gpu
@pytest.mark.parametrize("n", BIG_N)
def test_emit_sparse_selection_past_one_tile_per_scan_thread(n):
    recs, sel = big_records(n), sparse_selection(n)
    want_rows = np.flatnonzero(sel)
    m = len(want_rows)
    assert TILE + n // 8192 < m < TILE + n // 2048
    e = Emit(recs, 1, select=sel, cap=m + 1)
    assert e.call() == 0
    check_np(e, want_rows)


@gpu
def test_emit_capacity_at_two_tiles_per_scan_thread():
    n = BIG_N[1]
    recs, sel = big_records(n), sparse_selection(n)
    want_rows = np.flatnonzero(sel)
    m = len(want_rows)
    e = Emit(recs, 1, select=sel, cap=m - 1)
    assert e.call() == QK_E_CAPACITY and e.m.value == m
    assert e.untouched()
    e = Emit(recs, 1, select=sel, cap=m)
    assert e.call() == 0
    check_np(e, want_rows)


@gpu
def test_emit_every_flow_past_one_tile_per_scan_thread():
    """No selection at 1025 tiles: 44 MB of images, compared on the device."""
    n = BIG_N[1]
    recs = big_records(n)
    img, want_len = pack_np(recs, 1)
    e = Emit(recs, 1, off=1)
    assert e.stride == img.shape[1] and e.call() == 0 and e.m.value == n
    lo, hi = GUARD + e.off, GUARD + e.off + n * e.stride
    assert bool((e.buf[:lo] == 0xA5).all()) and bool((e.buf[hi:] == 0xA5).all()), "guard bytes"
    d_len = dev(want_len)
    assert torch.equal(e.lens, d_len)
    assert torch.equal(e.rows, torch.arange(n, dtype=torch.int32, device="cuda"))
    assert torch.equal(e.keys_out, e.d_keys)
    inside = torch.arange(e.stride, device="cuda")[None, :] < d_len[:, None]
    same = e.buf[lo:hi].view(n, e.stride) == dev(img)
    assert bool((same | ~inside).all()), "image bytes"


# ------------------------------------------------------------------ byte offsets past 2^32
@gpu
def test_emit_and_ingest_at_byte_offsets_past_2pow32():
    t, n, stride, off = 1, FAR_N, FAR_STRIDE, 5
    need = n * stride + 2 * GUARD + off + (64 << 20)
    if torch.cuda.mem_get_info()[0] < need + (2 << 30):
        pytest.skip("needs %.1f GB of free device memory" % ((need + (2 << 30)) / 1e9))
    recs = records(t, n, 32)
    img, want_len = pack_np(recs, t)
    e = Emit(recs, t, stride=stride, off=off, keys=False, rows=False)      # the buffer is filled on the device
    assert e.buf.numel() > (1 << 32) and e.call() == 0 and e.m.value == n
    lo, hi = GUARD + off, GUARD + off + n * stride
    assert bool((e.buf[:lo] == 0xA5).all()) and bool((e.buf[hi:] == 0xA5).all()), "guard bytes"
    slots = e.buf[lo:hi].view(n, stride)
    lens = e.lens.cpu().numpy()
    assert np.array_equal(lens, want_len)
    heads = slots[:, :wire_max(t)].contiguous().cpu().numpy()
    inside = np.arange(wire_max(t))[None, :] < want_len[:, None]
    assert np.array_equal(heads[inside], img[inside]), "image bytes"
    # the same bytes back in
    flow = torch.arange(n, dtype=torch.int32, device="cuda")
    g = DeviceIngest(e.buf.data_ptr() + lo, stride, e.lens, flow, n, t, n)
    assert g.call() == 0 and (g.status == 0).all() and g.acc.value == n
    peer, present = g.rows()
    assert (present == 1).all() and np.array_equal(peer, recs)
    # two slots past 2^32 spoilt: one a byte short, one with tag 2
    short, tag2 = FAR_N - 3, FAR_N - 1
    assert min(short, tag2) * stride >= 1 << 32
    e.lens[short] -= 1
    slots[tag2, 8 + 4 * t] = 2
    g = DeviceIngest(e.buf.data_ptr() + lo, stride, e.lens, flow, n, t, n)
    assert g.call() == 0 and g.acc.value == n - 2
    want = np.zeros(n, dtype=np.int32)
    want[[short, tag2]] = QK_E_FORMAT
    assert np.array_equal(g.status, want)
    peer, present = g.rows()
    keep = want == 0
    assert np.array_equal(present, keep.astype(np.uint8))
    assert np.array_equal(peer[keep], recs[keep]) and (peer[~keep] == SENTINEL).all()
    del slots, g, e
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ small batches, a wide flow range
@gpu
@pytest.mark.parametrize("n", SMALL_N)
def test_ingest_batches_smaller_than_a_workgroup(n):
    nseg = 7
    for t in (7, 65):
        for first_bad in (0, 1):
            recs = records(t, n, 10 * n + first_bad)
            images = [image(r) for r in recs]
            for i in range(first_bad, n, 2):               # every other one malformed: short, or a sum == p
                images[i] = images[i][:-1] if i % 4 < 2 else pack(t, [P32] * t, 0, 0, i)
            flows = [6, 0, 3, 5, 1][:n]
            g = Ingest(images, [len(b) for b in images], flows, t, nseg, stride=wire_max(t) + 2, off=1)
            assert g.call() == 0
            peer, present = g.rows()
            want_present = np.zeros(nseg, dtype=np.uint8)
            for i, b in enumerate(images):
                want, q = host_status(b, t)
                assert want == (QK_E_FORMAT if i % 2 == first_bad else 0) and g.status[i] == want, (t, i)
                if want == 0:
                    want_present[flows[i]] = 1
                    assert np.array_equal(peer[flows[i]], record_of(q)) and np.array_equal(peer[flows[i]], recs[i])
            assert np.array_equal(present, want_present) and g.acc.value == int(want_present.sum())
            assert (peer[want_present == 0] == SENTINEL).all()


@gpu
def test_ingest_three_datagrams_into_a_wide_flow_range_twice():
    t, nseg = 7, 100_000
    recs = records(t, 3, 77)
    images = [image(r) for r in recs]
    first, second = [0, 50_000, 99_999], [99_999, 7, 50_001]
    g = Ingest(images, [len(b) for b in images], first, t, nseg)
    assert g.call() == 0 and g.status[:3].tolist() == [0, 0, 0] and g.acc.value == 3
    peer, present = g.rows()
    assert np.flatnonzero(present).tolist() == first and present.max() == 1
    assert np.array_equal(peer[first], recs)
    rest = np.ones(nseg, dtype=bool)
    rest[first] = False
    assert (peer[rest] == SENTINEL).all()
    # the same object, the scratch reused: flow 99 999 won with datagram 2 above and takes datagram 0 now
    d_flow = dev(np.asarray(second, dtype=np.uint32))
    assert g.call(flow=d_flow.data_ptr()) == 0 and g.status[:3].tolist() == [0, 0, 0] and g.acc.value == 3
    peer, present = g.rows()
    assert np.flatnonzero(present).tolist() == sorted(second) and present.max() == 1
    assert np.array_equal(peer[second], recs)
    assert np.array_equal(peer[[0, 50_000]], recs[:2])     # rows of the first call that no datagram names now
    rest[second] = False
    assert (peer[rest] == SENTINEL).all()
