"""The record staging of records.h under both of its users, the packet batch
(qk_u32_encode_packets_device, k_pkt_kernel) and the per-flow batch
(qk_u32_encode_flows_device, k_flow_extract), at every record stride where it
changes shape and at every alignment of the batch's first byte.

Strides 67 ... 79 stage a tile software-pipelined (stage_issue / stage_commit,
STAGE_VEC 16-byte vectors per lane); 80 ... 512 take stage_records, whose loop
runs up to seven rounds; from stride 256 on the dynamic LDS tile is larger
than 64 KiB, at 512 it is 131 104 bytes.  A base that is not 16-byte aligned
takes the byte path for the head vector, an end that is not for the tail.

Everything is bit for bit against the models the suite already has
(make_batch / vector_sniff, make_flows / vector_flows, coracle.encode_u32) and
the oracle's literal sniff loops for the statistics.  The records sit inside a
larger device buffer, 0xFF in front and behind; their padding bytes are random.

The lists below are restated from the sources and held to them by a CPU test."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import coracle, quack_oracle as qo
from test_flows import MY_ADDR, make_flows, vector_flows
from test_packets import META_DT, MY_IP, PROTO_IP, make_batch, vector_sniff

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sidekick_amd", "csrc")

# ---- restated from records.h, packets.hip, flows.hip and quack_hip.h
REC_TILE = 256                     # records per LDS tile
STAGE_VEC = 5                      # 16-byte vectors per lane of the pipelined form
STRIDE_MIN, STRIDE_MAX = 67, 512   # accepted by both entry points
MIN_CHUNK_TILES = 4                # tiles per workgroup chunk, at least
LDS_64K = 1 << 16

STRIDES = (67, 68, 79, 80, 81, 96, 255, 256, 257, 511, 512)
REJECTED = (66, 513)
SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 2049)
FLOW_SIZES = (1, 257, 1025, 2049)
OFFS = (0, 5)
EDGE_OFFS = (0, 5, 15)             # 15: up to stride 81 the id of a full tile's last record ends in the tile's extra vector
RESIDUE_STRIDES = (67, 79, 80, 96)
PRE = 12345                        # in the quACK before the batch


def pipelined(stride, threads=REC_TILE, stage_vec=STAGE_VEC):
    """stage_pipelined(): a tile and its one extra vector of an unaligned base fit stage_vec vectors per lane."""
    return (REC_TILE * stride + 15) // 16 + 1 <= stage_vec * threads


def tile_bytes(stride):
    return REC_TILE * stride + 32


def check_lists_against_sources(strides, stage_vec):
    rec = open(os.path.join(CSRC, "records.h")).read()
    pkt = open(os.path.join(CSRC, "packets.hip")).read()
    flw = open(os.path.join(CSRC, "flows.hip")).read()
    api = open(os.path.join(ROOT, "include", "quack_hip.h")).read()
    assert int(re.search(r"constexpr int REC_TILE = (\d+);", rec).group(1)) == REC_TILE
    src_vec = int(re.search(r"constexpr int STAGE_VEC = (\d+);", rec).group(1))
    assert src_vec == stage_vec
    assert int(re.search(r"constexpr int STAGE_V = (\d+);", rec).group(1)) == src_vec    # one round at stride 67 in both forms
    assert "return ((uint64_t)REC_TILE * stride + 15) / 16 + 1 <= (uint64_t)STAGE_VEC * threads;" in rec
    assert "constexpr int PK_BLOCK = REC_TILE;" in pkt
    assert "stage_pipelined(stride, PK_BLOCK)" in pkt and "stage_pipelined(stride, REC_TILE)" in flw
    assert int(re.search(r"#define QK_BUFFER_SIZE (\d+)u", api).group(1)) == STRIDE_MIN
    for src in (pkt, flw):
        assert re.search(r"if \(stride < QK_BUFFER_SIZE \|\| stride > (\d+)\) return QK_E_INVAL;", src).group(1) == \
            str(STRIDE_MAX)
        assert re.search(r"std::max<uint64_t>\((\d+), \(n?tiles \+ wgs? - 1\) / wgs?\)", src).group(1) == \
            str(MIN_CHUNK_TILES)
    assert "(size_t)PK_BLOCK * stride + 32" in pkt and "(size_t)REC_TILE * stride + 32" in flw
    # the packet batch's kernel families by threshold
    for line in ("if (t <= 8) QK_PKT_FUSED(4, 2, 0);", "else if (t <= 12) QK_PKT_FUSED(4, 3, 0);",
                 "else if (t <= 16) QK_PKT_SHARED(2);", "else if (t <= 24) QK_PKT_SHARED(3);", "else QK_PKT_SHARED(4);",
                 "if (t >= 5 && t <= 32) {"):
        assert line in pkt, line
    # the boundaries, and both neighbours of each in the list
    pipe = [s for s in range(STRIDE_MIN, STRIDE_MAX + 1) if pipelined(s, stage_vec=stage_vec)]
    assert pipe == list(range(STRIDE_MIN, 80))                      # the largest pipelined stride is 79
    big = min(s for s in range(STRIDE_MIN, STRIDE_MAX + 1) if tile_bytes(s) > LDS_64K)
    assert big == 256 and tile_bytes(STRIDE_MAX) == 131_104
    for last, first in ((pipe[-1], pipe[-1] + 1), (big - 1, big)):
        assert last in strides and first in strides, (last, first)
    assert {STRIDE_MIN, STRIDE_MIN + 1, STRIDE_MAX - 1, STRIDE_MAX} <= set(strides)
    assert REJECTED == (STRIDE_MIN - 1, STRIDE_MAX + 1)
    assert all(STRIDE_MIN <= s <= STRIDE_MAX for s in strides)
    assert any(s % 16 == 0 and not pipelined(s) and tile_bytes(s) <= LDS_64K for s in strides)   # one alignment for all records
    rounds = {-(-(16 * s + 1) // (src_vec * REC_TILE)) for s in strides}     # stage_records' v0 loop
    assert {1, 2, 7} <= rounds and max(rounds) == 7
    assert all(s in strides for s in RESIDUE_STRIDES)
    assert {pipelined(s) for s in RESIDUE_STRIDES} == {True, False}
    # sizes: one record, a tile and a minimum chunk each minus / exactly / plus one, three chunks
    chunk = MIN_CHUNK_TILES * REC_TILE
    assert set(SIZES) == {1, REC_TILE - 1, REC_TILE, REC_TILE + 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1}
    assert set(FLOW_SIZES) <= set(SIZES)


def test_stride_list_is_the_sources():
    check_lists_against_sources(STRIDES, STAGE_VEC)


# ------------------------------------------------------------------ helpers
def place(flat, off, tail=32):
    """The bytes `flat` at byte `off` of a larger device tensor, 0xFF in front
    and behind: (the whole tensor, the slice that holds the records)."""
    import torch
    raw = np.full(off + len(flat) + tail, 0xFF, dtype=np.uint8)
    raw[off:off + len(flat)] = flat
    d_raw = torch.from_numpy(raw).cuda()
    assert d_raw.data_ptr() % 16 == 0
    return d_raw, d_raw[off:off + len(flat)]


def dev_meta(meta):
    import torch
    return torch.from_numpy(meta.view(np.int64).copy()).cuda()


def literal_stats(bufs, meta, my_ip=MY_IP):
    """The statistics of the literal sniff loop (it reads 67 bytes of a record)."""
    return qo.sniff_batch(qo.OracleQuack(1), bufs[:, :67], meta["pkttype"], meta["protocol_be"], meta["len"], my_ip)[1]


def put_id(bufs, i, ident):
    bufs[i, 63:67] = np.frombuffer(int(ident).to_bytes(4, "big"), dtype=np.uint8)


def make_insert(bufs, meta, i):
    """Record i passes every filter and is no reset."""
    meta["pkttype"][i], meta["protocol_be"][i], meta["len"][i] = 0, PROTO_IP, 67
    bufs[i, 23] = 17
    bufs[i, 30:34] = (192, 168, 1, 7)


class PacketCase:
    """A batch and what the sniff loop makes of it (threshold-independent)."""

    def __init__(self, bufs, meta):
        self.bufs, self.meta = bufs, meta
        self.n, self.stride = bufs.shape
        self.ids, self.last = vector_sniff(bufs, meta)
        self.stats = literal_stats(bufs, meta)
        assert self.stats["inserted"] == len(self.ids) and self.stats["last_reset_index"] == self.last
        self.d_meta = dev_meta(meta)

    def run(self, t, off, d_bufs=None):
        import sidekick_amd as sk
        from sidekick_amd.quack import encode_packets
        if d_bufs is None:
            self.keep, d_bufs = place(self.bufs.reshape(-1), off)
        tag = (self.stride, self.n, off, t, self.stats)
        q = sk.PowerSumQuackU32(t)
        q.insert(PRE)
        st = encode_packets(q, d_bufs, stride=self.stride, meta=self.d_meta, my_ipv4=MY_IP)
        ids = self.ids if self.last >= 0 else np.concatenate([np.array([PRE], dtype=np.uint32), self.ids])
        assert st == self.stats, tag
        assert st["filtered"] == self.n - st["inserted"] - st["discarded"] - st["resets"], tag
        assert q.count() == len(ids), tag
        last_value = int(self.ids[-1]) if len(self.ids) else PRE if self.last < 0 else None
        assert q.last_value() == last_value, tag
        got, want = q.power_sums(), coracle.encode_u32(ids, t)
        if got != want:
            bad = [m + 1 for m in range(t) if got[m] != want[m]]
            raise AssertionError(f"stride {self.stride} n {self.n} off {off} t {t}: powers {bad[:8]} ({len(bad)} wrong)")
        return q


# ------------------------------------------------------------- packet batch
@gpu
@pytest.mark.parametrize("stride", STRIDES)
def test_gpu_packets_every_stride(stride):
    """Both kernel families and the two-pass path at every size: t = 8, 12
    (Cfg<4,2>, Cfg<4,3>), 16, 32 (Shared<2>, Shared<4>), 33 (extract + encode)
    without a reset, t = 32 with one (the exact path after the fused pass)."""
    for n in SIZES:
        bufs, meta = make_batch(n, stride=stride, seed=1000 * stride + n)
        plain = PacketCase(bufs, meta)
        assert plain.last == -1
        bufs, meta = make_batch(n, stride=stride, seed=1000 * stride + n + 1, reset_at=(n // 3,))
        make_insert(bufs, meta, n // 3)
        bufs[n // 3, 30:34] = MY_IP
        reset = PacketCase(bufs, meta)
        assert reset.last == n // 3 and reset.stats["resets"] == 1
        for off in OFFS:
            keep, d_bufs = place(plain.bufs.reshape(-1), off)
            for t in (8, 12, 16, 32, 33):
                plain.run(t, off, d_bufs)
            reset.run(32, off)


@gpu
@pytest.mark.parametrize("stride", RESIDUE_STRIDES)
def test_gpu_packets_every_base_residue(golden, stride):
    """The batch's first byte at every residue mod 16: the head vector (byte
    path below an unaligned base) holds record 0, the tail vector record
    n - 1; both carry identifiers that force the exact recompute of the lazy
    folds, so a wrong byte in either shows in every power sum."""
    w32 = golden["bsgs_wrap_ids"]["8x4"]
    w12 = golden["bsgs_wrap_ids"]["4x3"]
    for n in (257, 1025):
        for off in range(16):
            for t, wraps, resets in ((32, w32, ()), (12, w12, (n - 2,))):
                bufs, meta = make_batch(n, stride=stride, seed=stride * 100 + n + off, reset_at=resets)
                for i in resets:
                    make_insert(bufs, meta, i)
                    bufs[i, 30:34] = MY_IP
                for i, w in ((0, wraps[off % len(wraps)]), (n - 1, wraps[(off + 1) % len(wraps)])):
                    make_insert(bufs, meta, i)
                    put_id(bufs, i, w)
                case = PacketCase(bufs, meta)
                assert case.last == (resets[0] if resets else -1) and int(case.ids[-1]) == wraps[(off + 1) % len(wraps)]
                assert resets or int(case.ids[0]) == wraps[off % len(wraps)]
                case.run(t, off)


@gpu
@pytest.mark.parametrize("stride", (67, 80))
def test_gpu_packets_resets_at_ballot_edges(stride):
    """A reset as the last lane of a wave and the first of the next, of a
    tile, of a chunk; nothing but resets; nothing but filtered packets; one
    record that is a reset."""
    n, t = 1025, 32
    for off in EDGE_OFFS:
        for at in (63, 64, 255, 256, 1023, 1024):
            bufs, meta = make_batch(n, stride=stride, seed=stride + at, reset_at=(at,))
            make_insert(bufs, meta, at)
            bufs[at, 30:34] = MY_IP
            case = PacketCase(bufs, meta)
            assert case.last == at and case.stats["resets"] == 1
            case.run(t, off)
        bufs, meta = make_batch(n, stride=stride, seed=stride + 1, reset_at=range(n), p_filter=0.0)
        case = PacketCase(bufs, meta)
        assert case.stats == {"inserted": 0, "discarded": 0, "resets": n, "filtered": 0, "last_reset_index": n - 1}
        q = case.run(t, off)
        assert q.count() == 0 and q.last_value() is None and q.power_sums() == [0] * t
        bufs, meta = make_batch(n, stride=stride, seed=stride + 2)
        meta["pkttype"] = 4                                  # every packet outgoing
        case = PacketCase(bufs, meta)
        assert case.stats["filtered"] == n
        q = case.run(t, off)
        assert q.count() == 1 and q.last_value() == PRE
        bufs, meta = make_batch(1, stride=stride, seed=stride + 3, reset_at=(0,), p_filter=0.0)
        case = PacketCase(bufs, meta)
        assert case.stats["resets"] == 1 and case.last == 0
        q = case.run(t, off)
        assert q.count() == 0 and q.last_value() is None and q.power_sums() == [0] * t


@gpu
@pytest.mark.parametrize("stride", REJECTED)
def test_gpu_stride_out_of_range_is_rejected(stride):
    """Both entry points answer QK_E_INVAL and leave the quACK, *n_flows, the
    outputs and the statistics as they were."""
    import sidekick_amd as sk
    from sidekick_amd._lib import QK_E_INVAL, QK_OK, lib
    from sidekick_amd.quack import FlowKey, PktStats, get_context
    n, t = 300, 32
    bufs, meta = make_batch(n, stride=stride, seed=stride)
    keep, d_bufs = place(bufs.reshape(-1), 0)
    d_meta = dev_meta(meta)
    handle = get_context(0).handle
    sentinel = (11, 22, 33, 44, 55)

    q = sk.PowerSumQuackU32(t)
    q.insert(PRE)
    before = bytes(q._buf.raw)
    st = PktStats(*sentinel)
    rc = lib().qk_u32_encode_packets_device(handle, d_bufs.data_ptr(), n, stride, d_meta.data_ptr(),
                                            (C.c_uint8 * 4)(*MY_IP), q._buf, C.byref(st), None)
    assert rc == QK_E_INVAL
    assert bytes(q._buf.raw) == before
    assert tuple(getattr(st, k) for k, _ in PktStats._fields_) == sentinel

    cap, rec = 64, lib().qk_u32_size(t)
    keys = (FlowKey * cap)()
    sketches = C.create_string_buffer(b"\xA5" * (cap * rec), cap * rec)
    nf = C.c_size_t(777)
    st = PktStats(*sentinel)
    rc = lib().qk_u32_encode_flows_device(handle, d_bufs.data_ptr(), n, stride, d_meta.data_ptr(),
                                          (C.c_uint8 * 6)(*MY_ADDR), t, keys, sketches, cap, C.byref(nf), C.byref(st),
                                          None)
    assert rc == QK_E_INVAL
    assert nf.value == 777 and sketches.raw == b"\xA5" * (cap * rec) and bytes(keys) == bytes(12 * cap)
    assert tuple(getattr(st, k) for k, _ in PktStats._fields_) == sentinel
    # the same calls at the nearest accepted stride succeed (the arguments, not the stride, were fine)
    ok = STRIDE_MIN if stride < STRIDE_MIN else STRIDE_MAX
    m = (n * stride) // ok
    assert lib().qk_u32_encode_packets_device(handle, d_bufs.data_ptr(), m, ok, d_meta.data_ptr(),
                                              (C.c_uint8 * 4)(*MY_IP), q._buf, C.byref(st), None) == QK_OK
    assert st.inserted + st.discarded + st.resets + st.filtered == m


# ------------------------------------------------------------ per-flow batch
FLOW_T = 16


def flow_case(stride, n, nflows, with_resets):
    """The records of one per-flow case and what the sniff loop makes of them:
    (bufs, meta, {key: ids}, resets, last reset)."""
    seed = 7919 * stride + 31 * n + nflows + int(with_resets)
    bufs, meta = make_flows(n, nflows, seed=seed, stride=stride, p_reset=0.02 if with_resets else 0.0, reset_until=0.9)
    if with_resets and n == 1:       # the single record a reset: nothing is left to run again
        meta["pkttype"][0], meta["protocol_be"][0], bufs[0, 23] = 0, 0x0008, 17
        bufs[0, 30:34], bufs[0, 36:38] = MY_ADDR[:4], MY_ADDR[4:]
    return (bufs, meta) + vector_flows(bufs, meta)


_residues = {}


def restart_residues():
    """{stride: residues mod 16 of the base of the pass that runs again after
    the last reset, d_bufs + (last_reset + 1) * stride}, over the cases of
    test_gpu_flows_every_stride.  CPU only."""
    if not _residues:
        for stride in STRIDES:
            got = set()
            for n in FLOW_SIZES:
                for nflows in (1, 40):
                    last = flow_case(stride, n, nflows, True)[4]
                    if 0 <= last < n - 1:
                        got |= {(off + (last + 1) * stride) % 16 for off in OFFS}
            _residues[stride] = got
    return _residues


def check_restart_residues():
    res = restart_residues()
    assert all(res[s] for s in STRIDES)                  # every stride runs the second pass from a moved base
    every = set().union(*res.values())
    assert 0 in every and len(every) >= 8, sorted(every)
    assert len(set().union(*(res[s] for s in STRIDES if pipelined(s)))) >= 8
    assert len(set().union(*(res[s] for s in STRIDES if not pipelined(s)))) >= 8


def test_flow_restart_bases_cover_the_residues():
    check_restart_residues()


def check_flow_table(table, flows, nres, pre_key, t, tag):
    want = {k: list(v) for k, v in flows.items()}
    if nres == 0:                                        # the entry made before the batch merges; a reset wipes it
        want[pre_key] = [424242] + want.get(pre_key, [])
    got = table.senders()
    assert set(got) == set(want), tag
    for k, ids in want.items():
        q = got[k]
        assert q.count() == len(ids) and q.last_value() == ids[-1], (tag, k.hex())
        assert q.power_sums() == coracle.encode_u32(np.array(ids, dtype=np.uint32), t), (tag, k.hex(), len(ids))


def run_flows(stride, bufs, meta, flows, nres, last_reset, off, pass_meta=True, my_addr=MY_ADDR, ost=None, tag=None):
    import sidekick_amd as sk
    n = len(bufs)
    table = sk.FlowQuacks(FLOW_T)
    pre_key = sorted(flows)[0] if flows else b"\x01" * 12
    table.insert(pre_key, 424242)
    keep, d_bufs = place(bufs.reshape(-1), off)
    st = table.insert_packets(d_bufs, stride=stride, meta=dev_meta(meta) if pass_meta else None, my_addr=my_addr)
    assert st["resets"] == nres and st["inserted"] == sum(len(v) for v in flows.values()), tag
    assert st["last_reset_index"] == last_reset, tag
    assert st["filtered"] == n - st["inserted"] - st["discarded"] - st["resets"], tag
    if ost is not None:
        assert st == ost, tag
    check_flow_table(table, flows, nres, pre_key, FLOW_T, tag)


@gpu
@pytest.mark.parametrize("stride", STRIDES)
def test_gpu_flows_every_stride(stride):
    """k_flow_extract at every stride, without a reset and with resets: after
    the last reset the pass runs again from d_bufs + p_from * stride, a base
    of another residue (restart_residues)."""
    check_restart_residues()
    for n in FLOW_SIZES:
        for nflows in (1, 40):
            for with_resets in (False, True):
                bufs, meta, flows, nres, last_reset = flow_case(stride, n, nflows, with_resets)
                assert (nres > 0) == with_resets, (n, nflows, nres)
                _, ost = qo.sniff_multi_batch({}, 1, bufs[:, :67], meta["pkttype"], meta["protocol_be"], meta["len"],
                                              MY_ADDR)
                assert ost["resets"] == nres and ost["last_reset_index"] == last_reset
                for off in OFFS:
                    run_flows(stride, bufs, meta, flows, nres, last_reset, off, ost=ost,
                              tag=(stride, n, nflows, with_resets, off))


@gpu
@pytest.mark.parametrize("stride", (67, 80))
@pytest.mark.parametrize("no_meta,no_addr", [(True, False), (False, True), (True, True)])
def test_gpu_flows_no_meta_no_addr(stride, no_meta, no_addr):
    """meta = NULL: every packet incoming IPv4 of full length (buf[23] still
    filters); my_addr = NULL: packets to the own address are ordinary inserts."""
    n, nflows = 1025, 40
    bufs, meta = make_flows(n, nflows, seed=stride + 2 * no_meta + no_addr, stride=stride, p_reset=0.02, p_filter=0.2,
                            reset_until=0.9)
    assert (meta["pkttype"] == 4).any() and (meta["len"] != 67).any() and (bufs[:, 23] == 6).any()
    if no_meta:
        model = np.zeros(n, dtype=META_DT)
        model["protocol_be"] = PROTO_IP
        model["len"] = 67
    else:
        model = meta
    addr = None if no_addr else MY_ADDR
    flows, nres, last_reset = vector_flows(bufs, model, my_addr=addr)
    assert (nres == 0 and last_reset == -1) if no_addr else nres > 0
    with_addr = vector_flows(bufs, model)
    assert with_addr[1] > 0                              # the batch holds packets to the own address
    if no_addr:
        assert sum(len(v) for v in flows.values()) > sum(len(v) for v in with_addr[0].values())
    for off in EDGE_OFFS:
        run_flows(stride, bufs, model, flows, nres, last_reset, off, pass_meta=not no_meta, my_addr=addr,
                  tag=(stride, no_meta, no_addr, off))


@gpu
def test_gpu_flows_device_resident_output_widest_stride():
    """Stride 512 (a 131 104-byte tile), three chunks, 40 flows with resets:
    the records written in place in HBM are the host-output path's and the
    oracle's."""
    import torch
    from sidekick_amd.quack import encode_flows
    stride, n, t = STRIDE_MAX, 2049, FLOW_T
    bufs, meta, flows, nres, last_reset = flow_case(stride, n, 40, True)
    assert nres > 0 and len(flows) == 40
    keep, d_bufs = place(bufs.reshape(-1), 0)
    d_meta = dev_meta(meta)
    hk, hq, hst = encode_flows(d_bufs, t, stride=stride, meta=d_meta, my_addr=MY_ADDR)
    dk, dq, dst = encode_flows(d_bufs, t, stride=stride, meta=d_meta, my_addr=MY_ADDR, device_out=True)
    torch.cuda.synchronize()
    assert hst == dst and dst["resets"] == nres and dst["last_reset_index"] == last_reset
    assert hk == sorted(flows) and [bytes(r) for r in dk.cpu().numpy()] == hk
    recs = dq.cpu().numpy().view(np.uint32)
    assert recs.shape == (len(hk), 4 + t)
    for i, (k, q) in enumerate(zip(hk, hq)):
        assert bytes(q._buf.raw) == recs[i].tobytes(), k.hex()
        assert q.count() == len(flows[k]) and q.last_value() == flows[k][-1]
        assert q.power_sums() == coracle.encode_u32(np.array(flows[k], dtype=np.uint32), t), k.hex()
