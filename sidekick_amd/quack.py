"""Host-side mirror of the reference `quack` crate API over libquack_hip.so.

Same names, argument meaning and error behaviour as the Rust calls the
reference tree makes:

    PowerSumQuackU32::new(threshold)        sidekick/src/sidekick.rs:32
    quack.insert(id)                        sidekick.rs:42, sidekick_multi.rs:82
    quack.remove(id)                        media_client.rs:319
    quack.count() / quack.last_value()      media_client.rs:231-233,259-260
    diff.sub_assign(quack)                  media_client.rs:296
    diff.to_coeffs()                        media_client.rs:304
    arithmetic::eval(&coeffs, id).value()   media_client.rs:310
    clone(), bincode serialize/deserialize  sidekick.rs:187,204; media_client.rs:227

plus the batch entry points of the MI355X engine:

    insert_batch(ids)        encode an id array on the GPU (device tensor:
                             HBM-resident path; numpy array: host path with
                             pipelined H2D).
    decode_with_log(log)     to_coeffs on the host, root test on the GPU.
    to_coeffs_segments(..)   to_coeffs of one diff sketch per flow, one device pass.
    decode_segments(..)      decode_with_log of many (diff, log segment) pairs,
                             one device pass (the per-flow quACKs of SidekickMulti).
    sender_step(..)          the sender loop of media_client.rs:233-322 for many
                             flows: prefix insert, reset test, decode, removes.
    sender_steps(..)         the same loop over every queued quACK of a flow, one
                             after the other, in one call (ingest_wire_queue).
    drain_segments(..)       seqno_ids.drain(..idx+1) of every flow's log.
    update_segments(..)      the same drain plus seqno_ids.push of a batch of sent
                             packets, one pass over the device-resident log.
    DeviceSenderLog          QuackReceiver for many flows: log, seqnos and my
                             quACKs stay in HBM between send and on_quacks.
    snapshot_segments(..)    the quACK after every packet that brings its flow's
                             count to a multiple of frequency_pkts, for a batch.
    DeviceFlowSnapshots      the proxy's table by flow index: a batch in, the
                             datagrams of sidekick_multi.rs:271-283 out, in order.
    snapshot_flows(..)       the same from captured packets against the table
                             held by AddrKey: filter, key, Resets, every
                             crossing in send order, the table after the batch.
    flows_merge / flows_diff / flows_lookup, DeviceFlowQuacks
                             SidekickMulti's flow table as key-sorted arrays in
                             HBM: merge a batch, diff against a peer, look up.

Per-packet insert/remove stay on the host (one insert is far cheaper than a
kernel launch); every batch call runs the gfx950 kernels and raises if the
device or the library is unavailable -- there is no CPU fallback.

This module is the public surface: what each call means, the order in which
its arguments are judged, and the library call.  How an argument becomes what
the library takes is written once, in _args.py.
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np

from dataclasses import dataclass

from ._args import (Records, _device_array, _host_array, csr, csr_drain, dev_index, is_record_tensor,
                    need_torch, packet_batch, ptr, retry_capacity, split_hits, stream_of, uint_len, uint_on_device)
from ._lib import (P32, P64, QK_E_CAPACITY, QK_E_INVAL, QK_E_MISMATCH, SND_ADVANCED, SND_IDLE, SND_RESET_EXCEEDS,
                   SND_RESET_REORDERED, SND_RESET_RETX, QuackError, check, lib)

__all__ = [
    "PowerSumQuackU32", "PowerSumQuackU64", "ModularInteger", "CoefficientVector",
    "arithmetic", "Context", "get_context", "device_count", "FlowQuacks",
    "to_coeffs_segments", "decode_segments", "sender_step", "drain_segments", "SenderStep",
    "update_segments", "DeviceSenderLog", "SenderLogStep", "sender_steps", "SenderSteps",
    "snapshot_segments", "Snapshots", "DeviceFlowSnapshots", "snapshot_flows", "FlowSnapshots",
    "flows_merge", "flows_diff", "flows_lookup", "DeviceFlowQuacks",
    "emit_wire", "ingest_wire", "ingest_wire_queue", "wire_max",
]


# --------------------------------------------------------------------------
# Device contexts (one per device, created lazily)
# --------------------------------------------------------------------------
class Context:
    """Owns a qk_ctx* (device scratch, streams, profiling events)."""

    def __init__(self, device: int = 0, handle=None):
        self.owned = handle is None
        if handle is None:
            handle = C.c_void_p()
            check(lib().qk_ctx_create(int(device), C.byref(handle)), f"qk_ctx_create({device})")
        self.handle = handle
        self.device = int(device)

    def close(self):
        if self.handle and self.owned:
            lib().qk_ctx_destroy(self.handle)
            self.handle = None

    def synchronize(self, stream=None):
        check(lib().qk_ctx_synchronize(self.handle, stream), "synchronize")

    def set_profiling(self, on: bool):
        check(lib().qk_ctx_set_profiling(self.handle, int(bool(on))))

    def kernel_stats(self):
        """(total_ms, launches) of the dominant kernel since the last call."""
        ms = C.c_double()
        n = C.c_uint64()
        check(lib().qk_ctx_kernel_stats(self.handle, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def set_grid(self, blocks: int):
        check(lib().qk_ctx_set_grid(self.handle, int(blocks)))

    def set_knob(self, name: str, value: int):
        """A measurement knob of this context (qk_ctx_set_knob)."""
        check(lib().qk_ctx_set_knob(self.handle, name.encode(), int(value)), f"set_knob({name}={value})")

    def trim(self):
        """Free grown-out scratch buffers (synchronises the device)."""
        check(lib().qk_ctx_trim(self.handle), "trim")

    def clock_probe_async(self, microseconds: int, out, stream) -> None:
        """Enqueue the shader-clock probe (qk_clock_probe) on `stream` (a raw
        stream handle): out (a CUDA int64 tensor of 2) receives (s_memtime
        ticks, 100 MHz ticks) over `microseconds` of wall time."""
        check(lib().qk_clock_probe(self.handle, int(microseconds), out.data_ptr(), stream), "clock_probe")


_ctx_lock = threading.Lock()
_contexts: dict = {}


def device_count() -> int:
    n = C.c_int()
    lib().qk_device_count(C.byref(n))
    return n.value


def get_context(device: int = 0) -> Context:
    with _ctx_lock:
        ctx = _contexts.get(device)
        if ctx is None:
            ctx = _contexts[device] = Context(device)
        return ctx


def _context(ctx, *tensors) -> Context:
    """`ctx or get_context(dev)` where dev has yet to be found: that of the
    first CUDA tensor among the arguments, else 0.  Called first, so that with
    no device a wrapper raises QK_E_NO_DEVICE whatever its arguments are."""
    if ctx is not None:
        return ctx
    for a in tensors:
        if getattr(a, "is_cuda", False):
            return get_context(dev_index(a))
    return get_context(0)


# --------------------------------------------------------------------------
# Field values and coefficient vectors
# --------------------------------------------------------------------------
class ModularInteger:
    """quack::arithmetic::ModularInteger: canonical value in [0, p)."""
    __slots__ = ("_v", "bits")

    def __init__(self, v: int, bits: int = 32):
        self.bits = bits
        self._v = int(v) % (P32 if bits == 32 else P64)

    def value(self) -> int:
        return self._v

    def __eq__(self, other):
        if isinstance(other, ModularInteger):
            return self._v == other._v and self.bits == other.bits
        return self._v == other

    def __hash__(self):
        return hash((self._v, self.bits))

    def __repr__(self):
        return f"ModularInteger<u{self.bits}>({self._v})"


class CoefficientVector(list):
    """Result of to_coeffs(): c_1..c_d of prod(z - x_missing), canonical ints."""

    def __init__(self, values, bits: int):
        super().__init__(int(v) for v in values)
        self.bits = bits


class _Arithmetic:
    """quack::arithmetic (media_client.rs:21,310)."""

    @staticmethod
    def eval(coeffs: CoefficientVector, x: int) -> ModularInteger:
        bits = getattr(coeffs, "bits", 32)
        d = len(coeffs)
        if bits == 32:
            arr = (C.c_uint32 * max(d, 1))(*coeffs)
            return ModularInteger(lib().qk_u32_eval(arr, d, int(x) & 0xFFFFFFFF), 32)
        arr = (C.c_uint64 * max(d, 1))(*coeffs)
        return ModularInteger(lib().qk_u64_eval(arr, d, int(x) & 0xFFFFFFFFFFFFFFFF), 64)


arithmetic = _Arithmetic()


def roots(coeffs, bits: int = 32) -> list:
    """The distinct roots in GF(p), ascending, of z^d + c_1 z^(d-1) + ... + c_d
    (qk_u32_roots / qk_u64_roots, roots.cpp): a log entry is a root-test hit
    exactly when it is congruent to one of them."""
    d = len(coeffs)
    T = C.c_uint32 if bits == 32 else C.c_uint64
    c = (T * max(d, 1))(*[int(v) for v in coeffs])
    out = (T * max(d, 1))()
    k = C.c_uint32()
    check(getattr(lib(), f"qk_u{bits}_roots")(c, d, out, d, C.byref(k)), "roots")
    return [int(v) for v in out[:k.value]]


# --------------------------------------------------------------------------
# The sketch
# --------------------------------------------------------------------------
class _PowerSumQuack:
    BITS = 32
    _ELEM = C.c_uint32
    _pre = "qk_u32_"

    def __init__(self, threshold: int):
        if threshold < 0 or threshold > 0xFFFFFFFF:
            raise ValueError("threshold must fit u32")
        self._t = int(threshold)
        self._buf = C.create_string_buffer(self._f("size")(self._t))
        check(self._f("init")(self._buf, self._t), "init")

    # -- plumbing -----------------------------------------------------------
    @classmethod
    def _f(cls, name):
        return getattr(lib(), cls._pre + name)

    @classmethod
    def new(cls, threshold: int):
        return cls(threshold)

    @classmethod
    def _from_record(cls, raw: bytes, threshold: int):
        """The sketch whose record (the qk_u32 / qk_u64 image, as _buf holds it) is `raw`."""
        q = cls.__new__(cls)
        q._t = threshold
        q._buf = C.create_string_buffer(raw, len(raw))
        return q

    def _record_i32(self) -> np.ndarray:
        """The record as int32 words (a view of _buf): a row of a record tensor."""
        return np.frombuffer(self._buf, dtype=np.int32)

    def _hdr(self):
        return np.frombuffer(self._buf, dtype=np.uint32, count=4)

    # -- accessors ----------------------------------------------------------
    def threshold(self) -> int:
        return self._t

    def count(self) -> int:
        return int(self._hdr()[1])

    def last_value(self):
        h = self._hdr()
        if not h[2]:
            return None
        if self.BITS == 32:
            return int(h[3])
        return int(np.frombuffer(self._buf, dtype=np.uint64, count=1, offset=16)[0])

    def power_sums(self) -> list:
        if self.BITS == 32:
            return [int(v) for v in np.frombuffer(self._buf, dtype=np.uint32, count=self._t, offset=16)]
        return [int(v) for v in np.frombuffer(self._buf, dtype=np.uint64, count=self._t, offset=24)]

    def clone(self):   # _from_record written out: one call less on the per-packet path
        q = type(self).__new__(type(self))
        q._t = self._t
        q._buf = C.create_string_buffer(self._buf.raw, len(self._buf))
        return q

    __copy__ = clone

    def __eq__(self, other):
        return type(self) is type(other) and self._buf.raw == other._buf.raw

    def __repr__(self):
        return (f"{type(self).__name__}(threshold={self._t}, count={self.count()}, "
                f"last_value={self.last_value()})")

    # -- per-packet host path -------------------------------------------------
    def insert(self, ident: int) -> None:
        check(self._f("insert")(self._buf, int(ident)), "insert")

    def remove(self, ident: int) -> None:
        check(self._f("remove")(self._buf, int(ident)), "remove")

    def sub_assign(self, rhs) -> None:
        check(self._f("sub_assign")(self._buf, rhs._buf), "sub_assign")

    def __isub__(self, rhs):
        self.sub_assign(rhs)
        return self

    def merge(self, later) -> None:
        """Union with the disjoint stream that follows this one (additivity)."""
        check(self._f("merge")(self._buf, later._buf), "merge")

    def to_coeffs(self) -> CoefficientVector:
        d = C.c_uint32()
        cap = max(self._t, 1)
        out = (self._ELEM * cap)()
        check(self._f("to_coeffs")(self._buf, out, cap, C.byref(d)), "to_coeffs")
        return CoefficientVector(out[: d.value], self.BITS)

    # -- bincode wire image ----------------------------------------------------
    def serialize(self) -> bytes:
        n = self._f("serialized_size")(self._buf)
        out = (C.c_uint8 * n)()
        ln = C.c_size_t()
        check(self._f("serialize")(self._buf, out, n, C.byref(ln)), "serialize")
        return bytes(out[: ln.value])

    @classmethod
    def deserialize(cls, data: bytes):
        src = (C.c_uint8 * len(data)).from_buffer_copy(data)
        t = C.c_uint32()
        check(cls._f("deserialize")(src, len(data), None, C.byref(t)), "deserialize")
        q = cls(t.value)
        check(cls._f("deserialize")(src, len(data), q._buf, None), "deserialize")
        return q

    # -- batch (GPU) path -------------------------------------------------------
    def insert_batch(self, ids, ctx: Context | None = None) -> None:
        """Insert every id of `ids` in array order, on the GPU.

        A CUDA tensor is encoded where it lies (HBM-resident path); a numpy
        array / sequence goes through the pipelined host->device path."""
        if self._t == 0:
            raise QuackError(-2, "insert_batch into a threshold-0 quACK")
        dev = _device_array(ids, self.BITS)
        if dev is not None:
            p, n, d, stream = dev
            check(self._f("encode_device")((ctx or get_context(d)).handle, p, n, self._buf, stream), "encode_device")
            return
        arr = _host_array(ids, self.BITS)
        ctx = ctx or get_context(0)
        check(self._f("encode_host")(ctx.handle, arr.ctypes.data, arr.size, self._buf), "encode_host")

    def root_test(self, coeffs, log, stop_value=None, ctx: Context | None = None, cap: int = 1 << 16):
        """Positions (log order) of entries of `log` that are roots of
        `coeffs`; with stop_value, only positions before its first
        occurrence (media_client.rs:306-313)."""
        return self._root_test(coeffs, log, stop_value, ctx, cap, shard=False)[0]

    def root_test_shard(self, coeffs, log, stop_value=None, ctx: Context | None = None, cap: int = 1 << 16):
        """root_test on one shard of a log: (positions, stop_index) where
        stop_index is the first position equal to stop_value in this shard,
        or len(log) (sidekick_amd.dist.root_test_sharded merges shards)."""
        return self._root_test(coeffs, log, stop_value, ctx, cap, shard=True)

    def _root_test(self, coeffs, log, stop_value, ctx, cap, shard):
        coeffs = list(coeffs)
        d = len(coeffs)
        carr = (self._ELEM * max(d, 1))(*coeffs)
        dev = _device_array(log, self.BITS)
        if dev is None:   # device memory for a host log: one H2D copy, then the GPU test
            keep = uint_on_device(log, "cuda", "log", self.BITS)
            dev = _device_array(keep, self.BITS)
        lptr, n, dv, stream = dev
        ctx = ctx or get_context(dv)
        stop_idx = C.c_uint64(n)

        def attempt(cap):
            hits = (C.c_uint64 * max(cap, 1))()
            nh = C.c_size_t()
            args = (ctx.handle, carr, d, lptr, n, int(stop_value is not None), int(stop_value or 0), hits, cap,
                    C.byref(nh))
            if shard:
                rc = self._f("root_test_shard_device")(*args, C.byref(stop_idx), stream)
            else:
                rc = self._f("root_test_device")(*args, stream)
            return rc, nh.value, (hits, nh.value)
        hits, nh = retry_capacity(attempt, cap, "root_test_device")
        return [int(h) for h in hits[:nh]], int(stop_idx.value)

    def decode_host(self, log, stop_at_last: bool = False) -> list:
        """Positions of the missing entries of a HOST log (numpy / sequence),
        tested on the CPU (qk_*_decode_host): to_coeffs, then the root test,
        cut at the first entry equal to last_value() when stop_at_last
        (media_client.rs:304-313).  For the short logs a receiver holds."""
        arr = _host_array(log, self.BITS)
        p = arr.ctypes.data_as(C.POINTER(self._ELEM))
        cap = max(self._t, 1)
        while True:   # ptr and retry_capacity written out: the receiver calls this per quACK, and each hop showed
            hits = (C.c_uint64 * cap)()
            nh = C.c_size_t()
            rc = self._f("decode_host")(self._buf, p, arr.size, int(stop_at_last), hits, cap, C.byref(nh))
            if rc != QK_E_CAPACITY:
                check(rc, "decode_host")
                return [int(h) for h in hits[: nh.value]]
            cap = nh.value

    def decode_with_log(self, log, ctx: Context | None = None) -> list:
        """quack's decode_with_log: the ids of `log` that are missing (every
        log entry congruent to a root, in log order)."""
        if self.count() == 0:
            return []
        coeffs = self.to_coeffs()
        pos = self.root_test(coeffs, log, ctx=ctx)
        dev = _device_array(log, self.BITS)
        if dev is not None:
            torch = need_torch()
            idx = torch.tensor(pos, dtype=torch.int64, device=log.device)
            vals = log[idx].cpu().numpy()
        else:
            vals = _host_array(log, self.BITS)[pos]
        mask = 0xFFFFFFFF if self.BITS == 32 else 0xFFFFFFFFFFFFFFFF
        return [int(v) & mask for v in vals]


class PowerSumQuackU32(_PowerSumQuack):
    """quack::PowerSumQuackU32 — u32 ids over GF(2^32 - 5)."""
    BITS = 32
    _ELEM = C.c_uint32
    _pre = "qk_u32_"


class PowerSumQuackU64(_PowerSumQuack):
    """quack::PowerSumQuackU64 — u64 ids over GF(2^64 - 59)."""
    BITS = 64
    _ELEM = C.c_uint64
    _pre = "qk_u64_"


# --------------------------------------------------------------------------
# Low-level async encode (bench / multi-GPU): partial vectors on the device
# --------------------------------------------------------------------------
class PktMeta(C.Structure):
    _fields_ = [("pkttype", C.c_uint8), ("reserved", C.c_uint8), ("protocol_be", C.c_uint16), ("len", C.c_uint32)]


class PktStats(C.Structure):
    _fields_ = [("inserted", C.c_uint64), ("discarded", C.c_uint64), ("resets", C.c_uint64),
                ("filtered", C.c_uint64), ("last_reset_index", C.c_int64)]


def encode_packets(q: "PowerSumQuackU32", bufs, stride: int = 67, meta=None, my_ipv4=None,
                   ctx: Context | None = None) -> dict:
    """Sniff-loop batch (sidekick.rs:76-124) on the GPU: `bufs` is a CUDA
    uint8 tensor of n*stride bytes (records), `meta` an optional CUDA tensor
    of n 8-byte qk_pkt_meta records (int64 view), `my_ipv4` 4 ints or None.
    Updates q in place (reset if a packet to my_ipv4 is seen); returns stats."""
    n, dev, mptr = packet_batch(bufs, stride, meta)
    ctx = ctx or get_context(dev)
    ip = (C.c_uint8 * 4)(*my_ipv4) if my_ipv4 is not None else None
    st = PktStats()
    check(lib().qk_u32_encode_packets_device(ctx.handle, bufs.data_ptr(), n, stride, mptr, ip, q._buf,
                                              C.byref(st), stream_of(bufs)), "encode_packets")
    return {k: getattr(st, k) for k, _ in PktStats._fields_}


class FlowKey(C.Structure):
    _fields_ = [("addr", C.c_uint8 * 12)]


_quack_from_bytes = PowerSumQuackU32._from_record   # the name tests/test_gpu_wire.py imports


def _quacks_from_records(raw: bytes, rec: int, n: int, threshold: int) -> list:
    """The PowerSumQuackU32 of the first n records, of `rec` bytes each, of `raw`."""
    return [PowerSumQuackU32._from_record(raw[i * rec:(i + 1) * rec], threshold) for i in range(n)]


def encode_segments(ids, offsets, threshold: int, ctx: Context | None = None) -> list:
    """Segmented encode: `ids` a CUDA u32 tensor grouped by flow, `offsets`
    nseg+1 ints (CSR).  Returns one PowerSumQuackU32 per segment."""
    iptr, n, dev, stream = _device_array(ids, 32)
    ctx = ctx or get_context(dev)
    offs, nseg = csr(offsets, "ids")
    rec = lib().qk_u32_size(threshold)
    out = C.create_string_buffer(max(nseg, 1) * rec)
    check(lib().qk_u32_encode_segments_device(ctx.handle, iptr, ptr(offs), nseg, threshold, out, stream),
          "encode_segments")
    return _quacks_from_records(out.raw, rec, nseg, threshold)


def to_coeffs_segments(diffs, threshold: int | None = None, ctx: Context | None = None):
    """to_coeffs() of every diff sketch of a batch in one device pass
    (qk_u32_to_coeffs_segments_device; media_client.rs:304 per flow of
    sidekick_multi.rs:65-90).  Returns (coeffs, status): one CoefficientVector
    per sketch (empty where status is QK_E_UNDECODABLE, count > threshold) and
    the per-sketch status codes."""
    r = Records.parse(diffs, PowerSumQuackU32, threshold)
    ctx = ctx or get_context(r.dev or 0)
    nseg, t = r.nseg, r.t
    coeffs = np.zeros((max(nseg, 1), t), dtype=np.uint32)
    deg = np.zeros(max(nseg, 1), dtype=np.uint32)
    status = np.zeros(max(nseg, 1), dtype=np.int32)
    check(lib().qk_u32_to_coeffs_segments_device(ctx.handle, r.ptr, nseg, t, ptr(coeffs), ptr(deg), ptr(status),
                                                  stream_of(r.keep, r.dev) if r.dev is not None else None),
          "to_coeffs_segments")
    return ([CoefficientVector(coeffs[g, :deg[g]].tolist(), 32) for g in range(nseg)],
            [int(s) for s in status[:nseg]])


def decode_segments(diffs, log, offsets, stop_at_last: bool = False, ctx: Context | None = None):
    """decode_with_log for a batch of flows in one device pass
    (qk_u32_decode_segments_device): `diffs` one diff sketch per flow (a list
    of PowerSumQuackU32 of one threshold, or the CUDA int32 record tensor of
    encode_flows(device_out=True)), `log` a CUDA u32/int32 tensor grouped by
    flow, `offsets` nseg + 1 ints (CSR).  Returns (positions, status):
    positions[g] are the positions, local to segment g, of its missing
    entries, equal to diffs[g].decode_host(log[offsets[g]:offsets[g+1]],
    stop_at_last); status[g] is QK_OK or QK_E_UNDECODABLE (no positions)."""
    r = Records.parse(diffs, PowerSumQuackU32)
    nseg = r.nseg
    ctx, log, (lptr, n, _, stream) = _log_on_device(log, ctx)
    offs, _ = csr(offsets, "diffs", nseg, n)
    hoffs = np.zeros(nseg + 1, dtype=np.uint64)
    status = np.zeros(max(nseg, 1), dtype=np.int32)

    def attempt(cap):
        hits = np.empty(max(cap, 1), dtype=np.uint64)
        nh = C.c_size_t()
        rc = lib().qk_u32_decode_segments_device(ctx.handle, r.ptr, lptr, ptr(offs), nseg, r.t, int(bool(stop_at_last)),
                                                 ptr(hits), cap, ptr(hoffs), ptr(status), C.byref(nh), stream)
        return rc, nh.value, hits
    hits = retry_capacity(attempt, max(1024, 4 * nseg), "decode_segments")
    return split_hits(hits, hoffs, offs), [int(s) for s in status[:nseg]]


def _log_on_device(log, ctx):
    """(context, log tensor, its _device_array): a CUDA u32/int32 log as it is, a host
    one uploaded (one H2D copy; no device: QK_E_NO_DEVICE, there is no CPU path)."""
    d_log = _device_array(log, 32)
    if d_log is None:
        ctx = ctx or get_context(0)
        log = uint_on_device(log, f"cuda:{ctx.device}", "log")
        d_log = _device_array(log, 32)
    return ctx or get_context(d_log[2]), log, d_log


@dataclass
class SenderStep:
    """What sender_step returns, one entry per flow."""
    mine_out: object      # CUDA int32 record tensor [nseg, 4 + t]: my quACKs after the step
    action: np.ndarray    # np.uint8: SND_IDLE, SND_ADVANCED, or the OR of the SND_RESET_* bits
    drain: np.ndarray     # np.uint64: log entries to drop (drain_segments)
    missing: list         # per flow, the segment-local positions to retransmit, ascending


def sender_step(mine, peer, log, offsets, present=None, ctx: Context | None = None) -> SenderStep:
    """listen_for_quacks_power_sum (media_client.rs:233-322; QuackReceiver.on_quack)
    for a batch of flows in one device pass (qk_u32_sender_step_segments_device).
    `mine` / `peer`: my quACK and the received one per flow, row g for flow g (a
    list of PowerSumQuackU32 of one threshold, uploaded here, or a CUDA int32
    record tensor [nseg, 4 + t]); `log` the sent ids grouped by flow (a CUDA
    u32/int32 tensor, or a host array, uploaded), `offsets` nseg + 1 ints (CSR);
    `present` nseg flags (a host sequence or a CUDA uint8 tensor), None when
    every flow has a quACK.  Per flow: the prefix up to the first entry equal to
    the peer's last value is inserted into mine, the three reset conditions are
    tested (a reset keeps the prefix insert and decodes nothing), otherwise
    mine - peer is decoded against the segment and every missing id removed
    from mine.  The reset debounce stays with the caller."""
    # what the host alone can judge, then the context (no device: QK_E_NO_DEVICE), then the uploads
    r_mine = Records.parse(mine, PowerSumQuackU32)
    r_mine.need_threshold("mine")
    r_peer = Records.parse(peer, PowerSumQuackU32)
    r_peer.need_threshold("peer")
    nseg, t = r_mine.nseg, r_mine.t
    if r_peer.t != t:
        raise QuackError(QK_E_MISMATCH, "mine and peer of different thresholds")
    if r_peer.nseg != nseg:
        raise ValueError("mine and peer must hold one record per flow")
    ctx = ctx or get_context(r_mine.dev or 0)
    d_mine, d_peer = r_mine.to_device(ctx, "mine"), r_peer.to_device(ctx, "peer")
    torch = need_torch()
    device = d_mine.device
    if d_peer.device != device:
        raise ValueError("mine and peer on different devices")
    d_log = _device_array(log, 32)
    if d_log is None:
        log = uint_on_device(log, device, "log")
        d_log = _device_array(log, 32)
    lptr, n, _, stream = d_log
    offs, _ = csr(offsets, "mine", nseg, n)
    d_present = None
    if present is not None:
        if isinstance(present, torch.Tensor):
            if not (present.is_cuda and present.dtype in (torch.uint8, torch.bool) and present.is_contiguous()):
                raise TypeError("present must be a contiguous CUDA uint8/bool tensor or a host sequence")
            d_present = present
        else:
            d_present = torch.from_numpy(np.ascontiguousarray(np.asarray(present, dtype=bool)).view(np.uint8)).to(device)
        if d_present.numel() != nseg:
            raise ValueError("present must hold one flag per flow")
    mine_out = torch.empty((nseg, 4 + t), dtype=torch.int32, device=device)
    action = np.zeros(max(nseg, 1), dtype=np.uint8)
    drain = np.zeros(max(nseg, 1), dtype=np.uint64)
    hoffs = np.zeros(nseg + 1, dtype=np.uint64)

    def attempt(cap):
        hits = np.empty(max(cap, 1), dtype=np.uint64)
        nh = C.c_size_t()
        rc = lib().qk_u32_sender_step_segments_device(
            ctx.handle, d_mine.data_ptr(), d_peer.data_ptr(), d_present.data_ptr() if d_present is not None else None,
            lptr, ptr(offs), nseg, t, mine_out.data_ptr(), ptr(action), ptr(drain), ptr(hits), cap, ptr(hoffs),
            C.byref(nh), stream)
        return rc, nh.value, hits
    hits = retry_capacity(attempt, max(1024, 4 * nseg), "sender_step")
    return SenderStep(mine_out, action[:nseg], drain[:nseg], split_hits(hits, hoffs, offs))


@dataclass
class SenderSteps:
    """What sender_steps returns: per queued quACK (queue order) and per flow."""
    mine_out: object      # CUDA int32 record tensor [nseg, 4 + t]: my quACKs after the flow's last stepped quACK
    q_action: np.ndarray  # np.uint8 per quACK: SND_IDLE, SND_ADVANCED, the OR of the SND_RESET_* bits, or SND_UNSTEPPED
    q_drain: np.ndarray   # np.uint64 per quACK: the log entries its step drops
    stepped: np.ndarray   # np.uint32 per flow: quACKs consumed, the resetting one included
    drain: np.ndarray     # np.uint64 per flow: the sum of its q_drain (drain_segments / update_segments)
    missing: list         # per quACK, the positions to retransmit, local to the flow's segment, ascending
    q_offsets: np.ndarray  # np.uint64 [nseg + 1]: the queue's CSR index by flow


def sender_steps(mine, queue, q_offsets, log, offsets, ctx: Context | None = None) -> SenderSteps:
    """listen_for_quacks_power_sum (media_client.rs:223-323) for a batch of
    flows with EVERY queued quACK of a flow stepped, one after the other, in one
    device call (qk_u32_sender_steps_segments_device).  `mine`: my quACK per
    flow; `queue`: the received quACKs grouped by flow, in arrival order within
    a flow, `q_offsets` their CSR index (nseg + 1 ints, q_offsets[0] == 0) —
    what ingest_wire_queue returns (both record batches: a list of
    PowerSumQuackU32 of one threshold, uploaded here, or a CUDA int32 record
    tensor); `log` / `offsets` as sender_step takes them.  Per flow the loop of
    sender_step runs over its quACKs on a log that each ADVANCED step shortens
    (by an offset: the log is not moved) and stops at the first reset: the
    quACKs behind it stay SND_UNSTEPPED, for the caller to drop (the reset
    fired) or to pass again (the debounce held it back)."""
    r_mine = Records.parse(mine, PowerSumQuackU32)
    r_mine.need_threshold("mine")
    nseg, t = r_mine.nseg, r_mine.t
    r_queue = Records.parse(queue, PowerSumQuackU32, threshold=t)
    if r_queue.t != t:
        raise QuackError(QK_E_MISMATCH, "mine and queue of different thresholds")
    qoffs, _ = csr(q_offsets, "mine", nseg, r_queue.nseg)
    nq = int(qoffs[-1])
    ctx = ctx or get_context(r_mine.dev or 0)
    d_mine = r_mine.to_device(ctx, "mine")
    d_queue = r_queue.to_device(ctx, "queue") if r_queue.nseg else None
    torch = need_torch()
    device = d_mine.device
    if d_queue is not None and d_queue.device != device:
        raise ValueError("mine and queue on different devices")
    d_log = _device_array(log, 32)
    if d_log is None:
        log = uint_on_device(log, device, "log")
        d_log = _device_array(log, 32)
    lptr, n, _, stream = d_log
    offs, _ = csr(offsets, "mine", nseg, n)
    mine_out = torch.empty((nseg, 4 + t), dtype=torch.int32, device=device)
    q_action = np.zeros(max(nq, 1), dtype=np.uint8)
    q_drain = np.zeros(max(nq, 1), dtype=np.uint64)
    stepped = np.zeros(max(nseg, 1), dtype=np.uint32)
    drain = np.zeros(max(nseg, 1), dtype=np.uint64)
    hoffs = np.zeros(nq + 1, dtype=np.uint64)

    def attempt(cap):
        hits = np.empty(max(cap, 1), dtype=np.uint64)
        nh = C.c_size_t()
        rc = lib().qk_u32_sender_steps_segments_device(
            ctx.handle, d_mine.data_ptr(), d_queue.data_ptr() if d_queue is not None else None, ptr(qoffs), lptr,
            ptr(offs), nseg, t, mine_out.data_ptr(), ptr(q_action), ptr(q_drain), ptr(stepped), ptr(drain), ptr(hits),
            cap, ptr(hoffs), C.byref(nh), stream)
        return rc, nh.value, hits
    hits = retry_capacity(attempt, max(1024, 4 * nseg), "sender_steps")
    # the segment start of every quACK's flow (q_offsets[0] == 0: the library refuses anything else)
    first = np.repeat(offs[:-1], (qoffs[1:] - qoffs[:-1]).astype(np.int64)) if nseg else offs[:0]
    return SenderSteps(mine_out, q_action[:nq], q_drain[:nq], stepped[:nseg], drain[:nseg],
                       split_hits(hits, hoffs, first), qoffs)


def drain_segments(log, offsets, drain, aux=None, ctx: Context | None = None):
    """seqno_ids.drain(..idx+1) (media_client.rs:298,316) for all flows on the
    device (qk_u32_log_drain_segments_device): segment g of the result is
    segment g of `log` (a CUDA u32/int32 tensor grouped by flow, CSR `offsets`)
    without its first drain[g] entries.  `aux`: an optional parallel tensor
    (the seqnos), moved alike.  Returns (log_out, offsets_out) or (log_out,
    offsets_out, aux_out)."""
    if drain is None:
        raise TypeError("drain must hold one count per segment")
    offs, nseg, dr, lens = csr_drain(offsets, drain, "drain_segments")
    d_log = _device_array(log, 32)
    if d_log is None:
        raise TypeError("log must be a CUDA u32/int32 tensor")
    lptr, n, dev, stream = d_log
    if nseg and int(offs[-1]) > n:
        raise ValueError("offsets run past the end of log")
    if aux is not None:
        d_aux = _device_array(aux, 32)
        if d_aux is None or d_aux[1] != n or aux.device != log.device:
            raise TypeError("aux must be a CUDA u32/int32 tensor as long as log, on its device")
    ctx = ctx or get_context(dev)
    torch = need_torch()
    left = int((lens - dr).sum())
    out = torch.empty((left,), dtype=log.dtype, device=log.device)
    aux_out = torch.empty((left,), dtype=aux.dtype, device=log.device) if aux is not None else None
    offs_out = np.zeros(nseg + 1, dtype=np.uint64)
    check(lib().qk_u32_log_drain_segments_device(
        ctx.handle, lptr, d_aux[0] if aux is not None and left else None, ptr(offs), ptr(dr), nseg,
        out.data_ptr() if left else None, aux_out.data_ptr() if aux is not None and left else None, left,
        ptr(offs_out), stream), "drain_segments")
    return (out, offs_out) if aux is None else (out, offs_out, aux_out)


def update_segments(log, offsets, drain, new_flow, new_ids, aux=None, new_aux=None, ctx: Context | None = None):
    """seqno_ids.push((seqno, id)) (media_client.rs:110, :318-322) for a batch of
    sent packets, with the drain of :298,316 in the same pass over the
    device-resident log (qk_u32_log_update_segments_device).  Segment g of the
    result is segment g of `log` (grouped by flow, CSR `offsets`) without its
    first drain[g] entries (`drain` None: nothing is drained), followed by the
    new_ids[i] with new_flow[i] == g in ascending i: the batch is given
    ungrouped, in send order, and a flow's log stays in send order.  `aux` /
    `new_aux`: the optional parallel array (the seqnos), both or neither.
    `log`, `aux` and the three new_* arrays are CUDA u32/int32 tensors, or host
    arrays, which are uploaded.  Returns (log_out, offsets_out) or (log_out,
    offsets_out, aux_out), as drain_segments does."""
    offs, nseg, dr, lens = csr_drain(offsets, drain, "update_segments")
    n_new = uint_len(new_flow, "new_flow")
    if uint_len(new_ids, "new_ids") != n_new:
        raise ValueError("new_flow and new_ids must be equally long")
    if (aux is None) != (new_aux is None):
        raise ValueError("aux and new_aux go together")
    if new_aux is not None and uint_len(new_aux, "new_aux") != n_new:
        raise ValueError("new_flow and new_aux must be equally long")
    ctx, log, (lptr, n, _, stream) = _log_on_device(log, ctx)
    torch, device = need_torch(), log.device
    if nseg and int(offs[-1]) > n:
        raise ValueError("offsets run past the end of log")
    if aux is not None:
        aux = uint_on_device(aux, device, "aux")
        if aux.numel() != n:
            raise TypeError("aux must be as long as log")
        new_aux = uint_on_device(new_aux, device, "new_aux")
    new_flow = uint_on_device(new_flow, device, "new_flow")
    new_ids = uint_on_device(new_ids, device, "new_ids")
    # the result's size is known here: no capacity retry
    total = int(lens.sum()) - (int(dr.sum()) if dr is not None else 0) + n_new
    out = torch.empty((total,), dtype=log.dtype, device=device)
    aux_out = torch.empty((total,), dtype=aux.dtype, device=device) if aux is not None else None
    offs_out = np.zeros(nseg + 1, dtype=np.uint64)
    has_in = nseg > 0 and int(offs[-1]) > int(offs[0])
    check(lib().qk_u32_log_update_segments_device(
        ctx.handle, lptr if has_in else None, aux.data_ptr() if aux is not None and has_in and total else None,
        ptr(offs), ptr(dr) if dr is not None else None, nseg,
        new_flow.data_ptr() if n_new else None, new_ids.data_ptr() if n_new else None,
        new_aux.data_ptr() if aux is not None and n_new else None, n_new, out.data_ptr() if total else None,
        aux_out.data_ptr() if aux is not None and total else None, total, ptr(offs_out), stream),
        "update_segments")
    return (out, offs_out) if aux is None else (out, offs_out, aux_out)


def _fresh_record(threshold: int, device):
    """The record of an empty PowerSumQuackU32, on the device: int32 [4 + t]."""
    return need_torch().from_numpy(PowerSumQuackU32(threshold)._record_i32().copy()).to(device)


@dataclass
class SenderLogStep:
    """What DeviceSenderLog.on_quacks returns, one entry per flow."""
    action: np.ndarray      # np.uint8: SND_IDLE, SND_ADVANCED, or the OR of the SND_RESET_* bits
    send_reset: np.ndarray  # bool: the reset fired (UDP [0] to the proxy, media_client.rs:272)
    reset_reason: list      # (reordered?, retx?, exceeds threshold?) per flow with reset bits, else ()
    retransmit: list        # per flow, the seqnos of the missing entries, in log order


class DeviceSenderLog:
    """QuackReceiver (receiver.py; media_client.rs:205-325) for many flows, its
    state in HBM between calls: flow g behaves exactly as a
    QuackReceiver(threshold, reset_debounce_s) given the same on_send /
    on_quack calls.  `log` / `seqnos` are CUDA int32 tensors grouped by flow
    (host CSR `offsets`), `mine` the record tensor [nflows, 4 + t];
    `last_quack_reset` (NaN: none) stays on the host.  A round is one send()
    (one pass over the log: the drain the last on_quacks left pending and the
    batch's push) and one on_quacks() (one sender step); the log never crosses
    to the host."""

    def __init__(self, threshold: int, nflows: int, reset_debounce_s: float = 0.1, device: int = 0):
        self.threshold = int(threshold)
        self.reset_debounce_s = reset_debounce_s
        self._ctx = get_context(device)          # no device: QK_E_NO_DEVICE, nothing falls back
        torch = need_torch()
        self._device = torch.device(f"cuda:{device}")
        self._fresh = _fresh_record(self.threshold, self._device)
        self.log = torch.empty((0,), dtype=torch.int32, device=self._device)
        self.seqnos = torch.empty((0,), dtype=torch.int32, device=self._device)
        self.mine = torch.empty((0, 4 + self.threshold), dtype=torch.int32, device=self._device)
        self.offsets = np.zeros(1, dtype=np.uint64)
        self.last_quack_reset = np.zeros(0, dtype=np.float64)
        self._pending = None                      # np.uint64 per flow: the drain not yet applied
        self._peer = None                         # on_wire's record tensor: the last quACK received per flow
        self.add_flows(nflows)

    @property
    def nflows(self) -> int:
        return len(self.offsets) - 1

    def add_flows(self, k: int) -> None:
        """k more flows, each with an empty log and a fresh quACK."""
        torch = need_torch()
        k = int(k)
        if k < 0:
            raise ValueError("k must not be negative")
        self.offsets = np.concatenate([self.offsets, np.full(k, self.offsets[-1], dtype=np.uint64)])
        self.mine = torch.cat([self.mine, self._fresh.unsqueeze(0).expand(k, -1)]).contiguous()
        self.last_quack_reset = np.concatenate([self.last_quack_reset, np.full(k, np.nan)])
        if self._pending is not None:
            self._pending = np.concatenate([self._pending, np.zeros(k, dtype=np.uint64)])

    def _update(self, flow, seqno, ids) -> None:
        self.log, self.offsets, self.seqnos = update_segments(
            self.log, self.offsets, self._pending, flow, ids, aux=self.seqnos, new_aux=seqno, ctx=self._ctx)
        self._pending = None

    def send(self, flow, seqno, ids) -> None:
        """on_send(seqno, id) on flow[i] for every i, in this order; applies a
        pending drain in the same pass."""
        n = uint_len(flow, "flow")
        if uint_len(seqno, "seqno") != n or uint_len(ids, "ids") != n:
            raise ValueError("flow, seqno and ids must be equally long")
        self._update(flow, seqno, ids)

    def flush(self) -> None:
        """Applies a pending drain alone."""
        if self._pending is not None and self._pending.any():
            empty = np.zeros(0, dtype=np.uint32)
            self._update(empty, empty, empty)
        self._pending = None

    def on_quacks(self, peer, present=None, now: float = 0.0) -> SenderLogStep:
        """on_quack(peer[g], now) on every flow g with present[g] (None: all):
        one sender step, the reset debounce of receiver.py:86-94 on the host."""
        torch = need_torch()
        self.flush()
        nf = self.nflows
        res = sender_step(self.mine, peer, self.log, self.offsets, present=present, ctx=self._ctx)
        self.mine = res.mine_out
        action = res.action.copy()
        drain = res.drain.copy()
        bits = (action & ~np.uint8(SND_ADVANCED)) != 0
        last = self.last_quack_reset
        with np.errstate(invalid="ignore"):
            fired = bits & (np.isnan(last) | (now > last + self.reset_debounce_s))
        if fired.any():                                                     # media_client.rs:267-276
            idx = torch.from_numpy(np.flatnonzero(fired)).to(self._device)
            self.mine[idx] = self._fresh
            lens = self.offsets[1:] - self.offsets[:-1]
            drain[fired] = lens[fired]
            last[fired] = now
        last[action == SND_ADVANCED] = np.nan                               # :280-283
        self._pending = drain if drain.any() else None
        reason = [((a & SND_RESET_REORDERED) != 0, (a & SND_RESET_RETX) != 0, (a & SND_RESET_EXCEEDS) != 0) if b else ()
                  for a, b in zip(action.tolist(), bits.tolist())]
        # the seqnos at the hit positions: the only log values that cross to the host
        counts = [len(m) for m in res.missing]
        retransmit = [[] for _ in range(nf)]
        if sum(counts):
            pos = np.concatenate([np.asarray(m, dtype=np.int64) + int(self.offsets[g])
                                  for g, m in enumerate(res.missing) if m])
            vals = self.seqnos[torch.from_numpy(pos).to(self._device)].cpu().numpy().view(np.uint32).tolist()
            at = 0
            for g, c in enumerate(counts):
                retransmit[g] = vals[at:at + c]
                at += c
        return SenderLogStep(action, fired, reason, retransmit)

    def on_quack_queue(self, queue, q_offsets, now: float = 0.0) -> SenderLogStep:
        """on_quack(q, now) on flow g for every queued quACK q of the flow, in
        queue order (sender_steps; `queue` / `q_offsets` as ingest_wire_queue
        returns them): flow g ends exactly as a QuackReceiver given them one
        after the other with this `now`.  A reset that fires clears the flow
        and drops the rest of its queue (the reference answers each of them
        with a reset the debounce holds back: nothing changes); one the
        debounce holds back is followed by a further step on the flow's
        unstepped tail, from the quACK the prefix insert left.  Per flow:
        action = its last stepped action that was not IDLE, reset_reason = its
        last reset's, retransmit = the seqnos of all its hits, in order."""
        torch = need_torch()
        nf, t = self.nflows, self.threshold
        qoffs, _ = csr(q_offsets, "the flows", nf)
        r_queue = Records.parse(queue, PowerSumQuackU32, threshold=t)
        if int(qoffs[0]) != 0 or int(qoffs[-1]) > r_queue.nseg or np.any(qoffs[1:] < qoffs[:-1]):
            raise QuackError(QK_E_INVAL, "on_quack_queue: q_offsets is no CSR index of queue")
        d_queue = (r_queue.to_device(self._ctx, "queue") if r_queue.nseg
                   else torch.empty((0, 4 + t), dtype=torch.int32, device=self._device))
        action = np.zeros(nf, dtype=np.uint8)
        fired = np.zeros(nf, dtype=bool)
        reason = [() for _ in range(nf)]
        retransmit = [[] for _ in range(nf)]
        lo, hi = qoffs[:-1].astype(np.int64), qoffs[1:].astype(np.int64)   # what is left of each flow's queue
        last = self.last_quack_reset
        whole = True
        while True:
            self.flush()            # the drain pending from before, or the previous pass's: the tails step a moved log
            k = hi - lo
            if whole:
                sub, soffs = d_queue, qoffs
            else:
                idx = np.concatenate([np.arange(a, b) for a, b in zip(lo.tolist(), hi.tolist()) if b > a])
                sub = d_queue[torch.from_numpy(idx).to(self._device)].contiguous()
                soffs = np.concatenate([[0], np.cumsum(k)]).astype(np.uint64)
            whole = False
            res = sender_steps(self.mine, sub, soffs, self.log, self.offsets, ctx=self._ctx)
            self.mine = res.mine_out
            drain = res.drain.copy()
            # the seqnos at the hit positions: the only log values that cross to the host
            counts = [len(m) for m in res.missing]
            at = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            vals = []
            if at[-1]:
                flow_of = np.repeat(np.arange(nf), k)
                pos = np.concatenate([np.asarray(m, dtype=np.int64) + int(self.offsets[flow_of[q]])
                                      for q, m in enumerate(res.missing) if m])
                vals = self.seqnos[torch.from_numpy(pos).to(self._device)].cpu().numpy().view(np.uint32).tolist()
            cleared = []
            for g in np.flatnonzero(k).tolist():
                a, s = int(soffs[g]), int(res.stepped[g])
                retransmit[g] += vals[at[a]:at[a + s]]
                lo[g] += s
                for act in res.q_action[a:a + s].tolist():
                    if act == SND_IDLE:
                        continue
                    action[g] = act
                    if act == SND_ADVANCED:
                        last[g] = np.nan                                            # :280-283
                        continue
                    reason[g] = ((act & SND_RESET_REORDERED) != 0, (act & SND_RESET_RETX) != 0,
                                 (act & SND_RESET_EXCEEDS) != 0)
                    if np.isnan(last[g]) or now > last[g] + self.reset_debounce_s:  # :267-276
                        fired[g] = True
                        last[g] = now
                        drain[g] = self.offsets[g + 1] - self.offsets[g]
                        lo[g] = hi[g]
                        cleared.append(g)
            if cleared:
                self.mine[torch.from_numpy(np.asarray(cleared, dtype=np.int64)).to(self._device)] = self._fresh
            self._pending = drain if drain.any() else None
            if not np.any(hi > lo):
                break
        return SenderLogStep(action, fired, reason, retransmit)

    def on_wire(self, wire, lens, flow, now: float = 0.0, every: bool = False):
        """A batch of received datagrams (ingest_wire: image i in row i of the
        CUDA uint8 tensor `wire`, lens[i] bytes, of flow flow[i]) through
        on_quacks: the newest accepted quACK of every flow is stepped, no
        per-flow host work in between.  every=True: through ingest_wire_queue
        and on_quack_queue instead, every accepted quACK of a flow stepped in
        arrival order.  Returns (SenderLogStep, status), status as the ingest
        gives it."""
        nf = self.nflows
        if every:
            queue, q_offsets, status, _ = ingest_wire_queue(wire, lens, flow, nf, self.threshold, ctx=self._ctx)
            return self.on_quack_queue(queue, q_offsets, now=now), status
        if self._peer is None or self._peer.shape[0] != nf:
            old = self._peer
            self._peer = self._fresh.unsqueeze(0).expand(nf, -1).contiguous()
            if old is not None:
                self._peer[:min(nf, old.shape[0])] = old[:nf]
        _, present, status, _ = ingest_wire(wire, lens, flow, nf, self.threshold, peer=self._peer, ctx=self._ctx)
        return self.on_quacks(self._peer, present=present, now=now), status


@dataclass
class Snapshots:
    """What snapshot_segments returns: the m snapshots ordered by flow, then by position."""
    records: object      # CUDA int32 [m, 4 + t]: the quACK after each triggering packet
    seg: object          # CUDA int32 [m]: the flow (segment) of each snapshot
    pos: object          # CUDA int64 [m]: the position of its triggering packet in `ids`
    arrival: object      # CUDA int32 [m]: `arrival` at that position, or None
    offsets: np.ndarray  # host uint64 [nseg + 1]: the CSR index of the snapshots by flow
    final: object        # CUDA int32 [nseg, 4 + t]: every flow's end-of-batch quACK, or None


def snapshot_segments(base, ids, offsets, frequency_pkts: int, arrival=None, final=False,
                      ctx: Context | None = None) -> Snapshots:
    """The quACK after every packet that brings its flow's count to a multiple
    of `frequency_pkts` (sidekick_multi.rs:271-283), for a batch grouped by flow,
    on the device (qk_u32_snapshot_segments_device).  `base`: one quACK per flow
    as it was before the batch (a list of PowerSumQuackU32 of one threshold, or
    a CUDA int32 record tensor [nseg, 4 + t]); `ids`: the batch grouped by flow
    in arrival order (a CUDA u32/int32 tensor, or a host array, uploaded) with
    CSR `offsets`; `arrival`: an optional parallel array carried through to the
    snapshots.  `final`: True for every flow's end-of-batch quACK as well, or a
    record tensor [nseg, 4 + t] to write it into (not `base`)."""
    ctx = _context(ctx, base, ids)
    torch = need_torch()
    r = Records.parse(base, PowerSumQuackU32)
    device = torch.device(f"cuda:{ctx.device}")
    d_base = r.to_device(ctx, "snapshot_segments") if r.nseg else None
    t, W = r.t, 4 + r.t
    ids = uint_on_device(ids, device, "ids")
    n = ids.numel()
    offs, nseg = csr(offsets, "base", r.nseg, n)
    f = int(frequency_pkts)
    if not 0 <= f < 1 << 32:
        raise ValueError("frequency_pkts must fit a u32")
    if arrival is not None:
        arrival = uint_on_device(arrival, device, "arrival")
        if arrival.numel() != n:
            raise ValueError("arrival must be as long as ids")
    if final is True:
        final = torch.empty((nseg, W), dtype=torch.int32, device=device)
    elif final is False or final is None:
        final = None
    elif not (is_record_tensor(final, 0) and tuple(final.shape) == (nseg, W) and final.device == device):
        raise TypeError("final must be a contiguous CUDA int32 record tensor [nseg, 4 + t] on the device of ids")
    lens = offs[1:] - offs[:-1]
    # at most one snapshot per packet, and per flow one per frequency_pkts packets, one for the phase, one for the wrap
    bound = int(np.minimum(lens, lens // np.uint64(f) + np.uint64(2)).sum()) if f and not np.any(offs[1:] < offs[:-1]) else 0
    snoffs = np.zeros(nseg + 1, dtype=np.uint64)
    stream = stream_of(ids)

    def attempt(cap):
        rows = max(cap, 1)   # an empty tensor has no address, and the arrival pointers go together
        rec = torch.empty((rows, W), dtype=torch.int32, device=device)
        seg = torch.empty((rows,), dtype=torch.int32, device=device)
        pos = torch.empty((rows,), dtype=torch.int64, device=device)
        arr = torch.empty((rows,), dtype=torch.int32, device=device) if arrival is not None and n else None
        m = C.c_size_t()
        rc = lib().qk_u32_snapshot_segments_device(
            ctx.handle, d_base.data_ptr() if nseg else None, ids.data_ptr() if n else None,
            arrival.data_ptr() if arr is not None else None, ptr(offs), nseg, t, f,
            rec.data_ptr(), seg.data_ptr(), pos.data_ptr(), arr.data_ptr() if arr is not None else None, cap,
            ptr(snoffs), C.byref(m), final.data_ptr() if final is not None and nseg else None, stream)
        if arr is None and arrival is not None:
            arr = seg   # no ids: no snapshot, an empty slice of it
        return rc, m.value, (rec, seg, pos, arr, m.value)
    rec, seg, pos, arr, m = retry_capacity(attempt, bound, "snapshot_segments")
    return Snapshots(rec[:m], seg[:m], pos[:m], arr[:m] if arr is not None else None, snoffs, final)


class DeviceFlowSnapshots:
    """The proxy's flow table addressed by flow index, in HBM: the twin of
    DeviceSenderLog on the other end.  insert() takes an ungrouped batch of
    (flow, id) in arrival order and returns the datagrams
    start_sidekick_multi_frequency_pkts (sidekick_multi.rs:271-283) would have
    sent for it, in its order: one per packet that brought its flow's count to
    a multiple of frequency_pkts.  `records` (CUDA int32 [nflows, 4 + t]) is
    the table; two tensors take turns, since the snapshot call writes the
    end-of-batch table beside the one it reads."""

    def __init__(self, threshold: int, nflows: int, frequency_pkts: int, device: int = 0):
        self.threshold = int(threshold)
        self.frequency_pkts = int(frequency_pkts)
        self._ctx = get_context(device)          # no device: QK_E_NO_DEVICE, nothing falls back
        torch = need_torch()
        self._device = torch.device(f"cuda:{device}")
        self._fresh = _fresh_record(self.threshold, self._device)
        self.records = torch.empty((0, 4 + self.threshold), dtype=torch.int32, device=self._device)
        self._spare = None
        self.add_flows(nflows)

    @property
    def nflows(self) -> int:
        return self.records.shape[0]

    def add_flows(self, k: int) -> None:
        """k more flows, each with a fresh quACK."""
        k = int(k)
        if k < 0:
            raise ValueError("k must not be negative")
        self.records = need_torch().cat([self.records, self._fresh.unsqueeze(0).expand(k, -1)]).contiguous()
        self._spare = None

    def insert(self, flow, ids, stride: int | None = None):
        """sc.insert(flow[i], ids[i]) for every i, in this order.  Returns
        (flow_of_image, wire, lens, records): CUDA tensors, datagram r the
        bincode image wire[r, :lens[r]] of records[r], the quACK of flow
        flow_of_image[r] after its triggering packet, in the order the
        reference would have sent them."""
        torch = need_torch()
        n = uint_len(flow, "flow")
        if uint_len(ids, "ids") != n:
            raise ValueError("flow and ids must be equally long")
        dev, nf, t = self._device, self.nflows, self.threshold
        empty = torch.empty((0,), dtype=torch.int32, device=dev)
        # grouped stably by flow, the arrival index riding along
        grouped, goffs, garr = update_segments(empty, np.zeros(nf + 1, dtype=np.uint64), None, flow, ids, aux=empty,
                                               new_aux=torch.arange(n, dtype=torch.int32, device=dev), ctx=self._ctx)
        if self._spare is None:
            self._spare = torch.empty_like(self.records)
        s = snapshot_segments(self.records, grouped, goffs, self.frequency_pkts, arrival=garr, final=self._spare,
                              ctx=self._ctx)
        self.records, self._spare = self._spare, self.records
        stride = wire_max(t) if stride is None else int(stride)
        if s.records.shape[0] == 0:
            return (s.seg, torch.empty((0, stride), dtype=torch.uint8, device=dev), s.seg.clone(), s.records)
        order = torch.argsort(s.arrival.to(torch.int64) & 0xFFFFFFFF)
        recs = s.records[order].contiguous()
        _, _, wire, lens = emit_wire(None, recs, stride=stride, ctx=self._ctx)
        return s.seg[order], wire, lens, recs


def encode_flows(bufs, threshold: int, stride: int = 67, meta=None, my_addr=None, ctx: Context | None = None,
                 device_out: bool = False, cap: int = 1024):
    """One SidekickMulti batch (sidekick_multi.rs:65-90,101-143) without the
    table merge: returns (keys, sketches, stats) for the batch's flows in
    ascending AddrKey order.  device_out=False: keys is a list of 12-byte
    AddrKeys and sketches a list of PowerSumQuackU32.  device_out=True: both
    stay in HBM as CUDA tensors (uint8 [nf, 12] and int32 [nf, 4 + t], the
    qk_u32 records), written in place by the finalize kernel.  `cap` is the
    flow count the outputs are first sized for (a batch of more flows runs a
    second time with the size the first run reports)."""
    n, dev, mptr = packet_batch(bufs, stride, meta)
    ctx = ctx or get_context(dev)
    torch = need_torch()
    addr = (C.c_uint8 * 6)(*my_addr) if my_addr is not None else None
    rec = lib().qk_u32_size(threshold)
    stream = stream_of(bufs)

    def attempt(cap):
        nf, st = C.c_size_t(), PktStats()
        if device_out:
            keys = torch.empty((cap, 12), dtype=torch.uint8, device=bufs.device)
            sk = torch.empty((cap, rec // 4), dtype=torch.int32, device=bufs.device)
            kp, sp = keys.data_ptr(), sk.data_ptr()
        else:
            keys = (FlowKey * cap)()
            sk = C.create_string_buffer(cap * rec)
            kp, sp = keys, sk
        rc = lib().qk_u32_encode_flows_device(ctx.handle, bufs.data_ptr(), n, stride, mptr, addr, threshold, kp, sp,
                                              cap, C.byref(nf), C.byref(st), stream)
        return rc, nf.value, (keys, sk, nf.value, st)
    keys, sk, m, st = retry_capacity(attempt, max(int(cap), 1), "encode_flows")
    stats = {k: getattr(st, k) for k, _ in PktStats._fields_}
    if device_out:
        return keys[:m], sk[:m], stats
    # .raw: one copy of the records (ctypes .raw copies the whole buffer per access)
    return [bytes(keys[i].addr) for i in range(m)], _quacks_from_records(sk.raw, rec, m, threshold), stats


class FlowQuacks:
    """SidekickMulti's flow table, HashMap<AddrKey, PowerSumQuackU32>
    (sidekick_multi.rs:22-37,57-90), with a GPU batch entry point.
    Keys are the 12-byte AddrKey (bytes)."""

    def __init__(self, threshold: int):
        self.threshold = int(threshold)
        self._senders: dict = {}

    # per-packet host path (sidekick_multi.rs:65-90)
    def insert(self, addr_key: bytes, sidekick_id: int) -> "PowerSumQuackU32":
        q = self._senders.get(bytes(addr_key))
        if q is None:
            q = self._senders[bytes(addr_key)] = PowerSumQuackU32(self.threshold)
        q.insert(sidekick_id)
        return q

    # SidekickMulti::reset (sidekick_multi.rs:59-63): only an existing entry is
    # reset.  The sniff loops never call it — a Reset packet replaces the whole
    # map (:205, :265), which insert_packets does.
    def reset(self, addr_key: bytes) -> None:
        if bytes(addr_key) in self._senders:
            self._senders[bytes(addr_key)] = PowerSumQuackU32(self.threshold)

    def quack(self, addr_key: bytes):
        q = self._senders.get(bytes(addr_key))
        return q.clone() if q is not None else None

    def senders(self) -> dict:
        return self._senders

    def insert_packets(self, bufs, stride: int = 67, meta=None, my_addr=None, ctx: Context | None = None) -> dict:
        """Batch of captured records (CUDA uint8 tensor) through the GPU:
        extract, group by AddrKey, encode per flow, merge into the table."""
        keys, quacks, stats = encode_flows(bufs, self.threshold, stride, meta, my_addr, ctx)
        if stats["resets"]:
            # a Reset wipes every flow (`senders = HashMap::new()`,
            # sidekick_multi.rs:205,265); the batch output is what follows it
            self._senders = {}
        for key, q in zip(keys, quacks):
            old = self._senders.get(key)
            if old is None:
                self._senders[key] = q
            else:
                old.merge(q)
        return stats


# --------------------------------------------------------------------------
# The flow table in HBM: key-sorted flow arrays and the three device calls
# --------------------------------------------------------------------------
def _flow_array(keys, sk, what: str):
    """(n, threshold) of a flow array: `keys` a CUDA uint8 tensor [n, 12], `sk` a
    CUDA int32 tensor [n, 4 + t] of qk_u32 records, both contiguous, as
    encode_flows(device_out=True) returns them."""
    torch = need_torch()
    ok = (is_record_tensor(sk) and isinstance(keys, torch.Tensor) and keys.is_cuda and keys.dtype == torch.uint8
          and keys.dim() == 2 and keys.shape[1] == 12 and keys.shape[0] == sk.shape[0] and keys.is_contiguous())
    if not ok:
        raise TypeError(f"{what}: a flow array is a contiguous CUDA uint8 [n, 12] key tensor and a contiguous CUDA "
                        "int32 [n, 4 + t] record tensor of the same n")
    return keys.shape[0], sk.shape[1] - 4


def _flow_pair(keys_a, sk_a, keys_b, sk_b):
    na, t = _flow_array(keys_a, sk_a, "a")
    nb, tb = _flow_array(keys_b, sk_b, "b")
    if t != tb:
        raise QuackError(QK_E_MISMATCH, "flow arrays of different thresholds")
    if keys_b.device != keys_a.device:
        raise ValueError("flow arrays on different devices")
    return na, nb, t


def _flows_merge_into(ctx, ka, sa, na, kb, sb, nb, t, frequency, ko, so, do) -> int:
    """qk_u32_flows_merge_device of flow arrays a (na rows) and b (nb rows, the
    later stream) into the tensors ko / so / do; returns the union's row count."""
    n = C.c_size_t()
    check(lib().qk_u32_flows_merge_device(ctx.handle, ka.data_ptr(), sa.data_ptr(), na, kb.data_ptr(), sb.data_ptr(),
                                          nb, t, int(frequency), ko.data_ptr(), so.data_ptr(), do.data_ptr(),
                                          ko.shape[0], C.byref(n), stream_of(ko)), "flows_merge")
    return n.value


def flows_merge(keys_a, sk_a, keys_b, sk_b, frequency_pkts: int = 0, ctx: Context | None = None):
    """table ∪ batch on the device (qk_u32_flows_merge_device; the per-flow
    insert of sidekick_multi.rs:65-90 for a whole encoded batch): a and b are
    flow arrays as encode_flows(device_out=True) returns them, b the later
    stream.  Returns (keys, sketches, due): the union in ascending key order
    and a uint8 tensor flagging the flows whose count crossed a multiple of
    frequency_pkts during b (all 0 when it is 0).  The outputs are views of
    na + nb freshly allocated rows, so the call never retries."""
    ctx = _context(ctx, keys_a, keys_b)
    na, nb, t = _flow_pair(keys_a, sk_a, keys_b, sk_b)
    torch = need_torch()
    cap = na + nb
    keys = torch.empty((cap, 12), dtype=torch.uint8, device=keys_a.device)
    sk = torch.empty((cap, 4 + t), dtype=torch.int32, device=keys_a.device)
    due = torch.empty((cap,), dtype=torch.uint8, device=keys_a.device)
    n = _flows_merge_into(ctx, keys_a, sk_a, na, keys_b, sk_b, nb, t, frequency_pkts, keys, sk, due)
    return keys[:n], sk[:n], due[:n]


def flows_diff(keys_a, sk_a, keys_b, sk_b, ctx: Context | None = None):
    """media_client.rs:295-296 for every flow of a (mine) against b (the
    peer's quACKs) on the device (qk_u32_flows_diff_device).  Returns (diffs,
    n_matched): diffs is the CUDA int32 record tensor [na, 4 + t] in a's key
    order — a[i] minus its b record where the key is in b, a[i] itself
    otherwise — which decode_segments accepts unchanged."""
    ctx = _context(ctx, keys_a, keys_b)
    na, nb, t = _flow_pair(keys_a, sk_a, keys_b, sk_b)
    torch = need_torch()
    out = torch.empty((na, 4 + t), dtype=torch.int32, device=keys_a.device)
    m = C.c_size_t()
    check(lib().qk_u32_flows_diff_device(ctx.handle, keys_a.data_ptr(), sk_a.data_ptr(), na, keys_b.data_ptr(),
                                         sk_b.data_ptr(), nb, t, out.data_ptr(), C.byref(m), stream_of(keys_a)),
          "flows_diff")
    return out, m.value


def flows_lookup(keys, sk, query, ctx: Context | None = None) -> list:
    """SidekickMulti::quack(&addr_key) (sidekick_multi.rs:92-94) for a list of
    12-byte AddrKeys against a flow array (qk_u32_flows_lookup_device): one
    PowerSumQuackU32 per queried key, None where the table has no such flow.
    Any order, repeats allowed."""
    ctx = _context(ctx, keys)
    n, t = _flow_array(keys, sk, "table")
    query = [bytes(k) for k in query]
    if any(len(k) != 12 for k in query):
        raise ValueError("an AddrKey is 12 bytes")
    nk = len(query)
    if nk == 0:
        return []
    rec = lib().qk_u32_size(t)
    hk = C.create_string_buffer(b"".join(query), nk * 12)
    out = C.create_string_buffer(nk * rec)
    found = C.create_string_buffer(nk)
    check(lib().qk_u32_flows_lookup_device(ctx.handle, keys.data_ptr(), sk.data_ptr(), n, t, hk, nk, out, found,
                                           stream_of(keys)), "flows_lookup")
    raw, f = out.raw, found.raw
    return [PowerSumQuackU32._from_record(raw[i * rec:(i + 1) * rec], t) if f[i] else None for i in range(nk)]


def wire_max(threshold: int) -> int:
    """The longest bincode image of a PowerSumQuackU32 of this threshold
    (qk_u32_wire_max: 4 * threshold + 17 bytes)."""
    return int(lib().qk_u32_wire_max(int(threshold)))


def emit_wire(keys, sketches, select=None, stride: int | None = None, ctx: Context | None = None):
    """bincode::serialize(&quack) for the selected flows of a flow array on the
    device (qk_u32_flows_emit_device; the per-flow send of
    sidekick_multi.rs:274-283).  `keys` / `sketches`: a flow array as
    encode_flows(device_out=True) returns it (`keys` may be None: no keys come
    back); `select`: a CUDA uint8/bool tensor of n flags, e.g. the `due` flags
    of flows_merge, or None for every flow; `stride`: bytes between images
    (default wire_max(t), the dense packing).  Returns (keys_out, rows, wire,
    lens) as CUDA tensors, the m selected flows in array order: uint8 [m, 12]
    (or None), int32 [m] row indices, uint8 [m, stride] images, int32 [m]
    image lengths.  Image r is wire[r, :lens[r]], byte-equal to
    sketches[rows[r]].serialize()."""
    ctx = _context(ctx, sketches, keys)
    torch = need_torch()
    if keys is None:
        if not is_record_tensor(sketches):
            raise TypeError("sketches must be a contiguous CUDA int32 [n, 4 + t] record tensor")
        n, t = sketches.shape[0], sketches.shape[1] - 4
    else:
        n, t = _flow_array(keys, sketches, "table")
    stride = wire_max(t) if stride is None else int(stride)
    if stride < wire_max(t):
        raise QuackError(QK_E_INVAL, "emit_wire: stride below wire_max(threshold)")
    if select is not None:
        if not (isinstance(select, torch.Tensor) and select.is_cuda and select.dtype in (torch.uint8, torch.bool)
                and select.is_contiguous() and select.numel() == n):
            raise TypeError("select must be a contiguous CUDA uint8/bool tensor of one flag per flow")
    device = sketches.device
    keys_out = torch.empty((n, 12), dtype=torch.uint8, device=device) if keys is not None else None
    rows = torch.empty((n,), dtype=torch.int32, device=device)
    wire = torch.empty((n, stride), dtype=torch.uint8, device=device)
    lens = torch.empty((n,), dtype=torch.int32, device=device)
    m = C.c_size_t()
    check(lib().qk_u32_flows_emit_device(
        ctx.handle, keys.data_ptr() if keys is not None and n else None, sketches.data_ptr() if n else None, n, t,
        select.data_ptr() if select is not None and n else None, stride,
        keys_out.data_ptr() if keys_out is not None and n else None, rows.data_ptr() if n else None,
        wire.data_ptr() if n else None, lens.data_ptr() if n else None, n, C.byref(m), stream_of(sketches)),
        "emit_wire")
    m = m.value
    return (keys_out[:m] if keys_out is not None else None), rows[:m], wire[:m], lens[:m]


def ingest_wire(wire, lens, flow, nflows: int, threshold: int, peer=None, ctx: Context | None = None):
    """bincode::deserialize per received datagram (media_client.rs:226-227) for a
    batch, placed by flow on the device (qk_u32_wire_ingest_device).  `wire`: a
    contiguous CUDA uint8 tensor [n, stride], datagram i in row i; `lens` its
    received lengths and `flow` its flow indices (CUDA int32 tensors, or host
    arrays, uploaded).  Returns (peer, present, status, n_accepted): `peer` the
    CUDA int32 record tensor [nflows, 4 + t] (the one passed in, else a fresh
    one of empty quACKs) with the newest accepted image of every flow in its
    row, `present` the CUDA uint8 flags of the flows that got one — both as
    sender_step takes them — and `status` a host int32 array: QK_OK for a
    winner, QK_WIRE_SUPERSEDED for an accepted image a later one of the same
    flow replaced, else what deserialize returns for it."""
    ctx = _context(ctx, wire, peer)
    torch = need_torch()
    nflows, t = int(nflows), int(threshold)
    if not (isinstance(wire, torch.Tensor) and wire.is_cuda and wire.dtype == torch.uint8 and wire.dim() == 2
            and wire.is_contiguous()):
        raise TypeError("wire must be a contiguous CUDA uint8 tensor [n, stride]")
    n, stride = wire.shape
    device = wire.device
    if uint_len(lens, "lens") != n or uint_len(flow, "flow") != n:
        raise ValueError("lens and flow must hold one entry per datagram")
    lens = uint_on_device(lens, device, "lens")
    flow = uint_on_device(flow, device, "flow")
    if peer is None:
        peer = _fresh_record(t, device).unsqueeze(0).expand(nflows, -1).contiguous()
    elif not (is_record_tensor(peer, 0) and tuple(peer.shape) == (nflows, 4 + t) and peer.device == device):
        raise TypeError("peer must be a contiguous CUDA int32 record tensor [nflows, 4 + t] on wire's device")
    present = torch.empty((nflows,), dtype=torch.uint8, device=device)
    status = np.zeros(max(n, 1), dtype=np.int32)
    acc = C.c_size_t()
    check(lib().qk_u32_wire_ingest_device(
        ctx.handle, wire.data_ptr() if n else None, max(int(stride), 1), lens.data_ptr() if n else None,
        flow.data_ptr() if n else None, n, t, nflows, peer.data_ptr() if nflows else None,
        present.data_ptr() if nflows else None, ptr(status), C.byref(acc), stream_of(wire)), "ingest_wire")
    return peer, present, status[:n], acc.value


def ingest_wire_queue(wire, lens, flow, nflows: int, threshold: int, ctx: Context | None = None):
    """ingest_wire with nothing superseded (qk_u32_wire_ingest_queue_device):
    every accepted datagram becomes a record of the queue, grouped by flow and,
    within a flow, in arrival order.  Arguments as ingest_wire's.  Returns
    (queue, q_offsets, status, n_accepted): the CUDA int32 record tensor
    [n_accepted, 4 + t], its CSR index by flow (np.uint64 [nflows + 1]) — both
    as sender_steps takes them — and `status` as ingest_wire gives it, without
    QK_WIRE_SUPERSEDED."""
    ctx = _context(ctx, wire)
    torch = need_torch()
    nflows, t = int(nflows), int(threshold)
    if not (isinstance(wire, torch.Tensor) and wire.is_cuda and wire.dtype == torch.uint8 and wire.dim() == 2
            and wire.is_contiguous()):
        raise TypeError("wire must be a contiguous CUDA uint8 tensor [n, stride]")
    n, stride = wire.shape
    device = wire.device
    if uint_len(lens, "lens") != n or uint_len(flow, "flow") != n:
        raise ValueError("lens and flow must hold one entry per datagram")
    lens = uint_on_device(lens, device, "lens")
    flow = uint_on_device(flow, device, "flow")
    q_offsets = np.zeros(nflows + 1, dtype=np.uint64)
    status = np.zeros(max(n, 1), dtype=np.int32)

    def attempt(cap):
        queue = torch.empty((cap, 4 + t), dtype=torch.int32, device=device)
        acc = C.c_size_t()
        rc = lib().qk_u32_wire_ingest_queue_device(
            ctx.handle, wire.data_ptr() if n else None, max(int(stride), 1), lens.data_ptr() if n else None,
            flow.data_ptr() if n else None, n, t, nflows, queue.data_ptr() if cap else None, cap, ptr(q_offsets),
            ptr(status), C.byref(acc), stream_of(wire))
        return rc, acc.value, (queue, acc.value)
    queue, m = retry_capacity(attempt, n, "ingest_wire_queue")   # every datagram accepted: n records
    return queue[:m], q_offsets, status[:n], m


@dataclass
class FlowSnapshots:
    """What snapshot_flows returns: the m quACKs the proxy loop sends for a
    batch of captures, in send order, and the flow table after the batch."""
    records: object          # CUDA int32 [m, 4 + t]: the quACK after each emitting packet
    keys: object             # CUDA uint8 [m, 12]: its flow's AddrKey
    index: object            # CUDA int32 [m]: the packet's index in the batch, ascending
    table_keys: object       # CUDA uint8 [nt, 12]: the table after the last packet, keys ascending
    table_sketches: object   # CUDA int32 [nt, 4 + t]
    stats: dict              # qk_pkt_stats, as encode_flows gives them


def snapshot_flows(bufs, threshold: int, frequency_pkts: int, keys=None, sketches=None, stride: int = 67, meta=None,
                   my_addr=None, ctx: Context | None = None, table_out=None, snap_cap: int | None = None
                   ) -> FlowSnapshots:
    """start_sidekick_multi_frequency_pkts over a batch of captured records
    (sidekick_multi.rs:240-287) on the device (qk_u32_snapshot_flows_device):
    every packet is filtered and keyed as encode_flows does, an Insert goes into
    its flow's quACK of the table `keys` / `sketches` (a flow array as
    encode_flows(device_out=True) returns it; None: an empty table), a Reset
    empties the table, and every packet that brings its flow's count to a
    multiple of `frequency_pkts` emits that quACK.  Returns the emitted quACKs
    in the reference's send order (Resets inside the batch honoured: those sent
    before one are included) and the table after the last packet.
    `table_out`: a (keys, sketches) pair of tensors to write the table into
    (DeviceFlowQuacks' spare buffer) when they hold enough rows; `snap_cap`: the
    snapshot rows first allocated (a batch of more runs a second time with the
    sizes the first run reports)."""
    ctx = _context(ctx, bufs, sketches)
    n, dev, mptr = packet_batch(bufs, stride, meta)
    torch = need_torch()
    t, f = int(threshold), int(frequency_pkts)
    if not 0 <= f < 1 << 32:
        raise ValueError("frequency_pkts must fit a u32")
    nt = 0
    if keys is not None or sketches is not None:
        nt, tt = _flow_array(keys, sketches, "table")
        if tt != t:
            raise QuackError(QK_E_MISMATCH, "snapshot_flows: the table's threshold differs")
    device, W = bufs.device, 4 + t
    addr = (C.c_uint8 * 6)(*my_addr) if my_addr is not None else None
    stream = stream_of(bufs)
    # one snapshot per frequency_pkts packets and one per flow for its phase, if every packet were an Insert
    if snap_cap is None:
        snap_cap = min(n, n // max(f, 1) + nt + 1024)

    def attempt(caps):
        tcap, scap = caps
        if table_out is not None and table_out[0].shape[0] >= tcap:
            ko, so = table_out[0], table_out[1]
            tcap = ko.shape[0]
        else:
            ko = torch.empty((max(tcap, 1), 12), dtype=torch.uint8, device=device)
            so = torch.empty((max(tcap, 1), W), dtype=torch.int32, device=device)
        rec = torch.empty((max(scap, 1), W), dtype=torch.int32, device=device)
        sk_ = torch.empty((max(scap, 1), 12), dtype=torch.uint8, device=device)
        si = torch.empty((max(scap, 1),), dtype=torch.int32, device=device)
        ntab, m, st = C.c_size_t(), C.c_size_t(), PktStats()
        rc = lib().qk_u32_snapshot_flows_device(
            ctx.handle, bufs.data_ptr() if n else None, n, stride, mptr, addr, t, f,
            keys.data_ptr() if nt else None, sketches.data_ptr() if nt else None, nt,
            ko.data_ptr(), so.data_ptr(), tcap, C.byref(ntab), rec.data_ptr(), sk_.data_ptr(), si.data_ptr(), scap,
            C.byref(m), C.byref(st), stream)
        return rc, (max(ntab.value, tcap), max(m.value, scap)), (ko, so, ntab.value, rec, sk_, si, m.value, st)
    ko, so, ntab, rec, sk_, si, m, st = retry_capacity(attempt, (nt + min(n, 1024), int(snap_cap)), "snapshot_flows")
    stats = {k: getattr(st, k) for k, _ in PktStats._fields_}
    return FlowSnapshots(rec[:m], sk_[:m], si[:m], ko[:ntab], so[:ntab], stats)


class DeviceFlowQuacks:
    """SidekickMulti's flow table (sidekick_multi.rs:36,65-90) resident in HBM:
    FlowQuacks' surface over a key-sorted flow array.  A batch goes
    encode_flows -> merge without a record crossing PCIe; `diff` feeds
    decode_segments the same way.  Two buffers, grown geometrically, take
    turns as the merge output; `.keys` / `.sketches` are views of the current
    one, valid until the next update."""

    def __init__(self, threshold: int, device: int = 0):
        self.threshold = int(threshold)
        self.device = int(device)
        self._bufs = [None, None]   # (keys, sketches, due) tensors
        self._cur = 0
        self._n = 0
        self._batch_cap = 1024

    def __len__(self) -> int:
        return self._n

    def _empty(self):
        torch = need_torch()
        dev = f"cuda:{self.device}"
        return (torch.empty((0, 12), dtype=torch.uint8, device=dev),
                torch.empty((0, 4 + self.threshold), dtype=torch.int32, device=dev))

    @property
    def keys(self):
        return self._bufs[self._cur][0][:self._n] if self._n else self._empty()[0]

    @property
    def sketches(self):
        return self._bufs[self._cur][1][:self._n] if self._n else self._empty()[1]

    def clear(self) -> None:
        """`senders = HashMap::new()` (sidekick_multi.rs:205,265)."""
        self._n = 0

    def merge(self, keys, sketches, frequency_pkts: int = 0, ctx: Context | None = None):
        """Merge a flow array (the later stream) into the table; returns the
        `due` flags of the new table (a view, valid until the next update)."""
        ctx = ctx or get_context(self.device)
        nb, t = _flow_array(keys, sketches, "batch")
        if t != self.threshold:
            raise QuackError(QK_E_MISMATCH, "batch threshold differs from the table's")
        ka, sa = self.keys, self.sketches
        need, o = self._n + nb, 1 - self._cur
        if self._bufs[o] is None or self._bufs[o][0].shape[0] < need:
            rows = max(need, 1024, 2 * (self._bufs[o][0].shape[0] if self._bufs[o] is not None else 0))
            torch, dev = need_torch(), f"cuda:{self.device}"
            self._bufs[o] = (torch.empty((rows, 12), dtype=torch.uint8, device=dev),
                             torch.empty((rows, 4 + t), dtype=torch.int32, device=dev),
                             torch.empty((rows,), dtype=torch.uint8, device=dev))
        ko, so, do = self._bufs[o]
        n = _flows_merge_into(ctx, ka, sa, self._n, keys, sketches, nb, t, frequency_pkts, ko, so, do)
        self._cur, self._n = o, n
        return do[:n]

    def emit(self, select=None, stride: int | None = None, ctx: Context | None = None):
        """The wire images of the selected flows of the table (emit_wire):
        (keys, rows, wire, lens) as CUDA tensors; `select` None: every flow."""
        ctx = ctx or get_context(self.device)
        return emit_wire(self.keys, self.sketches, select, stride, ctx)

    def insert_packets(self, bufs, stride: int = 67, meta=None, my_addr=None, frequency_pkts: int = 0,
                       ctx: Context | None = None, emit: bool = False, every: bool = False) -> dict:
        """Batch of captured records (CUDA uint8 tensor): extract, group by
        AddrKey and encode per flow on the device, then merge into the table
        there.  A batch with a Reset replaces the table, as FlowQuacks does.
        stats["due"] lists the AddrKeys of the flows whose count crossed a
        multiple of frequency_pkts during the batch
        (start_sidekick_multi_frequency_pkts, sidekick_multi.rs:274); the quACK
        to send for them is the end-of-batch one.  emit=True: the due flows'
        wire images are built on the device instead, stats["wire"] = the
        (keys, rows, wire, lens) of emit(select=due), and no key crosses to the
        host (stats["due"] is then left empty).
        every=True: the reference's loop itself (snapshot_flows): the table is
        updated packet by packet, Resets inside the batch included, and
        stats["wire"] = the (keys, index, wire, lens, records) of EVERY quACK
        the loop sends, in send order: one per crossing of frequency_pkts, not
        one per flow and batch (index: the emitting packet's)."""
        ctx = ctx or get_context(self.device)
        if every:
            return self._insert_packets_every(bufs, stride, meta, my_addr, frequency_pkts, ctx)
        keys, sk, stats = encode_flows(bufs, self.threshold, stride, meta, my_addr, ctx, device_out=True,
                                       cap=self._batch_cap)
        # room for the next batch's flows: a batch of more runs twice
        self._batch_cap = max(1024, keys.shape[0] + keys.shape[0] // 8)
        if stats["resets"]:
            self.clear()
        due = self.merge(keys, sk, frequency_pkts, ctx)
        stats["due"] = []
        if emit:
            stats["wire"] = self.emit(select=due, ctx=ctx)
        elif frequency_pkts:
            hit = self.keys[due.bool()].cpu().numpy()
            stats["due"] = [hit[i].tobytes() for i in range(hit.shape[0])]
        return stats

    def _insert_packets_every(self, bufs, stride, meta, my_addr, frequency_pkts, ctx) -> dict:
        o = 1 - self._cur
        spare = self._bufs[o][:2] if self._bufs[o] is not None else None
        s = snapshot_flows(bufs, self.threshold, frequency_pkts, self.keys if self._n else None,
                           self.sketches if self._n else None, stride, meta, my_addr, ctx, table_out=spare)
        n = s.table_keys.shape[0]
        if spare is None or s.table_keys.data_ptr() != spare[0].data_ptr():
            # a fresh table: room to grow, and a `due` column for merge()
            torch, dev = need_torch(), f"cuda:{self.device}"
            rows = max(n + n // 8, 1024)
            self._bufs[o] = (torch.empty((rows, 12), dtype=torch.uint8, device=dev),
                             torch.empty((rows, 4 + self.threshold), dtype=torch.int32, device=dev),
                             torch.empty((rows,), dtype=torch.uint8, device=dev))
            self._bufs[o][0][:n].copy_(s.table_keys)
            self._bufs[o][1][:n].copy_(s.table_sketches)
        self._cur, self._n = o, n
        _, _, wire, lens = emit_wire(None, s.records, ctx=ctx)
        stats = s.stats
        stats["due"] = []
        stats["wire"] = (s.keys, s.index, wire, lens, s.records)
        return stats

    def quacks(self, keys, ctx: Context | None = None) -> list:
        ctx = ctx or get_context(self.device)
        return flows_lookup(self.keys, self.sketches, keys, ctx)

    def quack(self, addr_key: bytes, ctx: Context | None = None):
        return self.quacks([addr_key], ctx)[0]

    def senders(self) -> dict:
        """The whole table in one D2H copy: {AddrKey: PowerSumQuackU32}."""
        if not self._n:
            return {}
        k = self.keys.cpu().numpy()
        raw = self.sketches.cpu().numpy().tobytes()
        quacks = _quacks_from_records(raw, 4 * (4 + self.threshold), self._n, self.threshold)
        return {k[i].tobytes(): q for i, q in enumerate(quacks)}

    def diff(self, peer, ctx: Context | None = None):
        """media_client.rs:295-296 per flow: this table minus `peer` (another
        DeviceFlowQuacks or a (keys, sketches) pair), one record per flow of
        this table in key order — what decode_segments accepts unchanged."""
        ctx = ctx or get_context(self.device)
        kb, sb = (peer.keys, peer.sketches) if isinstance(peer, DeviceFlowQuacks) else peer
        return flows_diff(self.keys, self.sketches, kb, sb, ctx)[0]


def partial_words(threshold: int, bits: int = 32) -> int:
    return int(getattr(lib(), f"qk_u{bits}_partial_words")(threshold))


def encode_device_async(ctx: Context, ids, threshold: int, partial, bits: int = 32, stream=None) -> None:
    """Enqueue encode of a CUDA id tensor into a CUDA int64 `partial` tensor
    of partial_words(threshold, bits) words (layout: include/quack_hip.h)."""
    iptr, n, _, s = _device_array(ids, bits)
    check(getattr(lib(), f"qk_u{bits}_encode_device_async")(
        ctx.handle, iptr, n, threshold, partial.data_ptr(), s if stream is None else stream), "encode_device_async")


def merge_partial(q: _PowerSumQuack, partial_host, has_last: bool, last: int) -> None:
    arr = np.ascontiguousarray(np.asarray(partial_host).astype(np.uint64))
    check(q._f("merge_partial")(q._buf, ptr(arr), int(has_last), int(last)), "merge_partial")


def fill_splitmix(ctx: Context, out, seed: int, start: int = 0, bits: int = 32, stream=None) -> None:
    """Fill a CUDA tensor with the synthetic splitmix64 id stream (device-side)."""
    optr, n, _, s = _device_array(out, bits)
    check(getattr(lib(), f"qk_fill_splitmix_u{bits}")(ctx.handle, optr, n, seed & 0xFFFFFFFFFFFFFFFF, start,
                                                        s if stream is None else stream), "fill_splitmix")
