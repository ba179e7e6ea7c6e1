"""The argument layer under the device calls of quack.py and dist.py: what a
wrapper does to its arguments before it calls libquack_hip.so, written once
(the lazy torch import, device index and stream of a tensor, ctypes pointers,
uploads, CSR offsets, the capacity retry, record batches, packet batches).
Nothing here loads the library or needs a device, and torch is imported on
first use: `import sidekick_amd` works without it."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import QK_E_CAPACITY, QK_E_INVAL, QK_E_MISMATCH, QuackError, check, i32p, u8p, u32p, u64p

_torch = False   # False: not tried yet; None: not installed


def torch_or_none():
    """The torch module, imported on first use; None where it is not installed."""
    global _torch
    if _torch is False:
        try:
            import torch as _torch
        except ImportError:  # pragma: no cover
            _torch = None
    return _torch


def need_torch():
    """The torch module, on a path that has no meaning without it."""
    torch = _torch or torch_or_none()
    if torch is None:  # pragma: no cover
        raise ImportError("torch is required for the device path")
    return torch


def dev_index(tensor) -> int:
    i = tensor.device.index
    return i if i is not None else need_torch().cuda.current_device()


def stream_of(tensor, dev: int | None = None):
    """The raw handle of the current stream of a CUDA tensor's device (index `dev`, if known)."""
    return (_torch or need_torch()).cuda.current_stream(dev_index(tensor) if dev is None else dev).cuda_stream


_PTR = {np.dtype(np.uint8): u8p, np.dtype(np.uint32): u32p, np.dtype(np.uint64): u64p, np.dtype(np.int32): i32p}


def ptr(a: np.ndarray):
    """The typed ctypes pointer of a contiguous numpy array (u8, u32, u64, i32)."""
    return a.ctypes.data_as(_PTR[a.dtype])


def _device_array(a, bits: int):
    """(ptr, n, device_index, stream_ptr) of a contiguous CUDA tensor, or None."""
    torch = _torch or torch_or_none()
    if torch is None or not isinstance(a, torch.Tensor):
        return None
    if not a.is_cuda:
        raise TypeError("CPU torch tensors are not accepted; pass a numpy array for the host path")
    ok = {32: (torch.int32, getattr(torch, "uint32", None)), 64: (torch.int64, getattr(torch, "uint64", None))}[bits]
    if a.dtype not in ok:
        raise TypeError(f"u{bits} ids must be a torch int{bits}/uint{bits} tensor, got {a.dtype}")
    if not a.is_contiguous():
        raise ValueError("ids tensor must be contiguous")
    dev = a.device.index   # dev_index and stream_of written out: every device call comes through here
    if dev is None:
        dev = torch.cuda.current_device()
    return a.data_ptr(), a.numel(), dev, torch.cuda.current_stream(dev).cuda_stream


def _host_array(a, bits: int) -> np.ndarray:
    dt = np.uint32 if bits == 32 else np.uint64
    arr = np.asarray(a)
    if arr.dtype.kind == "f" and not isinstance(a, np.ndarray):
        # a sequence of Python ints on both sides of 2^63 comes out of numpy as
        # float64 (53 bits); converted with the dtype given, every id is exact
        arr = np.asarray(a, dtype=dt)
    if arr.dtype != dt:
        arr = arr.astype(dt)
    return np.ascontiguousarray(arr)


def uint_len(a, what: str) -> int:
    try:
        return int(a.numel()) if hasattr(a, "numel") else len(a)
    except TypeError:
        raise TypeError(f"{what} must be a CUDA u32/int32 tensor or a host array") from None


def uint_on_device(a, device, what: str, bits: int = 32):
    """`a` as a contiguous CUDA int/uint tensor of `bits`: a CUDA tensor on
    `device` as it is, a host array uploaded there (one H2D copy)."""
    torch = need_torch()
    if isinstance(a, torch.Tensor):
        if _device_array(a, bits) is None or a.device != device:
            raise TypeError(f"{what} must be a CUDA u{bits}/int{bits} tensor on the log's device, or a host array")
        return a
    return torch.from_numpy(_host_array(a, bits).view(np.int32 if bits == 32 else np.int64)).to(device)


def csr(offsets, what: str, nseg: int | None = None, n_log: int | None = None):
    """(offs, nseg): `offsets` as a contiguous uint64 array of nseg + 1 entries.
    `nseg`: the count it must match, that of `what`; `n_log`: the length of the
    log it must stay within."""
    offs = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
    if nseg is None:
        nseg = len(offs) - 1
        if nseg < 0:
            raise ValueError("offsets must hold at least one entry")
    elif len(offs) != nseg + 1:
        raise ValueError(f"offsets must hold one entry more than {what}")
    if n_log is not None and nseg and int(offs[-1]) > n_log:
        raise ValueError("offsets run past the end of log")
    return offs, nseg


def csr_drain(offsets, drain, what: str):
    """(offs, nseg, dr, lens): csr(offsets) of a log that is drained, `drain`
    (None: nothing is) as a contiguous uint64 array of one entry per segment,
    and the segments' lengths.  Decreasing offsets or a drain longer than its
    segment are QK_E_INVAL; the caller checks the log's end once it has the log."""
    offs = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
    if len(offs) == 0:
        raise ValueError("offsets must hold at least one entry")
    lens = offs[1:] - offs[:-1]
    dr = None
    if drain is not None:
        dr = np.ascontiguousarray(np.asarray(drain, dtype=np.uint64))
        if len(dr) != len(lens):
            raise ValueError("offsets must hold one entry more than drain")
    if np.any(offs[1:] < offs[:-1]) or (dr is not None and np.any(dr > lens)):
        raise QuackError(QK_E_INVAL, f"{what}: drain[g] exceeds the segment's length")
    return offs, len(lens), dr, lens


def retry_capacity(call, cap: int, what: str):
    """call(cap) -> (rc, needed, result) until rc is not QK_E_CAPACITY, each
    further time with the capacity the library reported; then check(rc) and
    the last result.  Only the library's answer ends the loop."""
    while True:
        rc, needed, result = call(cap)
        if rc != QK_E_CAPACITY:
            check(rc, what)
            return result
        cap = needed


def split_hits(hits: np.ndarray, hit_offsets: np.ndarray, offsets: np.ndarray) -> list:
    """Segment g's hits, hits[hit_offsets[g]:hit_offsets[g + 1]] (positions in
    the whole log), as positions local to the segment, which starts at offsets[g]."""
    h = hit_offsets.tolist()
    return [(hits[a:b] - first).tolist() for a, b, first in zip(h, h[1:], offsets)]


def is_record_tensor(x, t_min: int = 1) -> bool:
    """A contiguous CUDA int32 tensor [n, 4 + t], t >= t_min: what encode_flows(device_out=True) returns."""
    torch = _torch or torch_or_none()
    return (torch is not None and isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.int32
            and x.dim() == 2 and x.shape[1] >= 4 + t_min and x.is_contiguous())


class Records:
    """A batch of qk_u32 records of one threshold, in two phases.  parse() needs
    neither library nor device: .ptr (of .keep, which owns the memory), .nseg,
    .t, and .dev, the device index of a record tensor, None for a list of
    sketches packed into host records; to_device(ctx) uploads those."""
    __slots__ = ("ptr", "nseg", "t", "dev", "keep")

    def __init__(self, ptr, nseg, t, dev, keep):
        self.ptr, self.nseg, self.t, self.dev, self.keep = ptr, nseg, t, dev, keep

    @classmethod
    def parse(cls, recs, sketch, threshold: int | None = None) -> "Records":
        """`recs`: a list of sketches of class `sketch` (PowerSumQuackU32) and one
        threshold (an empty one has none of its own: `threshold`, else 1), or a
        record tensor."""
        torch = _torch or torch_or_none()
        if torch is not None and isinstance(recs, torch.Tensor):
            if not is_record_tensor(recs):
                raise TypeError("device diffs must be a contiguous CUDA int32 tensor [nseg, 4 + t]")
            t = recs.shape[1] - 4 if threshold is None else int(threshold)
            if t != recs.shape[1] - 4:
                raise QuackError(QK_E_MISMATCH, "device diffs: record width is not 4 + threshold")
            dev = recs.device.index
            return cls(recs.data_ptr(), recs.shape[0], t, dev if dev is not None else dev_index(recs), recs)
        recs = list(recs)
        if not recs:
            return cls(None, 0, int(threshold) if threshold is not None else 1, None, None)
        t = recs[0].threshold() if threshold is None else int(threshold)
        for q in recs:
            if not isinstance(q, sketch):
                raise TypeError("diffs must be PowerSumQuackU32 sketches (the batched decode is u32 only)")
            if q.threshold() != t:
                raise QuackError(QK_E_MISMATCH, "diffs of different thresholds")
        buf = C.create_string_buffer(b"".join(q._buf.raw for q in recs))
        return cls(C.cast(buf, C.c_void_p), len(recs), t, None, buf)

    def need_threshold(self, what: str) -> None:
        if self.keep is None:
            raise ValueError(f"{what}: an empty list of sketches has no threshold; pass a record tensor")

    def to_device(self, ctx, what: str = "records"):
        """The CUDA int32 record tensor [nseg, 4 + t], host records uploaded to
        ctx's device (one H2D copy)."""
        if self.dev is not None:
            return self.keep
        self.need_threshold(what)
        host = np.frombuffer(self.keep, dtype=np.int32, count=self.nseg * (4 + self.t)).reshape(self.nseg, 4 + self.t)
        return need_torch().from_numpy(host.copy()).to(f"cuda:{ctx.device}")


def packet_batch(bufs, stride: int, meta):
    """(n, device index, meta pointer or None) of a batch of captured records:
    `bufs` a contiguous CUDA uint8 tensor of n * stride bytes, `meta` None or a
    contiguous CUDA tensor of n 8-byte qk_pkt_meta records."""
    torch = need_torch()
    if not (isinstance(bufs, torch.Tensor) and bufs.is_cuda and bufs.dtype == torch.uint8 and bufs.is_contiguous()):
        raise TypeError("bufs must be a contiguous CUDA uint8 tensor")
    n = bufs.numel() // stride
    if meta is None:
        return n, dev_index(bufs), None
    if not (meta.is_cuda and meta.is_contiguous() and meta.numel() * meta.element_size() == 8 * n):
        raise ValueError("meta must be a contiguous CUDA tensor of n 8-byte records")
    return n, dev_index(bufs), meta.data_ptr()
