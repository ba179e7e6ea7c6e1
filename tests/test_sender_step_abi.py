"""Batched sender step and log drain, the part that needs no GPU: both entry
points are exported and bound, the Python wrappers are public, a NULL context
is rejected before anything else, the wrappers refuse mixed thresholds and an
over-long drain themselves, and with no device they raise QK_E_NO_DEVICE (there
is no CPU fallback)."""
import ctypes as C
import os

import numpy as np
import pytest

import sidekick_amd as sk
from sidekick_amd import _lib
from sidekick_amd._lib import LIB_PATH, QK_E_INVAL, QK_E_MISMATCH, QK_E_NO_DEVICE, SIGNATURES, lib

NAMES = ("qk_u32_sender_step_segments_device", "qk_u32_log_drain_segments_device")


def test_symbols_exported_and_bound():
    L = C.CDLL(LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in SIGNATURES, name
        assert getattr(lib(), name).restype is C.c_int
    assert len(SIGNATURES["qk_u32_sender_step_segments_device"][1]) == 16
    assert len(SIGNATURES["qk_u32_log_drain_segments_device"][1]) == 11


def test_wrappers_and_constants_are_public():
    from sidekick_amd import SenderStep, drain_segments, sender_step  # noqa: F401
    from sidekick_amd import quack
    assert quack.sender_step is sender_step and quack.drain_segments is drain_segments
    assert "sender_step" in quack.__all__ and "drain_segments" in quack.__all__
    assert (_lib.SND_IDLE, _lib.SND_ADVANCED, _lib.SND_RESET_REORDERED, _lib.SND_RESET_RETX,
            _lib.SND_RESET_EXCEEDS) == (0, 1, 2, 4, 8)
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "quack_hip.h")).read()
    for name, val in (("IDLE", 0), ("ADVANCED", 1), ("RESET_REORDERED", 2), ("RESET_RETX", 4), ("RESET_EXCEEDS", 8)):
        assert f"#define QK_SND_{name}" in hdr
        assert int(hdr.split(f"#define QK_SND_{name}")[1].split()[0].rstrip("u")) == val


def test_null_context_is_invalid():
    t, nseg = 8, 2
    rec = C.create_string_buffer(nseg * lib().qk_u32_size(t))
    offs = (C.c_uint64 * (nseg + 1))(0, 0, 0)
    action = (C.c_uint8 * nseg)()
    drain = (C.c_uint64 * nseg)()
    hits = (C.c_uint64 * 4)()
    hoffs = (C.c_uint64 * (nseg + 1))()
    nh = C.c_size_t()
    f = lib().qk_u32_sender_step_segments_device
    assert f(None, rec, rec, None, None, offs, nseg, t, rec, action, drain, hits, 4, hoffs, C.byref(nh),
             None) == QK_E_INVAL
    # the NULL context wins over every other argument check (threshold 0 included)
    assert f(None, None, None, None, None, None, 0, 0, None, None, None, None, 0, None, None, None) == QK_E_INVAL
    g = lib().qk_u32_log_drain_segments_device
    assert g(None, None, None, offs, drain, nseg, None, None, 0, hoffs, None) == QK_E_INVAL
    assert g(None, None, None, None, None, 0, None, None, 0, None, None) == QK_E_INVAL


def test_mixed_thresholds_are_a_mismatch():
    """Sketches of different thresholds are refused by the wrapper itself
    (QK_E_MISMATCH), within one list or between mine and peer, with or without
    a device."""
    log = np.array([1, 2], dtype=np.uint32)
    with pytest.raises(sk.QuackError) as e:
        sk.sender_step([sk.PowerSumQuackU32(8), sk.PowerSumQuackU32(9)],
                       [sk.PowerSumQuackU32(8), sk.PowerSumQuackU32(8)], log, [0, 1, 2])
    assert e.value.code == QK_E_MISMATCH


def test_drain_longer_than_segment_raises_before_any_device():
    """drain[g] > length is refused by the wrapper before it looks at the log
    (which here is not even a device tensor)."""
    with pytest.raises(sk.QuackError) as e:
        sk.drain_segments(None, [0, 3, 5], [1, 3])
    assert e.value.code == QK_E_INVAL


def test_no_device_raises_and_does_not_fall_back():
    h = C.c_void_p()
    rc = lib().qk_ctx_create(0, C.byref(h))
    if rc != QK_E_NO_DEVICE:
        assert rc == 0
        lib().qk_ctx_destroy(h)
        return                      # a device is present: the GPU tests cover the wrappers
    mine, peer = sk.PowerSumQuackU32(4), sk.PowerSumQuackU32(4)
    peer.insert(7)
    with pytest.raises(sk.QuackError) as e:
        sk.sender_step([mine], [peer], np.array([7, 8], dtype=np.uint32), [0, 2])
    assert e.value.code == QK_E_NO_DEVICE
    assert _lib.QK_E_NO_DEVICE == -7
