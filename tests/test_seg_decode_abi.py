"""Batched per-flow decode, the part that needs no GPU: both entry points are
exported and bound, the Python wrappers are public, a NULL context is
rejected before anything touches the device, and with no device the wrappers
raise QK_E_NO_DEVICE (there is no CPU fallback)."""
import ctypes as C

import numpy as np
import pytest

import sidekick_amd as sk
from sidekick_amd import _lib
from sidekick_amd._lib import LIB_PATH, QK_E_INVAL, QK_E_MISMATCH, QK_E_NO_DEVICE, SIGNATURES, lib

NAMES = ("qk_u32_to_coeffs_segments_device", "qk_u32_decode_segments_device")


def test_symbols_exported_and_bound():
    L = C.CDLL(LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in SIGNATURES, name
        assert getattr(lib(), name).restype is C.c_int
    assert len(SIGNATURES["qk_u32_to_coeffs_segments_device"][1]) == 8
    assert len(SIGNATURES["qk_u32_decode_segments_device"][1]) == 13


def test_wrappers_are_public():
    from sidekick_amd import decode_segments, to_coeffs_segments  # noqa: F401
    from sidekick_amd import quack
    assert quack.decode_segments is decode_segments and quack.to_coeffs_segments is to_coeffs_segments
    assert "decode_segments" in quack.__all__ and "to_coeffs_segments" in quack.__all__


def test_null_context_is_invalid():
    t, nseg = 8, 2
    rec = C.create_string_buffer(nseg * lib().qk_u32_size(t))
    coeffs = (C.c_uint32 * (nseg * t))()
    deg = (C.c_uint32 * nseg)()
    status = (C.c_int32 * nseg)()
    assert lib().qk_u32_to_coeffs_segments_device(None, rec, nseg, t, coeffs, deg, status, None) == QK_E_INVAL
    offs = (C.c_uint64 * (nseg + 1))(0, 0, 0)
    hits = (C.c_uint64 * 4)()
    hoffs = (C.c_uint64 * (nseg + 1))()
    nh = C.c_size_t()
    assert lib().qk_u32_decode_segments_device(None, rec, None, offs, nseg, t, 0, hits, 4, hoffs, status,
                                               C.byref(nh), None) == QK_E_INVAL
    # the NULL context wins over every other argument check
    assert lib().qk_u32_decode_segments_device(None, None, None, None, 0, 0, 0, None, 0, None, None, None,
                                               None) == QK_E_INVAL


def test_mixed_thresholds_are_a_mismatch():
    """A list of sketches of different thresholds is refused by the wrapper
    itself (QK_E_MISMATCH), with or without a device."""
    with pytest.raises(sk.QuackError) as e:
        sk.to_coeffs_segments([sk.PowerSumQuackU32(8), sk.PowerSumQuackU32(9)])
    assert e.value.code == QK_E_MISMATCH


def test_no_device_raises_and_does_not_fall_back():
    h = C.c_void_p()
    rc = lib().qk_ctx_create(0, C.byref(h))
    if rc != QK_E_NO_DEVICE:
        assert rc == 0
        lib().qk_ctx_destroy(h)
        return                      # a device is present: the GPU tests cover the wrappers
    q = sk.PowerSumQuackU32(4)
    q.insert(7)
    with pytest.raises(sk.QuackError) as e:
        sk.to_coeffs_segments([q])
    assert e.value.code == QK_E_NO_DEVICE
    with pytest.raises(sk.QuackError) as e:
        sk.decode_segments([q], np.array([7, 8], dtype=np.uint32), [0, 2])
    assert e.value.code == QK_E_NO_DEVICE
    assert _lib.QK_E_NO_DEVICE == -7
