"""Sender log update, the part that needs no GPU: the entry point is exported
and bound, the wrappers and DeviceSenderLog are public, a NULL context is
rejected before anything else, the wrapper refuses an over-long drain and
batches of unequal lengths itself, and with no device update_segments and
DeviceSenderLog raise QK_E_NO_DEVICE (there is no CPU fallback)."""
import ctypes as C

import numpy as np
import pytest

import sidekick_amd as sk
from sidekick_amd._lib import LIB_PATH, QK_E_INVAL, QK_E_NO_DEVICE, SIGNATURES, lib

NAME = "qk_u32_log_update_segments_device"


def test_symbol_exported_and_bound():
    L = C.CDLL(LIB_PATH)
    assert hasattr(L, NAME)
    assert NAME in SIGNATURES
    assert getattr(lib(), NAME).restype is C.c_int
    assert len(SIGNATURES[NAME][1]) == 15


def test_wrappers_are_public():
    from sidekick_amd import DeviceSenderLog, SenderLogStep, update_segments  # noqa: F401
    from sidekick_amd import quack
    assert quack.update_segments is update_segments and quack.DeviceSenderLog is DeviceSenderLog
    for name in ("update_segments", "DeviceSenderLog", "SenderLogStep"):
        assert name in quack.__all__
    for method in ("add_flows", "send", "flush", "on_quacks"):
        assert callable(getattr(DeviceSenderLog, method))


def test_null_context_is_invalid():
    nseg = 2
    offs = (C.c_uint64 * (nseg + 1))(0, 0, 0)
    drain = (C.c_uint64 * nseg)()
    offs_out = (C.c_uint64 * (nseg + 1))()
    f = getattr(lib(), NAME)
    assert f(None, None, None, offs, drain, nseg, None, None, None, 0, None, None, 0, offs_out, None) == QK_E_INVAL
    # the NULL context wins over every other argument check (nseg == 0 would be QK_OK)
    assert f(None, None, None, None, None, 0, None, None, None, 0, None, None, 0, None, None) == QK_E_INVAL


def test_drain_longer_than_segment_raises_before_any_device():
    """drain[g] > length is refused by the wrapper before it looks at the log
    (which here is not even a device tensor)."""
    with pytest.raises(sk.QuackError) as e:
        sk.update_segments(None, [0, 3, 5], [1, 3], [0], [7])
    assert e.value.code == QK_E_INVAL
    with pytest.raises(sk.QuackError) as e:
        sk.update_segments(None, [0, 3, 2], None, [0], [7])       # decreasing offsets
    assert e.value.code == QK_E_INVAL


def test_unequal_batch_lengths_raise_before_any_device():
    with pytest.raises(ValueError, match="equally long"):
        sk.update_segments(None, [0, 3, 5], [1, 2], [0, 1], [7])
    with pytest.raises(ValueError, match="equally long"):
        sk.update_segments(None, [0, 3, 5], [1, 2], [0, 1], [7, 8], aux=[0] * 5, new_aux=[1])
    with pytest.raises(ValueError, match="go together"):
        sk.update_segments(None, [0, 3, 5], [1, 2], [0, 1], [7, 8], new_aux=[1, 2])


def test_no_device_raises_and_does_not_fall_back():
    h = C.c_void_p()
    rc = lib().qk_ctx_create(0, C.byref(h))
    if rc != QK_E_NO_DEVICE:
        assert rc == 0
        lib().qk_ctx_destroy(h)
        return                      # a device is present: the GPU tests cover the wrappers
    log = np.array([7, 8], dtype=np.uint32)
    with pytest.raises(sk.QuackError) as e:
        sk.update_segments(log, [0, 2], [1], [0], [9])
    assert e.value.code == QK_E_NO_DEVICE
    with pytest.raises(sk.QuackError) as e:
        sk.DeviceSenderLog(8, 4)
    assert e.value.code == QK_E_NO_DEVICE
