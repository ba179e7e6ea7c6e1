"""Device wire leg, the part that needs no GPU: the three entry points are
exported and bound with the header's parameter counts, the wrappers are public,
qk_u32_wire_max is 4t + 17, a NULL context is rejected before every other
check, and with no device the wrappers and DeviceSenderLog raise
QK_E_NO_DEVICE (there is no CPU fallback)."""
import ctypes as C

import numpy as np
import pytest

import sidekick_amd as sk
from sidekick_amd import _lib
from sidekick_amd._lib import LIB_PATH, QK_E_INVAL, QK_E_NO_DEVICE, SIGNATURES, lib

NAMES = {"qk_u32_wire_max": 1, "qk_u32_flows_emit_device": 14, "qk_u32_wire_ingest_device": 13}


def test_symbols_exported_and_bound():
    L = C.CDLL(LIB_PATH)
    for name, nparams in NAMES.items():
        assert hasattr(L, name), name
        assert name in SIGNATURES, name
        assert len(SIGNATURES[name][1]) == nparams, name
    assert lib().qk_u32_wire_max.restype is C.c_size_t
    assert lib().qk_u32_flows_emit_device.restype is C.c_int
    assert lib().qk_u32_wire_ingest_device.restype is C.c_int
    assert _lib.QK_WIRE_SUPERSEDED == 1


def test_wrappers_are_public():
    from sidekick_amd import DeviceFlowQuacks, DeviceSenderLog, emit_wire, ingest_wire, wire_max
    from sidekick_amd import quack
    assert quack.emit_wire is emit_wire and quack.ingest_wire is ingest_wire and quack.wire_max is wire_max
    for name in ("emit_wire", "ingest_wire", "wire_max"):
        assert name in quack.__all__
    assert callable(DeviceFlowQuacks.emit) and callable(DeviceSenderLog.on_wire)
    import inspect
    assert "emit" in inspect.signature(DeviceFlowQuacks.insert_packets).parameters


@pytest.mark.parametrize("t", (1, 32, 1024))
def test_wire_max_is_the_longest_image(t):
    assert lib().qk_u32_wire_max(t) == 4 * t + 17 == sk.wire_max(t)
    q = sk.PowerSumQuackU32(t)
    q.insert(5)                       # has a last value: the longest image
    assert len(q.serialize()) == 4 * t + 17


def test_null_context_is_invalid_before_every_other_check():
    n_out = C.c_size_t(77)
    emit, ingest = lib().qk_u32_flows_emit_device, lib().qk_u32_wire_ingest_device
    # threshold 0 would be QK_E_THRESHOLD, a stride below wire_max QK_E_INVAL after it
    assert emit(None, None, None, 0, 0, None, 0, None, None, None, None, 0, C.byref(n_out), None) == QK_E_INVAL
    assert emit(None, None, None, 5, 4096, None, 1, None, None, None, None, 0, None, None) == QK_E_INVAL
    assert n_out.value == 77
    status = (C.c_int32 * 4)()
    assert ingest(None, None, 0, None, None, 0, 0, 0, None, None, status, C.byref(n_out), None) == QK_E_INVAL
    assert ingest(None, None, 64, None, None, 4, 2000, 0, None, None, status, None, None) == QK_E_INVAL
    assert n_out.value == 77


def test_no_device_raises_and_does_not_fall_back():
    h = C.c_void_p()
    rc = lib().qk_ctx_create(0, C.byref(h))
    if rc != QK_E_NO_DEVICE:
        assert rc == 0
        lib().qk_ctx_destroy(h)
        return                      # a device is present: the GPU tests cover the wrappers
    with pytest.raises(sk.QuackError) as e:
        sk.emit_wire(None, np.zeros((2, 8), dtype=np.int32))
    assert e.value.code == QK_E_NO_DEVICE
    with pytest.raises(sk.QuackError) as e:
        sk.ingest_wire(np.zeros((2, 33), dtype=np.uint8), [33, 33], [0, 1], 2, 4)
    assert e.value.code == QK_E_NO_DEVICE
    # on_wire lives on a DeviceSenderLog, and none exists without a device
    with pytest.raises(sk.QuackError) as e:
        sk.DeviceSenderLog(8, 4).on_wire(None, [], [])
    assert e.value.code == QK_E_NO_DEVICE
