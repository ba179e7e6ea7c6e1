"""Device-resident flow table, the part that needs no GPU: the three entry
points are exported and bound, the Python surface is public, a NULL context is
rejected before anything touches the device, and with no device the wrappers
raise QK_E_NO_DEVICE (there is no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sidekick_amd as sk
from sidekick_amd import _lib
from sidekick_amd._lib import LIB_PATH, QK_E_INVAL, QK_E_NO_DEVICE, SIGNATURES, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {"qk_u32_flows_merge_device": 15, "qk_u32_flows_diff_device": 11, "qk_u32_flows_lookup_device": 10}


def test_symbols_exported_and_bound():
    L = C.CDLL(LIB_PATH)
    for name, nparams in PARAMS.items():
        assert hasattr(L, name), name
        assert name in SIGNATURES, name
        assert getattr(lib(), name).restype is C.c_int
        assert SIGNATURES[name][0] is C.c_int
        assert len(SIGNATURES[name][1]) == nparams, name


def test_join_tile_constant_matches_header():
    hdr = open(os.path.join(ROOT, "include", "quack_hip.h")).read()
    assert int(re.search(r"#define QK_FLOW_JOIN_TILE (\d+)u", hdr).group(1)) == _lib.FLOW_JOIN_TILE == 2048


def test_wrappers_are_public():
    from sidekick_amd import DeviceFlowQuacks, flows_diff, flows_lookup, flows_merge  # noqa: F401
    from sidekick_amd import quack
    for name in ("flows_merge", "flows_diff", "flows_lookup", "DeviceFlowQuacks"):
        assert getattr(quack, name) is getattr(sk, name), name
        assert name in quack.__all__, name
    for meth in ("insert_packets", "merge", "quack", "quacks", "senders", "diff", "__len__", "keys", "sketches"):
        assert hasattr(sk.DeviceFlowQuacks, meth), meth
    assert "FlowQuacks" in quack.__all__ and sk.FlowQuacks is quack.FlowQuacks


def test_null_context_is_invalid():
    t, n = 8, 2
    rec = lib().qk_u32_size(t)
    keys = C.create_string_buffer(n * 12)
    sks = C.create_string_buffer(n * rec)
    out_k = C.create_string_buffer(2 * n * 12)
    out_s = C.create_string_buffer(2 * n * rec)
    due = C.create_string_buffer(2 * n)
    found = C.create_string_buffer(n)
    cnt = C.c_size_t(77)
    assert lib().qk_u32_flows_merge_device(None, keys, sks, n, keys, sks, n, t, 0, out_k, out_s, due, 2 * n,
                                           C.byref(cnt), None) == QK_E_INVAL
    assert lib().qk_u32_flows_diff_device(None, keys, sks, n, keys, sks, n, t, out_s, C.byref(cnt),
                                          None) == QK_E_INVAL
    assert lib().qk_u32_flows_lookup_device(None, keys, sks, n, t, keys, n, out_s, found, None) == QK_E_INVAL
    # the NULL context wins over every other argument check (threshold 0, NULL everywhere)
    assert lib().qk_u32_flows_merge_device(None, None, None, 0, None, None, 0, 0, 0, None, None, None, 0, None,
                                           None) == QK_E_INVAL
    assert lib().qk_u32_flows_diff_device(None, None, None, 0, None, None, 0, 0, None, None, None) == QK_E_INVAL
    assert lib().qk_u32_flows_lookup_device(None, None, None, 0, 0, None, 0, None, None, None) == QK_E_INVAL
    assert lib().qk_u32_flows_merge_device(None, None, None, 1 << 40, None, None, 1 << 40, 5000, 0, None, None, None,
                                           0, None, None) == QK_E_INVAL


def test_no_device_raises_and_does_not_fall_back():
    h = C.c_void_p()
    rc = lib().qk_ctx_create(0, C.byref(h))
    if rc != QK_E_NO_DEVICE:
        assert rc == 0
        lib().qk_ctx_destroy(h)
        return                      # a device is present: the GPU tests cover the wrappers
    import torch
    table = sk.DeviceFlowQuacks(8)
    assert len(table) == 0
    bufs = torch.zeros(2 * 67, dtype=torch.uint8)
    with pytest.raises(sk.QuackError) as e:
        table.insert_packets(bufs, stride=67, my_addr=(10, 0, 2, 1, 0x1F, 0x90))
    assert e.value.code == QK_E_NO_DEVICE
    keys = torch.zeros((1, 12), dtype=torch.uint8)
    recs = torch.from_numpy(np.array([[8, 0, 0, 0] + [0] * 8], dtype=np.int32))
    with pytest.raises(sk.QuackError) as e:
        sk.flows_merge(keys, recs, keys, recs)
    assert e.value.code == QK_E_NO_DEVICE
    with pytest.raises(sk.QuackError) as e:
        sk.flows_diff(keys, recs, keys, recs)
    assert e.value.code == QK_E_NO_DEVICE
    with pytest.raises(sk.QuackError) as e:
        sk.flows_lookup(keys, recs, [b"\x00" * 12])
    assert e.value.code == QK_E_NO_DEVICE
    with pytest.raises(sk.QuackError) as e:
        table.quack(b"\x00" * 12)
    assert e.value.code == QK_E_NO_DEVICE
