"""The proxy loop on captured packets (qk_u32_snapshot_flows_device), the part
that needs no GPU: the entry point is exported and bound, the wrappers are
public, a NULL context is rejected before anything else, with no device the
wrappers raise QK_E_NO_DEVICE (there is no CPU fallback), the model's known
answer with a Reset between two crossings of one flow, and the protocol
property from raw captures: a sender that steps every quACK the loop emits
recovers a loss that the end-of-batch table's quACK alone makes it reset on.

The last three (known answer, filter order, loss case) check the model of
packet_snapshot_model.py, not the call: without a device nothing else can run.
test_gpu_packet_snapshots.py holds the device to that model, the known answer
included."""
import ctypes as C

import numpy as np
import pytest

import sidekick_amd as sk
from sidekick_amd._lib import LIB_PATH, QK_E_INVAL, QK_E_NO_DEVICE, SIGNATURES, lib
from packet_snapshot_model import make_packets, packet_loop, sent_arrays, set_reset, table_arrays
from snapshot_model import LOSS_F, LOSS_LOST, LOSS_T, loss_case_ids, run_loss_case, to_sketch

NAME = "qk_u32_snapshot_flows_device"
MY_ADDR = (10, 0, 2, 1, 0x1F, 0x90)
KEY = np.array([[10, 1, 2, 3, 0x30, 0x39, 192, 168, 0, 9, 0x11, 0x5C]], dtype=np.uint8)


def test_symbol_exported_and_bound():
    L = C.CDLL(LIB_PATH)
    assert hasattr(L, NAME)
    assert NAME in SIGNATURES
    assert getattr(lib(), NAME).restype is C.c_int
    assert len(SIGNATURES[NAME][1]) == 22


def test_wrappers_are_public():
    from sidekick_amd import DeviceFlowQuacks, FlowSnapshots, snapshot_flows  # noqa: F401
    from sidekick_amd import quack
    import inspect
    assert quack.snapshot_flows is snapshot_flows and quack.FlowSnapshots is FlowSnapshots
    for name in ("snapshot_flows", "FlowSnapshots"):
        assert name in quack.__all__
    assert [f for f in FlowSnapshots.__dataclass_fields__] == ["records", "keys", "index", "table_keys",
                                                               "table_sketches", "stats"]
    every = inspect.signature(DeviceFlowQuacks.insert_packets).parameters["every"]
    assert every.default is False


def test_null_context_is_invalid_before_every_other_check():
    f = getattr(lib(), NAME)
    nt, m = C.c_size_t(), C.c_size_t()
    # threshold 0 would be QK_E_THRESHOLD, frequency 0 and a stride of 10 QK_E_INVAL, n == 0 QK_OK: the NULL context wins
    for t, freq, n, stride in ((4, 2, 2, 67), (0, 2, 2, 67), (2000, 2, 2, 67), (4, 0, 2, 67), (4, 2, 0, 67), (4, 2, 2, 10)):
        assert f(None, None, n, stride, None, None, t, freq, None, None, 0, None, None, 0, C.byref(nt), None, None, None,
                 0, C.byref(m), None, None) == QK_E_INVAL


def test_no_device_raises_and_does_not_fall_back():
    h = C.c_void_p()
    rc = lib().qk_ctx_create(0, C.byref(h))
    if rc != QK_E_NO_DEVICE:
        assert rc == 0
        lib().qk_ctx_destroy(h)
        return                      # a device is present: the GPU tests cover the wrappers
    bufs, _ = make_packets(KEY, [0, 0], [7, 8])
    with pytest.raises(sk.QuackError) as e:
        sk.snapshot_flows(bufs.reshape(-1), 4, 2)
    assert e.value.code == QK_E_NO_DEVICE
    with pytest.raises(sk.QuackError) as e:
        sk.DeviceFlowQuacks(4).insert_packets(bufs.reshape(-1), frequency_pkts=2, every=True)
    assert e.value.code == QK_E_NO_DEVICE


def test_model_known_answer_with_a_reset_between_two_crossings():
    # one key: ids 1, 2, 3, a Reset, then ids 4, 5; t = 4, f = 2
    bufs, meta = make_packets(KEY, [0] * 6, [1, 2, 3, 0, 4, 5])
    set_reset(bufs, 3, MY_ADDR)
    sent, table, stats = packet_loop({}, 4, 2, bufs, meta, MY_ADDR)
    key = KEY[0].tobytes()
    assert [(i, k, q.count, q.last_value, q.power_sums) for i, k, q in sent] == [
        (1, key, 2, 2, [3, 5, 9, 17]),
        (5, key, 2, 5, [4 + 5, 16 + 25, 64 + 125, 256 + 625])]
    # the table: that second record alone (the Reset wiped ids 1, 2, 3, which had already emitted)
    assert list(table) == [key]
    assert (table[key].count, table[key].last_value, table[key].power_sums) == (2, 5, [9, 41, 189, 881])
    assert stats == {"inserted": 2, "discarded": 3, "resets": 1, "filtered": 0, "last_reset_index": 3}
    rec, keys, index = sent_arrays(sent, 4)
    assert rec.tolist() == [[4, 2, 1, 2, 3, 5, 9, 17], [4, 2, 1, 5, 9, 41, 189, 881]]
    assert keys.tolist() == [KEY[0].tolist()] * 2 and index.tolist() == [1, 5]
    tk, tr = table_arrays(table, 4)
    assert tk.tolist() == KEY.tolist() and tr.tolist() == [[4, 2, 1, 5, 9, 41, 189, 881]]


def test_model_filters_in_the_reference_order():
    # a Reset is recognised before the length test; direction, protocol and not-UDP come before the Reset test
    bufs, meta = make_packets(KEY, [0] * 6, [1, 2, 3, 4, 5, 6])
    set_reset(bufs, 1, MY_ADDR)
    meta["len"][1] = 40                    # a short Reset still resets
    set_reset(bufs, 3, MY_ADDR)
    meta["pkttype"][3] = 4                 # an outgoing packet to my address does not
    meta["len"][4] = 40                    # a short Insert is skipped
    sent, table, stats = packet_loop({}, 4, 1, bufs, meta, MY_ADDR)
    assert [(i, q.count, q.last_value) for i, _, q in sent] == [(0, 1, 1), (2, 1, 3), (5, 2, 6)]
    assert stats == {"inserted": 2, "discarded": 1, "resets": 1, "filtered": 2, "last_reset_index": 1}
    assert len(sent) == stats["inserted"] + stats["discarded"]


def test_every_emitted_quack_recovers_what_the_end_of_batch_table_resets_on():
    ids = loss_case_ids()
    received = [int(v) for s, v in enumerate(ids.tolist()) if s not in LOSS_LOST]
    bufs, meta = make_packets(KEY, [0] * len(received), received)      # the received packets as captures, no Reset
    sent, table, stats = packet_loop({}, LOSS_T, LOSS_F, bufs, meta, MY_ADDR)
    assert stats["inserted"] == len(received) and stats["resets"] == 0 and len(sent) == 6
    retx, resets = run_loss_case([to_sketch(q) for _, _, q in sent])
    assert resets == 0 and retx == LOSS_LOST
    # the end-of-batch table's quACK alone: 16 missing > t, the sender resets and recovers nothing
    retx, resets = run_loss_case([to_sketch(table[KEY[0].tobytes()])])
    assert resets == 1 and retx == []
