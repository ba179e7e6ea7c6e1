"""Per-flow quACK snapshots, the part that needs no GPU: the entry point is
exported and bound, the wrappers are public, a NULL context is rejected before
anything else, with no device the wrappers raise QK_E_NO_DEVICE (there is no
CPU fallback), the model's known answer, and the protocol property the call
exists for: a sender that steps every snapshot the reference would have sent
recovers a loss that the end-of-batch quACK alone makes it reset on."""
import ctypes as C

import numpy as np
import pytest

import sidekick_amd as sk
from sidekick_amd._lib import LIB_PATH, QK_E_INVAL, QK_E_NO_DEVICE, SIGNATURES, lib
from snapshot_model import (LOSS_F, LOSS_LOST, LOSS_T, base_quack, loss_case_ids, reference_loop, run_loss_case, serialize,
                            to_sketch)

NAME = "qk_u32_snapshot_segments_device"


def test_symbol_exported_and_bound():
    L = C.CDLL(LIB_PATH)
    assert hasattr(L, NAME)
    assert NAME in SIGNATURES
    assert getattr(lib(), NAME).restype is C.c_int
    assert len(SIGNATURES[NAME][1]) == 17


def test_wrappers_are_public():
    from sidekick_amd import DeviceFlowSnapshots, Snapshots, snapshot_segments  # noqa: F401
    from sidekick_amd import quack
    assert quack.snapshot_segments is snapshot_segments and quack.DeviceFlowSnapshots is DeviceFlowSnapshots
    for name in ("snapshot_segments", "Snapshots", "DeviceFlowSnapshots"):
        assert name in quack.__all__
    for method in ("add_flows", "insert"):
        assert callable(getattr(DeviceFlowSnapshots, method))
    assert [f for f in Snapshots.__dataclass_fields__] == ["records", "seg", "pos", "arrival", "offsets", "final"]


def test_null_context_is_invalid_before_threshold_and_frequency():
    f = getattr(lib(), NAME)
    offs = (C.c_uint64 * 3)(0, 0, 0)
    snoffs = (C.c_uint64 * 3)()
    m = C.c_size_t()
    # threshold 0 would be QK_E_THRESHOLD, frequency 0 QK_E_INVAL, nseg == 0 QK_OK: the NULL context wins
    for t, freq, nseg in ((4, 2, 2), (0, 2, 2), (2000, 2, 2), (4, 0, 2), (4, 2, 0)):
        assert f(None, None, None, None, offs, nseg, t, freq, None, None, None, None, 0, snoffs, C.byref(m),
                 None, None) == QK_E_INVAL


def test_no_device_raises_and_does_not_fall_back():
    h = C.c_void_p()
    rc = lib().qk_ctx_create(0, C.byref(h))
    if rc != QK_E_NO_DEVICE:
        assert rc == 0
        lib().qk_ctx_destroy(h)
        return                      # a device is present: the GPU tests cover the wrappers
    with pytest.raises(sk.QuackError) as e:
        sk.snapshot_segments([sk.PowerSumQuackU32(4)], np.array([7, 8], dtype=np.uint32), [0, 2], 2)
    assert e.value.code == QK_E_NO_DEVICE
    with pytest.raises(sk.QuackError) as e:
        sk.DeviceFlowSnapshots(8, 4, 2)
    assert e.value.code == QK_E_NO_DEVICE


def test_model_known_answer():
    sent = reference_loop({0: base_quack(4)}, [0] * 5, [1, 2, 3, 4, 5], 2)
    assert [(g, q.count, q.last_value, q.power_sums) for g, q in sent] == [
        (0, 2, 2, [3, 5, 9, 17]), (0, 4, 4, [10, 30, 100, 354])]
    # the image a snapshot goes out as: u64 threshold, the sums, the Option tag, last_value, count
    assert serialize(sent[0][1]) == (b"\x04" + b"\0" * 7 + b"".join(int(v).to_bytes(4, "little") for v in (3, 5, 9, 17))
                                     + b"\x01" + (2).to_bytes(4, "little") + (2).to_bytes(4, "little"))
    assert to_sketch(sent[1][1]).power_sums() == [10, 30, 100, 354]


def test_model_count_wrapping_to_zero_triggers():
    sent = reference_loop({0: base_quack(2, count=(1 << 32) - 3)}, [0] * 8, range(1, 9), 5)
    # counts 2^32-2, 2^32-1, 0, 1, 2, 3, 4, 5: 2^32 - 1 = 5 * 858993459 triggers, then 0, then 5
    assert [q.count for _, q in sent] == [(1 << 32) - 1, 0, 5]


def test_every_snapshot_recovers_what_the_end_of_batch_quack_resets_on():
    ids = loss_case_ids()
    received = [int(v) for s, v in enumerate(ids.tolist()) if s not in LOSS_LOST]
    table = {0: base_quack(LOSS_T)}
    sent = reference_loop(table, [0] * len(received), received, LOSS_F)
    assert len(sent) == 6
    retx, resets = run_loss_case([to_sketch(q) for _, q in sent])
    assert resets == 0 and retx == LOSS_LOST
    # the end-of-batch quACK alone: 16 missing > t, the sender resets and recovers nothing
    retx, resets = run_loss_case([to_sketch(table[0])])
    assert resets == 1 and retx == []


def test_threshold_list_covers_the_dispatch_rule():
    """The rule of snapshots.hip, restated: a threshold <= SN_KC_SMALL walks its
    item once with SN_KC_SMALL powers per pass, a larger one ceil(t / SN_KC)
    times with SN_KC; a work item is SN_ITEM positions.  A changed rule fails
    here, so that the list of the GPU test is looked at again."""
    import os
    import re
    from snapshot_model import THRESHOLDS
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sidekick_amd", "csrc")
    hdr = open(os.path.join(csrc, "snapshots.h")).read()
    hip = open(os.path.join(csrc, "snapshots.hip")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr uint32_t (SN_\w+) = (\d+);", hdr)}
    assert const == {"SN_ITEM": 2048, "SN_KC_SMALL": 32, "SN_KC": 64}
    assert len(re.findall(r"k_sn_walk<(\w+)>\)", hip)) == 2 and "if (T <= SN_KC_SMALL)" in hip
    assert "for (uint32_t k0 = 0; k0 < T; k0 += KC)" in hip
    small, kc = const["SN_KC_SMALL"], const["SN_KC"]
    for t in (1, small - 1, small, small + 1, kc, kc + 1, 2 * kc, 2 * kc + 1, 1024):
        assert t in THRESHOLDS, t
    assert any(t % 4 for t in THRESHOLDS) and max(THRESHOLDS) == 1024
