"""Every queued quACK stepped in one call, the part that needs no GPU: the two
entry points are exported and bound, the wrappers are public, a NULL context is
rejected before anything else, with no device the wrappers raise
QK_E_NO_DEVICE (there is no CPU fallback), the model's known answer, and the
protocol property the calls exist for: a sender that steps every quACK of a
batch recovers losses that the newest quACK alone makes it reset on."""
import ctypes as C

import numpy as np
import pytest

import sidekick_amd as sk
from sidekick_amd import _lib
from sidekick_amd._lib import LIB_PATH, QK_E_INVAL, QK_E_NO_DEVICE, SIGNATURES, lib
from oracle import quack_oracle as qo
import sender_steps_model as sm

INGEST, STEPS = "qk_u32_wire_ingest_queue_device", "qk_u32_sender_steps_segments_device"


def test_symbols_exported_and_bound():
    L = C.CDLL(LIB_PATH)
    for name, nargs in ((INGEST, 14), (STEPS, 18)):
        assert hasattr(L, name)
        assert name in SIGNATURES
        assert getattr(lib(), name).restype is C.c_int
        assert len(SIGNATURES[name][1]) == nargs
    assert _lib.SND_UNSTEPPED == 16 == sm.SND_UNSTEPPED


def test_wrappers_are_public():
    from sidekick_amd import DeviceSenderLog, SenderSteps, ingest_wire_queue, sender_steps  # noqa: F401
    from sidekick_amd import quack
    assert quack.sender_steps is sender_steps and quack.ingest_wire_queue is ingest_wire_queue
    for name in ("sender_steps", "SenderSteps", "ingest_wire_queue"):
        assert name in quack.__all__
    assert callable(DeviceSenderLog.on_quack_queue)
    import inspect
    assert inspect.signature(DeviceSenderLog.on_wire).parameters["every"].default is False
    assert [f for f in SenderSteps.__dataclass_fields__] == ["mine_out", "q_action", "q_drain", "stepped", "drain",
                                                            "missing", "q_offsets"]


def test_null_context_is_invalid_before_threshold():
    steps, ingest = getattr(lib(), STEPS), getattr(lib(), INGEST)
    offs = (C.c_uint64 * 3)(0, 0, 0)
    hoffs = (C.c_uint64 * 3)()
    m = C.c_size_t()
    # threshold 0 / 2000 would be QK_E_THRESHOLD, nseg == 0 QK_OK: the NULL context wins
    for t, nseg in ((4, 2), (0, 2), (2000, 2), (4, 0)):
        assert steps(None, None, None, offs, None, offs, nseg, t, None, None, None, None, None, None, 0, hoffs,
                     C.byref(m), None) == QK_E_INVAL
        assert ingest(None, None, 1, None, None, 0, t, nseg, None, 0, hoffs, None, C.byref(m), None) == QK_E_INVAL


def test_no_device_raises_and_does_not_fall_back():
    h = C.c_void_p()
    rc = lib().qk_ctx_create(0, C.byref(h))
    if rc != QK_E_NO_DEVICE:
        assert rc == 0
        lib().qk_ctx_destroy(h)
        return                      # a device is present: the GPU tests cover the wrappers
    with pytest.raises(sk.QuackError) as e:
        sk.sender_steps([sk.PowerSumQuackU32(4)], [sk.PowerSumQuackU32(4)], [0, 1], np.array([7, 8], dtype=np.uint32),
                        [0, 2])
    assert e.value.code == QK_E_NO_DEVICE


def test_model_known_answer():
    """t = 2, log 10..15, quACKs after 11 (10 lost) and after 14 (13 lost), then a duplicate of the second."""
    t, seg = 2, [10, 11, 12, 13, 14, 15]
    q1 = sm.peer_after([], [11], t)
    q2 = sm.peer_after([], [11, 12, 14], t)
    m, actions, drains, hits, stepped, b = sm.steps_flow(qo.OracleQuack(t), [q1, q2, q2.clone()], seg, t)
    assert actions == [sm.SND_ADVANCED, sm.SND_ADVANCED, sm.SND_IDLE]
    assert drains == [2, 3, 0] and hits == [[0], [3], []] and stepped == 3 and b == 5
    assert (m.count, m.last_value, m.power_sums) == (3, 14, [11 + 12 + 14, 11 * 11 + 12 * 12 + 14 * 14])
    out = sm.steps([sm.Flow(qo.OracleQuack(t), [], []), sm.Flow(qo.OracleQuack(t), [q1, q2], seg)], t)
    assert out["hit_offsets"].tolist() == [0, 1, 2] and out["hits"].tolist() == [0, 3]
    assert out["stepped"].tolist() == [0, 2] and out["drain"].tolist() == [0, 5]


def test_model_stops_at_the_first_reset():
    t, seg = 2, [10, 11, 12, 13, 14, 15, 16, 17]
    q1 = sm.peer_after([], [13], t)              # 10, 11, 12 lost: 3 > t
    q2 = sm.peer_after([], [13, 14, 15], t)
    m, actions, drains, hits, stepped, b = sm.steps_flow(qo.OracleQuack(t), [q1, q2], seg, t)
    assert actions == [sm.SND_RESET_EXCEEDS, sm.SND_UNSTEPPED] and drains == [0, 0] and hits == [[], []]
    assert stepped == 1 and b == 0 and m.count == 4 and m.last_value == 13      # the prefix insert is kept


def test_every_quack_recovers_what_the_newest_alone_resets_on():
    sent, final = sm.case_quacks()
    assert len(sent) == 6 and len(sm.CASE_LOST) == 16 and sent[-1].count == final.count
    # at most t losses per interval
    edges = [-1] + [sm.case_ids().index(q.last_value) for q in sent]
    per = [sum(1 for p in sm.CASE_LOST if a < p <= b) for a, b in zip(edges, edges[1:])]
    assert max(per) <= sm.CASE_T and sum(per) == 16
    found, resets = sm.run_case(sent)
    assert resets == 0 and found == sm.CASE_LOST
    found, resets = sm.run_case([final])
    assert resets == 1 and found == []
    # the same through QuackReceiver, one quACK per loop turn
    sends = list(enumerate(sm.case_ids()))
    _, retx, fired, reasons = sm.receiver_run(sm.CASE_T, 0.1, sends, sent, 1.0)
    assert retx == sm.CASE_LOST and fired == 0 and reasons == 0
    _, retx, fired, reasons = sm.receiver_run(sm.CASE_T, 0.1, sends, [final], 1.0)
    assert retx == [] and fired == 1
