"""The argument layer under the device calls (sidekick_amd/_args.py) and the
record helpers of the sketch classes, without a GPU: the capacity retry against
a stub, the CSR checks, the hit split, record <-> sketch, and the parse phase of
a record batch.  Only the record tests and the decode_host one load the library."""
import numpy as np
import pytest

import sidekick_amd as sk
from sidekick_amd._args import Records, csr, csr_drain, retry_capacity, split_hits
from sidekick_amd._lib import QK_E_CAPACITY, QK_E_INVAL, QK_E_MISMATCH, QK_E_THRESHOLD, QK_OK

U32 = sk.PowerSumQuackU32


# ------------------------------------------------------------ retry_capacity
class Stub:
    """A library call: answers[i] = (rc, needed) for the i-th call."""

    def __init__(self, *answers):
        self.answers, self.caps = list(answers), []

    def __call__(self, cap):
        self.caps.append(cap)
        rc, needed = self.answers[len(self.caps) - 1]
        return rc, needed, ("result", len(self.caps))


def test_retry_capacity_calls_again_with_the_reported_size():
    stub = Stub((QK_E_CAPACITY, 7), (QK_OK, 7))
    assert retry_capacity(stub, 2, "stub") == ("result", 2)
    assert stub.caps == [2, 7]


def test_retry_capacity_raises_another_error_after_one_call():
    stub = Stub((QK_E_THRESHOLD, 0), (QK_OK, 0))
    with pytest.raises(sk.QuackError) as e:
        retry_capacity(stub, 2, "stub")
    assert e.value.code == QK_E_THRESHOLD and stub.caps == [2]


def test_retry_capacity_success_is_one_call():
    stub = Stub((QK_OK, 1), (QK_OK, 1))
    assert retry_capacity(stub, 5, "stub") == ("result", 1)
    assert stub.caps == [5]


def test_decode_host_grows_past_the_threshold():
    """decode_host sizes its hits for `threshold` positions; a log that repeats
    a missing id holds more, and the second call takes the reported count."""
    q = sk.PowerSumQuackU32(2)
    q.insert(11)
    q.insert(12)
    log = [11, 5, 12, 11, 11, 6, 12]
    assert q.decode_host(log) == [0, 2, 3, 4, 6]


# ------------------------------------------------------------------------ csr
@pytest.mark.parametrize("offsets", ([0, 3, 5], np.array([0, 3, 5], dtype=np.int64),
                                     np.array([0, 3, 5], dtype=np.uint64),
                                     np.array([0, 9, 3, 9, 5], dtype=np.uint64)[::2]))
def test_csr_gives_contiguous_uint64_and_nseg(offsets):
    for kw in ({}, {"nseg": 2}, {"nseg": 2, "n_log": 5}):
        offs, nseg = csr(offsets, "diffs", **kw)
        assert offs.dtype == np.uint64 and offs.flags["C_CONTIGUOUS"] and offs.tolist() == [0, 3, 5]
        assert nseg == 2


def test_csr_length_and_end():
    with pytest.raises(ValueError):
        csr([0, 3, 5], "diffs", nseg=3)
    with pytest.raises(ValueError):
        csr([0, 3, 5], "diffs", nseg=1)
    with pytest.raises(ValueError):
        csr([], "ids")
    with pytest.raises(ValueError):
        csr([0, 3, 5], "diffs", nseg=2, n_log=4)
    assert csr([7], "diffs", nseg=0, n_log=0)[1] == 0      # no segment: nothing runs past the end


def test_csr_drain():
    offs, nseg, dr, lens = csr_drain([0, 3, 5], [1, 2], "drain_segments")
    assert offs.dtype == np.uint64 and offs.flags["C_CONTIGUOUS"] and offs.tolist() == [0, 3, 5] and nseg == 2
    assert dr.dtype == np.uint64 and dr.flags["C_CONTIGUOUS"] and dr.tolist() == [1, 2] and lens.tolist() == [3, 2]
    offs, nseg, dr, lens = csr_drain(np.array([0, 3, 5], dtype=np.int64), None, "update_segments")
    assert offs.dtype == np.uint64 and nseg == 2 and dr is None and lens.tolist() == [3, 2]
    with pytest.raises(ValueError):
        csr_drain([0, 3, 5], [1], "drain_segments")
    with pytest.raises(ValueError):
        csr_drain([], None, "update_segments")
    with pytest.raises(sk.QuackError) as e:
        csr_drain([0, 3, 5], [1, 3], "drain_segments")
    assert e.value.code == QK_E_INVAL
    for drain in (None, [0, 0]):
        with pytest.raises(sk.QuackError) as e:
            csr_drain([0, 3, 2], drain, "update_segments")
        assert e.value.code == QK_E_INVAL


def test_the_wrappers_check_csr_before_they_look_at_the_log():
    with pytest.raises(sk.QuackError) as e:
        sk.drain_segments(None, [0, 3, 2], [0, 0])
    assert e.value.code == QK_E_INVAL
    with pytest.raises(ValueError):
        sk.drain_segments(None, [0, 3, 5], [1])
    with pytest.raises(ValueError):
        sk.update_segments(None, [], None, [0], [7])
    with pytest.raises(TypeError):
        sk.drain_segments(None, [0, 3, 5], None)


# ----------------------------------------------------------------- split_hits
def test_split_hits_empty_segment_and_nonzero_first_offset():
    u64 = lambda v: np.array(v, dtype=np.uint64)   # noqa: E731
    assert split_hits(u64([6, 8, 11]), u64([0, 0, 2, 3]), u64([5, 5, 9, 12])) == [[], [1, 3], [2]]
    assert split_hits(np.empty(4, dtype=np.uint64), u64([0]), u64([0])) == []


# ---------------------------------------------------- _from_record / _record_i32
@pytest.mark.parametrize("t", (1, 32))
@pytest.mark.parametrize("ids", ((), (5, 0xFFFFFFFE, 77)))
def test_record_round_trip(t, ids):
    q = sk.PowerSumQuackU32(t)
    for v in ids:
        q.insert(v)
    assert (q.last_value() is None) == (not ids)
    rec = q._record_i32()
    assert rec.dtype == np.int32 and rec.shape == (4 + t,)
    assert rec.view(np.uint32)[:4].tolist() == [t, len(ids), int(bool(ids)), ids[-1] if ids else 0]
    back = sk.PowerSumQuackU32._from_record(rec.tobytes(), t)
    assert type(back) is sk.PowerSumQuackU32 and back == q and back == q.clone()
    assert back.threshold() == t and back.count() == len(ids) and back.last_value() == q.last_value()
    assert back.power_sums() == q.power_sums()
    back.insert(9)                       # its own memory
    assert back != q and q.count() == len(ids)


def test_from_record_keeps_the_class():
    q = sk.PowerSumQuackU64(3)
    q.insert(1 << 40)
    back = sk.PowerSumQuackU64._from_record(q._buf.raw, 3)
    assert type(back) is sk.PowerSumQuackU64 and back == q == q.clone()


# ------------------------------------------------------- Records: the parse phase
def test_parse_mixed_thresholds_are_a_mismatch():
    with pytest.raises(sk.QuackError) as e:
        Records.parse([sk.PowerSumQuackU32(8), sk.PowerSumQuackU32(9)], U32)
    assert e.value.code == QK_E_MISMATCH
    with pytest.raises(sk.QuackError) as e:
        Records.parse([sk.PowerSumQuackU32(8)], U32, 9)
    assert e.value.code == QK_E_MISMATCH


def test_parse_takes_u32_sketches_only():
    with pytest.raises(TypeError):
        Records.parse([sk.PowerSumQuackU32(8), sk.PowerSumQuackU64(8)], U32)
    with pytest.raises(TypeError):
        Records.parse([sk.PowerSumQuackU32(8), 5], U32)
    with pytest.raises(TypeError):
        Records.parse([sk.PowerSumQuackU32(8), sk.quack._PowerSumQuack(8)], U32)   # BITS == 32, yet no PowerSumQuackU32


def test_parse_an_empty_list():
    r = Records.parse([], U32)
    assert (r.ptr, r.nseg, r.t, r.dev, r.keep) == (None, 0, 1, None, None)
    assert Records.parse([], U32, 7).t == 7
    with pytest.raises(ValueError):
        r.need_threshold("mine")
    with pytest.raises(ValueError):
        r.to_device(None, "mine")


def test_parse_packs_the_sketches_in_order():
    qs = [sk.PowerSumQuackU32(4) for _ in range(3)]
    for i, q in enumerate(qs):
        q.insert(100 + i)
    r = Records.parse(iter(qs), U32)
    assert (r.nseg, r.t, r.dev) == (3, 4, None) and r.ptr.value
    assert r.keep.raw[:3 * 32] == b"".join(q._buf.raw for q in qs)
    r.need_threshold("mine")


# ---------------------------------------------------------------- host arrays
def test_host_array_keeps_python_ints_on_both_sides_of_2_63_exact():
    """numpy makes float64 of such a sequence (53 bits); the ids must arrive bit for bit."""
    from sidekick_amd._args import _host_array
    ids = [1, 2**63 + 5, 2**64 - 60, 3, 2**53 + 1]
    arr = _host_array(ids, 64)
    assert arr.dtype == np.uint64 and [int(v) for v in arr] == ids
    assert [int(v) for v in _host_array([7, 2**32 - 1], 32)] == [7, 2**32 - 1]
    # arrays and same-sided sequences as before
    assert _host_array(np.array([-1], dtype=np.int64), 64)[0] == 2**64 - 1
    assert _host_array(np.array([1.0, 2.0]), 64).tolist() == [1, 2]
    q = sk.PowerSumQuackU64(2)
    q.insert(2**63 + 5)
    q.insert(3)
    assert q.decode_host(ids) == [1, 3]
