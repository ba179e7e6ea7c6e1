"""Sender log update (qk_u32_log_update_segments_device, update_segments,
DeviceSenderLog) on the GPU against Python lists per flow: the kept tail of
every segment followed by the flow's new entries in send order.  aux is the
running entry index, so the order is checked even where ids repeat.  The
closed loop drives a DeviceSenderLog by send / on_quacks only and compares it
with one QuackReceiver per flow after every round."""
import ctypes as C
import random

import numpy as np
import pytest

import sidekick_amd as sk
from sidekick_amd._lib import QK_E_CAPACITY, QK_E_INVAL, SND_ADVANCED, SND_IDLE, lib
from sidekick_amd.receiver import QuackReceiver

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U64 = C.POINTER(C.c_uint64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint32)


class Case:
    """Input log (random ids, or ids from `pool`), aux = the running entry
    index, and the list model of the update."""

    def __init__(self, lens, first, drains, new_flow, seed=1, pool=None):
        rng = np.random.default_rng(seed)
        self.nseg = len(lens)
        self.offs = np.zeros(self.nseg + 1, dtype=np.uint64)
        self.offs[0] = first
        self.offs[1:] = first + np.cumsum(np.asarray(lens, dtype=np.uint64))
        n = int(self.offs[-1]) + 5
        self.new_flow = np.asarray(new_flow, dtype=np.uint32)
        k = len(self.new_flow)

        def ids(m):
            if pool is not None:
                return rng.choice(np.asarray(pool, dtype=np.uint32), size=m)
            return rng.integers(0, 1 << 32, size=m, dtype=np.uint64).astype(np.uint32)
        self.log, self.new_ids = ids(n), ids(k)
        self.aux = np.arange(n, dtype=np.uint32)
        self.new_aux = np.arange(n, n + k, dtype=np.uint32)
        self.drains = None if drains is None else np.asarray(drains, dtype=np.uint64)

    def model(self):
        """(log, aux, offsets) of the result from per-flow lists."""
        flows = [[] for _ in range(self.nseg)]
        for g in range(self.nseg):
            d = 0 if self.drains is None else int(self.drains[g])
            for p in range(int(self.offs[g]) + d, int(self.offs[g + 1])):
                flows[g].append((int(self.log[p]), int(self.aux[p])))
        for f, v, a in zip(self.new_flow.tolist(), self.new_ids.tolist(), self.new_aux.tolist()):
            flows[f].append((v, a))
        flat = [e for fl in flows for e in fl]
        offs = np.concatenate([[0], np.cumsum([len(fl) for fl in flows])]).astype(np.uint64)
        return (np.array([e[0] for e in flat], dtype=np.uint32), np.array([e[1] for e in flat], dtype=np.uint32), offs)

    def run(self, with_aux=True, device_batch=False):
        up = dev if device_batch else (lambda a: a)
        return sk.update_segments(dev(self.log), self.offs, self.drains, up(self.new_flow), up(self.new_ids),
                                  aux=dev(self.aux) if with_aux else None,
                                  new_aux=up(self.new_aux) if with_aux else None)

    def check(self, with_aux=True, device_batch=False):
        out = self.run(with_aux, device_batch)
        wlog, waux, woffs = self.model()
        assert np.array_equal(out[1], woffs)
        assert np.array_equal(host(out[0]), wlog)
        if with_aux:
            assert np.array_equal(host(out[2]), waux)
        else:
            assert len(out) == 2
        return out


# ---------------------------------------------------------------- semantics
# 7 flows: kept parts of four lengths; flow 4 is empty and receives entries,
# flow 2 has entries and receives none, flow 5 is fully drained and receives
# entries, flow 6 is empty before and after.  Odd first offsets and drains put
# dr_copy's sources and destinations at every relative alignment.
SMALL = {
    "1-2-3-5": dict(kept=(1, 2, 3, 5), drains=(1, 0, 2, 3, 0, 4, 0)),
    "2049-5-3-1": dict(kept=(2049, 5, 3, 1), drains=(3, 1, 0, 2, 0, 6, 0)),
}


def small_case(name, first, drain_none=False, pool=None):
    kept, drains = SMALL[name]["kept"], list(SMALL[name]["drains"])
    lens = [kept[g] + drains[g] for g in range(4)] + [0, drains[5], 0]
    rng = random.Random(5)
    new_flow = [rng.choice((0, 1, 3, 4, 5)) for _ in range(41)] + [4, 5, 0]
    return Case(lens, first, None if drain_none else drains, new_flow, seed=first + 2, pool=pool)


@pytest.mark.parametrize("first", (1, 3))
@pytest.mark.parametrize("with_aux", (False, True))
@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_shapes_equal_the_list_model(name, with_aux, first):
    c = small_case(name, first)
    out = c.check(with_aux)
    n = np.diff(out[1].astype(np.int64))
    assert n[6] == 0 and n[2] == SMALL[name]["kept"][2] and n[4] > 0 and n[5] > 0
    small_case(name, first, drain_none=True).check(with_aux)
    # the same id repeated across and within flows: aux tells the entries apart
    small_case(name, first, pool=(7, 7, 9)).check(with_aux, device_batch=True)


def test_empty_batch_is_byte_equal_to_drain_segments():
    lens = np.array([0, 1, 2, 5, 63, 64, 65, 2047, 2048, 2049, 4097, 7, 0, 4100, 3], dtype=np.uint64)
    rng = np.random.default_rng(12)
    mixed = np.array([rng.integers(0, n + 1) for n in lens], dtype=np.uint64)
    empty = np.zeros(0, dtype=np.uint32)
    for first in (0, 1, 3):
        for drains in (np.zeros_like(lens), lens.copy(), mixed):
            c = Case(lens, first, drains, [], seed=4)
            d_log, d_aux = dev(c.log), dev(c.aux)
            want = sk.drain_segments(d_log, c.offs, drains, aux=d_aux)
            got = sk.update_segments(d_log, c.offs, drains, empty, empty, aux=d_aux, new_aux=empty)
            assert np.array_equal(got[1], want[1])
            assert host(got[0]).tobytes() == host(want[0]).tobytes()
            assert host(got[2]).tobytes() == host(want[2]).tobytes()
            got = sk.update_segments(d_log, c.offs, drains, empty, empty)
            assert len(got) == 2 and host(got[0]).tobytes() == host(want[0]).tobytes()


# ------------------------------------------------------- the sort's tiling
N_TILES = 3 * 4096 + 5     # more than one 4096-item sub-tile, more than one chunk


@pytest.mark.parametrize("pattern", ("random", "last", "round_robin"))
@pytest.mark.parametrize("nseg", (1, 3))
def test_stable_across_sub_tiles_and_chunks(nseg, pattern):
    rng = np.random.default_rng(nseg)
    if pattern == "random":
        flow = rng.integers(0, nseg, size=N_TILES)
    elif pattern == "last":
        flow = np.full(N_TILES, nseg - 1)
    else:
        flow = np.arange(N_TILES) % nseg
    Case([3] * nseg, 1, [1] * nseg, flow, seed=nseg + 10).check(device_batch=True)


@pytest.mark.parametrize("nseg", (256, 257, 65537))
def test_digit_boundaries_of_the_flow_index(nseg):
    """One, two and three 8-bit passes; two old entries per flow, 70 000 new."""
    rng = np.random.default_rng(nseg)
    flow = rng.integers(0, nseg, size=70_000)
    must = [f for f in (0, 255, 256, nseg - 1) if f < nseg]
    at = rng.choice(len(flow), size=2 * len(must), replace=False)
    flow[at] = must + must
    c = Case([2] * nseg, 0, None, flow, seed=3)
    out = c.check(device_batch=True)
    assert set(must) <= set(flow.tolist()) and int(out[1][-1]) == 2 * nseg + 70_000


@pytest.mark.parametrize("n_new", (2047, 2048, 2049, 4097))
def test_item_split_of_the_new_part(n_new):
    """One flow takes n_new entries behind an odd-length kept part."""
    rng = np.random.default_rng(n_new)
    flow = np.concatenate([np.full(n_new, 1), np.repeat([0, 2], 25)])
    rng.shuffle(flow)
    c = Case([4, 9, 2], 1, [1, 2, 0], flow, seed=8)
    out = c.check()
    assert int(out[1][2] - out[1][1]) == 7 + n_new


# ------------------------------------------------------------------ errors
class Raw:
    """The C entry point on device tensors of a small two-flow case."""

    def __init__(self):
        self.ctx = sk.get_context(0)
        self.log = torch.arange(100, dtype=torch.int32, device="cuda")
        self.aux = torch.arange(1000, 1100, dtype=torch.int32, device="cuda")
        self.flow = dev([0, 1, 1, 0, 1, 0])
        self.ids = dev([11, 12, 13, 14, 15, 16])
        self.naux = dev([21, 22, 23, 24, 25, 26])
        self.out = torch.full((128,), -7, dtype=torch.int32, device="cuda")
        self.aout = torch.full((128,), -9, dtype=torch.int32, device="cuda")
        self.offs = np.array([0, 40, 100], dtype=np.uint64)
        self.offs_out = np.zeros(3, dtype=np.uint64)
        self.f = lib().qk_u32_log_update_segments_device

    def call(self, drain=(10, 20), cap=128, n_new=6, nseg=2, **kw):
        a = dict(log=self.log.data_ptr(), aux=None, flow=self.flow.data_ptr(), ids=self.ids.data_ptr(), naux=None,
                 out=self.out.data_ptr(), aout=None)
        a.update(kw)
        dr = None if drain is None else np.array(drain, dtype=np.uint64)
        return self.f(self.ctx.handle, a["log"], a["aux"], self.offs.ctypes.data_as(U64),
                      dr.ctypes.data_as(U64) if dr is not None else None, nseg, a["flow"], a["ids"], a["naux"], n_new,
                      a["out"], a["aout"], cap, self.offs_out.ctypes.data_as(U64), None)


def test_flow_index_out_of_range_leaves_the_output_untouched():
    r = Raw()
    r.flow = dev([0, 1, 1, 2, 1, 0])          # == nseg in the middle of the batch
    assert r.call(aux=r.aux.data_ptr(), naux=r.naux.data_ptr(), aout=r.aout.data_ptr()) == QK_E_INVAL
    torch.cuda.synchronize()
    assert bool((r.out == -7).all()) and bool((r.aout == -9).all())
    r.flow = dev([0, 1, 1, 0xFFFFFFFF, 1, 0])
    assert r.call() == QK_E_INVAL
    assert bool((r.out == -7).all())


def test_capacity_reports_the_offsets_and_a_larger_cap_succeeds():
    r = Raw()
    total = 30 + 40 + 6
    assert r.call(cap=total - 1) == QK_E_CAPACITY and r.offs_out.tolist() == [0, 33, 76]
    assert bool((r.out == -7).all())
    assert r.call(cap=total) == 0 and r.offs_out.tolist() == [0, 33, 76]
    got = host(r.out)[:total].tolist()
    assert got == list(range(10, 40)) + [11, 14, 16] + list(range(60, 100)) + [12, 13, 15]


def test_argument_errors():
    r = Raw()
    assert r.call(drain=(41, 0)) == QK_E_INVAL                                  # longer than the segment
    assert r.call(out=r.log.data_ptr() + 4 * 50) == QK_E_INVAL                  # output inside the input log
    assert r.call(out=r.ids.data_ptr()) == QK_E_INVAL                           # output over the batch
    assert r.call(aux=r.aux.data_ptr(), naux=r.naux.data_ptr(), aout=r.out.data_ptr() + 4 * 8) == QK_E_INVAL
    assert r.call(naux=r.naux.data_ptr()) == QK_E_INVAL                         # d_new_aux without d_aux_out
    assert r.call(aux=r.aux.data_ptr()) == QK_E_INVAL                           # d_aux without d_aux_out
    assert r.call(aout=r.aout.data_ptr()) == QK_E_INVAL                         # aux mode without d_aux / d_new_aux
    h = np.zeros(100, dtype=np.uint32)
    assert r.call(flow=h.ctypes.data) == QK_E_INVAL                             # host pointers
    assert r.call(ids=h.ctypes.data) == QK_E_INVAL
    assert r.call(log=h.ctypes.data) == QK_E_INVAL
    assert r.call(out=h.ctypes.data) == QK_E_INVAL
    r.offs = np.array([0, 40, 30], dtype=np.uint64)
    assert r.call(drain=None) == QK_E_INVAL                                     # decreasing offsets
    r.offs = np.array([0, 40, 100], dtype=np.uint64)
    assert r.call(n_new=1 << 32) == QK_E_INVAL
    assert r.call(nseg=1 << 32) == QK_E_INVAL
    assert bool((r.out == -7).all())
    # nseg == 0 is accepted
    r.offs_out[0] = 5
    assert r.f(r.ctx.handle, None, None, r.offs.ctypes.data_as(U64), None, 0, None, None, None, 0, None, None, 0,
               r.offs_out.ctypes.data_as(U64), None) == 0 and r.offs_out[0] == 0
    # drain == NULL: nothing is drained
    assert r.call(drain=None) == 0 and r.offs_out.tolist() == [0, 43, 106]


def test_same_shape_twice_gives_equal_bytes():
    rng = np.random.default_rng(77)
    c = Case([5, 0, 2050, 3], 1, [1, 0, 1, 3], rng.integers(0, 4, size=9000), seed=9)
    a = c.check(device_batch=True)
    b = c.check(device_batch=True)
    assert host(a[0]).tobytes() == host(b[0]).tobytes() and host(a[2]).tobytes() == host(b[2]).tobytes()
    assert np.array_equal(a[1], b[1])


# -------------------------------------------------------------- closed loop
LOOP_SEED = 0xC105ED


def closed_loop(seed, device_log):
    """64 flows, T = 16, 40 rounds of send -> lossy proxy (now and then a quACK
    whose last value the sender never logged) -> on_quacks.  Each round's
    fresh packets and the previous round's retransmissions go out shuffled
    across flows in one batch; `now` advances 0.04 s a round against a 0.1 s
    debounce.  With device_log None only the QuackReceivers run (the host model
    alone, to see what the seed exercises)."""
    t, nflow, rounds = 16, 64, 40
    rnd = random.Random(seed)
    rx = [QuackReceiver(t, reset_debounce_s=0.1, batch_min=1 << 30) for _ in range(nflow)]
    proxy = [sk.PowerSumQuackU32(t) for _ in range(nflow)]
    resend = [0] * nflow
    seq = 0
    stats = {"adv": 0, "fired": 0, "held": 0, "idle": 0, "retx": 0}
    d = device_log

    def compare_logs(where):
        log, seqs = host(d.log), host(d.seqnos)
        for g in range(nflow):
            a, b = int(d.offsets[g]), int(d.offsets[g + 1])
            assert list(zip(seqs[a:b].tolist(), log[a:b].tolist())) == rx[g].seqno_ids, (where, g)

    def compare_mine(where):
        got = host(d.mine)
        for g in range(nflow):
            assert np.array_equal(got[g], np.frombuffer(rx[g].my_quack._buf, dtype=np.uint32)), (where, g)

    for rno in range(rounds):
        now = 0.04 * rno
        batch = []
        for g in range(nflow):
            k = resend[g] + (0 if rnd.random() < 0.1 else rnd.randrange(0, 301))
            batch += [g] * k
            resend[g] = 0
        rnd.shuffle(batch)
        seqnos, ids = [], []
        for g in batch:
            seq += 1
            v = rnd.getrandbits(32)
            rx[g].on_send(seq, v)
            seqnos.append(seq)
            ids.append(v)
            if rnd.random() >= 0.01:
                proxy[g].insert(v)
        if d is not None:
            d.send(np.array(batch, dtype=np.uint32), np.array(seqnos, dtype=np.uint32), np.array(ids, dtype=np.uint32))
            compare_logs(("send", rno))       # the pending drain and the push, one pass
        present = [rnd.random() < 0.9 for _ in range(nflow)]
        quacks = []
        for g in range(nflow):
            q = proxy[g].clone()
            if rnd.random() < 0.03:
                q.insert(0xDEADBEEF)          # reordering: a last value that is not in the log
            quacks.append(q)
        step = d.on_quacks(quacks, present=present, now=now) if d is not None else None
        for g in range(nflow):
            if not present[g]:
                if d is not None:
                    assert step.action[g] == SND_IDLE and step.retransmit[g] == [] and not step.send_reset[g]
                continue
            idle = quacks[g].last_value() == rx[g].my_quack.last_value()
            want = rx[g].on_quack(quacks[g], now)
            if d is not None:
                assert (step.action[g] == SND_IDLE) == idle, (rno, g)
                assert step.reset_reason[g] == want.reset_reason, (rno, g)
                assert bool(step.send_reset[g]) == want.send_reset, (rno, g)
                assert step.retransmit[g] == want.retransmit, (rno, g)
                assert (step.action[g] == SND_ADVANCED) == (not idle and not want.reset_reason), (rno, g)
            if want.reset_reason:
                stats["fired" if want.send_reset else "held"] += 1
                if want.send_reset:           # the proxy's part of a reset
                    proxy[g] = sk.PowerSumQuackU32(t)
            elif idle:
                stats["idle"] += 1
            else:
                stats["adv"] += 1
            resend[g] = len(want.retransmit)
            stats["retx"] += len(want.retransmit)
        if d is not None:
            compare_mine(rno)
            if rno % 2:
                d.flush()                     # the drain alone
                compare_logs(("flush", rno))
    if d is not None:
        d.flush()
        compare_logs("end")
    return stats


def test_closed_loop_log_never_re_uploaded():
    d = sk.DeviceSenderLog(16, 60)
    d.add_flows(4)
    stats = closed_loop(LOOP_SEED, d)
    assert stats["adv"] > 1000 and stats["fired"] > 20 and stats["held"] > 0 and stats["idle"] > 20 \
        and stats["retx"] > 1000, stats
