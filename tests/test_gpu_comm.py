"""The native multi-GPU path (qk_comm_*, comm.hip: RCCL over xGMI) on the
GPU box: a one-device communicator, built both ways (ncclCommInitAll from one
process; unique id + ncclCommInitRank), must give the single-GPU encode and
decode bit-exactly — the sharded encode's one ncclReduce, the pack of the
per-rank last-id slots and the root's fold all run; so do the sharded
decode's broadcast and two all-gathers.  (A box has one GPU and RCCL takes
one rank per GPU, so N > 1 runs only on the driver's 8-GPU node; the same
protocol at world 2-3 is rehearsed on CPU in tests/test_dist.py.)"""
import numpy as np
import pytest

from oracle import coracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["create", "init_rank"])
def comm(request):
    from sidekick_amd.dist import Comm
    c = Comm.create([0]) if request.param == "create" else Comm.init_rank(Comm.unique_id(), 0, 1, 0)
    assert (c.world, c.nlocal, c.first_rank) == (1, 1, 0)
    yield c
    c.close()


def _ids(bits, n, seed):
    import torch
    a = coracle.splitmix_u32(seed, n) if bits == 32 else coracle.splitmix_u64(seed, n)
    return a, torch.from_numpy(a.view(np.int32 if bits == 32 else np.int64)).cuda()


@pytest.mark.parametrize("bits,t,n", [(32, 32, 3_000_001), (32, 16, 1000), (32, 80, 100_003), (64, 80, 200_001),
                                      (64, 20, 7)])
def test_sharded_encode_one_device_bit_exact(comm, bits, t, n):
    import sidekick_amd as sk
    Q = sk.PowerSumQuackU32 if bits == 32 else sk.PowerSumQuackU64
    host, ids = _ids(bits, n, 0xC0 + t + bits)
    want = Q(t)
    want.insert(12345)                      # existing content: the stream follows it
    want.insert_batch(ids)
    got = Q(t)
    got.insert(12345)
    comm.encode_sharded([ids], got)
    assert got == want
    full = np.concatenate([np.array([12345], dtype=host.dtype), host])
    assert got.power_sums() == (coracle.encode_u32(full, t) if bits == 32 else coracle.encode_u64(full, t))
    assert got.count() == n + 1 and got.last_value() == int(host[-1])


def test_sharded_encode_async_steps_and_empty_shard(comm):
    import torch
    import sidekick_amd as sk
    host, ids = _ids(32, 1_000_000, 0xA5)
    for _ in range(3):                      # back-to-back async steps reuse the payload buffer
        comm.encode_sharded_async([ids], 32)
    q = sk.PowerSumQuackU32(32)
    comm.encode_sharded_wait(q)
    assert q.power_sums() == coracle.encode_u32(host, 32) and q.count() == len(host)
    empty = torch.empty(0, dtype=torch.int32, device="cuda")
    q2 = sk.PowerSumQuackU32(32)
    q2.insert(9)
    comm.encode_sharded([empty], q2)         # an empty shard keeps the last value and adds nothing
    assert q2.count() == 1 and q2.last_value() == 9
    with pytest.raises(sk.QuackError):
        comm.encode_sharded_wait(q2)         # nothing in flight
    comm.barrier()


@pytest.mark.parametrize("bits", [32, 64])
def test_sharded_decode_one_device_matches_single_gpu(comm, bits):
    import sidekick_amd as sk
    Q = sk.PowerSumQuackU32 if bits == 32 else sk.PowerSumQuackU64
    host, log = _ids(bits, 500_000, 0xDEC + bits)
    rng = np.random.default_rng(bits)
    drops = np.sort(rng.choice(len(host), 24, replace=False))
    keep = np.ones(len(host), bool)
    keep[drops] = False
    a, b = Q(32), Q(32)
    a.insert_batch(log)
    import torch
    b.insert_batch(torch.from_numpy(host[keep].view(np.int32 if bits == 32 else np.int64)).cuda())
    a.sub_assign(b)
    want = a.root_test(a.to_coeffs(), log, stop_value=a.last_value())
    got = comm.decode_sharded(a, [log], bits=bits, stop_at_last=True)
    assert got == want
    assert set(drops.tolist()) - {len(host) - 1} <= set(got)
    # no stop: every hit of the log
    assert comm.decode_sharded(a, [log], bits=bits, stop_at_last=False) == a.root_test(a.to_coeffs(), log)


def test_sharded_decode_undecodable_and_empty(comm):
    import sidekick_amd as sk
    from sidekick_amd._lib import UndecodableError
    host, log = _ids(32, 10_000, 0x77)
    q = sk.PowerSumQuackU32(4)
    for v in host[:9]:
        q.insert(int(v))
    with pytest.raises(UndecodableError):
        comm.decode_sharded(q, [log])
    z = sk.PowerSumQuackU32(4)
    assert comm.decode_sharded(z, [log]) == []


# ----------------------------------------------------------------------------
# World 2-8 on one GPU: the native protocol (comm.hip) with its collectives over
# a host channel between threads (qk_comm_init_host + LoopbackHub).  RCCL takes
# one rank per GPU, so this is how the multi-rank payload packing, the
# failed-rank word, the root fold, the status gather and the chunked hit
# gather run before the driver's 8-GPU node.
# ----------------------------------------------------------------------------
import threading  # noqa: E402


def _run_ranks(world, fn, timeout=120.0, comms=None):
    """fn(rank, comm) on one thread per rank, each with its own host-channel
    communicator on device 0; returns [(ok, value_or_exception)] per rank."""
    from sidekick_amd.dist import Comm, LoopbackHub
    own = comms is None
    if own:
        hub = LoopbackHub(world, timeout=timeout)
        comms = [Comm.init_host(hub.channel(r), r, world, 0) for r in range(world)]
    out = [None] * world

    def run(r):
        try:
            out[r] = (True, fn(r, comms[r]))
        except Exception as e:  # noqa: BLE001
            out[r] = (False, e)
    ths = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for th in ths:
        th.start()
    for th in ths:
        th.join(timeout + 60)
    assert not any(th.is_alive() for th in ths), "a rank hung"
    if own:
        for c in comms:
            c.close()
    return out


def _shards(n_total, world, empty=()):
    """Contiguous shards of a global stream; ranks in `empty` get none."""
    from sidekick_amd.dist import shard
    live = [r for r in range(world) if r not in empty]
    bounds, pos = [], 0
    for r in range(world):
        if r in empty:
            bounds.append((pos, 0))
        else:
            s, c = shard(n_total, live.index(r), len(live))
            bounds.append((s, c))
            pos = s + c
    return bounds


@pytest.mark.parametrize("world,bits,t,empty", [(2, 32, 32, ()), (4, 32, 16, (0, 2)), (8, 32, 32, (3, 7)),
                                                (8, 64, 80, (0, 5)), (3, 64, 20, (2,))])
def test_host_channel_world_n_encode_bit_exact(world, bits, t, empty):
    import torch
    import sidekick_amd as sk
    Q = sk.PowerSumQuackU32 if bits == 32 else sk.PowerSumQuackU64
    n_total = 400_003 if bits == 32 else 150_001
    host, ids = _ids(bits, n_total, 0x5A + world + t)
    bounds = _shards(n_total, world, empty)
    views = [ids[s:s + c] if c else torch.empty(0, dtype=ids.dtype, device="cuda") for s, c in bounds]

    def rank_fn(r, comm):
        q = Q(t)
        q.insert(777)                   # the root's existing content: the stream follows it
        comm.encode_sharded([views[r]], q)
        return q

    res = _run_ranks(world, rank_fn)
    assert all(ok for ok, _ in res), res
    root = res[0][1]
    full = np.concatenate([np.array([777], dtype=host.dtype), host])
    assert root.power_sums() == (coracle.encode_u32(full, t) if bits == 32 else coracle.encode_u64(full, t))
    assert root.count() == n_total + 1 and root.last_value() == int(host[-1])
    for r in range(1, world):           # non-root: untouched
        q = res[r][1]
        assert q.count() == 1 and q.last_value() == 777


def test_host_channel_async_steps_and_root_not_zero():
    import sidekick_amd as sk
    world, t = 4, 32
    host, ids = _ids(32, 1_000_000, 0xA7)
    bounds = _shards(len(host), world)

    def rank_fn(r, comm):
        for _ in range(3):              # back-to-back async steps reuse the payload buffer
            comm.encode_sharded_async([ids[bounds[r][0]:sum(bounds[r])]], t, root=2)
        q = sk.PowerSumQuackU32(t)
        comm.encode_sharded_wait(q)
        comm.barrier()
        return q

    res = _run_ranks(world, rank_fn)
    assert all(ok for ok, _ in res), res
    assert res[2][1].power_sums() == coracle.encode_u32(host, t) and res[2][1].count() == len(host)
    assert all(res[r][1].count() == 0 for r in (0, 1, 3))


def _decode_case_gpu(bits, n_total, seed, dup_rank_pos=None, n_dup=0):
    """Log with `n_dup` copies of one dropped id placed at dup_rank_pos (so one
    shard holds more hits than a gather round carries)."""
    import torch
    import sidekick_amd as sk
    Q = sk.PowerSumQuackU32 if bits == 32 else sk.PowerSumQuackU64
    a = (coracle.splitmix_u32 if bits == 32 else coracle.splitmix_u64)(seed, n_total).copy()
    rng = np.random.default_rng(seed & 0xFFFF)
    drops = np.sort(rng.choice(n_total, 30, replace=False))
    if n_dup:
        a[dup_rank_pos:dup_rank_pos + n_dup] = a[drops[0]]
    keep = np.ones(n_total, bool)
    keep[drops] = False
    dt = np.int32 if bits == 32 else np.int64
    log = torch.from_numpy(a.view(dt)).cuda()
    A, B = Q(32), Q(32)
    A.insert_batch(log)
    B.insert_batch(torch.from_numpy(a[keep].view(dt)).cuda())
    A.sub_assign(B)
    return a, log, A


@pytest.mark.parametrize("world,bits,n_dup,stop", [(8, 32, 0, True), (8, 32, 2500, False), (4, 64, 1200, True),
                                                   (2, 32, 0, False), (5, 64, 0, False)])
def test_host_channel_world_n_decode_matches_single_gpu(world, bits, n_dup, stop):
    n_total = 200_000
    a, log, diff = _decode_case_gpu(bits, n_total, 0xDE0 + world + bits, dup_rank_pos=60_000, n_dup=n_dup)
    want = diff.root_test(diff.to_coeffs(), log, stop_value=diff.last_value() if stop else None)
    assert len(want) >= (n_dup or 25)
    bounds = _shards(n_total, world)

    def rank_fn(r, comm):
        s, c = bounds[r]
        return comm.decode_sharded(diff if r == 0 else None, [log[s:s + c]], bits=bits, stop_at_last=stop)

    res = _run_ranks(world, rank_fn)
    assert all(ok for ok, _ in res), res
    for ok, got in res:
        assert got == want


def test_host_channel_decode_stop_in_middle_shard():
    """The stop value first occurs in rank 2's shard: every later hit is cut."""
    world, n_total = 4, 100_000
    a, log, diff = _decode_case_gpu(32, n_total, 0x5707)
    want_all = diff.root_test(diff.to_coeffs(), log)
    stop_pos = 55_000
    stop_val = int(a[stop_pos])
    first = int(np.nonzero(a == stop_val)[0][0])
    want = [h for h in want_all if h < first]
    assert len(want) < len(want_all)
    import ctypes as C
    q = diff.clone()                        # the same difference, last_value = the stop id
    C.memmove(C.addressof(q._buf) + 8, np.array([1, stop_val], dtype=np.uint32).ctypes.data, 8)
    assert q.last_value() == stop_val and q.count() == diff.count()
    assert diff.root_test(diff.to_coeffs(), log, stop_value=stop_val) == want
    bounds = _shards(n_total, world)

    def rank_fn(r, comm):
        s, c = bounds[r]
        return comm.decode_sharded(q if r == 0 else None, [log[s:s + c]], stop_at_last=True)

    res = _run_ranks(world, rank_fn)
    assert all(ok for ok, _ in res), res
    assert all(got == want for _, got in res)


@pytest.mark.parametrize("stop", [False, True])
@pytest.mark.parametrize("n_dup", [0, 5000])
@pytest.mark.parametrize("bits", [32, 64])
def test_host_channel_decode_by_root_set_scan(bits, n_dup, stop):
    """The sharded decode with the root-set scan forced on every rank (knob
    root_test = 2; small logs otherwise pick Horner): one plan, its roots found
    once, shared by the shards; the scan's set by the H2D copy form, its hits
    through the pinned slots.  With 5000 copies of one dropped id in rank 1's
    shard that rank runs past its slots and past the 4096-entry hit buffer
    (the counters read back, the buffer grown, the scan rerun from the same
    plan).  Every rank returns the single-GPU Horner answer, which is the
    numpy positions of the dropped ids cut at the stop."""
    import torch
    import sidekick_amd as sk
    world, n_total, d = 3, 30_000, 30
    dup_at = 12_000                                   # rank 1 holds [10 000, 20 000)
    Q = sk.PowerSumQuackU32 if bits == 32 else sk.PowerSumQuackU64
    p = (1 << 32) - 5 if bits == 32 else (1 << 64) - 59
    a = (coracle.splitmix_u32 if bits == 32 else coracle.splitmix_u64)(0x5CA0 + bits, n_total).copy()
    rng = np.random.default_rng(bits + n_dup)
    free = np.setdiff1d(np.arange(n_total - 1), np.arange(dup_at, dup_at + 5000))   # not the copies, not the last id
    drops = np.sort(rng.choice(free, d, replace=False))
    assert len({int(v) % p for v in a[drops]}) == d
    if n_dup:
        a[dup_at:dup_at + n_dup] = a[drops[0]]
    keep = np.ones(n_total, bool)
    keep[drops] = False
    dt = np.int32 if bits == 32 else np.int64
    log = torch.from_numpy(a.view(dt)).cuda()
    diff, recv = Q(32), Q(32)
    diff.insert_batch(log)
    recv.insert_batch(torch.from_numpy(a[keep].view(dt)).cuda())
    diff.sub_assign(recv)
    assert diff.count() == d
    coeffs = diff.to_coeffs()
    assert len(coeffs) == d

    last = diff.last_value()
    assert last == int(a[-1])
    dropped = {int(v) % p for v in a[drops]}
    pos = [i for i, v in enumerate(a.tolist()) if v % p in dropped]
    cut = int(np.flatnonzero(a == a[-1])[0]) if stop else n_total
    want = [i for i in pos if i < cut]
    assert len(want) == d + n_dup and set(drops.tolist()) <= set(want)

    ctx = sk.get_context(0)
    ctx.set_knob("root_test", 1)
    try:
        assert diff.root_test(coeffs, log, stop_value=last if stop else None) == want
    finally:
        ctx.set_knob("root_test", 0)
    bounds = _shards(n_total, world)

    def rank_fn(r, comm):
        comm.context(0).set_knob("root_test", 2)
        try:
            s, c = bounds[r]
            return comm.decode_sharded(diff if r == 0 else None, [log[s:s + c]], bits=bits, stop_at_last=stop)
        finally:
            comm.context(0).set_knob("root_test", 0)

    res = _run_ranks(world, rank_fn)
    assert all(ok for ok, _ in res), res
    for _, got in res:
        assert got == want


def test_host_channel_failure_on_one_rank_errors_everywhere_no_hang():
    """A bad shard on one rank (misaligned device pointer): the sharded encode
    returns its error on that rank and QK_E_PEER on the root, q untouched; the
    sharded decode returns the same error on every rank; the communicator
    stays usable."""
    import torch
    import sidekick_amd as sk
    from sidekick_amd._lib import QK_E_INVAL, QK_E_PEER
    world, t = 3, 16
    host, ids = _ids(32, 30_000, 0xFA11)
    raw = torch.zeros(10_001, dtype=torch.int32, device="cuda")
    bad = raw.view(torch.uint8)[1:1 + 4 * 10_000]          # misaligned by one byte
    bounds = _shards(len(host), world)
    from sidekick_amd.dist import Comm, LoopbackHub
    hub = LoopbackHub(world, timeout=60)
    comms = [Comm.init_host(hub.channel(r), r, world, 0) for r in range(world)]
    try:
        from sidekick_amd._lib import lib
        import ctypes as C

        def enc(r, comm, bad_rank):
            q = sk.PowerSumQuackU32(t)
            q.insert(5)
            before = q.power_sums()
            s, c = bounds[r]
            if r == bad_rank:
                ptr, cnt = bad.data_ptr(), 10_000
            else:
                ptr, cnt = ids[s:s + c].data_ptr(), c
            rc = lib().qk_u32_encode_sharded(comm.handle, (C.c_void_p * 1)(ptr), (C.c_size_t * 1)(cnt), q._buf, 0,
                                             None)
            return rc, q.power_sums() == before and q.count() == 1

        for bad_rank in (1, 0):
            res = _run_ranks(world, lambda r, cm: enc(r, cm, bad_rank), comms=comms)
            assert all(ok for ok, _ in res), res
            rcs = [v[0] for _, v in res]
            assert rcs[bad_rank] == QK_E_INVAL
            if bad_rank != 0:
                assert rcs[0] == QK_E_PEER
            assert all(v[1] for _, v in res)               # q untouched everywhere

        a, log, diff = _decode_case_gpu(32, 60_000, 0xBAD)

        def dec(r, comm):
            s, c = bounds[r]
            ptr = bad.data_ptr() if r == 2 else log[s:s + c].data_ptr()
            hits = (C.c_uint64 * 64)()
            nh = C.c_size_t()
            return lib().qk_u32_decode_sharded(comm.handle, diff._buf if r == 0 else None, 0,
                                               (C.c_void_p * 1)(ptr), (C.c_size_t * 1)(c), 1, hits, 64,
                                               C.byref(nh), None)

        res = _run_ranks(world, dec, comms=comms)
        assert [v for _, v in res] == [QK_E_INVAL] * world

        # still usable: a clean round after the failures
        def good(r, comm):
            q = sk.PowerSumQuackU32(t)
            s, c = bounds[r]
            comm.encode_sharded([ids[s:s + c]], q)
            return q
        res = _run_ranks(world, good, comms=comms)
        assert res[0][1].power_sums() == coracle.encode_u32(host, t)
    finally:
        for c in comms:
            c.close()


def test_host_channel_peer_never_arrives_fails_instead_of_hanging():
    """A rank that never joins: the channel times out, the caller gets
    QK_E_COMM and the communicator stays failed (no hang)."""
    import sidekick_amd as sk
    from sidekick_amd._lib import QK_E_COMM, QuackError
    from sidekick_amd.dist import Comm, LoopbackHub
    hub = LoopbackHub(2, timeout=3)
    c0 = Comm.init_host(hub.channel(0), 0, 2, 0)
    try:
        host, ids = _ids(32, 1000, 0x1)
        q = sk.PowerSumQuackU32(8)
        with pytest.raises(QuackError) as ei:
            c0.encode_sharded([ids], q)
        assert ei.value.code == QK_E_COMM and q.count() == 0
        with pytest.raises(QuackError) as ei:
            c0.barrier()
        assert ei.value.code == QK_E_COMM
    finally:
        c0.close()


def test_rccl_world1_local_failure_leaves_q_untouched(comm):
    """World-1 RCCL communicator: a bad shard fails the call, q is untouched,
    and the communicator keeps working."""
    import torch
    import ctypes as C
    import sidekick_amd as sk
    from sidekick_amd._lib import QK_E_INVAL, lib
    raw = torch.zeros(1001, dtype=torch.int32, device="cuda")
    q = sk.PowerSumQuackU32(32)
    q.insert(3)
    rc = lib().qk_u32_encode_sharded(comm.handle, (C.c_void_p * 1)(raw.data_ptr() + 2), (C.c_size_t * 1)(1000),
                                     q._buf, 0, None)
    assert rc == QK_E_INVAL and q.count() == 1 and q.power_sums()[0] == 3
    host, ids = _ids(32, 5000, 0x33)
    comm.encode_sharded([ids], q)
    assert q.count() == 5001


@pytest.mark.parametrize("how", ["create", "init_rank"])
def test_rccl_world1_pre_collective_wait_is_bounded(how):
    """Local work in front of an RCCL collective (knob comm_delay_ms: a kernel
    of that many ms on the rank's stream before its reduce) is waited for
    under its own limit, 4 x the communicator's timeout: a delay inside the
    limit completes bit-exactly; one past it returns QK_E_COMM within about
    that limit (no unbounded hipEventSynchronize), q untouched, the
    communicator broken — later calls fail at once — and its destroy aborts
    RCCL once the local work has drained.  (A world-1 in-place ncclReduce
    enqueues no kernel: profiles/r06/comm1/, so nothing of RCCL's runs after
    the abort.)"""
    import time
    import ctypes as C
    import sidekick_amd as sk
    from sidekick_amd._lib import QK_E_COMM, QK_OK, lib
    from sidekick_amd.dist import Comm
    host, ids = _ids(32, 200_003, 0x3D)
    want = sk.PowerSumQuackU32(32)
    want.insert_batch(ids)
    c = Comm.create([0]) if how == "create" else Comm.init_rank(Comm.unique_id(), 0, 1, 0)
    try:
        c.set_timeout(200)                     # collective 200 ms, local work before it 800 ms
        q = sk.PowerSumQuackU32(32)
        c.context(0).set_knob("comm_delay_ms", 300)
        c.encode_sharded([ids], q)
        assert q == want
        q = sk.PowerSumQuackU32(32)
        q.insert(7)
        c.context(0).set_knob("comm_delay_ms", 3000)
        t0 = time.time()
        rc = lib().qk_u32_encode_sharded(c.handle, (C.c_void_p * 1)(ids.data_ptr()), (C.c_size_t * 1)(len(host)),
                                         q._buf, 0, None)
        dt = time.time() - t0
        assert rc == QK_E_COMM, rc
        assert 0.7 < dt < 2.0, dt              # the 800 ms limit, not the 3 s kernel
        assert q.count() == 1 and q.power_sums()[0] == 7
        t0 = time.time()
        rc = lib().qk_u32_encode_sharded(c.handle, (C.c_void_p * 1)(ids.data_ptr()), (C.c_size_t * 1)(len(host)),
                                         q._buf, 0, None)
        assert rc == QK_E_COMM and q.count() == 1 and time.time() - t0 < 0.5
        assert rc != QK_OK
    finally:
        import torch
        torch.cuda.synchronize()               # the 3 s kernel drains before the context goes
        c.close()


def test_host_channel_staging_fault_at_every_step_same_status_everywhere():
    """A rank whose payload staging fails (knob comm_fault = k: the copy into
    its k-th collective of the call) keeps joining and sends the failure as
    data.  Sharded encode (one reduce, step 1): that rank returns QK_E_HIP, the
    root QK_E_PEER, q untouched everywhere.  Sharded decode (broadcast = 1,
    status gather = 2, hit rounds = 3..): every rank returns the same status,
    QK_E_HIP, within one call — no rank waits on a peer that left — and the
    communicator then runs a clean round."""
    import ctypes as C
    import time
    import sidekick_amd as sk
    from sidekick_amd._lib import QK_E_HIP, QK_E_PEER, QK_OK, lib
    from sidekick_amd.dist import Comm, LoopbackHub
    world, t = 4, 16
    host, ids = _ids(32, 40_000, 0xFA57)
    bounds = _shards(len(host), world)
    hub = LoopbackHub(world, timeout=60)
    comms = [Comm.init_host(hub.channel(r), r, world, 0) for r in range(world)]
    try:
        def enc(r, comm, bad, k):
            if r == bad:
                comm.context(0).set_knob("comm_fault", k)
            q = sk.PowerSumQuackU32(t)
            q.insert(5)
            s, c = bounds[r]
            rc = lib().qk_u32_encode_sharded(comm.handle, (C.c_void_p * 1)(ids[s:s + c].data_ptr()),
                                             (C.c_size_t * 1)(c), q._buf, 0, None)
            return rc, q.count() == 1 and q.power_sums()[0] == 5
        for bad in (2, 0):
            res = _run_ranks(world, lambda r, cm: enc(r, cm, bad, 1), comms=comms)
            assert all(ok for ok, _ in res), res
            rcs = [v[0] for _, v in res]
            assert rcs[bad] == QK_E_HIP
            assert all(rcs[r] == QK_OK for r in range(1, world) if r != bad)
            if bad != 0:
                assert rcs[0] == QK_E_PEER
            assert all(v[1] for _, v in res)               # q untouched everywhere

        a, log, diff = _decode_case_gpu(32, 80_000, 0xFA58)
        want = diff.root_test(diff.to_coeffs(), log, stop_value=diff.last_value())
        assert want
        dbounds = _shards(80_000, world)

        def dec(r, comm, bad, k):
            if r == bad:
                comm.context(0).set_knob("comm_fault", k)
            s, c = dbounds[r]
            hits = (C.c_uint64 * 4096)()
            nh = C.c_size_t()
            rc = lib().qk_u32_decode_sharded(comm.handle, diff._buf if r == 0 else None, 0,
                                             (C.c_void_p * 1)(log[s:s + c].data_ptr()), (C.c_size_t * 1)(c), 1,
                                             hits, 4096, C.byref(nh), None)
            return rc, [int(h) for h in hits[: nh.value]]

        for k in (1, 2, 3):
            for bad in (0, 3):
                t0 = time.time()
                res = _run_ranks(world, lambda r, cm: dec(r, cm, bad, k), comms=comms)
                assert time.time() - t0 < 30
                assert all(ok for ok, _ in res), res
                assert [v[0] for _, v in res] == [QK_E_HIP] * world, (k, bad, res)
                # reusable: a clean round gives the single-GPU answer on every rank
                res = _run_ranks(world, lambda r, cm: dec(r, cm, -1, 0), comms=comms)
                assert all(v == (QK_OK, want) for _, v in res), (k, bad)
    finally:
        for c in comms:
            c.close()


@pytest.mark.slow
def test_configs3_full_size_world8_host_channel():
    """configs[3] at full size on one GPU (skipped below ~40 GB of device
    memory; marked slow, `-m "gpu and not slow"` deselects it): 8e9 u32 ids (32 GB, the bench's
    global stream at N = 8: seed 0x5EED0002) at t = 32, one contiguous shard
    per rank of a world-8 communicator — the native protocol (per-rank encode,
    k_comm_pack, one sum-reduce, the root's fold) with its collectives over
    the host channel, since RCCL takes one rank per GPU.  The root's sketch
    must equal the single-GPU encode of the whole stream (> 2^32 ids, count
    wrapping as the crate's u32) and the merge of uneven pieces; the same
    with uneven shards (two ranks empty); a 2e6 prefix against the oracle.
    The digests of the N = 2, 4, 8 global streams are checked against the
    ones bench.py records for the driver's scaling runs."""
    import torch
    import bench
    import sidekick_amd as sk
    from sidekick_amd.quack import fill_splitmix
    if torch.cuda.get_device_properties(0).total_memory < 40 * (1 << 30):
        pytest.skip("needs ~40 GB of device memory (8e9 u32 ids + the single-GPU pass)")
    n, t, world, seed = 8_000_000_000, 32, 8, 0x5EED0002
    ctx = sk.get_context(0)
    d = torch.empty(n, dtype=torch.int32, device="cuda")
    try:
        fill_splitmix(ctx, d, seed)
        whole = sk.PowerSumQuackU32(t)
        whole.insert_batch(d)
        assert whole.count() == n & 0xFFFFFFFF
        assert whole.last_value() == int(coracle.splitmix_u32(seed, 1, start=n - 1)[0])
        pieces = sk.PowerSumQuackU32(t)
        for a, b in ((0, 3_000_000_007), (3_000_000_007, 4_294_967_301), (4_294_967_301, n - 1), (n - 1, n)):
            pieces.insert_batch(d[a:b])
        assert pieces == whole
        assert pieces.power_sums() != sk.PowerSumQuackU32(t).power_sums()

        for bounds in (_shards(n, world),
                       [(0, 1_000_000_000), (1_000_000_000, 0), (1_000_000_000, 2_500_000_001),
                        (3_500_000_001, 1), (3_500_000_002, 0), (3_500_000_002, 3_000_000_000),
                        (6_500_000_002, 1_499_999_997), (7_999_999_999, 1)]):
            assert sum(c for _, c in bounds) == n
            views = [d[s:s + c] if c else d[:0] for s, c in bounds]

            def rank_fn(r, comm):
                q = sk.PowerSumQuackU32(t)
                comm.encode_sharded([views[r]], q)
                return q

            res = _run_ranks(world, rank_fn, timeout=600)
            assert all(ok for ok, _ in res), res
            assert res[0][1] == whole
            assert all(res[r][1].count() == 0 for r in range(1, world))

        head = sk.PowerSumQuackU32(t)
        head.insert_batch(d[:2_000_000])
        assert head.power_sums() == coracle.encode_u32_seed(seed, 2_000_000, t)

        got = {n: bench.digest_of(whole.power_sums(), whole.count())}
        for m in (2_000_000_000, 4_000_000_000):
            q = sk.PowerSumQuackU32(t)
            q.insert_batch(d[:m])
            got[m] = bench.digest_of(q.power_sums(), q.count())
        print("configs[3] digests:", {f"{m:.0e}": v for m, v in got.items()})
        for m, v in got.items():
            rec = bench.RECORDED_DIGESTS.get((32, t, m, seed))
            assert rec is None or rec == v, (m, rec, v)
    finally:
        del d
        torch.cuda.empty_cache()
