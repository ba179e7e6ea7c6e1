"""Batched per-flow decode (qk_u32_to_coeffs_segments_device,
qk_u32_decode_segments_device) on the GPU, bit-exact against the oracle
(newton_coeffs, root_test_indices) per segment, with the single-segment
decode_host as a second witness."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sidekick_amd as sk
from oracle import coracle, quack_oracle as qo
from sidekick_amd._lib import (QK_E_CAPACITY, QK_E_INVAL, QK_E_MISMATCH, QK_E_THRESHOLD, QK_E_UNDECODABLE, QK_OK,
                               lib)

pytestmark = pytest.mark.gpu

P = qo.P32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def item_len():
    """Log entries per work item of the batched root test, as the header documents it."""
    hdr = open(os.path.join(ROOT, "include", "quack_hip.h")).read()
    return int(re.search(r"#define QK_SEG_DECODE_ITEM (\d+)u", hdr).group(1))


def quack(t, ids=(), count=None, last=None, sums=None):
    """A qk_u32 record: the power sums of `ids` (or `sums`), any count / last_value."""
    q = sk.PowerSumQuackU32(t)
    w = np.frombuffer(q._buf, dtype=np.uint32)
    if sums is None:
        sums = coracle.encode_u32(np.array(ids, dtype=np.uint32), t) if len(ids) else [0] * t
    w[4:] = np.array(sums, dtype=np.uint32)
    w[1] = len(ids) if count is None else count
    w[2] = int(last is not None)
    w[3] = 0 if last is None else last
    return q


def records(qs):
    return np.frombuffer(b"".join(q._buf.raw for q in qs), dtype=np.uint32).reshape(len(qs), -1).copy()


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def oracle_segment(q, log, stop):
    """(positions, undecodable) of one segment by the oracle."""
    if q.count() > q.threshold():
        return [], True
    c = qo.newton_coeffs(q.power_sums()[:q.count()], P)
    sv = q.last_value() if stop else None
    return qo.root_test_indices(c, log, P, sv), False


def check_batch(qs, log, offs, stop, witness=True):
    got, status = sk.decode_segments(qs, to_dev(log), offs, stop_at_last=stop)
    assert len(got) == len(qs) == len(status)
    for g, q in enumerate(qs):
        seg = log[offs[g]:offs[g + 1]]
        want, und = oracle_segment(q, seg, stop)
        assert status[g] == (QK_E_UNDECODABLE if und else QK_OK), g
        assert got[g] == want, (g, q, stop)
        if witness and not und:
            assert q.decode_host(seg, stop) == want, g
    return got


# ------------------------------------------------------------ 1. coefficients
@pytest.mark.parametrize("t", [1, 2, 8, 20, 32, 33, 80, 200])
def test_coefficients(t):
    rng = np.random.default_rng(1000 + t)
    counts = [0, 1, 2, t - 1, t, t + 1, 2**32 - 1]
    qs = []
    for g in range(300):
        cnt = counts[int(rng.integers(len(counts)))]
        if g % 2 == 0 and cnt <= t + 1:      # a real diff: the power sums of cnt ids
            ids = rng.integers(0, 2**32, size=cnt, dtype=np.uint64).astype(np.uint32)
            qs.append(quack(t, ids))
        else:                                # arbitrary canonical sums, 0 and p - 1 among them
            s = rng.integers(0, P, size=t, dtype=np.uint64)
            s[rng.random(t) < 0.15] = 0
            s[rng.random(t) < 0.15] = P - 1
            qs.append(quack(t, count=cnt, sums=s))
    want = [qo.newton_coeffs(q.power_sums()[:q.count()], P) if q.count() <= t else [] for q in qs]
    want_status = [QK_OK if q.count() <= t else QK_E_UNDECODABLE for q in qs]
    assert QK_E_UNDECODABLE in want_status and QK_OK in want_status
    for diffs in (qs, to_dev(records(qs))):            # host-resident, then device-resident records
        got, status = sk.to_coeffs_segments(diffs, t)
        assert status == want_status
        assert [list(c) for c in got] == want
    for q, w in zip(qs[:40], want):                    # second witness: the host to_coeffs
        if q.count() <= t:
            assert list(q.to_coeffs()) == w


# ----------------------------------------------------- 2. many short segments
def short_segments(nseg, t, seed):
    rng = np.random.default_rng(seed)
    special = [0, 1, 2, 63, 64, 65, 255, 256, 257]
    logs, qs, prev_k = [], [], -1
    for g in range(nseg):
        n = special[int(rng.integers(len(special)))] if g % 4 == 0 else int(rng.integers(0, 41))
        log = rng.integers(0, 2**31, size=n).astype(np.uint32) * 2 + 1
        log = log[(log > 10) & (log < P - 10)]                   # odd, away from the edge values used below
        n = len(log)
        k = int(rng.integers(0, min(t, n) + 1))
        if k == prev_k and n:                                    # neighbours differ in degree
            k = k - 1 if k else min(1, n)
        if g % 7 == 3:
            k = 0                                                # count == 0 beside a non-empty log
        drop = rng.choice(n, size=k, replace=False) if k else np.zeros(0, np.int64)
        ids = [int(v) for v in log[drop]]
        if g % 5 == 1 and k and n >= 2:
            # congruence: the missing id is 3 (then 0); the log holds 3, p + 3 (and 0, p, p - 1, 2^32 - 1)
            log = np.concatenate([log, np.array([3, P + 3, 0, P, P - 1, 2**32 - 1], dtype=np.uint32)])
            ids = ids[:max(0, t - 2)] + [3, 0]
        if g % 5 == 2 and k:
            log = np.concatenate([log[:n // 2], np.array([ids[0]] * 2, dtype=np.uint32), log[n // 2:]])  # duplicates
        if g % 11 == 4 and 0 < len(ids) < t:
            ids = ids + [ids[0]]                                 # dropped twice: a double root
        last = None
        if len(log) and g % 3 != 0:
            last = int(log[int(rng.integers(len(log)))])         # the cut lands anywhere, roots included
        qs.append(quack(t, ids, last=last))
        logs.append(log)
        prev_k = len(ids)
    offs = np.concatenate([[0], np.cumsum([len(x) for x in logs])]).astype(np.uint64)
    return qs, np.concatenate(logs).astype(np.uint32), offs


@pytest.fixture(scope="module")
def shorts():
    return short_segments(3000, 32, seed=7)


@pytest.mark.parametrize("stop", [False, True])
def test_many_short_segments(shorts, stop):
    qs, log, offs = shorts
    assert len(log) <= 300_000
    degs = [q.count() for q in qs]
    assert any(d == 0 and offs[g + 1] > offs[g] for g, d in enumerate(degs))
    got = check_batch(qs, log, offs, stop)
    assert sum(len(h) for h in got) > 5_000


# ----------------------------------------------------------------- 3. stop rule
def test_stop_rule_per_segment():
    t = 8
    rng = np.random.default_rng(33)
    base = (rng.choice(2**30, size=8 * 50, replace=False).astype(np.uint32) * 4 + 2).reshape(8, 50)
    logs = [base[i].copy() for i in range(8)]
    drops = [[int(l[5]), int(l[20]), int(l[44])] for l in logs]
    lasts = []
    lasts.append(123456789 * 4 + 1)                 # 0: absent from the log
    lasts.append(int(logs[1][0]))                   # 1: at position 0 -> no hits
    lasts.append(int(logs[2][-1]))                  # 2: at the last position
    logs[3][10] = logs[3][30] = 77 * 4 + 3          # 3: present twice, the first wins
    lasts.append(77 * 4 + 3)
    lasts.append(drops[4][1])                       # 4: itself a root -> not a hit, and it cuts
    lasts.append(int(logs[6][3]))                   # 5: present in the next segment only
    lasts.append(int(logs[5][2]))                   # 6: present in the previous segment only
    lasts.append(None)                              # 7: has_last == 0
    logs[7][12] = 0                                 #    (a record's last_value word is 0 then)
    qs = [quack(t, drops[i], last=lasts[i]) for i in range(8)]
    offs = np.arange(9, dtype=np.uint64) * 50
    log = np.concatenate(logs)
    got = check_batch(qs, log, offs, True)
    assert got[0] == [5, 20, 44] and got[1] == [] and got[2] == [5, 20, 44]
    assert got[3] == [5] and got[4] == [5] and got[5] == [5, 20, 44] and got[6] == [5, 20, 44]
    assert got[7] == [5, 20, 44]
    assert check_batch(qs, log, offs, False) == [[5, 20, 44]] * 8


# ------------------------------------------ 4. one long segment among short ones
@pytest.mark.parametrize("t", [8, 80])
def test_long_segment_between_short_ones(t):
    item, n_long = item_len(), 200_003
    assert n_long > 4 * item
    rng = np.random.default_rng(400 + t)
    pre_q, pre_log, pre_offs = short_segments(5, t, seed=41)
    post_q, post_log, post_offs = short_segments(6, t, seed=42)
    long_log = rng.integers(0, 2**31, size=n_long).astype(np.uint32) * 2      # even: apart from the shorts
    missing = [int(v) for v in long_log[rng.choice(n_long, size=t, replace=False)]]
    # position 0, the last one and both sides of every internal work-item
    # boundary hold (copies of) missing ids: all of them are hits
    edge = [0, n_long - 1]
    for b in range(item, n_long, item):
        edge += [b - 1, b]
    for j, pos in enumerate(edge):
        long_log[pos] = missing[j % t]
    stop_pos = 3 * item + 5
    long_q = quack(t, missing, last=int(long_log[stop_pos]))
    qs = pre_q + [long_q] + post_q
    log = np.concatenate([pre_log, long_log, post_log])
    offs = np.concatenate([pre_offs, pre_offs[-1] + n_long + post_offs]).astype(np.uint64)
    d_log = to_dev(log)
    c = qo.newton_coeffs(long_q.power_sums()[:t], P)
    want_long = qo.root_test_u32_np(c, long_log).tolist()
    assert set(edge) <= set(want_long)
    first_stop = int(np.nonzero(long_log == long_log[stop_pos])[0][0])
    for stop in (False, True):
        got, status = sk.decode_segments(qs, d_log, offs, stop_at_last=stop)
        assert status == [QK_OK] * len(qs)
        g_long = len(pre_q)
        assert got[g_long] == ([p for p in want_long if p < first_stop] if stop else want_long)
        for g, q in enumerate(qs):
            if g != g_long:
                assert got[g] == oracle_segment(q, log[offs[g]:offs[g + 1]], stop)[0], g
    assert got[g_long] == long_q.decode_host(long_log, True)


# ------------------------------------------------------------------ 5. capacity
def raw_decode(ctx, rec, d_log, offs, nseg, t, stop, cap):
    hits = np.full(max(cap, 1), 2**64 - 1, dtype=np.uint64)
    hoffs = np.full(nseg + 1, 2**64 - 1, dtype=np.uint64)
    status = np.zeros(max(nseg, 1), dtype=np.int32)
    nh = C.c_size_t(12345)
    rc = lib().qk_u32_decode_segments_device(ctx.handle, rec.ctypes.data, d_log.data_ptr() if d_log is not None else None,
                                             offs.ctypes.data_as(C.POINTER(C.c_uint64)), nseg, t, int(stop),
                                             hits.ctypes.data_as(C.POINTER(C.c_uint64)), cap,
                                             hoffs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                             status.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nh), None)
    return rc, hits, hoffs, nh.value


def test_capacity_and_argument_errors(ctx):
    t = 8
    qs, log, offs = short_segments(200, t, seed=5)
    d_log = to_dev(log)
    rec = records(qs).copy()
    want = [oracle_segment(q, log[offs[g]:offs[g + 1]], False)[0] for g, q in enumerate(qs)]
    want_offs = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint64)
    total = int(want_offs[-1])
    assert total > 10
    for cap in (0, total - 1):
        rc, _, hoffs, nh = raw_decode(ctx, rec, d_log, offs, len(qs), t, False, cap)
        assert rc == QK_E_CAPACITY and nh == total
        assert np.array_equal(hoffs, want_offs)
    rc, hits, hoffs, nh = raw_decode(ctx, rec, d_log, offs, len(qs), t, False, total)
    assert rc == QK_OK and nh == total and np.array_equal(hoffs, want_offs)
    flat = [int(offs[g]) + p for g, w in enumerate(want) for p in w]
    assert hits[:total].tolist() == flat
    # nseg == 0
    rc, _, hoffs, nh = raw_decode(ctx, rec, d_log, offs[:1], 0, t, False, 4)
    assert rc == QK_OK and nh == 0 and hoffs[0] == 0
    # a record of another threshold: host records, then device records
    bad = rec.copy()
    bad[17, 0] = t + 1
    assert raw_decode(ctx, bad, d_log, offs, len(qs), t, False, total)[0] == QK_E_MISMATCH
    d_bad = to_dev(bad)
    with pytest.raises(sk.QuackError) as e:
        sk.decode_segments(d_bad, d_log, offs)
    assert e.value.code == QK_E_MISMATCH
    with pytest.raises(sk.QuackError) as e:
        sk.to_coeffs_segments(d_bad)
    assert e.value.code == QK_E_MISMATCH
    # thresholds, a host log, decreasing offsets
    assert raw_decode(ctx, rec, d_log, offs, len(qs), 0, False, total)[0] == QK_E_THRESHOLD
    assert raw_decode(ctx, rec, d_log, offs, len(qs), 1025, False, total)[0] == QK_E_THRESHOLD
    host_log = np.ascontiguousarray(log)

    class HostLog:
        @staticmethod
        def data_ptr():
            return host_log.ctypes.data
    assert raw_decode(ctx, rec, HostLog, offs, len(qs), t, False, total)[0] == QK_E_INVAL
    down = offs.copy()
    down[5] = down[6] + 1
    assert raw_decode(ctx, rec, d_log, down, len(qs), t, False, total)[0] == QK_E_INVAL


# ------------------------------------------------ 6. device records end to end
def test_device_records_end_to_end():
    """encode_flows(device_out=True) on a sent and on a received batch, the
    difference taken on the device, decoded against the grouped sent ids: the
    recovered ids of every flow are the dropped ones."""
    import torch
    from sidekick_amd.quack import encode_flows
    from test_flows import make_flows, vector_flows
    t, nflows = 16, 300
    bufs, meta = make_flows(60_000, nflows, seed=61, p_filter=0.0, p_reset=0.0)
    # distinct ids, so that a dropped packet is the only log entry with its id
    ids = np.random.default_rng(62).permutation(2**24)[:len(bufs)].astype(np.uint32) + 1000
    bufs[:, 63:67] = ids.astype(">u4").view(np.uint8).reshape(-1, 4)
    rng = np.random.default_rng(63)
    lost = np.zeros(len(bufs), dtype=bool)
    lost[rng.choice(len(bufs), size=900, replace=False)] = True
    sent, _, _ = vector_flows(bufs, meta, my_addr=None)
    keys = sorted(sent)
    # at most t losses per flow, and never a flow's last packet (the received
    # batch must keep every flow and end each flow where the sent batch does)
    pos = {}
    for i in range(len(bufs)):
        k = bytes(np.concatenate([bufs[i, 26:30], bufs[i, 34:36], bufs[i, 30:34], bufs[i, 36:38]]))
        pos.setdefault(k, []).append(i)
    for k, idx in pos.items():
        lost[idx[-1]] = False
        for i in [i for i in idx if lost[i]][t:]:
            lost[i] = False
    dropped = {k: [int(ids[i]) for i in idx if lost[i]] for k, idx in pos.items()}
    assert sum(len(v) for v in dropped.values()) > 500

    def run(sel):
        d_b = torch.from_numpy(bufs[sel].reshape(-1).copy()).cuda()
        d_m = torch.from_numpy(meta[sel].view(np.int64).copy()).cuda()
        return encode_flows(d_b, t, meta=d_m, device_out=True)
    ks, qs, _ = run(np.ones(len(bufs), dtype=bool))
    kr, qr, _ = run(~lost)
    torch.cuda.synchronize()
    assert torch.equal(ks, kr) and [bytes(r) for r in ks.cpu().numpy()] == keys
    # diff = sent - received on the device: sums mod p, counts wrap, header of the sent sketch kept
    s64, r64 = (x[:, 4:].to(torch.int64) & 0xFFFFFFFF for x in (qs, qr))
    diff = qs.clone()
    dsum = (s64 - r64) % P
    diff[:, 4:] = torch.where(dsum >= 2**31, dsum - 2**32, dsum).to(torch.int32)
    diff[:, 1] = qs[:, 1] - qr[:, 1]
    log = np.concatenate([np.array(sent[k], dtype=np.uint32) for k in keys])
    offs = np.concatenate([[0], np.cumsum([len(sent[k]) for k in keys])]).astype(np.uint64)
    for stop in (False, True):
        got, status = sk.decode_segments(diff.contiguous(), to_dev(log), offs, stop_at_last=stop)
        assert status == [QK_OK] * len(keys)
        for g, k in enumerate(keys):
            assert [sent[k][p] for p in got[g]] == dropped[k], k.hex()


# ------------------------------------------------------------- 7. scratch reuse
def test_scratch_reuse(shorts):
    import torch
    qs, log, offs = shorts
    d_log = to_dev(log)
    first = sk.decode_segments(qs, d_log, offs, stop_at_last=True)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    second = sk.decode_segments(qs, d_log, offs, stop_at_last=True)
    third = sk.decode_segments(qs, d_log, offs, stop_at_last=True)
    torch.cuda.synchronize()
    assert first == second == third
    # the context's arenas are grow-only and already large enough: no device allocation
    assert torch.cuda.mem_get_info()[0] >= free0
