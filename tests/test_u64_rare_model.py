"""The model of the u64 kernels' lazy reduction (tests/golden/make_u64_rare_ids.py)
and its fixture tests/golden/u64_rare_ids.json, on the CPU: the model's products
are products mod p, every fixture id takes the fix-up of its label in the
schedule of its label (and a dropped fix-up changes its sums), the committed
file is what the generator writes, the dispatch the model restates is the one
in encode.hip / decode.hip, and the host's insert and root test are right on
the ids and polynomials that take the wrap branch of mul64_lazy / mad64_lazy."""
import os
import random
import re

import pytest

import sidekick_amd as sk
from u64_rare import CHAIN_T, FOUR_T, EIGHT_T, PASS_T, P, rare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sidekick_amd", "csrc")
M64 = 2**64 - 1
EDGES = (0, 1, 59, P - 1, P, P + 1, M64)
FX = rare.load()


def pairs():
    rng = random.Random(64)
    out = [(a, b) for a in EDGES for b in EDGES]
    out += [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(10_000)]
    # operands whose product is a small value: the wrap branch itself
    out += [(x, pow(x, k - 1, P)) for (_, site, k), ids in FX.items() if site in ("baby", "fold") for x in ids]
    return out


def test_model_products_are_products_mod_p():
    wraps = 0
    for V, x in pairs():
        r, w = rare.mulv(V, x)
        wraps += w
        assert r <= M64 and r % P == V * x % P, (V, x)
        r, _ = rare.shift32(V)
        assert r <= M64 and r % P == (V << 32) % P, V
        r, _ = rare.mul64_lazy(V, x)
        assert r % P == V * x % P
        r, _ = rare.mul64_lazy(V, x, x ^ V)
        assert r % P == (V * x + (x ^ V)) % P
        c = (V ^ x) % P                                  # a coefficient is canonical
        r, _ = rare.horner_step(V, x, c)
        assert r <= M64 and r % P == (V * x + c) % P
        th0 = min(x & 63, 59)                            # t-form: th <= 59
        t, th, _ = rare.tmul(V, th0, x)
        assert th <= 59 and (t + (th << 64)) % P == (V + (th0 << 64)) * x % P
        v, _ = rare.vfold64(V, th0)
        assert v <= M64 and v % P == (V + (th0 << 64)) % P
    assert wraps > 100      # the fixture pairs reach mulv's wrap


def test_model_schedules_compute_the_powers():
    rng = random.Random(65)
    for t in CHAIN_T + FOUR_T + EIGHT_T + PASS_T:
        for x in (rng.getrandbits(64), P - 1, M64, FX["serial8", "baby", 2][0]):
            assert rare.encode_one(x, t)[0] == [pow(x, k, P) for k in range(1, t + 1)], (t, x)
    x = rng.getrandbits(64)
    for t, G in ((41, 2), (100, 4), (300, 8)):           # the chains with lane groups (the fallback)
        assert rare.chain_shape(t)[0] == G
        assert rare.encode_group(x, t, *rare.chain_shape(t))[0] == [pow(x, k, P) for k in range(1, t + 1)]
    x8 = pow(x, 8, P)
    for base in (80, 160, 240, 1016):                    # an offset pass without the x^base cache
        assert rare.pow_sqm(x8, base) % P == pow(x, base, P)
    for t in (1, 7, 8, 13, 80, 301):
        got, _ = rare.host_walk(x, t)
        assert [v % P for v in got] == [pow(x, k, P) for k in range(1, t + 1)]


def events_of(schedule, x):
    if schedule in ("serial8", "serial4"):
        return rare.serial(x, int(schedule[-1]), 10 if schedule == "serial8" else 9, schedule == "serial8")[4]
    if schedule == "chain":
        return [("fold", k + 1, w) for k, w in enumerate(rare.chain(x, x, 16)[1])]
    if schedule == "group":
        return rare.group_powers(x, 8)[1]
    return rare.run_schedule(x, 300)[1]


def test_every_fixture_id_takes_its_labelled_fixup():
    assert len(FX) == 83
    for (schedule, site, power), ids in FX.items():
        assert len(set(ids)) == len(ids) >= 4, (schedule, site, power)
        for x in ids:
            assert 0 < x < P
            assert (site, power, 1) in events_of(schedule, x), (schedule, site, power, x)


def test_labels_of_every_threshold_are_in_the_fixture():
    for t in range(1, 301):       # (the passes above t = 300 repeat the offset pass at further bases)
        for lab in rare.labels_for(t):
            assert lab in FX, (t, lab)
    # and every entry is some threshold's (the lane-group chains run only as the fallback for huge n)
    used = {lab for t in range(1, 301) for lab in rare.labels_for(t)}
    assert {lab for lab in FX if lab not in used} == {("group", "vfold64", g) for g in range(2, 9)}


SITE_FIX = {"baby": "mulv", "giant": "mulv", "handoff": "mulv", "offset": "mulv", "shift32": "shift32",
            "fold": "fold", "vfold64": "vfold64"}


def sums_of(lab, x):
    """The sums the id x contributes at the smallest threshold that runs label lab."""
    schedule, site, power = lab
    if schedule == "group":
        G = 2 if power <= 2 else 4 if power <= 4 else 8
        return rare.encode_group(x, 12 * G, G, 12)[0]
    t = next(t for t in range(1, 301) if lab in rare.labels_for(t))
    return rare.encode_one(x, t)[0]


def test_a_dropped_fixup_changes_the_sums_of_every_fixture_id(monkeypatch):
    for lab, ids in FX.items():
        right = [sums_of(lab, x) for x in ids]
        monkeypatch.setitem(rare.FIX, SITE_FIX[lab[1]], 0)
        wrong = [sums_of(lab, x) for x in ids]
        monkeypatch.undo()
        for x, a, b in zip(ids, right, wrong):
            assert a != b, (lab, x)
            assert a == [pow(x, k, P) for k in range(1, len(a) + 1)]


def test_regenerating_reproduces_the_committed_file():
    with open(rare.FIXTURE) as f:
        assert rare.dumps(rare.generate()) == f.read()
    assert os.path.getsize(rare.FIXTURE) < 1 << 20


def test_dispatch_is_the_sources():
    """The t -> kernel map the model restates (schedule_of, chain_shape) and the
    threshold lists of the GPU tests, against enc64 / enc_passes_chunk."""
    hip = open(os.path.join(CSRC, "encode.hip")).read()
    hdr = open(os.path.join(CSRC, "bsgs64.h")).read()
    enc = hip[hip.index("static int enc64("):hip.index("int launch_encode_u32(")]
    lo, hi = re.search(r"if \(T >= (\d+) && T <= (\d+) && bsgs_ok\) \{", enc).groups()
    assert (int(lo), int(hi)) == (14, 80)
    cap, four = re.search(r"with_int\(T <= (\d+) \? \(T \+ 3\) / 4 : 0, ints<([\d, ]+)>\{\}, 1,", enc).groups()
    assert int(cap) == 36 and [int(v) for v in four.split(",")] == [4, 5, 7, 9]
    eight = re.search(r"return with_int\(\(T \+ 7\) / 8, ints<([\d, ]+)>\{\}, QK_E_THRESHOLD,", enc).group(1)
    assert [int(v) for v in eight.split(",")] == list(range(2, 11))
    assert "if (T > 80 && bsgs_ok) return enc_passes(ctx, ids, n, head, T, out, acc, s);" in enc
    kmax, gs = re.search(r"return enc_chain<(\d+), K64_G1, K64_GN>\(T, ints<([\d, ]+)>\{\},", enc).groups()
    assert int(kmax) == 40 and [int(v) for v in gs.split(",")] == [1, 2, 4, 8, 16, 32, 64]
    assert [int(v) for v in re.search(r"using K64_G1 = ints<([\d, ]+)>;", hip).group(1).split(",")] == \
        [1, 2, 4, 8, 12, 16, 20, 24, 32, 40]
    assert [int(v) for v in re.search(r"using K64_GN = ints<([\d, ]+)>;", hip).group(1).split(",")] == \
        [12, 16, 20, 24, 32, 40]
    assert "while ((T + G - 1) / G > (uint32_t)KMAX) G *= 2;" in hip
    # the u64 passes: pass 0 the x80 kernel, then offset passes of <= 80 powers, NA = ceil(Tp / 8), with the cache
    p64 = hip[hip.index("static int enc_passes_chunk(qk_ctx *ctx, const uint64_t *ids"):hip.index("// The x^base cache holds")]
    assert "const uint32_t npass = (T - 80 + 79) / 80;" in p64
    assert "const uint32_t Tp = std::min<uint32_t>(80, T - base);" in p64
    assert "if (xc) launch(k_encode_u64_bsgs_x80, nb, s, ids, (uint64_t)n, head, 80u, partials, xc);" in p64
    assert "const int xcm = !xc ? 0 : 1 | (pass < npass ? 2 : 0);" in p64
    assert "rc = off(std::integral_constant<int, 10>{}, std::integral_constant<int, 3>{});" in p64
    na = re.search(r"rc = with_int\(\(Tp \+ 7\) / 8, ints<([\d, ]+)>\{\}, QK_E_THRESHOLD,", p64).group(1)
    assert [int(v) for v in na.split(",")] == list(range(1, 11))
    # every product kernel: the serial step 1 is the only step 1, B 2^32 is recomputed by the owner wave
    assert "pow_tree" not in hdr and "mulv2" not in hdr and hdr.count("// ---- step 1") == 1
    step1 = hdr[hdr.index("// ---- step 1"):hdr.index("__syncthreads();", hdr.index("// ---- step 1"))]
    assert "for (int b = 0; b < NBT; ++b) {\n            if (b) mulv(V, x0, x1);\n" in step1
    assert "mulv(V, g0, g1);\n            sm.ga[G8 ? a - 1 : a][tid]" in step1 and "shift32" not in step1
    assert hdr.count("struct Smem") == 1                               # one layout: babies and giants as (lo, hi)
    smem = hdr[hdr.index("struct Smem {"):hdr.index("};", hdr.index("struct Smem {"))]
    assert re.findall(r"^\s+(\w+) (\w+)\[", smem, re.M) == [("uint2", "bb"), ("uint2", "ga")]
    step3 = hdr[hdr.index("// ---- step 3"):hdr.index("// ---- reduction")]
    assert "const uint2 B = sm.bb[cb + c][j];\n                const uint64_t sh = shift32(" in step3
    assert "template <int NA_, int NBT_, int SG_, int XC_ = 0, bool OFF_ = false>\nstruct Cfg {" in hdr
    bodies = re.findall(r"bsgs64::body<bsgs64::Cfg<([^>]*)>>", hip)
    assert len(bodies) == hip.count("bsgs64::body<") == 4
    assert [a.split(",")[1].strip() for a in bodies] == ["8", "4", "8", "8"]      # babies per id (NBT)
    assert "constexpr int NB = 8;" in hdr

    # the map, at the thresholds the GPU tests run: both ends of every dispatch row
    assert [rare.schedule_of(t)[1:] for t in CHAIN_T] == [(1, 2), (1, 4), (1, 8), (1, 8), (1, 16)]
    assert [rare.schedule_of(t) for t in FOUR_T] == [("serial4", na) for na in (4, 4, 5, 5, 7, 7, 9, 9)]
    assert [rare.schedule_of(t) for t in EIGHT_T] == [("serial8", na) for na in range(3, 11) for _ in "lh"]
    rows = {}
    for t in range(14, 81):
        rows.setdefault(rare.schedule_of(t), []).append(t)
    assert sorted(FOUR_T + EIGHT_T) == sorted(t for ts in rows.values() for run in _runs(ts) for t in (run[0], run[-1]))
    assert {rare.schedule_of(t)[2] for t in range(2, 14)} == {2, 4, 8, 12, 16}      # K = 12 (t = 9..12): as 16, one size down
    assert [rare.schedule_of(t)[1] for t in PASS_T] == [
        [(80, 1, False)], [(80, 1, False)], [(80, 2, False)], [(80, 10, False)],
        [(80, 10, True), (160, 1, False)], [(80, 10, True), (160, 1, False)],
        [(80, 10, True), (160, 10, False)], [(80, 10, True), (160, 10, True), (240, 8, False)]]


def _runs(ts):
    out = [[ts[0]]]
    for t in ts[1:]:
        if t == out[-1][-1] + 1:
            out[-1].append(t)
        else:
            out.append([t])
    return out


def test_root_test_constants_are_the_sources():
    from u64_rare import rt64_bsgs_range
    lo, hi = rt64_bsgs_range()
    assert 8 < lo < hi <= 1024 and lo % 8 == 0      # the test degrees sit either side of lo, with and without a top block


# ------------------------------------------------------------ the host paths
HOST_T = (3, 7, 8, 13, 16, 17, 80, 81)   # the plain chain, four chains, sixteen (AVX-512 hosts, t >= 16)


def host_ids():
    return [x for (schedule, _, _), ids in FX.items() if schedule in ("serial8", "chain") for x in ids]


def test_host_insert_of_the_rare_ids():
    ids = host_ids()
    assert len(ids) == (24 + 11) * 8
    # some of them take mul64_lazy's wrap branch in the host's own schedule
    assert sum(rare.host_walk(x, 7)[1] for x in ids) > 20 and sum(rare.host_walk(x, 80)[1] for x in ids) > 20
    for t in HOST_T:
        q, one = sk.PowerSumQuackU64(t), None
        want = [0] * t
        for x in ids:
            one = sk.PowerSumQuackU64(t)
            one.insert(x)
            assert one.power_sums() == [pow(x, k, P) for k in range(1, t + 1)], (t, x)
            q.insert(x)
            want = [(s + pow(x, k + 1, P)) % P for k, s in enumerate(want)]
        assert q.power_sums() == want and q.count() == len(ids) and q.last_value() == ids[-1], t
        for x in ids[::2]:
            q.remove(x)
            want = [(s - pow(x, k + 1, P)) % P for k, s in enumerate(want)]
        assert q.power_sums() == want, t


def quack_with_coeffs(c):
    """A u64 quACK (threshold = count = d) whose to_coeffs() is c: its power
    sums by Newton's identities, written into a serialized image."""
    d = len(c)
    S = []
    for k in range(1, d + 1):     # S_k + c_1 S_(k-1) + .. + c_(k-1) S_1 + k c_k = 0
        S.append(-(k * c[k - 1] + sum(c[i - 1] * S[k - i - 1] for i in range(1, k))) % P)
    q = sk.PowerSumQuackU64(d)
    for i in range(d):
        q.insert(i + 1)
    raw = bytearray(q.serialize())
    assert raw[:8] == d.to_bytes(8, "little") and len(raw) == 8 + 8 * d + 9 + 4
    raw[8:8 + 8 * d] = b"".join(s.to_bytes(8, "little") for s in S)
    q = sk.PowerSumQuackU64.deserialize(bytes(raw))
    assert q.power_sums() == S and q.count() == d
    return q


@pytest.mark.parametrize("d", [3, 5, 16, 33])
def test_host_root_test_on_a_wrapping_horner_step(d):
    """decode_host's root64: a polynomial with root x whose Horner mad at step i
    is a small value that takes mad64_lazy's wrap branch (the model says so);
    a missed + 59 there turns the root into a non-root.  (Step 1 is x + c_1 <
    2^65: it cannot wrap.)"""
    rng = random.Random(d)
    xs = FX["serial8", "baby", 2][:2] + [rng.getrandbits(64) % P for _ in range(2)]
    for n, x in enumerate(xs):
        for i in sorted({2, max(d // 2, 2), d - 1}):
            c = rare.poly_horner(x, d, i, rare.horner_host, seed=n)
            assert c is not None and rare.horner_host(c, x)[1][i - 1] == 1
            assert rare.poly_eval(c, x) == 0
            q = quack_with_coeffs(c)
            assert list(q.to_coeffs()) == c
            log = [rng.getrandbits(64) for _ in range(9)]
            log[2] = log[7] = x
            want = [j for j, v in enumerate(log) if rare.poly_eval(c, v) == 0]
            assert want == [2, 7]
            assert q.decode_host(log) == want, (d, i, x)
