"""The u64 encode and the u64 root test on the rare 2^64-wrap fix-ups of their
lazy reduction mod p = 2^64 - 59, bit for bit against Python integers
(pow(x, k, p) sums; polynomial values by Horner mod p).

The ids are tests/golden/u64_rare_ids.json: each takes the fix-up of its label
(mulv at a baby, a giant, the x^80 hand-off or an offset giant; shift32 at a
baby; the chain's fold) in the kernel family of its label, as the model in
tests/golden/make_u64_rare_ids.py says (tests/test_u64_rare_model.py holds
model, fixture and dispatch together on the CPU).  A stream is N = 4 099
splitmix ids (16 tiles of 256 and 3 ids) with fixture ids written in; its
reference is the base stream's sums, computed once, plus the difference of the
replaced ids.

At both ends of every row of the dispatch (u64_rare.py), with the tensor 0 and
1 ids past a 16-byte boundary (1: the chains' head, no tail), every label the
threshold's kernels can reach is placed
  single  in one lane, nothing else rare in the stream (one stream per label:
          a failure names the label)
  lanes   in lanes 0, 31, 32 and 63 of one wave (a wave per label)
  wave    in all 64 lanes of one wave: the carry mask all ones
  tile    all 256 ids of one tile rare, the labels mixed
  ends    at positions 0, N - 3, N - 2, N - 1: the chains' head and tail, the
          last, partial tile
A lane is the kernel's: position mod 64 in the tile kernels; in the chains a
thread takes two ids (.x and .y), so lane l of wave w is ids 2 (64 w + l) and
+ 1 past the head.

The lane-group chains (vfold64; `group` in the fixture) run only when one
workgroup would take 2^30 ids: no test here reaches them."""
import contextlib
import functools

import numpy as np
import pytest

from u64_rare import CHAIN_T, EIGHT_T, FOUR_T, PASS_T, P, rare, rt64_bsgs_range

gpu = pytest.mark.gpu

N = 4099
FX = rare.load()
TMAX = max(PASS_T)
THRESHOLDS = CHAIN_T + FOUR_T + EIGHT_T + PASS_T


def name(lab):
    return "%s/%s/%d" % lab


@functools.lru_cache(maxsize=None)
def base():
    from oracle import coracle
    return [int(v) for v in coracle.splitmix_u64(0x64AA5E, N)]


@functools.lru_cache(maxsize=None)
def powers(x):
    """x^1 .. x^TMAX mod p."""
    out, y = [], x % P
    for _ in range(TMAX):
        out.append(y)
        y = y * x % P
    return out


@functools.lru_cache(maxsize=None)
def base_sums():
    s = [0] * TMAX
    for x in base():
        y = x % P
        for k in range(TMAX):
            s[k] += y
            y = y * x % P
    return [v % P for v in s]


def sums(ids, t):
    s = [0] * t
    for x in ids:
        for k, v in enumerate(powers(x)[:t]):
            s[k] += v
    return [v % P for v in s]


def want_for(t, repl):
    return _want_for(t, tuple(sorted(repl.items())))


@functools.lru_cache(maxsize=None)
def _want_for(t, repl):      # (the tile kernels' placements are the same at both tensor offsets)
    w = base_sums()[:t]
    for pos, x in repl:
        old, new = powers(base()[pos]), powers(x)
        for k in range(t):
            w[k] += new[k] - old[k]
    return [v % P for v in w]


def on_device(ids, off=0):
    """The ids as a CUDA int64 tensor whose first element lies `off` ids past a 16-byte boundary."""
    import torch
    buf = np.zeros(off + len(ids), dtype=np.uint64)
    buf[off:] = np.array(ids, dtype=np.uint64)
    d = torch.from_numpy(buf.view(np.int64)).cuda()
    assert d.data_ptr() % 16 == 0
    return d[off:]


def encode(t, ids, off=0, q=None):
    import sidekick_amd as sk
    q = q or sk.PowerSumQuackU64(t)
    q.insert_batch(on_device(ids, off))
    return q


def check(t, off, repl):
    """Encode the base stream with the ids of `repl` written in; True if sums, count and last value are right."""
    ids = list(base())
    for pos, x in repl.items():
        ids[pos] = x
    q = encode(t, ids, off)
    return q.power_sums() == want_for(t, repl) and q.count() == N and q.last_value() == ids[-1]


def position(t, off, wave, lane, half=0):
    """The id of lane `lane` of wave `wave` (the chains: its .x / .y id)."""
    if rare.schedule_of(t)[0] == "chain":
        return off + 2 * (64 * wave + lane) + half      # head = off ids; N - off is even or leaves a tail of 1
    return 64 * wave + lane


def nwaves(t):
    return (N - 1) // 128 if rare.schedule_of(t)[0] == "chain" else N // 64


def all_labels(t):
    return [x for lab in rare.labels_for(t) for x in FX[lab]]


def placements(t, off):
    """{placement: [(labels, {position: id})]} for the labels of threshold t."""
    labs = rare.labels_for(t)
    chain = rare.schedule_of(t)[0] == "chain"
    halves = (0, 1) if chain else (0,)
    nw = nwaves(t)
    assert len(labs) <= nw
    pos = functools.partial(position, t, off)
    single, lanes, wave, tile, ends = [], {}, {}, {}, []
    for i, lab in enumerate(labs):
        ids = FX[lab]
        single.append(([lab], {pos((3 + 5 * i) % nw, (7 * i + 3) % 64, i % len(halves)): ids[i % len(ids)]}))
        for j, lane in enumerate((0, 31, 32, 63)):      # wave i
            lanes[pos(i, lane, j % len(halves))] = ids[j]
        w = (4 * i) % nw + (4 * i) // nw                 # one wave per tile first
        for lane in range(64):
            for h in halves:
                wave[pos(w, lane, h)] = ids[(2 * lane + h) % len(ids)]
    pool = all_labels(t)
    for j in range(256 if pool else 0):                  # tile 5 (the chains: workgroup 2's 512 ids)
        for h in halves:
            tile[pos(4 * (2 if chain else 5) + j // 64, j % 64, h)] = pool[(2 * j + h) % len(pool)]
    for i in range(0, len(labs), 4):
        four = labs[i:i + 4]
        ends.append((four, {p: FX[lab][(i + k) % len(FX[lab])]
                            for k, (p, lab) in enumerate(zip((0, N - 3, N - 2, N - 1), four))}))
    out = {"single": single, "ends": ends}
    out.update({k: [(labs, v)] for k, v in (("lanes", lanes), ("wave", wave), ("tile", tile)) if v})
    return out


@gpu
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("t", THRESHOLDS)
def test_rare_ids_at_every_dispatch_row(t, off):
    assert check(t, off, {}), "the base stream itself"
    bad = []
    for place, streams in placements(t, off).items():
        for labs, repl in streams:
            assert all(0 <= p < N for p in repl)
            if not check(t, off, repl):     # a label by name where it stood alone, else the placement
                bad.append(name(labs[0]) if place == "single" else "%s (%d labels)" % (place, len(labs)))
    assert not bad, "t = %d, offset %d, wrong sums with: %s" % (t, off, ", ".join(bad))


@gpu
@pytest.mark.parametrize("t", [13, 36, 80, 300])
def test_nothing_but_rare_ids(t):
    ids = all_labels(t) * 11
    for off in (0, 1):
        q = encode(t, ids, off)
        assert q.power_sums() == sums(ids, t) and q.count() == len(ids) and q.last_value() == ids[-1], (t, off)


@gpu
@pytest.mark.parametrize("t", [13, 36, 80, 161])
def test_accumulate_rare_ids_into_a_filled_quack(t):
    first = base()[:1500]
    second = base()[1500:1700] + all_labels(t) + base()[1700:1703]
    q = encode(t, first)
    encode(t, second, 1, q)
    assert q.power_sums() == sums(first + second, t)
    assert q.count() == len(first) + len(second) and q.last_value() == second[-1]


@contextlib.contextmanager
def grid(blocks):
    import sidekick_amd as sk
    ctx = sk.get_context(0)
    ctx.set_grid(blocks)
    try:
        yield
    finally:
        ctx.set_grid(0)


@gpu
@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("t", [80, 161])
def test_one_workgroup_walks_many_tiles(t, blocks):
    """grid 1 and 3: a workgroup's accumulators and carry counts run over 16 / 6
    tiles, the offset passes read the x^base cache tile after tile."""
    with grid(blocks):
        for place in ("lanes", "wave", "tile"):
            for labs, repl in placements(t, 0)[place]:
                assert check(t, 0, repl), (t, blocks, place)
        ids = all_labels(t) * 3
        assert encode(t, ids, 1).power_sums() == sums(ids, t)


@gpu
def test_host_batch_path_with_rare_ids():
    """insert_batch of a host array: the ids staged to the device in chunks."""
    import sidekick_amd as sk
    for t in (13, 80, 161):
        ids = base()[:700] + all_labels(t) + base()[700:705]
        q = sk.PowerSumQuackU64(t)
        q.insert_batch(np.array(ids, dtype=np.uint64))
        assert q.power_sums() == sums(ids, t) and q.count() == len(ids), t


# ------------------------------------------------------------ the u64 root test
NLOG = 1027
MIND, MAXD = rt64_bsgs_range()
SPOTS = (0, 1, 2 * 31, 2 * 32 + 1, 2 * 63, 2 * (64 * 3 + 5) + 1, 2 * 256 + 64, NLOG - 1)   # lanes 0, 31, 32, 63, a second block, the end


@contextlib.contextmanager
def direct_root_test():
    import sidekick_amd as sk
    ctx = sk.get_context(0)
    ctx.set_knob("root_test", 1)
    try:
        yield sk.PowerSumQuackU64(1)
    finally:
        ctx.set_knob("root_test", 0)


@functools.lru_cache(maxsize=None)
def log_base():
    from oracle import coracle
    return [int(v) for v in coracle.splitmix_u64(0x64106, NLOG)]


def root_check(q, c, roots, tag):
    """The candidates `roots` planted at SPOTS (cycled): the hits are the positions where P is 0 mod p."""
    log = list(log_base())
    for k, pos in enumerate(SPOTS):
        log[pos] = roots[k % len(roots)]
    want = [j for j, v in enumerate(log) if rare.poly_eval(c, v % P) == 0]
    assert set(SPOTS) <= set(want), tag
    for off in (0, 1):
        assert q.root_test(c, on_device(log, off)) == want, (tag, off)


def poly_from_roots(roots):
    """c_1 .. c_d of prod (X - r)."""
    c = [1]
    for r in roots:
        c = [(a - r * b) % P for a, b in zip(c + [0], [0] + c)]
    return c[1:]


def bsgs_degrees():
    """Either side of the range's low end, d % 8 == 0 and != 0, 2 and 4 full
    blocks (below MIND = 16 there is no form with one)."""
    return [MIND, MIND + 1, MIND + 7, 2 * MIND, 2 * MIND + 3]


@gpu
@pytest.mark.parametrize("d", bsgs_degrees())
def test_root_test_candidates_whose_baby_steps_wrap(d):
    """The candidates are `serial8` baby ids, the roots of P = prod (X - id): the
    kernel's baby steps x^2 .. x^8 are the encode's, so each wraps in mulv at its power."""
    labs = [("serial8", "baby", b) for k in range(8) for b in range(2, 9)][:d]
    roots = [FX[lab][k // 7] for k, lab in enumerate(labs)]
    assert len(set(roots)) == d
    c = poly_from_roots(roots)
    for x, (_, _, b) in zip(roots[:7], labs):
        assert ("baby", b, 1) in rare.root_bsgs(c, x)[1] and rare.root_bsgs(c, x)[0] % P == 0
    with direct_root_test() as q:
        root_check(q, c, roots, d)


@gpu
@pytest.mark.parametrize("d", bsgs_degrees())
def test_root_test_giant_step_wraps(d):
    """The product R x^8 in front of each block of the Horner in x^8 is a small
    value and wraps in mulv (the model says so): the block constant above it is
    solved for that, p_0 for P(x) = 0."""
    nf, top = d // 8, d % 8 != 0
    xs = [FX["serial8", "giant", 16][0], log_base()[7] % P]
    with direct_root_test() as q:
        for block in range(nf - 1 if not top else nf):
            for n, x in enumerate(xs):
                c = rare.poly_bsgs(x, d, block, seed=n + 1)
                assert c is not None and rare.poly_eval(c, x) == 0
                assert ("giant", block, 1) in rare.root_bsgs(c, x)[1]
                root_check(q, c, [x], (d, block, n))


@gpu
@pytest.mark.parametrize("d", [2, 5, MIND - 1])
def test_root_test_horner_step_wraps(d):
    """Below the baby-step/giant-step range: the product r x of Horner step i
    wraps in mulv, c_(i-1) solved for it, c_d for P(x) = 0."""
    xs = [FX["serial8", "baby", 3][0], log_base()[9] % P]
    with direct_root_test() as q:
        for i in sorted({2, d // 2 + 1, d}):
            for n, x in enumerate(xs):
                c = rare.poly_horner(x, d, i, rare.horner_dev, seed=n + 1)
                assert c is not None and rare.poly_eval(c, x) == 0 and rare.horner_dev(c, x)[1][i - 1] == 1
                root_check(q, c, [x], (d, i, n))


def test_root_test_degrees_straddle_the_sources_range():
    """MIND and MAXD are read from decode.hip: the degree lists follow them."""
    ds = bsgs_degrees()
    assert MIND % 8 == 0 and all(MIND <= d <= MAXD for d in ds) and min(ds) == MIND
    assert {d % 8 == 0 for d in ds} == {True, False} and {d // 8 for d in ds} >= {MIND // 8, MIND // 4}
