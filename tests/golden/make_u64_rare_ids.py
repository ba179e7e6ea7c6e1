#!/usr/bin/env python3
"""The u64 kernels' lazy reduction modulo p = 2^64 - 59, restated in Python
integers, and the ids that take its rare 2^64-wrap fix-ups
(tests/golden/u64_rare_ids.json).  Run:  python tests/golden/make_u64_rare_ids.py

Every u64 product keeps values < 2^64 that are congruent to, not equal to,
the canonical residue, and reduces 2^64 == 59 in steps.  The last step of a
product adds 59 F.hi to a 64-bit word; when that add wraps, 59 more are owed.
On random ids it wraps with probability ~ 59 * 60 / 2^64 per product (the
`mulv` step, the chain's fold, `vfold64`, the host's `mul64_lazy`) or
~ 59 / 2^32 per (id, baby) (`shift32`): no random stream reaches them.

The wrap leaves the product's value in [59, 59 * 61), so the ids are built,
not searched for: for a product that computes x^k, take a small r in that
range and solve x^k == r.  p - 1 = 4 * 11 * m; in the subgroup of order D =
(p - 1) / gcd-part(k) the map x -> x^k is a bijection, so for every r with
r^D == 1, x = r^(k^-1 mod D).  Whether x really wraps depends on the
non-canonical words the kernel carries at that product: the model below runs
the kernel's schedule word for word and keeps the x that do (a quarter to a
half of them).  `shift32` wraps for B.lo >= 2^32 - 58 and a large B.hi: for
baby 1 that is the id itself, for baby b the b-th root of such a B.

The functions restate, instruction by instruction, bsgs64.h QK_U64_MULV_ASM
(`mulv`) and `shift32`, encode.hip QK_U64_STEP_ASM / QK_U64_MUL_ASM (`chain`,
`tmul`) and `vfold64`, field.h `mul64_lazy` / `mad64_lazy`, decode.hip
`horner64_step` and `is_root64_bsgs`, and the product schedules of
bsgs64::body (serial step 1, B 2^32 by the owner wave) and of enc64 /
enc_passes_chunk.  FIX holds the constants of the fix-ups, so a test can zero
one and see which sums change.
"""
from __future__ import annotations

import json
import math
import os

P = 2**64 - 59
M32 = 2**32 - 1
M64 = 2**64 - 1
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "u64_rare_ids.json")
NIDS = 8                                   # ids per entry
SMALL = range(59, 59 * 61)                 # a wrapped product's value

# what each fix-up adds (59; a test zeroes one to model a dropped fix-up)
FIX = {"mulv": 59, "shift32": 59, "fold": 59, "vfold64": 59}


# ------------------------------------------------------------ the products
def _prod(V, x):
    """P = V x, then E = P_L + 59 PH.lo (carry ce), F = E.hi + ce 2^32 + 59 PH.hi:
    the seven mads that mulv, the chain step and tmul share.  Returns (E, F)."""
    v2, v3, x0, x1 = V & M32, V >> 32, x & M32, x >> 32
    A = v2 * x0
    B = v3 * x0 + (A >> 32)
    assert B <= M64
    Cc = v2 * x1 + B
    cc, Cc = Cc >> 64, Cc & M64
    PH = v3 * x1 + ((Cc >> 32) | (cc << 32))
    assert PH <= M64                       # P < 2^128
    PL = (A & M32) | ((Cc & M32) << 32)
    E = (PH & M32) * 59 + PL
    ce, E = E >> 64, E & M64
    F = (PH >> 32) * 59 + ((E >> 32) | (ce << 32))
    assert F <= M64
    return E, F


def _add_lo(V, c):
    """v_add_u32 on the low word alone (the wrapped value is < 59 * 60)."""
    return (V >> 32 << 32) | ((V + c) & M32)


def mulv(V, x):
    """bsgs64.h mulv: V x mod p, < 2^64.  Returns (V', wrapped)."""
    E, F = _prod(V, x)
    W = (F >> 32) * 59 + ((E & M32) | ((F & M32) << 32))
    cw, W = W >> 64, W & M64
    if cw:
        assert W < 59 * 60
        W = _add_lo(W, FIX["mulv"])
    return W, cw


def shift32(B):
    """bsgs64.h shift32: B 2^32 mod p, < 2^64.  Returns (r, wrapped)."""
    r = (B >> 32) * 59 + ((B << 32) & M64)
    cw, r = r >> 64, r & M64
    r = cw * FIX["shift32"] + r
    assert r <= M64                        # "the second mad cannot wrap"
    return r, cw


def _fold(t, th):
    """V = (t0:t1) + 59 th, +59 into the low word after a wrap."""
    V = th * 59 + t
    cw, V = V >> 64, V & M64
    if cw:
        assert V < 59 * 60
        V = _add_lo(V, FIX["fold"])
    return V, cw


def tmul(t, th, x):
    """encode.hip tmul64_asm: t-form in and out.  Returns (t, th, wrapped)."""
    V, cw = _fold(t, th)
    E, F = _prod(V, x)
    return (E & M32) | ((F & M32) << 32), F >> 32, cw


def chain(start, step, K):
    """encode.hip chain64<K>: the K accumulated t-form values start step^k, and
    for each of the K - 1 steps whether its fold wrapped."""
    t, th, vals, wraps = start, 0, [], []
    for k in range(K):
        vals.append(t + (th << 64))
        if k + 1 < K:
            t, th, cw = tmul(t, th, step)
            wraps.append(cw)
    return vals, wraps


def vfold64(t, th):
    """encode.hip vfold64.  Returns (v, wrapped)."""
    v = (t + th * 59) & M64
    if v < t:
        return v + FIX["vfold64"], 1
    return v, 0


def group_powers(x, G):
    """encode.hip group_powers64<G>: the folded x^1 .. x^G (lane j starts at
    [j], the step is [G - 1]) and the events (site, power, wrapped)."""
    t, th, out, ev = x, 0, [x], []
    for g in range(1, G):
        t, th, cw = tmul(t, th, x)
        ev.append(("fold", g, cw))
        v, w = vfold64(t, th)
        ev.append(("vfold64", g + 1, w))
        out.append(v)
    return out, ev


def mul64_lazy(a, b, c=0):
    """field.h mul64_lazy (c = 0) / mad64_lazy.  Returns (r, wrapped)."""
    H, L = divmod(a * b + c, 2**64)
    th, tl = divmod(H * 59 + L, 2**64)
    uh, ul = divmod(th * 59 + tl, 2**64)
    assert uh <= 1 and ul + 59 * uh <= M64
    return ul + 59 * uh, uh


def host_walk(x, t):
    """host.cpp power_walk<F64> without AVX-512: x^1 .. x^t as lazy values, and
    how many of its mul64_lazy took the wrap branch."""
    n = 0

    def mul(a, b):
        nonlocal n
        r, w = mul64_lazy(a, b)
        n += w
        return r
    out = []
    if t < 8:
        y = x
        for _ in range(t):
            out.append(y)
            y = mul(y, x)
        return out, n
    p = [x, 0, 0, 0]
    for j in range(1, 4):
        p[j] = mul(p[(j - 1) // 2], p[j // 2])
    xc = p[3]
    while len(out) + 4 <= t:
        out += p
        p = [mul(v, xc) for v in p]
    return (out + p)[:t], n


# ----------------------------------------------------- the encode schedules
def chain_shape(t):
    """enc_chain<40, K64_G1, K64_GN>: (G, K) of the power chain at threshold t."""
    G = 1
    while -(-t // G) > 40:
        G *= 2
    ks = (1, 2, 4, 8, 12, 16, 20, 24, 32, 40) if G == 1 else (12, 16, 20, 24, 32, 40)
    return G, next(k for k in ks if k >= -(-t // G))


def schedule_of(t):
    """enc64: the kernel family of threshold t (while n / grid < 2^30; above, the chain at every t).
    ("chain", G, K) | ("serial4", NA) | ("serial8", NA) | ("passes", [(base, NA, middle)])"""
    if t <= 13:
        return ("chain",) + chain_shape(t)
    if t <= 80:
        if t <= 36 and (t + 3) // 4 in (4, 5, 7, 9):
            return ("serial4", (t + 3) // 4)
        return ("serial8", (t + 7) // 8)
    npass, passes, base = (t - 80 + 79) // 80, [], 80
    for p in range(1, npass + 1):
        tp = min(80, t - base)
        passes.append((base, (tp + 7) // 8, p < npass))
        base += tp
    return ("passes", passes)


def serial(x, nbt, na, handoff=False):
    """bsgs64::body step 1 (serial) and the owner waves' shift32 of step 3:
    babies B_b = x^b (b = 1..nbt), giants A_a = x^(nbt a) (a = 1..na - 1), the
    hand-off x^(nbt na).  Returns (babies, shifted babies, giants incl. A_1,
    hand-off or None, events)."""
    ev, V, bb = [], x, [x]
    for b in range(2, nbt + 1):
        V, w = mulv(V, x)
        ev.append(("baby", b, w))
        bb.append(V)
    g, ga = V, [V]
    for a in range(2, na):
        V, w = mulv(V, g)
        ev.append(("giant", nbt * a, w))
        ga.append(V)
    out = None
    if handoff:
        out, w = mulv(V, g)
        ev.append(("handoff", nbt * na, w))
    sh = []
    for b, B in enumerate(bb, 1):
        s, w = shift32(B)
        ev.append(("shift32", b, w))
        sh.append(s)
    return bb, sh, ga, out, ev


def offset_pass(x, xbase, base, na, handoff):
    """An offset pass with the x^base cache (XC bit 0): the babies again, giants
    x^(base + 8a), a = 0..na - 1, the hand-off x^(base + 8 na) of a middle pass."""
    bb, sh, _, _, ev = serial(x, 8, 2)
    ev = [e for e in ev if e[0] != "giant"]
    g, V, ga = bb[7], xbase, [xbase]
    for a in range(1, na):
        V, w = mulv(V, g)
        ev.append(("offset", base + 8 * a, w))
        ga.append(V)
    out = None
    if handoff:
        out, w = mulv(V, g)
        ev.append(("offset", base + 8 * na, w))
    return bb, sh, ga, out, ev


def pow_sqm(x8, base):
    """x^base by square-and-multiply from x^8 (an offset pass without the cache:
    enc_passes_chunk takes it only when the scratch for the cache cannot grow)."""
    q, r, sq, have = base // 8, 0, x8, False
    while True:
        if q & 1:
            r = mulv(r, sq)[0] if have else sq
            have = True
        q >>= 1
        if not q:
            return r
        sq = mulv(sq, sq)[0]


def _mac(B, Bsh, A):
    """step 3: A B == B a0 + Bsh a1 (the carries are counted, nothing is lost)."""
    return (B * (A & M32) + Bsh * (A >> 32)) % P


def run_schedule(x, t):
    """The operands of every pass of threshold t's BSGS kernels: ([(babies,
    shifted babies, giants)], events)."""
    sch = schedule_of(t)
    if sch[0] in ("serial4", "serial8"):
        bb, sh, ga, _, ev = serial(x, 4 if sch[0] == "serial4" else 8, sch[1])
        return [(bb, sh, ga)], ev
    bb, sh, ga, xb, ev = serial(x, 8, 10, True)
    rows = [(bb, sh, ga)]
    for base, na, middle in sch[1]:
        bb, sh, ga, xb, e = offset_pass(x, xb, base, na, middle)
        rows.append((bb, sh, ga))
        ev += e
    return rows, ev


def encode_one(x, t):
    """(x^1 .. x^t mod p as the kernels of threshold t compute them, events)."""
    sch = schedule_of(t)
    if sch[0] == "chain":
        _, G, K = sch
        if G == 1:
            vals, wraps = chain(x, x, K)
            return [v % P for v in vals[:t]], [("fold", k + 1, w) for k, w in enumerate(wraps)]
        return encode_group(x, t, G, K)
    rows, ev = run_schedule(x, t)
    out = [B % P for B in rows[0][0]]              # the a = 0 row of pass 0
    for i, (bb, sh, ga) in enumerate(rows):
        for A in ga:
            out += [_mac(B, s, A) for B, s in zip(bb, sh)]
    return out[:t], ev


def encode_group(x, t, G, K):
    """k_encode_u64_gn<G, K>: lane j's chain from x^(j+1) by x^G."""
    pw, ev = group_powers(x, G)
    out = [0] * (G * K)
    for j in range(G):
        vals, _ = chain(pw[j], pw[G - 1], K)
        for k, v in enumerate(vals):
            out[j + k * G] = v % P
    return out[:t], ev


def labels_for(t):
    """The fixture entries (schedule, site, power) whose product the kernels of
    threshold t compute and whose result reaches one of the t sums."""
    sch = schedule_of(t)
    if sch[0] == "chain":
        if sch[1] != 1:
            return [("group", "vfold64", g) for g in range(2, sch[1] + 1)]
        return [("chain", "fold", j) for j in range(2, t)]     # the fold of x^j feeds x^(j+1)
    if sch[0] in ("serial4", "serial8"):
        nbt = 4 if sch[0] == "serial4" else 8
        return ([(sch[0], "baby", b) for b in range(2, nbt + 1)] +
                [(sch[0], "giant", nbt * a) for a in range(2, sch[1])] +
                [(sch[0], "shift32", b) for b in range(1, nbt + 1)])
    out = labels_for(80) + [("serial8", "handoff", 80)]
    for base, na, middle in sch[1]:
        out += [("offset", "offset", base + 8 * a) for a in range(1, na + (1 if middle else 0))]
    return out


# ---------------------------------------------------------- the root tests
def horner_host(coeffs, x):
    """host.cpp root64: r <- mad64_lazy(r, x, c_i).  Returns (r, [wrapped])."""
    r, ws = 1, []
    for c in coeffs:
        r, w = mul64_lazy(r, x, c)
        ws.append(w)
    return r, ws


def horner_step(V, x, c):
    """decode.hip horner64_step: mulv, then + c with 2^64 == 59."""
    V, w = mulv(V, x)
    r = V + c
    cy, r = r >> 64, r & M64
    r += 59 * cy
    assert r <= M64
    return r, w


def horner_dev(coeffs, x):
    """decode.hip is_root64.  Returns (r, [the mulv of each step wrapped])."""
    r, ws = 1, []
    for c in coeffs:
        r, w = horner_step(r, x, c)
        ws.append(w)
    return r, ws


def bsgs_table(coeffs):
    """rootset.h rt64_bsgs_table: out[3k + j] = p_k 2^(22 j) mod p."""
    d = len(coeffs)
    nblk = d // 8 + (1 if d % 8 else 0)
    out = []
    for k in range(8 * nblk):
        pk = 0 if k > d else 1 if k == d else coeffs[d - k - 1]
        out += [pk % P, (pk << 22) % P, (pk << 44) % P]
    return out


def _rt_block(tab, a, limbs):
    slo = shi = 0
    for b in range(1, 8):
        for j in range(3):
            c = tab[(a * 8 + b) * 3 + j]
            slo += limbs[b - 1][j] * (c & M32)
            shi += limbs[b - 1][j] * (c >> 32)
    assert slo < 2**59 and shi < 2**59
    v = slo + ((shi & M32) << 32) + (shi >> 32) * 59 + tab[a * 24]     # rt_limb_sum
    r, top = v & M64, v >> 64
    q = (r + top * 59) & M64
    return q + 59 if q < r else q


def root_bsgs(coeffs, x):
    """decode.hip is_root64_bsgs.  Returns (R, events): ("baby", b, wrapped) for
    x^2 .. x^8, ("giant", a, wrapped) for the product R x^8 in front of block a."""
    d = len(coeffs)
    tab, nf, top = bsgs_table(coeffs), d // 8, d % 8 != 0
    V, limbs, ev = x, [], []
    for b in range(1, 8):
        if b > 1:
            V, w = mulv(V, x)
            ev.append(("baby", b, w))
        limbs.append((V & 0x3FFFFF, (V >> 22) & 0x3FFFFF, V >> 44))
    g, w = mulv(V, x)
    ev.append(("baby", 8, w))
    R = _rt_block(tab, nf, limbs) if top else 1
    for a in range(nf - 1, -1, -1):
        q = _rt_block(tab, a, limbs)
        R, w = mulv(R, g)
        ev.append(("giant", a, w))
        R += q
        if R > M64:
            R = (R & M64) + 59                                         # rt_add64
    return R, ev


def poly_eval(coeffs, x):
    """The monic polynomial x^d + c_1 x^(d-1) + .. + c_d at x, mod p."""
    r = 1
    for c in coeffs:
        r = (r * x + c) % P
    return r


def _filler(seed, n):
    """n deterministic coefficients (an LCG mod p; any values do)."""
    out, v = [], seed % P
    for _ in range(n):
        v = (v * 6364136223846793005 + 1442695040888963407) % P
        out.append(v)
    return out


def poly_horner(x, d, i, model, seed=1):
    """A degree-d monic polynomial with root x whose Horner step i (1-based)
    wraps in `model`: for horner_host the mad r_(i-1) x + c_i is a small value
    (c_i solved, 1 <= i < d); for horner_dev the product r_(i-1) x is (c_(i-1)
    solved, 2 <= i <= d).  c_d is solved for P(x) == 0.  None if no small value
    wraps for this x."""
    inv, j = pow(x, -1, P), i if model is horner_host else i - 1     # the coefficient solved: c_j
    assert 1 <= j < d
    for r in SMALL:
        c = _filler(seed + r, d)
        pre = poly_eval(c[:j - 1], x)                                  # r_(j-1)
        c[j - 1] = ((r if model is horner_host else r * inv) - pre * x) % P
        c[d - 1] = 0
        c[d - 1] = (-poly_eval(c, x)) % P
        if model(c, x)[1][i - 1]:
            return c
    return None


def poly_bsgs(x, d, block, seed=1):
    """A degree-d monic polynomial with root x whose product R x^8 in front of
    block `block` (the kernel's Horner in x^8) wraps in root_bsgs: the constant
    of block `block` + 1 is solved for R == r / x^8, p_0 for P(x) == 0."""
    nf, top = d // 8, d % 8 != 0
    assert 0 <= block < nf and (block + 1 < nf or top)
    inv8 = pow(x, -8, P)
    k = 8 * (block + 1)                    # the coefficient solved: p_k = coeffs[d - k - 1]
    for r in SMALL:
        c = _filler(seed + r, d)
        c[d - k - 1] = 0
        # R in front of `block` is the Horner value of the terms of degree >= k, divided by x^k
        hi = (pow(x, d, P) + sum(c[d - j - 1] * pow(x, j, P) for j in range(k, d))) * pow(x, -k, P) % P
        c[d - k - 1] = (r * inv8 - hi) % P
        c[d - 1] = 0
        c[d - 1] = (-poly_eval(c, x)) % P
        _, ev = root_bsgs(c, x)
        if ("giant", block, 1) in ev:
            return c
    return None


# ------------------------------------------------------------- the fixture
def _order(k):
    """The order D of the largest subgroup on which x -> x^k is a bijection."""
    D = P - 1
    g = math.gcd(k, D)
    while g > 1:
        D //= g
        g = math.gcd(k, D)
    return D


def power_roots(k):
    """(r, x) with x^k == r for the small r that have such an x in the subgroup."""
    D = _order(k)
    e = pow(k, -1, D)
    for r in SMALL:
        if pow(r, D, P) == 1:
            x = pow(r, e, P)
            assert pow(x, k, P) == r
            yield r, x


def _take(k, events_of, want):
    """The first NIDS x with x^k small whose schedule has the event `want`."""
    ids = []
    for _, x in power_roots(k):
        if want in events_of(x) and x not in ids:
            ids.append(x)
            if len(ids) == NIDS:
                break
    assert len(ids) >= 4, (k, want, len(ids))
    return ids


def _shift_ids(b, nbt):
    """ids whose baby b wraps in shift32: b-th roots of B = (hi : 2^32 - d)."""
    ids, D = [], _order(b)
    e = pow(b, -1, D)
    for i in range(1, 4000):
        B = ((M32 - 977 * i) << 32) | (2**32 - 1 - i % 58)
        if pow(B, D, P) != 1:
            continue
        x = pow(B, e, P)
        if ("shift32", b, 1) in serial(x, nbt, 2)[4] and x not in ids:
            ids.append(x)
            if len(ids) == NIDS:
                break
    assert len(ids) >= 4, (b, nbt, len(ids))
    return ids


def generate():
    entries = []

    def add(schedule, site, power, ids):
        entries.append({"schedule": schedule, "site": site, "power": power, "ids": [str(x) for x in ids]})

    for name, nbt, na in (("serial8", 8, 10), ("serial4", 4, 9)):
        ev = lambda x: serial(x, nbt, na, nbt == 8)[4]
        for b in range(2, nbt + 1):
            add(name, "baby", b, _take(b, ev, ("baby", b, 1)))
        for a in range(2, na):
            add(name, "giant", nbt * a, _take(nbt * a, ev, ("giant", nbt * a, 1)))
        if nbt == 8:
            add(name, "handoff", 80, _take(80, ev, ("handoff", 80, 1)))
        for b in range(1, nbt + 1):
            add(name, "shift32", b, _shift_ids(b, nbt))
    for j in range(2, 13):      # the fold of x^j in front of the product x^(j+1), t <= 13: K <= 16
        add("chain", "fold", j, _take(j, lambda x: [("fold", k + 1, w) for k, w in enumerate(chain(x, x, 16)[1])],
                                      ("fold", j, 1)))
    for g in range(2, 9):       # vfold64 of x^g: the chains with lane groups (G = 2, 4, 8)
        add("group", "vfold64", g, _take(g, lambda x: group_powers(x, 8)[1], ("vfold64", g, 1)))
    ev300 = lambda x: run_schedule(x, 300)[1]
    for k in list(range(88, 241, 8)) + list(range(248, 297, 8)):
        add("offset", "offset", k, _take(k, ev300, ("offset", k, 1)))
    return {"p": str(P), "ids_per_entry": NIDS, "entries": entries}


def dumps(obj):
    return json.dumps(obj, indent=1) + "\n"


def load():
    """{(schedule, site, power): [ids]} of the committed fixture."""
    with open(FIXTURE) as f:
        doc = json.load(f)
    return {(e["schedule"], e["site"], e["power"]): [int(x) for x in e["ids"]] for e in doc["entries"]}


def main():
    with open(FIXTURE, "w") as f:
        f.write(dumps(generate()))


if __name__ == "__main__":
    main()
