#!/usr/bin/env python3
"""Static kernel stats from a gfx950 assembly file (hipcc -S / --save-temps).

    python tools/kstat.py FILE.s [NAME_SUBSTRING ...]

For every kernel whose mangled name contains one of the substrings: VGPR,
SGPR and spill counts from the metadata, and the instruction mix of its first
loop (the block from the first 'Loop Header' label to the branch back to it):
VALU / SALU totals, multiplies, s_nop count.  Not part of the product.

    python tools/kstat.py --compare OLD.s NEW.s [RENAMES.tsv]

Two builds of one source file, kernel by kernel: the resource figures of the
metadata, the text of every loop, and how many lines differ outside loops.
"""
import collections
import re
import sys


def kernels(text):
    return re.findall(r"^\s+\.name:\s+(\S+)\n", text, re.M)


def meta(text, name):
    k = text.find(".name:           " + name)
    a = text.rfind("  - .", 0, k)          # this kernel's metadata entry
    b = text.find("\n  - .", k)
    m = text[a:b if b > 0 else len(text)]
    get = lambda key: int(re.search(key + r":\s+(\d+)", m).group(1))
    return {"vgpr": get(r"\.vgpr_count"), "sgpr": get(r"\.sgpr_count"), "vspill": get(r"\.vgpr_spill_count"),
            "lds": get(r"\.group_segment_fixed_size")}


def loop_mix(text, name):
    i = text.find(name + ":")
    j = text.find(".Lfunc_end", i)
    body = [l for l in text[i:j].split("\n")]
    hdrs = [k for k, l in enumerate(body) if "Loop Header" in l]
    if not hdrs:
        return None
    h = hdrs[0]
    lab = body[h].split(":")[0]
    end = next((k for k in range(h, len(body)) if ("s_cbranch" in body[k] or "s_branch" in body[k])
                and lab in body[k]), len(body) - 1)
    seg = [l.strip() for l in body[h:end + 1]
           if l.strip() and not l.strip().startswith((";", ".")) and not l.strip().endswith(":")]
    c = collections.Counter(l.split()[0] for l in seg)
    valu = sum(v for k, v in c.items() if k.startswith("v_"))
    salu = sum(v for k, v in c.items() if k.startswith("s_") and k != "s_nop")
    mul = sum(v for k, v in c.items() if k.startswith(("v_mad_u64", "v_mul", "v_mad_u32", "v_lshl_add_u64")))
    return {"valu": valu, "mul": mul, "salu": salu, "nop": c["s_nop"], "insts": len(seg)}


# ---- compare mode ------------------------------------------------------------
META_KEYS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
             "group_segment_fixed_size")
MAY_FALL = ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")   # a lower figure is accepted


def meta_all(text, name):
    k = text.find(".name:           " + name + "\n")
    a = text.rfind("  - .", 0, k)
    b = text.find("\n  - .", k)
    m = text[a:b if b > 0 else len(text)]
    return {key: int(re.search(r"\." + key + r":\s+(\d+)", m).group(1)) for key in META_KEYS}


def norm_body(text, name):
    """The kernel's instructions and labels, comments and local label numbers
    taken out; a 'Loop Header' comment leaves the mark '@loop' on its label."""
    i = text.find("\n" + name + ":")
    j = text.find(".Lfunc_end", i)
    out = []
    for l in text[i + 1:j].split("\n")[1:]:
        hdr = "Loop Header" in l
        l = re.sub(r"\.LBB\d+_(\d+)", r".L\1", l.split(";")[0].strip())
        if not l or l.startswith("."):
            if not (l.startswith(".L") and l.endswith(":")):
                continue
        out.append(l + (" @loop" if hdr else ""))
    return out


def loops(body):
    """[(first, last)] line ranges: a loop header's label to the last branch back to it."""
    out = []
    for h, l in enumerate(body):
        if not l.endswith("@loop"):
            continue
        lab = l.split(":")[0]
        back = [k for k in range(h, len(body)) if re.match(r"s_c?branch\S*\s+" + re.escape(lab) + r"$", body[k])]
        out.append((h, back[-1] if back else h))
    return out


def renumber(lines):
    """Label numbers -> order of first appearance, so that equal code compares equal."""
    seen = {}
    f = lambda m: ".L%d" % seen.setdefault(m.group(0), len(seen))
    return [re.sub(r"\.L\d+", f, l) for l in lines]


REG = re.compile(r"\b([vsa])(?:(\d+)|\[(\d+):(\d+)\])(?![\w\[])")


def same_up_to_registers(xs, ys):
    """True if ys is xs with its registers renamed one to one (the same
    instructions, operands and labels otherwise; a range renames register by
    register)."""
    if len(xs) != len(ys):
        return False
    fwd, back = {}, {}
    for x, y in zip(xs, ys):
        if REG.sub("@", x) != REG.sub("@", y):
            return False
        for a, b in zip(REG.finditer(x), REG.finditer(y)):
            if a.group(1) != b.group(1):
                return False
            ra = range(int(a.group(2) or a.group(3)), int(a.group(2) or a.group(4)) + 1)
            rb = range(int(b.group(2) or b.group(3)), int(b.group(2) or b.group(4)) + 1)
            if len(ra) != len(rb):
                return False
            for i, j in zip(ra, rb):
                ki, kj = a.group(1) + str(i), b.group(1) + str(j)
                if fwd.setdefault(ki, kj) != kj or back.setdefault(kj, ki) != ki:
                    return False
    return True


def compare(old_text, new_text, renames):
    """Rows (old, new, meta verdict, loops, loops differing, of those differing
    by more than a one-to-one renaming of registers, lines differing outside loops)."""
    import difflib
    rows = []
    new_names = set(kernels(new_text))
    for old in kernels(old_text):
        new = renames.get(old, old)
        if new not in new_names:
            rows.append((old, new, "MISSING", 0, 0, 0, 0))
            continue
        mo, mn = meta_all(old_text, old), meta_all(new_text, new)
        notes = []
        for k in META_KEYS:
            if mn[k] == mo[k]:
                continue
            notes.append("%s %d -> %d%s" % (k, mo[k], mn[k], "" if k in MAY_FALL and mn[k] < mo[k] else " DEFECT"))
        bo, bn = norm_body(old_text, old), norm_body(new_text, new)
        lo, ln = loops(bo), loops(bn)
        pairs = [(renumber(bo[a:b + 1]), renumber(bn[c:d + 1])) for (a, b), (c, d) in zip(lo, ln)]
        bad = sum(x != y for x, y in pairs) + abs(len(lo) - len(ln))
        worse = sum(not same_up_to_registers(x, y) for x, y in pairs) + abs(len(lo) - len(ln))
        inloop = lambda rs, k: any(a <= k <= b for a, b in rs)
        oo = renumber([l for k, l in enumerate(bo) if not inloop(lo, k)])
        nn = renumber([l for k, l in enumerate(bn) if not inloop(ln, k)])
        outside = sum(1 for d in difflib.ndiff(oo, nn) if d[0] in "+-") if oo != nn else 0
        rows.append((old, new, "; ".join(notes) or "equal", len(lo), bad, worse, outside))
    return rows


def main_compare(argv):
    """python tools/kstat.py --compare OLD.s NEW.s [RENAMES.tsv]: every kernel of
    OLD.s against its pair in NEW.s (the same name, or the old -> new table of
    mangled names, one tab-separated pair per line), as a markdown table.
    Exit status 1 if a resource figure rose, a loop's text differs (a loop that
    differs only by a one-to-one renaming of registers is counted apart, and
    still fails) or a kernel has no pair."""
    old_text, new_text = open(argv[0]).read(), open(argv[1]).read()
    renames = dict(l.rstrip("\n").split("\t") for l in open(argv[2]) if l.strip()) if len(argv) > 2 else {}
    rows = compare(old_text, new_text, renames)
    print("| kernel (parent name) | resources | loops | loops differing | ... by more than register names | lines "
          "differing outside loops |")
    print("|---|---|---|---|---|---|")
    ok = True
    for old, new, verdict, nl, bad, worse, outside in rows:
        ok = ok and "DEFECT" not in verdict and verdict != "MISSING" and bad == 0
        print("| `%s`%s | %s | %d | %d | %d | %d |" %
              (old, "" if new == old else " -> `%s`" % new, verdict, nl, bad, worse, outside))
    same = sum(1 for r in rows if r[2] == "equal" and r[4] == 0 and r[6] == 0)
    print("\n%d kernels: %d identical, %d differing outside loops only, %d with a loop differing (%d by more than "
          "register names): %s" %
          (len(rows), same, sum(1 for r in rows if r[4] == 0 and (r[6] > 0 or r[2] != "equal")),
           sum(1 for r in rows if r[4] > 0), sum(1 for r in rows if r[5] > 0), "PASS" if ok else "FAIL"))
    return 0 if ok else 1


def main():
    if sys.argv[1] == "--compare":
        sys.exit(main_compare(sys.argv[2:]))
    text = open(sys.argv[1]).read()
    subs = sys.argv[2:]
    for name in kernels(text):
        if subs and not any(s in name for s in subs):
            continue
        try:
            m = meta(text, name)
        except AttributeError:
            continue
        print(name, m, loop_mix(text, name))


if __name__ == "__main__":
    main()
