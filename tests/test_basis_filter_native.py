"""Native CPU check of the id filter of the u32 t = 31..32 encode
(sidekick_amd/csrc/basis_filter.h): tests/native/basis_filter_check.cpp walks
all 2^32 ids on at most 16 threads (about 15 s) and checks that every id whose
lazy chain differs mod p from chain_exact is a candidate of the filter (no false
negative), that those ids are exactly the header's list (61, also committed as
tests/golden/basis_wrong_ids.json), and that the number of candidates is the
header's cap; the same stand-alone program once more under ASan + UBSan on the
first 2^24 ids."""
import json
import os
import re
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "basis_filter_check.cpp")
HDR = os.path.join(os.path.dirname(HERE), "sidekick_amd", "csrc", "basis_filter.h")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]
THREADS = str(max(1, min(16, os.cpu_count() or 1)))
SUMMARY = re.compile(r"enumerate: ok \(0 failures, (\d+) ids, (\d+) wrong, (\d+) flagged and right, "
                     r"(\d+) candidates, cap (\d+)\)")


def build(tag, flags):
    out = os.path.join(tempfile.gettempdir(), f"qk_basis_filter_{tag}_{os.getpid()}")
    subprocess.run(["g++", "-std=c++17", "-pthread", *flags, "-o", out, SRC], check=True)
    return out


@pytest.fixture(scope="module")
def exe():
    out = build("check", ["-O2"])
    yield out
    os.unlink(out)


@pytest.fixture(scope="module")
def exe_san():
    out = build("san", ["-O1", *SAN])
    yield out
    os.unlink(out)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "basis_wrong_ids.json")) as f:
        return json.load(f)


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert ": ok " in r.stdout, r.stdout[-2000:]
    return r.stdout


def listed(out, word):
    return [int(line.split()[1]) for line in out.splitlines() if line.startswith(word + " ")]


@pytest.fixture(scope="module")
def whole(exe):
    """the exhaustive run, once for the tests below"""
    return run(exe, "enumerate", str(2**32), THREADS)


def header_ids():
    with open(HDR) as f:
        text = f.read()
    body = text[text.index("WRONG[NWRONG] = {"):]
    return [int(x) for x in re.findall(r"(\d+)u", body[:body.index("};")])]


def test_table_as_built(exe):
    run(exe, "table")


def test_every_wrong_id_is_a_candidate_and_the_list_is_the_enumerated_set(whole, golden):
    ids, wrong, flagged, cand, cap = map(int, SUMMARY.search(whole).groups())
    assert ids == 2**32 and wrong == 61 and flagged == 122
    assert listed(whole, "wrong") == golden["wrong"] == header_ids()
    assert listed(whole, "flag") == golden["flagged_right"]


def test_candidate_fraction_below_the_header_cap(whole):
    _, _, _, cand, cap = map(int, SUMMARY.search(whole).groups())
    with open(HDR) as f:
        text = f.read()
    used = int(re.search(r"USED_SLOTS = (\d+);", text).group(1))
    assert cap == used * 36 + (4096 - used) * 32          # CANDIDATES as the header writes it
    assert 61 <= cand <= cap
    assert cap / 2**32 < 4e-5                              # under 1 % of the 256-id trips


def test_prefix_under_sanitizers(exe_san, golden):
    run(exe_san, "table")
    out = run(exe_san, "enumerate", str(2**24), THREADS)
    assert listed(out, "wrong") == [i for i in golden["wrong"] if i < 2**24] == [15362091]
    assert int(SUMMARY.search(out).group(1)) == 2**24
