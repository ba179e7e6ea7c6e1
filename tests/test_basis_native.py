"""Native CPU check of the nine-power basis of the u32 t = 31..32 encode
(sidekick_amd/csrc/basis32.h): tests/native/basis_check.cpp checks the table's
invariants, runs the lazy chain with its redo and the table's terms against
pow32 on 10^6 random ids and the edge ids, and re-verifies that the committed
wrap ids (tests/golden/basis_wrap_ids.json, from the program's `find` mode)
wrap at the product they name; table and chain once more as the same
stand-alone program under ASan + UBSan."""
import json
import os
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "basis_check.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]
CHAIN_POWERS = (2, 3, 6, 8, 12, 13, 15, 16)


def build(tag, flags):
    out = os.path.join(tempfile.gettempdir(), f"qk_basis_{tag}_{os.getpid()}")
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
def wraps():
    with open(os.path.join(HERE, "golden", "basis_wrap_ids.json")) as f:
        return json.load(f)["wraps"]


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ": ok " in r.stdout, r.stdout
    return r.stdout


def test_table_invariants(exe):
    run(exe, "table")


def test_lazy_chain_with_redo_against_pow32(exe):
    out = run(exe, "chain")
    assert "1000000 ids" in out


def test_committed_wrap_ids_wrap_where_they_say(exe, wraps):
    assert {w["power"] for w in wraps} == set(CHAIN_POWERS)   # at least one id per product
    out = run(exe, "wraps", *[f"{w['power']}:{w['id']}" for w in wraps])
    assert f"{len(wraps)} ids" in out


def test_find_mode_reports_what_it_finds(exe):
    """`find` over a range too short to hold a wrap for every product ends
    with a failure status and names the count; the full search that produced
    the fixture takes tens of seconds and is not repeated here."""
    r = subprocess.run([exe, "find", "100000", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "basis_check find: FAIL" in r.stdout and "100000 ids searched" in r.stdout


def test_table_and_chain_under_sanitizers(exe_san):
    run(exe_san, "table")
    assert "1000000 ids" in run(exe_san, "chain")
