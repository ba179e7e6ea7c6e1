"""Native CPU check of the lazy product's remainder taken from the quotient
word (field.h mulfold32_min, r = Pl + 5 Qh): tests/native/lazy_product_check.cpp
compares it with the earlier form written out literally, on edge operands,
10^7 random pairs and the committed wrap ids run through the kernels' power
chains; once more as a stand-alone program under ASan + UBSan."""
import os
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "lazy_product_check.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def build(tag, flags):
    out = os.path.join(tempfile.gettempdir(), f"qk_lazy_product_{tag}_{os.getpid()}")
    subprocess.run(["g++", "-std=c++17", *flags, "-o", out, SRC], check=True)
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


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " ok " in r.stdout, r.stdout
    return r.stdout


def chains(exe, golden):
    for cfg, ids in golden["bsgs_wrap_ids"].items():
        nb, na = cfg.split("x")
        out = run(exe, "chain", nb, na, *[str(i) for i in ids])
        assert f"chain {cfg}: ok" in out


def test_new_form_equals_old_on_edges_and_random_pairs(exe):
    out = run(exe, "check")
    assert "10000000 pairs" in out


def test_wrap_ids_through_the_power_chains(exe, golden):
    chains(exe, golden)


def test_under_sanitizers(exe_san, golden):
    run(exe_san, "check")
    chains(exe_san, golden)
