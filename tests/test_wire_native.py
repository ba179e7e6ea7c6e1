"""Native CPU check of the wire leg's shared rules (sidekick_amd/csrc/wire.h):
tests/native/wire_check.cpp runs wire_validate — the one copy of the per-image
rules, the same function the ingest kernel runs — over every malformed and edge
image of the ingest tests, each at the end of an exactly sized heap block, and
compares the statuses with a table written out in the program; and wire_byte /
wire_dword, which the emit kernel gathers its stores from, with a literal
packer.  Once plain, once as the same stand-alone program under ASan + UBSan
(a read past an image's length is then an error)."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "wire_check.cpp")
INC = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "sidekick_amd", "csrc")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def build(tag, flags):
    out = os.path.join(tempfile.gettempdir(), f"qk_wire_{tag}_{os.getpid()}")
    subprocess.run(["g++", "-std=c++17", *flags, *INC, "-o", out, SRC], check=True)
    return out


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wire_check: ok " in r.stdout, r.stdout
    return r.stdout


def test_rules_match_the_table():
    exe = build("check", ["-O2"])
    try:
        out = run(exe)
    finally:
        os.unlink(exe)
    assert int(out.split(": ok ")[1].split()[0]) > 10000


def test_rules_under_sanitizers():
    exe = build("san", ["-O1", *SAN])
    try:
        run(exe)
    finally:
        os.unlink(exe)
