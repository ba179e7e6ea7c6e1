"""Native CPU check of the decode root test's pure host logic
(sidekick_amd/csrc/rootset.h): tests/native/rootset_check.cpp builds the hash
set of the roots in both layouts for 1 .. 256 roots of both id widths and looks
every root (and 1000 non-roots) up literally, pins the sizes at which the
compact set stops fitting the kernel arguments (56 roots u32, 40 u64), compares
the u64 baby-step/giant-step coefficient table with unsigned __int128
arithmetic, and reads hand-built images of the pinned result slots; once plain,
once as the same stand-alone program under ASan + UBSan."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "rootset_check.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def build(tag, flags):
    out = os.path.join(tempfile.gettempdir(), f"qk_rootset_{tag}_{os.getpid()}")
    subprocess.run(["g++", "-std=c++17", *flags, "-o", out, SRC], check=True)
    return out


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rootset_check: ok " in r.stdout, r.stdout
    return r.stdout


def test_rootset_matches_the_literal_models():
    exe = build("check", ["-O2"])
    try:
        out = run(exe)
    finally:
        os.unlink(exe)
    # 2 widths x 2 layouts x 256 sizes x (roots + 1000 non-roots) lookups at the least
    assert int(out.split(": ok ")[1].split()[0]) > 2 * 2 * 256 * 1000


def test_rootset_under_sanitizers():
    exe = build("san", ["-O1", *SAN])
    try:
        run(exe)
    finally:
        os.unlink(exe)
