"""Native CPU check of the host plan of the per-flow quACK snapshots
(sidekick_amd/csrc/snapshots.h): tests/native/snapshot_plan_check.cpp compares
the cut arithmetic with a per-packet wrapping count, and the kernel chain of
snapshots.hip, restated on the host over the plan, with a per-flow model:
every row and final record written once and where the model puts it, no
scratch row read before it is written, every index inside what the entry
point allocates.  Edge shapes (empty flows, the u32 wrap, flows of one work
item +- 1 and of several, runs of empty flows) and random ones; once plain,
once as the same stand-alone program under ASan + UBSan."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "snapshot_plan_check.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def build(tag, flags):
    out = os.path.join(tempfile.gettempdir(), f"qk_snapshot_{tag}_{os.getpid()}")
    subprocess.run(["g++", "-std=c++17", *flags, "-o", out, SRC], check=True)
    return out


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "snapshot_plan_check: ok " in r.stdout, r.stdout
    return r.stdout


def test_plan_matches_the_per_packet_model():
    exe = build("check", ["-O2"])
    try:
        out = run(exe)
    finally:
        os.unlink(exe)
    assert int(out.split(": ok ")[1].split()[0]) > 1000


def test_plan_under_sanitizers():
    exe = build("san", ["-O1", *SAN])
    try:
        run(exe)
    finally:
        os.unlink(exe)
