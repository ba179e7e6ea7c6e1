"""Native CPU check of the host plan of the packet snapshots
(sidekick_amd/csrc/pktsnap.h): tests/native/pktsnap_plan_check.cpp compares the
epochs the plan cuts a batch into with the per-packet loop's Reset-free runs
(every pattern of up to ten packets, random batches with rare, dense and
consecutive Resets, a Reset first and last), and the two-level send-order rank
with a running count of the emitting packets; once plain, once as the same
stand-alone program under ASan + UBSan."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "pktsnap_plan_check.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def build(tag, flags):
    out = os.path.join(tempfile.gettempdir(), f"qk_pktsnap_{tag}_{os.getpid()}")
    subprocess.run(["g++", "-std=c++17", *flags, "-o", out, SRC], check=True)
    return out


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pktsnap_plan_check: ok " in r.stdout, r.stdout
    return r.stdout


def test_plan_matches_the_per_packet_loop():
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
