"""Native CPU check of the host side of the queued sender step and its ingest
(sidekick_amd/csrc/sendersteps.h): tests/native/sender_steps_plan_check.cpp
restates the queue's CSR index and stable grouping, the round plan, every
carved buffer and LDS index against the sizes allocated, and the kernel chain
of sendersteps.hip round by round on the host, and compares every output with
a per-flow list model that takes one quACK per loop turn on a list it really
drains.  Edge shapes (interval ends on both sides of the work item boundaries,
b in one item and the stop in a later one, duplicates, resets in the middle of
a queue, runs of short flows) and random ones; once plain, once as the same
stand-alone program under ASan + UBSan."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "sender_steps_plan_check.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def build(tag, flags):
    out = os.path.join(tempfile.gettempdir(), f"qk_sender_steps_{tag}_{os.getpid()}")
    subprocess.run(["g++", "-std=c++17", *flags, "-o", out, SRC], check=True)
    return out


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sender_steps_plan_check: ok " in r.stdout, r.stdout
    return r.stdout


def test_chain_matches_the_per_packet_model():
    exe = build("check", ["-O2"])
    try:
        out = run(exe)
    finally:
        os.unlink(exe)
    assert int(out.split(": ok ")[1].split()[0]) > 500


def test_chain_under_sanitizers():
    exe = build("san", ["-O1", *SAN])
    try:
        run(exe)
    finally:
        os.unlink(exe)
