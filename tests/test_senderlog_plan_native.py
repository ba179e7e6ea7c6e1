"""Native CPU check of the sender log update's host plan
(sidekick_amd/csrc/senderlog.h): tests/native/senderlog_plan_check.cpp compares
offsets_out and the copy items with a literal per-flow list model over the edge
shapes (empty flows, drain equal to the segment, kept parts and new runs of
2047 / 2048 / 2049 / 4097 entries) and random ones; once plain, once as the
same stand-alone program under ASan + UBSan."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "senderlog_plan_check.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def build(tag, flags):
    out = os.path.join(tempfile.gettempdir(), f"qk_senderlog_{tag}_{os.getpid()}")
    subprocess.run(["g++", "-std=c++17", *flags, "-o", out, SRC], check=True)
    return out


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "senderlog_plan_check: ok " in r.stdout, r.stdout
    return r.stdout


def test_plan_matches_the_list_model():
    exe = build("check", ["-O2"])
    try:
        out = run(exe)
    finally:
        os.unlink(exe)
    assert int(out.split(": ok ")[1].split()[0]) > 300


def test_plan_under_sanitizers():
    exe = build("san", ["-O1", *SAN])
    try:
        run(exe)
    finally:
        os.unlink(exe)
