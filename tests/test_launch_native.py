"""The launch record (backend/hip/launch.h) under AddressSanitizer and UBSan, in
a stand-alone program (tests/native/launch_test.cc) that includes that header
and nothing of the executor: every kind with its payload, the typed accessors,
copies and moves (the kConvGroup payload owns a vector).  The run must end with
status 0 and without a sanitizer report."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "band_amd", "csrc")


def test_launch_record_under_sanitizers(tmp_path):
    exe = str(tmp_path / "launch_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "native", "launch_test.cc"), "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith(": ok") and r.stdout.startswith("43 kinds, "), r.stdout[-2000:]
