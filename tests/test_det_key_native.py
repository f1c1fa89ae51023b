"""Host-only unit test of the detection postprocess's candidate key
(kernels/det_key.hpp, tests/native/det_key_test.cc): the key's order is the
reference's stable sort by score descending (edge values: the two zeros,
denormals, infinities, equal scores), it is injective in the index, never 0,
and gives the score back."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_native_det_key_unit_tests(tmp_path):
    exe = str(tmp_path / "det_key_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I" + os.path.join(ROOT, "band_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "det_key_test.cc"), "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
