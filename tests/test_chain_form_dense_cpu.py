"""Host-only unit test of the chain form descriptor with the dense raster form
(backend/hip/chain_form.h, tests/native/chain_form_dense_test.cc): every
candidate the tuner times, with 3 and with 2 launches, encodes to a distinct
integer and decodes back; the integers of the forms that existed before are
listed literally and unchanged; the dense form is 8004 / 8014."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_native_chain_form_dense_unit_tests(tmp_path):
    exe = str(tmp_path / "chain_form_dense_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "band_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "chain_form_dense_test.cc"), "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
