"""Host-only unit test of the chain tuner's form descriptor
(backend/hip/chain_form.h, tests/native/chain_form_test.cc): Encode / Decode
round trip and injectivity over the candidate list and the forced forms, the
persisted integers against the table of the decode arithmetic they replaced,
the candidates' timing order."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_native_chain_form_unit_tests(tmp_path):
    exe = str(tmp_path / "chain_form_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "band_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "chain_form_test.cc"), "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
