"""The Args functions (backend/hip/lower_args.{h,cc}) under AddressSanitizer and
UBSan, in a stand-alone program (tests/native/lower_args_test.cc) linked with
the TFLite reader, quant.cc and nothing of the executor: it reads the
malformed and the well-formed models of tests/lower_args_models.py from files
and calls the Args function of every op.  The run must end with status 0 and
without a sanitizer report, every malformed model refused with its reason."""
import os
import subprocess

from tests import lower_args_models as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "band_amd", "csrc")


def test_args_functions_under_sanitizers(tmp_path):
    models = {name: build() for name, (build, _, _) in L.MALFORMED.items()}
    models["families"] = L.families()
    models["float_families"] = L.float_families()
    paths = []
    for name, buf in models.items():
        paths.append(str(tmp_path / (name + ".tflite")))
        with open(paths[-1], "wb") as f:
            f.write(buf)
    exe = str(tmp_path / "lower_args_test")
    src = [os.path.join(ROOT, "tests", "native", "lower_args_test.cc")]
    src += [os.path.join(CSRC, "backend", "hip", f) for f in ("tflite_reader.cc", "lower_args.cc", "quant.cc")]
    src.append(os.path.join(CSRC, "compat", "band", "common.cc"))
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(CSRC, "compat"), "-I" + CSRC] + src +
                   ["-o", exe], check=True, timeout=600)
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    for name, (_, op, reason) in L.MALFORMED.items():
        want = "%s.tflite op %d " % (name, op)
        hit = [ln for ln in lines if want in ln]
        assert len(hit) == 1 and hit[0].endswith(": " + reason), (name, hit)
    for name in ("families", "float_families"):
        ours = [ln for ln in lines if "/%s.tflite op " % name in ln]
        assert ours and all(ln.endswith(": ok") or ln.endswith(": no Args function") for ln in ours), ours
        assert sum(ln.endswith(": ok") for ln in ours) >= 5
