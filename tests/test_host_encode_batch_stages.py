"""Batch encode of quantiser->bitswap1->lz4 on the host, under AddressSanitizer + UndefinedBehaviorSanitizer, built with g++ as
test_host_batch_plan.py builds its target: the planner's classification and the plan with the per-volume table bytes
(tests/sanitize/encode_batch_form_test.cpp), and the LUT routine the batch_quantiser_lut kernel compiles, in its host form, against
sqy::quantiser_build_luts (tests/sanitize/quantiser_lut_test.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sqeazy_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=97:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("name, says", [("encode_batch_form_test", "encode_batch_form ok"), ("quantiser_lut_test", "quantiser_lut ok")])
def test_under_asan_ubsan(tmp_path, name, says):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++"] + SAN + [os.path.join(ROOT, "tests", "sanitize", name + ".cpp"), os.path.join(CSRC, "sqy_pipeline.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and says in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
