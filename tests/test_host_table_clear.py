"""Who empties the duplicate search's table of an encode call (lz4_table_clear_plan, csrc/sqy_pipeline.cpp) and where the in-place
transposer's stores of that clear land (lz4_table_clear_stores / lz4_table_clear_dword, sqy_pipeline.hpp -- the kernel calls the same two
functions) under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program, built with g++ as test_host_batch_layout.py
builds its target."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sqeazy_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=97:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_table_clear_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "table_clear_test")
    subprocess.check_call(["g++"] + SAN + [os.path.join(ROOT, "tests", "sanitize", "table_clear_test.cpp"), os.path.join(CSRC, "sqy_pipeline.cpp"), "-o", exe,
                                          "-lpthread"])
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "table_clear ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
