"""CPU: the parse-lane picker (csrc/sqy_lanes.hpp: fewest calls leased, round robin among equals, release on error) built with g++
under AddressSanitizer + UndefinedBehaviorSanitizer, and the lane options of the loaded library.  No GPU, no hipcc."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=97:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_lane_picker(tmp_path):
    exe = str(tmp_path / "lane_picker_test")
    subprocess.check_call(["g++"] + SAN + [os.path.join(ROOT, "tests", "sanitize", "lane_picker_test.cpp"), "-o", exe])
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lane_picker ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]


def test_lane_options(sqy):
    """stage_lanes (0 never / 1 always / 2 where transpose_chain_caller_streams is on) and parse_lanes (1-8): names, ranges, defaults"""
    L = sqy.lib()
    assert sqy.get_option("stage_lanes") == 2 and sqy.get_option("parse_lanes") == 3
    assert L.SQYAMD_Set_Option(b"stage_lanes", 3) == 1 and L.SQYAMD_Set_Option(b"stage_lanes", -1) == 1
    assert L.SQYAMD_Set_Option(b"parse_lanes", 0) == 1 and L.SQYAMD_Set_Option(b"parse_lanes", 9) == 1
    with sqy.option("parse_lanes", 8), sqy.option("stage_lanes", 0):
        assert sqy.get_option("parse_lanes") == 8 and sqy.get_option("stage_lanes") == 0
    assert sqy.get_option("stage_lanes") == 2 and sqy.get_option("parse_lanes") == 3
