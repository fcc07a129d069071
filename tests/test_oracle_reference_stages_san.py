"""The reference driver over the whole stage case table under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU: a stand-alone
program (tests/sanitize/ref_stages_san.cpp + oracle/ref_driver.cpp, built here with g++) that runs every case the goldens of
tests/golden/ref_stages.json and tests/golden/ref_shuffles.json were taken from, with 1 and 3 threads (the refused shuffle shapes too: the
driver must answer them without reaching the stand-in median), and the reference's quantiser on two volumes of
tests/quantiser_cases.py (LUTs and codes, the default weighting and both weighting functors).  A case on which the reference reads or writes out of bounds is
marked `undefined` in the table of oracle/gen_golden.py and is not among them.  Needs the reference tree: the program is built from it here.

UBSan's `shift` check is off, for two habits of the reference that it reports on every run and that change no result here:
  * bit masks built as ~(~0 << n) (bitplane_reorder_scalar.hpp:42 and :94, scalar_utils.hpp:79, compass.hpp:415): a left shift of a
    negative int, undefined before C++20 by the letter, two's complement on every compiler this is built with;
  * morton_at_ct<>::from (morton.hpp:145-147) shifts a 32-bit term by span_shift * 24 = 48 and 24 bits.  For coordinates below 256 --
    all that zcurve_reorder hands it, in-tile coordinates of tiles up to 128 -- the term shifted by 48 is the table entry of 0, which is
    0, so whatever the hardware does with the count, the code is that of the low span alone.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=97:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1",
           OMP_NUM_THREADS="3")


def _make(target):
    return subprocess.check_output(["make", "-s", "--no-print-directory", "-C", os.path.join(ROOT, "oracle"), target], text=True).split()


def test_reference_driver_over_the_table_under_asan_ubsan(tmp_path):
    from oracle import gen_golden
    reference, lz4_lib = _make("ref-tree")[0], _make("ref-lz4-lib")[0]
    if shutil.which("g++") is None or not os.path.isdir(reference) or not os.path.exists(lz4_lib):
        pytest.skip("the reference tree is not available here")
    n = gen_golden.dump_stage_cases(str(tmp_path / "cases"))
    exe = str(tmp_path / "ref_stages_san")
    # the driver's own compile flags (oracle/Makefile, `ref-flags`), plus the sanitizers
    cmd = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=shift", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    cmd += _make("ref-flags") + [os.path.join(ROOT, "tests", "sanitize", "ref_stages_san.cpp"), os.path.join(ROOT, "oracle", "ref_driver.cpp"),
                                 lz4_lib, "-o", exe]
    subprocess.check_call(cmd)
    r = subprocess.run([exe, str(tmp_path / "cases")], env=ENV, capture_output=True, text=True, timeout=600)
    assert r.returncode not in (97, 98) and r.returncode >= 0, (r.returncode, r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and ("ref_stages_san: %d cases, 0 failed" % n) in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    assert ("ref_stages_san: %d quantiser volumes, 0 failed" % len(gen_golden.QUANTISER_SAN_CASES)) in r.stdout, r.stdout[-2000:]
