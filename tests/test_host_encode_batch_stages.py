"""Batch encode of quantiser->bitswap1->lz4 on the host, under AddressSanitizer + UndefinedBehaviorSanitizer, built with g++ as
test_host_batch_plan.py builds its target: the planner's classification and the plan with the per-volume table bytes
(tests/sanitize/encode_batch_form_test.cpp), and the LUT routine the batch_quantiser_lut kernel compiles, in its host form, against
sqy::quantiser_build_luts (tests/sanitize/quantiser_lut_test.cpp) -- and both of them against the oracle's tables on the histograms of
tests/quantiser_cases.py, where the walk rounds in binary32, meets ties and sees a count above 2^24 (the oracle is held to the reference's own
quantiser on those volumes by tests/test_oracle_reference_quantiser.py)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sqeazy_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=97:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")


_built = {}


def _exe(name, tmp_path_factory):
    """the sanitized program of tests/sanitize/<name>.cpp, built once per run"""
    if name not in _built:
        exe = str(tmp_path_factory.mktemp(name) / name)
        subprocess.check_call(["g++"] + SAN + [os.path.join(ROOT, "tests", "sanitize", name + ".cpp"), os.path.join(CSRC, "sqy_pipeline.cpp"), "-o", exe, "-lpthread"])
        _built[name] = exe
    return _built[name]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("name, says", [("encode_batch_form_test", "encode_batch_form ok"), ("quantiser_lut_test", "quantiser_lut ok")])
def test_under_asan_ubsan(tmp_path_factory, name, says):
    r = subprocess.run([_exe(name, tmp_path_factory)], env=ENV, capture_output=True, text=True, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and says in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_luts_on_the_case_table(tmp_path, tmp_path_factory, oracle):
    import quantiser_cases as Q
    cases = tmp_path / "cases"
    cases.mkdir()
    for k, name in enumerate(Q.NAMES):
        histo = Q.histogram(Q.volume(name))
        enc, dec = oracle.quantiser_build_luts(histo)
        histo.astype("<u4").tofile(str(cases / ("%d.histo" % k)))
        enc.tofile(str(cases / ("%d.enc" % k)))
        dec.astype("<u2").tofile(str(cases / ("%d.dec" % k)))
    (cases / "names.txt").write_text("\n".join(Q.NAMES) + "\n")
    r = subprocess.run([_exe("quantiser_lut_test", tmp_path_factory), str(cases)], env=ENV, capture_output=True, text=True, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and ("quantiser_lut table ok (%d histograms)" % len(Q.NAMES)) in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
