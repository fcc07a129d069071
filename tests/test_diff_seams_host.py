"""tests/diff_seam_cases.py without a GPU: the table means what it says, and its cases bite.
  * the geometry the module restates gives, for every case, the branch the case is named for (numbers written out here by hand);
  * where the host-only code exposes a number -- kDiffStripRows, kDiffChainFrames, decode_batch_plan's strips and steps
    (tests/sanitize/diff_seam_plan_test.cpp, built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer) -- the table agrees;
  * no case rests on a mean that happens to be 0: the oracle's encoded volume differs from the input at the last voxel of a rewritten
    run and equals it everywhere the stage does not reach;
  * the numpy model of the chain's strip schedule equals the oracle's decode on every chain case, and its wrong variants -- the halo one
    row short, the second item slot dropped, the reach one column longer or shorter -- are caught by the cases meant to catch them; the
    first wrong voxel of each is printed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import diff_seam_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sqeazy_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=97:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")

CHAIN_CASES = [c for c in D.CASES if c["decode"]["route"] == "chain_frames"]
_enc = {}


def _encoded(oracle, case):
    if case["name"] not in _enc:
        _enc[case["name"]] = oracle.diff3x3x1_encode(D.volume(case))
    return _enc[case["name"]]


# what each case is for, by hand: (encode route, side_w, rows per block, lanes used of threads per row | decode route, w, item slots,
# launches, frames of the last launch)
WANT = {
    "10x5x10-random": ("rows", 0, 1, None, "generic", 0, 0, 0, 0),
    "11x5x10-random": ("generic", 0, 0, None, "generic", 0, 0, 0, 0),
    "12x5x10-random": ("generic", 0, 0, None, "generic", 0, 0, 0, 0),
    "9x4x24-random": ("rows", 0, 1, None, "chain_frames", 16, 1, 1, 8),
    "10x4x24-random": ("rows", 0, 1, None, "chain_frames", 16, 1, 2, 1),
    "3x3x2048-random": ("rows", 0, 1, None, "chain_frames", 8, 1, 1, 2),
    "3x3x2056-random": ("rows", 0, 1, None, "chain_frames", 8, 1, 1, 2),
    "3x64x256-random": ("side", 128, 16, (16, 16), "chain_frames", 8, 1, 1, 2),
    "128x3x256-random": ("side", 128, 16, (16, 16), "chain_frames", 128, 1, 16, 7),
    "129x32x256-random": ("side", 128, 16, (16, 16), "chain_frames", 136, 1, 16, 8),
    "130x16x256-random": ("rows", 0, 1, None, "chain_frames", 136, 1, 17, 1),
    "130x16x512-random": ("side", 256, 8, (32, 32), "chain_frames", 136, 1, 17, 1),
    "64x5x256-random": ("side", 128, 16, (16, 16), "chain_frames", 64, 1, 8, 7),
    "64x17x256-random": ("side", 128, 16, (16, 16), "chain_frames", 64, 1, 8, 7),
    "272x3x512-random": ("side", 384, 4, (48, 64), "chain_frames", 272, 2, 34, 7),
    "63x5x256-random": ("rows", 0, 1, None, "chain_frames", 64, 1, 8, 6),
    "14x5x16-random": ("rows", 0, 1, None, "chain_frames", 16, 1, 2, 5),
    "14x5x24-random": ("rows", 0, 1, None, "chain_frames", 16, 1, 2, 5),
    "16x5x24-random": ("rows", 0, 1, None, "chain_frames", 16, 1, 2, 7),
    "17x5x24-random": ("rows", 0, 1, None, "chain_frames", 24, 1, 2, 8),
    "17x33x16-random": ("generic", 0, 0, None, "generic", 0, 0, 0, 0),
    "18x33x16-random": ("generic", 0, 0, None, "generic", 0, 0, 0, 0),
    "17x33x24-random": ("rows", 0, 1, None, "chain_frames", 24, 1, 2, 8),
    "18x33x24-random": ("rows", 0, 1, None, "chain_frames", 24, 1, 3, 1),
    "176x3x176-random": ("rows", 0, 1, None, "chain_frames", 176, 2, 22, 7),
    "170x35x176-random": ("rows", 0, 1, None, "chain_frames", 176, 2, 22, 1),
    "170x40x176-random": ("rows", 0, 1, None, "chain_frames", 176, 2, 22, 1),
    "320x3x320-random": ("rows", 0, 1, None, "chain_frames", 320, 2, 40, 7),
    "313x34x320-random": ("rows", 0, 1, None, "chain_frames", 320, 2, 39, 8),
    "321x3x328-random": ("rows", 0, 1, None, "chain_per_frame", 328, 0, 320, 1),
}


def test_every_case_reaches_the_branch_it_is_named_for():
    assert len({c["name"] for c in D.CASES}) == len(D.CASES)
    assert max(int(np.prod(c["shape"])) for c in D.CASES) == 313 * 34 * 320                  # the largest: 3.4 M voxels
    for name, (er, sw, rpb, lanes, dr, w, slots, launches, last) in WANT.items():
        c = D.BY_NAME[name]
        e, d = c["encode"], c["decode"]
        assert (e["route"], e["side_w"], e["rows_per_block"]) == (er, sw, rpb), D.describe(c)
        if lanes:
            assert (e["lanes_used"], e["threads_per_row"]) == lanes, D.describe(c)
        assert (d["route"], d["w"], d["item_slots"], d["launches"], d["last_frames"]) == (dr, w, slots, launches, last), D.describe(c)
        assert not c["single"], name
    # (Z, 33, 16), Z = 2 .. 10: 1 .. 8 frames in one launch, then a second launch of one frame; two strips, the second of one row
    for Z in range(2, 11):
        d = D.BY_NAME["%dx33x16-random" % Z]["decode"]
        assert (d["route"], d["launches"], d["last_frames"], d["strips"]) == ("chain_frames", 1 if Z < 10 else 2, (Z - 2) % 8 + 1, 2), Z
    for Y, strips in ((3, 1), (4, 1), (31, 1), (32, 1), (33, 2), (64, 2), (65, 3)):
        d = D.BY_NAME["10x%dx16-random" % Y]["decode"]
        assert (d["route"], d["w"], d["launches"], d["strips"]) == ("chain_frames", 16, 2, strips), Y
    # the boundary of the rows kernel: hx + 2 <= X
    assert [D.rows_geometry(s) for s in ((10, 5, 10), (11, 5, 10), (12, 5, 10))] == [True, False, False]
    # full and partial vectors, one and two blocks per row
    assert [D.BY_NAME["4x3x%d-random" % X]["encode"]["lanes_used"] for X in (8, 9, 15, 16, 17)] == [1, 2, 2, 2, 3]
    assert [D.BY_NAME["3x3x%d-random" % X]["encode"]["bx"] for X in (2048, 2056)] == [1, 2]
    # the side path: whole tiles, a block whose rows run past Y, the near misses
    for c in D.SIDE_CASES:
        Z, Y, X = c["shape"]
        assert (Z * Y * X) % D.TILE_VOXELS == 0 or c["name"].startswith("63x5x256"), c["name"]
    assert D.BY_NAME["64x5x256-random"]["encode"]["by"] == 1 and D.BY_NAME["64x17x256-random"]["encode"]["by"] == 2
    assert D.BY_NAME["272x3x512-random"]["encode"]["by"] == 1                                   # Y = 3 < rpb = 4
    assert D.encode_route((64, 5, 256), source_aligned=False)["route"] == "rows"
    assert D.encode_route((64, 5, 256), bitswap1_behind=False)["route"] == "rows"
    # the widest chain: the LDS term binds at 320, the item term would allow 328
    assert D.frames_fit(320) and not D.frames_fit(328)
    assert D.IMAGE_ROWS * (328 // 8 + 1) <= D.CHAIN_ITEMS * D.CHAIN_THREADS < D.IMAGE_ROWS * (336 // 8 + 1)
    assert D.IMAGE_ROWS * (160 // 8 + 1) <= D.CHAIN_THREADS < D.IMAGE_ROWS * (168 // 8 + 1)    # the second slot: from w = 168
    # the batch calls
    assert all(D.batch_joint(D.BY_NAME[n]["shape"]) for n in D.BATCH_JOINT)
    assert [D.batch_joint(D.BY_NAME[n]["shape"]) for n in D.BATCH_MIXED] == [False, True]
    assert D.MISALIGNED in D.BY_NAME and all(n in D.BY_NAME for s in D.REACH_SETS for n in s)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_table_agrees_with_the_host_only_planner(tmp_path):
    """kDiffStripRows, kDiffChainFrames, and decode_batch_plan's strips, steps and widest chain for every case the joint chain takes"""
    exe = str(tmp_path / "diff_seam_plan_test")
    subprocess.check_call(["g++"] + SAN + [os.path.join(ROOT, "tests", "sanitize", "diff_seam_plan_test.cpp"), os.path.join(CSRC, "sqy_pipeline.cpp"),
                                          "-o", exe, "-lpthread"])
    cases = [c for c in D.CASES if D.batch_joint(c["shape"])]
    assert cases == CHAIN_CASES
    args = [str(v) for c in cases for v in c["shape"] + (c["decode"]["w"],)]
    r = subprocess.run([exe] + args, env=ENV, capture_output=True, text=True, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "diff_seam_plan ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.split("\n")
    assert lines[0] == "consts %d %d" % (D.STRIP_ROWS, D.CHAIN_FRAMES)
    for c, line in zip(cases, lines[1:]):
        d = c["decode"]
        assert line == "blob %d %d %d %d %d %d" % (c["shape"] + (d["strips"], d["launches"], d["w"])), (D.describe(c), line)
    assert lines[1 + len(cases)] == "group %d %d %d %d" % (len(cases), sum(c["decode"]["strips"] for c in cases), max(c["decode"]["launches"] for c in cases),
                                                            max(c["decode"]["w"] for c in cases))


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_no_case_rests_on_a_zero_mean(oracle, case):
    """on some touched row the encoded volume differs from the input at the last rewritten voxel; it equals the input at every voxel the
    stage does not reach, the first one behind each run among them; and the oracle's own decode restores the input"""
    vol, enc = D.volume(case), _encoded(oracle, case)
    touched = D.touched_mask(case["shape"]).reshape(vol.shape)
    assert np.array_equal(enc[~touched], vol[~touched]), D.failure(case, "rewritten outside the reach", D.first_difference(np.where(touched, vol, enc), vol))
    last, first = D.reach_edges(case["shape"])
    if case["hx"] == 0:                                     # two frames: nothing is rewritten at all
        assert case["shape"][0] == 2 and not len(last) and np.array_equal(enc, vol)
        return
    assert len(last) and len(first) == len(last)
    f_enc, f_vol = enc.reshape(-1), vol.reshape(-1)
    assert (f_enc[last] != f_vol[last]).any(), D.describe(case)
    assert (f_enc[first] == f_vol[first]).all(), D.describe(case)
    if D.rows_geometry(case["shape"]):                      # the columns, as the issue names them: hx the last rewritten, 1 + hx the first not
        hx = case["hx"]
        assert (enc[1:case["zlim"], 1:-1, hx] != vol[1:case["zlim"], 1:-1, hx]).any(), D.describe(case)
        assert np.array_equal(enc[:, :, 1 + hx], vol[:, :, 1 + hx]), D.describe(case)
    assert np.array_equal(oracle.diff3x3x1_decode(enc), vol), D.describe(case)


@pytest.mark.parametrize("case", CHAIN_CASES, ids=D.case_id)
def test_model_with_the_true_parameters_is_the_oracles_decode(oracle, case):
    got = D.chain_model(_encoded(oracle, case))
    diff = D.first_difference(got, D.volume(case))
    assert diff is None, D.failure(case, "the model of the strip schedule", diff)


def _wrong(oracle, case, what, **kw):
    """the first voxel a wrong variant of the model gets wrong (None: the case does not notice); printed"""
    diff = D.first_difference(D.chain_model(_encoded(oracle, case), **kw), D.volume(case))
    print(D.failure(case, what, diff) if diff else "%s: %s: not noticed" % (D.describe(case), what))
    return diff


def test_a_halo_one_row_short_shows_where_there_are_two_strips(oracle):
    for c in CHAIN_CASES:
        diff = _wrong(oracle, c, "halo one row short", halo_shift=-1)
        two = c["decode"]["strips"] > 1 and c["zlim"] > 2                               # a neighbour strip, and a frame that needs its rows
        assert (diff is not None) == two, D.describe(c)
        if diff:
            assert diff[1] % D.STRIP_ROWS in (0, D.STRIP_ROWS - 1), (D.describe(c), diff)     # the first wrong row lies at a strip's edge
    assert sum(c["decode"]["strips"] > 1 and c["zlim"] > 2 for c in CHAIN_CASES) >= 10


def test_a_dropped_second_item_slot_shows_on_the_wide_chains(oracle):
    """every case whose second slot holds a row of the volume notices; the cases whose second slot holds only rows past Y do not -- there
    the GPU test holds the kernel to leaving those items off"""
    noticed = []
    for c in CHAIN_CASES:
        if c["decode"]["item_slots"] < 2:
            continue
        diff = _wrong(oracle, c, "second item slot dropped", items=1)
        w, Y = c["decode"]["w"], c["shape"][1]
        first_row = D.CHAIN_THREADS // (w // 8 + 1) - D.CHAIN_FRAMES                     # volume row of strip 0's first item in slot 1
        live = first_row < min(Y, D.STRIP_ROWS + D.CHAIN_FRAMES - 1) and c["decode"]["launches"] > 0
        assert (diff is not None) == live, (D.describe(c), first_row)
        if diff:
            noticed.append(c["name"])
    assert {"170x40x176-random", "313x34x320-random"} <= set(noticed), noticed
    assert all(D.BY_NAME[n]["decode"]["w"] >= 176 for n in noticed)


@pytest.mark.parametrize("shift", [1, -1])
def test_a_reach_one_column_off_shows_on_both_sides_of_every_boundary(oracle, shift):
    for names in D.REACH_SETS:
        for n in names:
            c = D.BY_NAME[n]
            diff = _wrong(oracle, c, "reach one column %s" % ("longer" if shift > 0 else "shorter"), reach_shift=shift)
            assert diff is not None, D.describe(c)
            assert diff[:3] == (1, 1, c["hx"] + (1 if shift > 0 else 0)), (D.describe(c), diff)     # the first touched row's last column
    for c in CHAIN_CASES:                                   # .. and everywhere else where anything is rewritten
        if c["hx"] > 0:
            assert D.first_difference(D.chain_model(_encoded(oracle, c), reach_shift=shift), D.volume(c)) is not None, D.describe(c)
