"""The oracle's filter stages against the REFERENCE's own templates (oracle/ref_driver.cpp compiles the reference's utility headers in
place; tests/golden/ref_stages.json holds what they give for the case table of oracle/gen_golden.py):
  * everywhere: for every golden case the oracle's stage output hashes to the golden, the estimator's supports and threshold are
    equal exactly, and what the golden calls refused the oracle refuses;
  * where oracle/_ref loads: the oracle equals the live driver byte for byte on the table and on 200 seeded random shape and
    parameter draws per stage (extents <= 24), the reference run with 1 and 3 threads.
Stages: diff3x3x1 (uint16, uint8, the signed-char tail form), rmestbkrd, rmbkrd_neighbor5x5x5, zcurve_reorder, raster_reorder, bitswap1
(scalar and SSE branch as the reference routes them) and the histogram with its support."""
import hashlib
import os

import numpy as np
import pytest

import bkrd_restate as R
from ref_stage_inputs import load_cases
from oracle import gen_golden as G

HERE = os.path.dirname(os.path.abspath(__file__))
META, CASES = load_cases(os.path.join(HERE, "golden", "ref_stages.json"))
NUMBERS = ("supports", "threshold", "support")       # histogram: the bins and the support; no other statistic is pinned


def _ref():
    """the same skip as _ref() of test_oracle_golden.py; on top of it, a library that loads without the stage entry points is skipped only
    where it cannot be rebuilt (a prebuilt one from an older driver, no reference tree) and is an error everywhere else"""
    from oracle import ref
    if not ref.available():
        pytest.skip("oracle/_ref/libsqy_ref.so not available here")
    if not ref.stages_available():
        assert ref.reference_tree() is None, "oracle/_ref/libsqy_ref.so lacks stage entry points although it can be built here: %r" % (
            [f for f in ref.STAGE_ENTRY_POINTS if not hasattr(ref.lib(), f)],)
        pytest.skip("oracle/_ref/libsqy_ref.so was built from an older driver and cannot be rebuilt here")
    return ref


def test_table_and_golden_are_the_same_cases():
    rows = G.stage_table()
    assert [r["id"] for r in rows] == [c["id"] for c in CASES]
    for r, c in zip(rows, CASES):
        for k in ("stage", "dtype", "shape", "kind", "seed", "params"):
            assert r[k] == c[k], (r["id"], k)
        assert r.get("undefined") == c.get("undefined") and r.get("serial_only") == c.get("serial_only"), r["id"]
        assert ("sha256" in c) + ("refused" in c) + ("undefined" in c) == 1, c["id"]


def test_undefined_cases_stay_few():
    """per stage at most one case in ten may be `undefined` -- except where the reference itself cannot stay within that:
    rmbkrd_neighbor5x5x5 reads behind the volume for every shape whose X is not below Z (see the summary of the change that added this)"""
    for stage in {c["stage"] for c in CASES}:
        mine = [c for c in CASES if c["stage"] == stage]
        und = [c for c in mine if "undefined" in c]
        if stage == "rmbkrd_neighbor5x5x5":
            assert all(c["undefined"] == "neighbour_oob" and not G.neighbor5_reads_in_bounds(c["shape"]) for c in und)
        else:
            assert 10 * len(und) <= len(mine), stage
    assert not [c for c in CASES if c["stage"] == "diff3x3x1" and "undefined" in c]


def _no_voxel_decides(c):
    """cases whose payload is all zero whatever the stage's criterion does"""
    if c["kind"] in ("zero", "max"):                                    # nothing above the level / the level skips or removes everything
        return True
    if c["stage"] == "rmbkrd_neighbor5x5x5":
        Z, Y, X = c["shape"]
        walked = R.neighbor5_centres(c["shape"]).any() and (max(2, min(X - 2, Z)) - 2) * Z * Y * X > 0
        first_row_inside = 2 * Y * X + 2 * X + 2 < Z * Y * X          # the first row start lies in the volume
        return not (walked and first_row_inside) or c["params"]["threshold"] == np.iinfo(G.stage_volume(c).dtype).max
    return c["stage"] == "rmestbkrd" and c["kind"] == "equal_faces" and c["shape"][0] == 2      # two frames: both are faces


def test_payloads_depend_on_what_the_stage_decides():
    """an all-zero payload pins nothing: a product that skipped every voxel would give it too.  Only the cases meant to be empty may have it."""
    for c in CASES:
        if "sha256" in c and c["stage"] != "histogram" and c["sha256"] == hashlib.sha256(bytes(c["bytes"])).hexdigest():
            assert _no_voxel_decides(c), c["id"]
    wrap = [c for c in CASES if c["kind"] == "near_wrap" and "sha256" in c and not _no_voxel_decides(c)]
    assert len(wrap) >= 10


@pytest.mark.parametrize("stage", sorted({c["stage"] for c in CASES}))
def test_oracle_equals_the_golden(oracle, stage):
    ran = 0
    for c in CASES:
        if c["stage"] != stage or "undefined" in c:
            continue
        vol = G.stage_volume(c)
        assert hashlib.sha256(vol.tobytes()).hexdigest()[:12] == c["input_sha256"], c["id"]
        if "refused" in c:                                  # the product's policy (_meta.refused); the flag was taken from the oracle, so
            with pytest.raises(ValueError):                  # this only says that golden and oracle have not drifted apart since
                G.oracle_stage(c, vol)
            continue
        out, extra = G.oracle_stage(c, vol)
        assert len(out) == c["bytes"] and hashlib.sha256(out).hexdigest() == c["sha256"], c["id"]
        for k in NUMBERS:
            if k in c:
                assert extra[k] == c[k], (c["id"], k, extra[k], c[k])
        ran += 1
    assert ran


@pytest.mark.parametrize("stage", sorted({c["stage"] for c in CASES}))
def test_oracle_equals_the_live_reference_on_the_table(oracle, stage):
    _ref()
    for c in CASES:
        if c["stage"] != stage or "undefined" in c or "refused" in c:
            continue
        vol = G.stage_volume(c)
        want, extra = G.oracle_stage(c, vol)
        for nthreads in ((1,) if "serial_only" in c else (1, 3)):
            got, rextra = G.reference_stage(c, vol, nthreads)
            assert got == want, (c["id"], nthreads)
            for k in NUMBERS:
                if k in rextra:
                    assert extra[k] == rextra[k], (c["id"], k)
        assert hashlib.sha256(want).hexdigest() == c["sha256"], c["id"]


def _draw_shape(rng, lo=1):
    return [int(d) for d in rng.integers(lo, 25, 3)]


def _live(row):
    """1 when the case was compared, 0 when the oracle refuses it"""
    vol = G.stage_volume(row)
    try:
        want, extra = G.oracle_stage(row, vol)
    except ValueError:
        return 0
    for nthreads in ((1,) if "serial_only" in row else (1, 3)):
        got, rextra = G.reference_stage(row, vol, nthreads)
        assert got == want, (row, nthreads)
        for k in NUMBERS:
            if k in rextra:
                assert extra[k] == rextra[k], (row, k)
    back = None if row["stage"] == "histogram" else G.reference_stage_decode(row, np.frombuffer(want, vol.dtype).reshape(vol.shape))
    if back is not None:
        assert np.array_equal(back.reshape(vol.shape), vol), row
    return 1


def _row(stage, dtype, shape, kind, seed, **params):
    return {"stage": stage, "dtype": dtype, "shape": list(shape), "kind": kind, "seed": seed, "params": params}


def test_random_draws_diff3x3x1(oracle):
    _ref()
    rng = np.random.default_rng(20261018)
    ran = 0
    for k in range(200):
        dtype = ("uint16", "uint8", "char")[k % 3]
        kind = ("random", "ramp", "pm128", "max")[int(rng.integers(0, 4))]
        ran += _live(_row("diff3x3x1", dtype, _draw_shape(rng), kind, k))
    assert ran > 100


def test_random_draws_diff3x3x1_offsets(oracle):
    ref = _ref()
    rng = np.random.default_rng(7)
    for k in range(200):
        shape = _draw_shape(rng)
        try:
            offs, hx = oracle.diff3x3x1_offsets(shape)
        except ValueError:
            continue
        roffs, rhx = ref.diff3x3x1_offsets(shape)
        assert np.array_equal(offs, roffs), shape
        assert len(offs) == 0 or hx == rhx, shape


def test_random_draws_rmestbkrd(oracle):
    _ref()
    rng = np.random.default_rng(20261019)
    for k in range(200):
        kind = ("gamma", "two_level", "random", "equal_faces", "low80")[int(rng.integers(0, 5))]
        assert _live(_row("rmestbkrd", ("uint16", "uint8")[k % 2], _draw_shape(rng, 2), kind, k))


def test_random_draws_neighbor5(oracle):
    _ref()
    rng = np.random.default_rng(20261020)
    ran = 0
    for k in range(200):
        while True:                                             # the reference reads behind the volume unless X < Z, roughly
            shape = _draw_shape(rng, 5)
            if G.neighbor5_reads_in_bounds(shape):
                break
        t = int(rng.choice([0, 1, 20, 40, 79, 255, 65535, 70000]))
        f = float(rng.choice([0.0, 0.25, 0.5, 1.0]))
        kind = "near_wrap" if t == 70000 else "low80"
        ran += _live(_row("rmbkrd_neighbor5x5x5", ("uint16", "uint8")[k % 2], shape, kind, k, threshold=t, fraction=f))
    assert ran > 150


def test_random_draws_reorders(oracle):
    _ref()
    rng = np.random.default_rng(20261021)
    ran = {"zcurve_reorder": 0, "raster_reorder": 0}
    for k in range(200):
        shape = _draw_shape(rng)
        dtype = ("uint16", "uint8")[k % 2]
        ran["zcurve_reorder"] += _live(_row("zcurve_reorder", dtype, shape, "random", k, tile_size=int(rng.choice([2, 4, 8, 16]))))
        ran["raster_reorder"] += _live(_row("raster_reorder", dtype, shape, "random", k, tile_size=int(rng.choice([2, 3, 4, 5, 8, 16]))))
    assert min(ran.values()) > 50, ran


def test_random_draws_bitswap1(oracle):
    _ref()
    rng = np.random.default_rng(20261022)
    for k in range(200):
        n = int(rng.integers(1, 600)) if k % 4 else 128 * int(rng.integers(1, 40))
        dtype = ("uint16", "uint8")[k % 2]
        sse = dtype == "uint16" and n % 128 == 0
        row = _row("bitswap1", dtype, (1, 1, n), "random", k, offset_bytes=0 if sse else int(rng.choice([0, 1, 2, 6])) * (2 if dtype == "uint16" else 1))
        if not sse:
            row["serial_only"] = "race"
        assert _live(row)


def test_random_draws_histogram(oracle):
    _ref()
    rng = np.random.default_rng(20261023)
    for k in range(200):
        kind = ("gamma", "two_level", "random", "low80", "max")[int(rng.integers(0, 5))]
        assert _live(_row("histogram", ("uint16", "uint8")[k % 2], (1, 1, int(rng.integers(1, 3000))), kind, k))
