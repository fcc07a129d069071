"""GPU: the product's stage-only pipelines through the C-ABI against what the REFERENCE's own templates give
(tests/golden/ref_stages.json, taken by oracle/gen_golden.py --stages from oracle/ref_driver.cpp, which compiles the reference's utility
headers in place).  The oracle is not in between: the payload behind the header must hash to the reference's golden, shapes the table
calls refused must return non-zero, and the decode of that payload must restore the input for the lossless stages.  Reads tests/golden/
only; inputs come from their seeds (tests/ref_stage_inputs.py, numpy only).  Which shapes are refused is the product's own policy, not a
statement of the reference (_meta.refused in the golden).
The char form of diff3x3x1 runs as "pass_through->diff3x3x1" on uint8 voxels, not behind the quantiser: pass_through hands the bytes to the
tail filter as they are, so the payload is the reference's diff_scheme<char> of exactly the golden's input, which a quantiser's lossy
table in between would not allow."""
import hashlib
import os

import numpy as np
import pytest

from ref_stage_inputs import load_cases, stage_volume, stage_tile

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
META, _ALL = load_cases(os.path.join(HERE, "golden", "ref_stages.json"))
CASES = [c for c in _ALL if c["stage"] != "histogram" and "undefined" not in c]
LOSSLESS = ("diff3x3x1", "zcurve_reorder", "raster_reorder", "bitswap1")
HEADER_END = b"|01307#!"


def _pipeline(c):
    st, p = c["stage"], c["params"]
    if st == "diff3x3x1":
        return "pass_through->diff3x3x1" if c["dtype"] == "char" else "diff3x3x1"      # behind a sink the stream is `char`
    if st == "rmbkrd_neighbor5x5x5":
        return "rmbkrd_neighbor5x5x5(threshold=%d,fraction=%r)" % (p["threshold"], p["fraction"])
    if st in ("zcurve_reorder", "raster_reorder"):
        return "%s(tile_size=%d)" % (st, stage_tile(c))
    return st


def _volume(c):
    vol = stage_volume(c)
    off = c["params"].get("offset_bytes", 0)
    if off:                                                 # the same voxels, `off` bytes behind where numpy put the buffer
        raw = np.zeros(vol.nbytes + off, np.uint8)
        raw[off:] = vol.reshape(-1).view(np.uint8)
        vol = raw[off:].view(vol.dtype).reshape(vol.shape)
    return vol


@pytest.mark.parametrize("stage", sorted({c["stage"] for c in CASES}))
def test_stage_payload_is_the_reference_golden(sqy, options, stage):
    options("host_l2_bytes", META["host_l2_bytes"])
    ran = refused = 0
    for c in CASES:
        if c["stage"] != stage:
            continue
        vol = _volume(c)
        assert hashlib.sha256(vol.tobytes()).hexdigest()[:12] == c["input_sha256"], c["id"]
        pipeline = _pipeline(c)
        rc, blob = sqy.encode(pipeline, vol, nthreads=2)
        if "refused" in c:
            assert rc != 0, c["id"]
            refused += 1
            continue
        assert rc == 0, c["id"]
        payload = blob[blob.index(HEADER_END) + len(HEADER_END):]
        assert len(payload) == c["bytes"], (c["id"], len(payload))
        assert hashlib.sha256(payload).hexdigest() == c["sha256"], c["id"]
        if stage in LOSSLESS:                               # the payload IS the reference's output: its decode restores the input
            rc, back = sqy.decode(blob)
            assert rc == 0 and np.array_equal(back, vol), c["id"]
        ran += 1
    assert ran, stage
    assert refused or stage in ("zcurve_reorder", "raster_reorder", "bitswap1"), stage
