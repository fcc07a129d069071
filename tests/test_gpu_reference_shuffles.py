"""GPU: frame_shuffle and tile_shuffle through the C-ABI against what the REFERENCE's own sqeazy::detail::frame_shuffle and
sqeazy::detail::tile_shuffle give (tests/golden/ref_shuffles.json, taken by oracle/gen_golden.py --shuffles from oracle/ref_driver.cpp,
which compiles the reference's two headers in place).  The oracle is not in between: the payload behind the header must hash to the
reference's output, the reorder_map in the header -- read out of the header text here -- must be the reference's decode_map entry for
entry, the decode of the blob must hash to the reference's zero-filled decode (the input itself where the map is a permutation), and
shapes with a remainder must return non-zero.  Each stage runs alone and with lz4 behind it; with lz4 the decode is what is checked.
Reads tests/golden/ only; inputs come from their seeds (tests/ref_stage_inputs.py, numpy only).
The char forms run as "pass_through->frame_shuffle" and "pass_through->tile_shuffle(tile_size=...)" on uint8 voxels: pass_through hands
the bytes to the tail filter as they are, so the stage sees the golden's input as signed bytes."""
import base64
import hashlib
import json
import os
import time

import numpy as np
import pytest

from ref_stage_inputs import load_shuffle_cases, shuffle_volume

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
META, CASES, _ = load_shuffle_cases(os.path.join(HERE, "golden", "ref_shuffles.json"))
GROUPS = sorted({(c["stage"], c["dtype"]) for c in CASES})
HEADER_END = b"|01307#!"
NTHREADS = 2


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _pipeline(c):
    stage = "frame_shuffle(frame_chunk_size=%d)" % c["frame_chunk_size"] if c["stage"] == "frame_shuffle" else "tile_shuffle(tile_size=%d)" % c["tile_size"]
    return ("pass_through->" if c["dtype"] == "char" else "") + stage          # behind a sink the stream is `char`


def _header_map(blob):
    """the reorder_map of the blob's one shuffle stage: base64 of little-endian u64 between <verbatim> and </verbatim> in the pipeline's
    name, which the header holds as a JSON string"""
    name = json.loads(blob[:blob.index(HEADER_END)].decode("latin-1"))["pipename"]
    a, b = name.index("<verbatim>") + len("<verbatim>"), name.index("</verbatim>")
    assert name.count("<verbatim>") == 1
    return np.frombuffer(base64.b64decode(name[a:b]), dtype="<u8").tolist()


def _is_permutation(m):
    return sorted(m) == list(range(len(m)))


@pytest.mark.parametrize("stage,dtype", GROUPS)
def test_shuffle_is_the_reference_golden(sqy, stage, dtype):
    t0 = time.perf_counter()
    ran = refused = ties = 0
    for c in CASES:
        if (c["stage"], c["dtype"]) != (stage, dtype):
            continue
        vol = shuffle_volume(c)
        assert _sha(vol.tobytes())[:12] == c["input_sha256"], c["id"]
        units = len(c.get("map", ()))
        for pipeline in (_pipeline(c), _pipeline(c) + "->lz4"):
            what = (c["id"], pipeline)
            rc, blob = sqy.encode(pipeline, vol, nthreads=NTHREADS, extra_capacity=16 * units + 512)
            if "refused" in c:
                assert rc != 0, what
                continue
            assert rc == 0, what
            if not pipeline.endswith("->lz4"):
                got = _header_map(blob)                     # (first: a wrong map says more than the wrong payload that follows from it)
                assert got == c["map"], "%s through %s: reorder_map %s, the reference's decode_map is %s" % (c["id"], pipeline, got, c["map"])
                payload = blob[blob.index(HEADER_END) + len(HEADER_END):]
                assert len(payload) == c["bytes"], (what, len(payload))
                assert _sha(payload) == c["sha256"], what
            rc, back = sqy.decode(blob)
            assert rc == 0 and back.shape == vol.shape and back.dtype == vol.dtype, what
            assert _sha(back.tobytes()) == c["decode_sha256"], what
            if _is_permutation(c["map"]):                   # nothing is lost: the decode is the input itself
                assert c["decode_sha256"] == _sha(vol.tobytes()) and np.array_equal(back, vol), what
        if "refused" in c:
            refused += 1
        else:
            ran += 1
            ties += not _is_permutation(c["map"])
    assert ran and refused and ties, (stage, dtype, ran, refused, ties)
    print("\n%s %s: %d cases, %d of them with equal metrics, %d refused, %.2f s" % (stage, dtype, ran, ties, refused, time.perf_counter() - t0))
