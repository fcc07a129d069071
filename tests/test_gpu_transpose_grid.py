"""GPU: the in-place transposer's grid (a fixed number of tiles per wavefront, option transpose_tiles_per_wave) and the duplicate search's
table emptied by the transposer's own launch (a frames-in-place call on the lanes launches no lz4_dedupe_clear).

 1 tile counts at the edges of the wave-to-tile mapping -- 1, 2, 3, 5, 7, 33 tiles of 8192 voxels; at the default, at one tile per wave
   and at 64 (one workgroup takes every tile, and its loop over the table runs more than once): the blob is the oracle's, on the lanes
   and on the caller's stream, with and without diff3x3x1 in front (the transposer's side buffer).
 2 the clear.  The hash only nominates and the byte compare decides: a table that was not emptied cannot corrupt a blob, it can only lose
   duplicates.  So the duplicate map is read (option dedupe_report) after each of three calls through one context: A holds two patterns
   repeated across chunks and all-zero chunks; B, same shape, holds each pattern ONCE, in chunks 0 and 1 -- in front of where A has
   them -- and nothing else twice but the zero chunks; C is A again.  Entries of B left in the table would nominate chunks 0 and 1 for
   C's patterns, the compare would say "different", and C's map would show no duplicate of either pattern (a build whose transposer
   skips the stores fails exactly there, in all six cases: chunks 5, 7, 9, .. of the third call reported as their own).
   Who clears is read from the profile hooks: on the lanes no lz4_dedupe_clear; a frames-in-place call on its caller's stream still
   counts one per call.  SQYAMD_PipelineEncode_UI16_Device (no frames in place) never launched that kernel: its table is emptied by the two
   fills inside the "lz4_dedupe" scope, as before -- what is asserted there is that scope and the map.
 3 four threads on the lanes that change shape among those tile counts from call to call: every blob is the oracle's."""
import numpy as np
import pytest

import dedupe_collisions as DC
from test_gpu_lane_return import _Job, _in_flight

pytestmark = pytest.mark.gpu

TILES = (1, 2, 3, 5, 7, 33)
SETTINGS = (None, 1, 64)                                    # transpose_tiles_per_wave: the default and the option's extreme values
LZ4 = "lz4(blocksize_kb=4,framestep_kb=4)"                  # 4 KiB chunks: a single tile is four of them (frames in place need two)
PLAIN, SIDE = "bitswap1->" + LZ4, "diff3x3x1->bitswap1->" + LZ4


def _shape(pipeline, n):
    """n tiles; behind diff3x3x1 a shape whose touched columns (1 + Z - 2, rounded up to 128) leave columns out: the side buffer's path"""
    return (n, 64, 128) if pipeline == PLAIN else (n, 32, 256)


@pytest.fixture(scope="module")
def jobs(sqy, oracle):
    import torch
    dev = torch.device("cuda", 0)
    return {(p, n): _Job(sqy, oracle, p, _shape(p, n), dev) for p in (PLAIN, SIDE) for n in TILES if not (p == SIDE and n == 1)}


@pytest.mark.parametrize("tpw", SETTINGS, ids=["default", "1", "64"])
@pytest.mark.parametrize("pipeline", [PLAIN, SIDE], ids=["plain", "side"])
def test_tile_counts(sqy, options, jobs, pipeline, tpw):
    import torch
    dev = torch.device("cuda", 0)
    if tpw is not None:
        options("transpose_tiles_per_wave", tpw)
    s = torch.cuda.Stream(device=dev)
    for lanes in (1, 0):
        options("stage_lanes", lanes)
        sqy.set_option("lane_calls", 0)
        mine = [j for (p, n), j in sorted(jobs.items()) if p == pipeline]
        for j in mine:
            out = torch.full((j.cap,), 0xA5, dtype=torch.uint8, device=dev)
            with torch.cuda.stream(s):
                rc, off, n = sqy.encode_device_at(j.pipeline, j.d_vol.data_ptr(), j.shape, np.uint16, out.data_ptr(), j.cap, nthreads=2, stream=s.cuda_stream)
                s.synchronize()
            assert rc == 0 and off > 0, (j.shape, "not frames in place: not the path this test is about")
            assert n == len(j.want) and torch.equal(out[off:off + n], j.d_want), (pipeline, j.shape, tpw, lanes)
        # (a call alone on the lanes that gets no answer from an idle lane in time stays on its caller's stream: seldom, and no error)
        took = sqy.get_option("lane_calls")
        assert (took >= (len(mine) + 1) // 2) if lanes else took == 0, "the calls did not run where this test wants them"


# ---- the clear ---------------------------------------------------------------------------------------------------------------------------
def _streams(chunk, nchunks, nzero):
    """plane streams A and B of nchunks chunks, the last nzero of them all zero (see the module text)"""
    rng = np.random.default_rng(chunk + nchunks)
    noise = lambda: rng.integers(0, 256, chunk, dtype=np.uint8)
    p1, p2 = noise(), noise()
    a = np.zeros((nchunks, chunk), dtype=np.uint8)
    b = np.zeros((nchunks, chunk), dtype=np.uint8)
    for k in range(nchunks - nzero):
        a[k] = p1 if k % 4 == 1 else p2 if k % 4 == 3 else noise()
        b[k] = p1 if k == 0 else p2 if k == 1 else noise()
    return a.reshape(-1), b.reshape(-1)


# (chunk, tiles): 4 KiB chunks, 256 of them -- a table of 512 slots, 16-byte aligned, more vectors than one workgroup has threads;
# 16 KiB chunks, 33 of them -- an odd number of 8-byte keys in front of the table: it starts and ends 8 bytes off a 16-byte boundary
CLEAR_CASES = [(4 << 10, 64), (16 << 10, 33)]


@pytest.fixture(scope="module", params=CLEAR_CASES, ids=["4k_aligned", "16k_off8"])
def abc(request, oracle):
    chunk, tiles = request.param
    nchunks = tiles * 16384 // chunk
    calls = []
    for stream in _streams(chunk, nchunks, nchunks // 4):
        vol = oracle.bitswap1_decode(stream.view(np.uint16)).reshape(1, 1, -1)        # voxels whose bit planes are that stream
        planes = np.ascontiguousarray(oracle.bitswap1_encode_planes(vol.reshape(-1))).view(np.uint8).reshape(-1)
        assert np.array_equal(planes, stream)
        calls.append(dict(vol=vol, dup_of=DC.expected_dup_of(planes, chunk), keys=DC.chunk_keys(planes, chunk)))
    a, b = calls
    # what the test is built on: A repeats, B does not (but for zero chunks, which all share the first one's frame)
    first_zero = nchunks - nchunks // 4
    assert np.count_nonzero(a["dup_of"][:first_zero] != np.arange(first_zero)) >= first_zero // 2 - 2
    assert np.array_equal(b["dup_of"][:first_zero + 1], np.arange(first_zero + 1)) and np.all(b["dup_of"][first_zero:] == first_zero)
    assert b["keys"][0] == a["keys"][1] and b["keys"][1] == a["keys"][3]
    pipe = "bitswap1->lz4" + DC.lz4_config(chunk) if chunk != (4 << 10) else PLAIN
    for c in calls:
        c["want"] = oracle.pipeline_encode(pipe, c["vol"], nthreads=2)
    return dict(pipe=pipe, order=(a, b, a), shape=a["vol"].shape)


def _three_calls(sqy, options, abc, in_place, tag):
    """A, B, A through one context; the blob and the duplicate map after each; returns the profile of the three calls"""
    import torch
    dev = torch.device("cuda", 0)
    pipe, shape = abc["pipe"], abc["shape"]
    cap = sqy.max_compressed_length(pipe, shape, np.uint16)
    out = torch.full((cap,), 0xA5, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    sqy.profile_reset()
    sqy.profile_enable(True)
    try:
        for i, c in enumerate(abc["order"]):
            d_vol = torch.from_numpy(c["vol"].copy()).to(dev)
            options("dedupe_report", 1)                                                 # (drops the record of the call before)
            with torch.cuda.stream(s):
                if in_place:
                    rc, off, n = sqy.encode_device_at(pipe, d_vol.data_ptr(), shape, np.uint16, out.data_ptr(), cap, nthreads=2, stream=s.cuda_stream)
                else:
                    rc, n = sqy.encode_device(pipe, d_vol.data_ptr(), shape, np.uint16, out.data_ptr(), cap, nthreads=2, stream=s.cuda_stream)
                    off = 0
                s.synchronize()
            assert rc == 0 and (off > 0) == in_place, (tag, i, "not the path this test is about")
            keys, dup_of = sqy.dedupe_report()
            assert np.array_equal(keys, c["keys"]), (tag, "call", "ABA"[i], "the fixture's keys are not the kernels'")
            bad = np.flatnonzero(dup_of != c["dup_of"]).tolist()
            assert not bad, (tag, "call", "ABA"[i], "dup_of (chunk, reported, expected)", [(k, int(dup_of[k]), int(c["dup_of"][k])) for k in bad[:16]])
            assert bytes(out[off:off + n].cpu().numpy().tobytes()) == c["want"], (tag, "call", "ABA"[i])
    finally:
        sqy.profile_enable(False)
    prof = sqy.profile_get()
    sqy.profile_reset()
    return prof


@pytest.mark.parametrize("tpw", SETTINGS, ids=["default", "1", "64"])
def test_table_is_clear_for_every_call(sqy, options, abc, tpw):
    if tpw is not None:
        options("transpose_tiles_per_wave", tpw)
    # on the lanes: the transposer clears, no clear launch
    options("stage_lanes", 1)
    sqy.set_option("lane_calls", 0)
    prof = _three_calls(sqy, options, abc, True, "lanes")
    took = sqy.get_option("lane_calls")                     # (3, but for a call whose idle lane did not answer in time: that one stays on its stream)
    assert took >= 2 and prof.get("lz4_dedupe_clear", (0, 0))[1] == 3 - took and prof["bitswap1_u16"][1] == 3, (took, prof)
    # frames in place on the caller's stream: the clear kernel, one per call
    options("stage_lanes", 0)
    prof = _three_calls(sqy, options, abc, True, "caller's stream")
    assert prof["lz4_dedupe_clear"][1] == 3 and prof["bitswap1_u16"][1] == 3, prof
    # no frames in place (no offset to hand back): the fills inside the duplicate search's scope
    prof = _three_calls(sqy, options, abc, False, "_Device")
    assert "lz4_dedupe_clear" not in prof and prof["lz4_dedupe"][1] == 3, prof


# ---- calls in flight ---------------------------------------------------------------------------------------------------------------------
def test_four_in_flight_changing_tile_counts(sqy, options, jobs):
    import torch
    dev = torch.device("cuda", 0)
    options("stage_lanes", 1)
    options("transpose_chain_caller_streams", 1)
    sqy.set_option("lane_calls", 0)
    plain = [jobs[(PLAIN, n)] for n in TILES]
    rounds = 4

    def body(t, s):
        out = torch.empty(max(j.cap for j in plain), dtype=torch.uint8, device=dev)
        for r in range(rounds):
            for i in range(len(plain)):
                plain[(i * (t + 1) + t + r) % len(plain)].run(sqy, out, s)         # (every thread its own walk through the tile counts)

    _in_flight(4, body)
    assert sqy.get_option("lane_calls") >= 4 * rounds * len(plain) // 2
