"""GPU: bitswap1 at the seams of the transposer kernels it runs through today, on the cases of tests/bitswap_seam_cases.py
(tests/test_bitswap_seams_host.py holds that table, and the plain definition planes() / voxels(), to what they claim, without a GPU): the
register-tile kernels against the generic ones at no tile, one tile, one tile and a tail-only launch, a plane size that drops the register
kernel, rest words, odd and even tile counts; a source off the 16-byte grid; the in-place transposer with full-range planes, single-bit
pieces and the noise digest next to holes; the 8-bit kernels around a word, a workgroup and a wave of the LUT decode; the fused quantiser
transposer's loop beyond its first trip.
Which kernel a call takes is restated in bitswap_seam_cases.py, not observed -- except behind the quantiser, where the profile tells the
fused kernels from the plain ones.  The non-in-place register kernel's grid-stride loop (beyond 64 x CUs tiles, 128 Mi voxels) is out of
scope here on purpose: tests/test_gpu_fullsize.py reaches it.
Expected everywhere, byte for byte and without a tolerance: the blob is the oracle's, the `bitswap1` payload is planes() of the volume, the
oracle's blob decodes to the volume twice in a row.  No expectation comes from the code under test.  A failure names the case, the route
it claims and the first differing plane, word, bit and voxel."""
import numpy as np
import pytest

import bitswap_seam_cases as B
from test_gpu_decode_batch import CANARY, GAP, _dev
from test_gpu_decode_frames import _profile_names
from test_gpu_transpose_grid import TILES

pytestmark = pytest.mark.gpu

HEADER_END = b"|01307#!"
PIPELINES = ("bitswap1", "bitswap1->lz4")
_want = {}


@pytest.fixture(autouse=True)
def _lane_counter_left_at_zero(sqy):
    """calls that ran on the lanes count in `lane_calls`; tests that come later save and restore that counter through `options`, which
    only takes it back as 0"""
    yield
    sqy.set_option("lane_calls", 0)


def _blob(oracle, key, pipeline, vol):
    """the oracle's blob of a volume, made once"""
    k = (key, pipeline)
    if k not in _want:
        _want[k] = oracle.pipeline_encode(pipeline, vol, nthreads=2)
    return _want[k]


def _payload(blob):
    return blob[blob.index(HEADER_END) + len(HEADER_END):]


def _planes_failure(case, route, what, got_blob):
    """what to say about a blob that is not the expected one: for the plain pipeline the first difference of its payload from planes()"""
    vol = B.volume(case)
    try:
        diff = B.first_difference(np.frombuffer(_payload(got_blob), vol.dtype), B.planes(vol))
    except ValueError as e:                                 # (no end mark, or a payload that is no whole number of voxels)
        diff = "no payload to compare: %s" % e
    return B.failure(case, route, what, diff)


def _lz4_failure(oracle, case, route, what, got_blob):
    """.. and behind lz4: the first difference of planes() of what the oracle decodes the blob to"""
    vol = B.volume(case)
    try:
        back = oracle.pipeline_decode(got_blob)
        diff = B.first_difference(B.planes(np.asarray(back).reshape(-1)), B.planes(vol))
        if diff is None:
            diff = "the blob decodes to the volume: the LZ4 frames differ, not the planes"
    except Exception as e:                                  # noqa: BLE001 (whatever the oracle makes of a broken blob)
        diff = "the oracle cannot decode the blob: %s" % type(e).__name__
    return B.failure(case, route, what, diff)


# ---- encode ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", B.CASES, ids=B.case_id)
def test_encode_is_the_oracles_blob_and_the_definitions_planes(sqy, oracle, case):
    """the host entry point, from the driver's own aligned buffers.  (In front of lz4 it hands its staging buffer over with an offset: whole
    tiles may go through the in-place transposer where lz4_inplace_plan finds room -- the device test below pins the other route)"""
    vol = B.volume(case)
    rc, blob = sqy.encode("bitswap1", vol, nthreads=2)
    assert rc == 0, B.describe(case)
    got = np.frombuffer(_payload(blob), vol.dtype)
    want = B.planes(vol)
    assert np.array_equal(got, want), B.failure(case, "encode", "bitswap1: payload against planes()", B.first_difference(got, want))
    assert blob == _blob(oracle, case["name"], "bitswap1", vol), B.failure(case, "encode", "bitswap1: the planes are right, the header is not the oracle's", None)
    rc, blob = sqy.encode("bitswap1->lz4", vol, nthreads=2)
    assert rc == 0, B.describe(case, "encode_lz4")
    assert blob == _blob(oracle, case["name"], "bitswap1->lz4", vol), _lz4_failure(oracle, case, "encode_lz4", "bitswap1->lz4: blob against the oracle's", blob)


def _encode_device(sqy, pipeline, vol, shift):
    """encode_device from a source `shift` bytes behind a 16-byte boundary into a destination between canaries -> the blob"""
    import torch
    raw = torch.zeros(vol.nbytes + 32, dtype=torch.uint8, device=_dev())
    assert raw.data_ptr() % 16 == 0
    raw[shift:shift + vol.nbytes] = torch.from_numpy(np.frombuffer(vol.tobytes(), dtype=np.uint8).copy()).to(_dev())
    cap = sqy.max_compressed_length(pipeline, vol.shape, vol.dtype)
    out = torch.full((GAP + cap + GAP,), CANARY, dtype=torch.uint8, device=_dev())
    rc, n = sqy.encode_device(pipeline, raw.data_ptr() + shift, vol.shape, vol.dtype, out.data_ptr() + GAP, cap, nthreads=2)
    torch.cuda.synchronize()
    assert rc == 0 and 0 < n <= cap, (pipeline, vol.shape, shift, rc, n)
    h = out.cpu().numpy()
    assert (h[:GAP] == CANARY).all() and (h[GAP + cap:] == CANARY).all(), "written outside the destination: %s, %r, source %d bytes off" % (pipeline, vol.shape, shift)
    return h[GAP:GAP + n].tobytes()


OFF_GRID_CASES = B.TILE_CASES + [c for c in B.U8_CASES if c["encode"]["seg"]]


@pytest.mark.parametrize("case", OFF_GRID_CASES, ids=B.case_id)
def test_encode_from_a_device_source_on_and_off_the_16_byte_grid(sqy, oracle, case):
    """SQYAMD_PipelineEncode_*_Device takes no offset, so no frames in place: on the grid the register kernel, with piece hashes in front of
    lz4 for whole tiles, and the generic one for the rest; 2 and 8 bytes (8-bit voxels: 1 byte) behind a 16-byte boundary the register kernel
    is dropped, and with it the piece hashes -- all generic.  The same blob, nothing written outside the destination"""
    vol = B.volume(case)
    for pipeline in PIPELINES:
        for shift in B.SHIFTS[case["dtype"]]:
            got = _encode_device(sqy, pipeline, vol, shift)
            what = "%s, source %d bytes off" % (pipeline, shift)
            route = "encode_off_grid" if shift else "encode" if pipeline == "bitswap1" else "encode_lz4"
            if got != _blob(oracle, case["name"], pipeline, vol):
                assert False, (_planes_failure(case, route, what, got) if pipeline == "bitswap1" else _lz4_failure(oracle, case, route, what, got))


# ---- frames in place -------------------------------------------------------------------------------------------------------------------------
LZ4_4K = "bitswap1->lz4(blocksize_kb=4,framestep_kb=4)"     # 4 KiB chunks: a single tile is four of them (frames in place need two)
LZ4_16K = "bitswap1->lz4(blocksize_kb=16,framestep_kb=16)"  # 16 KiB chunks, 16 tiles: a plane segment is one chunk -- the noise digest is offered


def _in_place(sqy, oracle, pipeline, key, vol, what):
    """encode_device_at on a stream of its own: the path was taken (off > 0), the bytes are the oracle's blob, the blob decodes to the volume"""
    import torch
    dev = _dev()
    want = _blob(oracle, key, pipeline, vol)
    cap = sqy.max_compressed_length(pipeline, vol.shape, np.uint16)
    d_vol = torch.from_numpy(vol.copy()).to(dev)
    out = torch.full((cap,), 0xA5, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        rc, off, n = sqy.encode_device_at(pipeline, d_vol.data_ptr(), vol.shape, np.uint16, out.data_ptr(), cap, nthreads=2, stream=s.cuda_stream)
        s.synchronize()
    assert rc == 0 and off > 0, (what, "not frames in place: not the path this test is about")
    assert off + n <= cap, what
    got = bytes(out[off:off + n].cpu().numpy().tobytes())
    if got != want:
        try:
            diff = B.first_difference(B.planes(np.asarray(oracle.pipeline_decode(got)).reshape(-1)), B.planes(vol))
        except Exception as e:                              # noqa: BLE001
            diff = "the oracle cannot decode the blob: %s" % type(e).__name__
        assert False, "%s: %d bytes against the oracle's %d; first difference of the planes the blob holds: %r" % (what, len(got), len(want), diff)
    return want


@pytest.mark.parametrize("tpw", [None, 1], ids=["default", "1"])
@pytest.mark.parametrize("tiles", TILES)
def test_frames_in_place_with_full_range_planes(sqy, oracle, options, tiles, tpw):
    """the tile counts of test_gpu_transpose_grid.py on volumes whose top planes are busy: noise, single-bit pieces (one busy lane in one
    plane), plane 15 full with fourteen holes under it, all ones -- on the lanes and on the caller's stream"""
    if tpw is not None:
        options("transpose_tiles_per_wave", tpw)
    route = B.encode_route_u16(tiles * B.TILE_VOXELS, lz4_behind=True, in_place=True, tiles_per_wave=1)
    assert route["in_place"] and route["tiles"] == tiles
    for lanes in (1, 0):
        options("stage_lanes", lanes)
        for kind in B.KINDS:
            vol = B.frames_volume(tiles, kind)
            want = _in_place(sqy, oracle, LZ4_4K, ("frames", tiles, kind), vol, "%d tiles, %s, stage_lanes %d, tiles per wave %r, route %r" % (tiles, kind, lanes, tpw, route))
            if lanes:
                rc, back = sqy.decode(want)
                assert rc == 0 and np.array_equal(back, vol), (tiles, kind)


@pytest.mark.parametrize("zeroed", [(), (3, 4, 15)], ids=["noise", "holes"])
def test_frames_in_place_noise_digest_next_to_holes(sqy, oracle, options, zeroed):
    """16 tiles, 16 KiB chunks: every plane is one chunk of noise the digest is written for.  With tiles 3, 4 and 15 zeroed every chunk has
    holes (no digest entries from there: the parse reads such a chunk's bytes), and the last lane of tiles 2 and 14 takes its fifth byte
    from a piece that is never written.  The oracle's blob with the digest and without"""
    vol = B.frames_volume(16, "random", zeroed)
    for digest in (1, 0):
        options("noise_digest", digest)
        want = _in_place(sqy, oracle, LZ4_16K, ("frames", 16, "random", zeroed), vol, "16 tiles, noise, tiles %r zeroed, noise_digest %d" % (zeroed, digest))
    rc, back = sqy.decode(want)
    assert rc == 0 and np.array_equal(back, vol)


# ---- decode ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", B.CASES, ids=B.case_id)
def test_decode_restores_the_volume_twice(sqy, oracle, case):
    """`bitswap1`: the planes sit behind the header, off the 16-byte grid -- all generic; `bitswap1->lz4`: the LZ4 stage's output buffer --
    the register kernel and the rest"""
    vol = B.volume(case)
    for pipeline, route in (("bitswap1", "decode_off_grid"), ("bitswap1->lz4", "decode")):
        blob = _blob(oracle, case["name"], pipeline, vol)
        if pipeline == "bitswap1":
            assert sqy.header_size(blob) % 16 != 0 or case["dtype"] == "uint8", B.describe(case, route)
        for turn in (1, 2):
            rc, back = sqy.decode(blob)
            assert rc == 0, B.describe(case, route)
            assert back.shape == vol.shape and back.dtype == vol.dtype, B.describe(case, route)
            if not np.array_equal(back, vol):
                bad = np.flatnonzero(back.reshape(-1) != vol.reshape(-1))
                i = int(bad[0])
                assert False, B.failure(case, route, "%s, decode %d" % (pipeline, turn),
                                        {"voxel": i, "got": int(back.reshape(-1)[i]), "want": int(vol.reshape(-1)[i]), "differing": len(bad), "last": int(bad[-1])})


# ---- behind the quantiser --------------------------------------------------------------------------------------------------------------------
QUANTISER_CASES = B.QUANTISER_LENGTHS + ["fused"]


@pytest.mark.parametrize("n", QUANTISER_CASES, ids=[str(n) for n in QUANTISER_CASES])
def test_quantiser_bitswap1_fused_kernels(sqy, oracle, n):
    """narrow-band 16-bit voxels whose sink bytes have the lengths of the 8-bit cases, and the long case of the fused transposer's loop
    (sized from the device's CU count): the oracle's blob; its decode is the oracle's; and the kernels the profile names"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if n == "fused":
        n = B.fused_length(cus)
        assert 1 << 20 < n < 8 << 20, (cus, n)
    trips = B.fused_quantiser_trips(n, cus)
    vol = B.narrow_band(n, 7700 + n % 97)
    for pipeline in ("quantiser->bitswap1->lz4", "quantiser->bitswap1"):
        what = "%s, %d voxels, loop %r, LUT decode %r" % (pipeline, n, trips, B.lut_decode_possible(n))
        want = _blob(oracle, ("narrow", n), pipeline, vol)
        if pipeline == "quantiser->bitswap1":               # the definition on the oracle's own quantiser bytes
            sink = np.frombuffer(_payload(_blob(oracle, ("narrow", n), "quantiser", vol)), np.uint8)
            assert np.array_equal(np.frombuffer(_payload(want), np.uint8), B.planes(sink)), what
        got = {}
        names = _profile_names(sqy, lambda: got.update(zip(("rc", "blob"), sqy.encode(pipeline, vol, nthreads=2))))
        assert got["rc"] == 0, what
        assert "quantiser_bitswap1_u8" in names and "bitswap1_u8" not in names and "quantiser_apply" not in names, (what, sorted(names))
        if got["blob"] != want and pipeline == "quantiser->bitswap1":
            diff = B.first_difference(np.frombuffer(_payload(got["blob"]), np.uint8), np.frombuffer(_payload(want), np.uint8))
            assert False, "%s: first difference of the planes %r" % (what, diff)
        assert got["blob"] == want, what
        expect = oracle.pipeline_decode(want).reshape(vol.shape)
        # the fused inverse needs whole 16-byte vectors per plane and planes on the 16-byte grid: behind lz4 always, behind the header seldom
        aligned = pipeline.endswith("lz4") or sqy.header_size(want) % 16 == 0
        for turn in (1, 2):
            names = _profile_names(sqy, lambda: got.update(zip(("rc", "back"), sqy.decode(want))))
            assert got["rc"] == 0, what
            if B.lut_decode_possible(n) and aligned:
                assert "bitswap1_quantiser_decode" in names and "bitswap1_decode" not in names and "quantiser_decode" not in names, (what, sorted(names))
            else:
                assert {"bitswap1_decode", "quantiser_decode"} <= names and "bitswap1_quantiser_decode" not in names, (what, sorted(names))
            back = got["back"]
            if not np.array_equal(back, expect):
                bad = np.flatnonzero(back.reshape(-1) != expect.reshape(-1))
                i = int(bad[0])
                assert False, "%s, decode %d: voxel %d is %d, the oracle's %d; %d differ, the last %d" % (
                    what, turn, i, int(back.reshape(-1)[i]), int(expect.reshape(-1)[i]), len(bad), int(bad[-1]))
