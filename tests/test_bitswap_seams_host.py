"""tests/bitswap_seam_cases.py without a GPU: the definition is the oracle's operation, and the table means what it says.
  * planes() equals the oracle's bitswap1 on every case, kind and type, voxels() undoes it, and the payload of the oracle's `bitswap1` blob
    (behind the header's end mark, as tests/test_gpu_reference_stages.py takes it) is planes() of the volume;
  * planes() of the payload of the oracle's `quantiser` blob is the payload of its `quantiser->bitswap1` blob;
  * the routes the module restates give, for every length, the branch the length is named for (numbers written out here by hand), and every
    value a route function can return is claimed by some case;
  * the data kinds are what the GPU tests take them for: `top` leaves fourteen planes empty, `onehot` has pieces with one busy lane in one
    plane only; first_difference names plane, word, bit and voxel of a planted error."""
import numpy as np
import pytest

import bitswap_seam_cases as B

HEADER_END = b"|01307#!"
_planes = {}


def _payload(blob):
    return blob[blob.index(HEADER_END) + len(HEADER_END):]


def _p(case):
    if case["name"] not in _planes:
        _planes[case["name"]] = B.planes(B.volume(case))
    return _planes[case["name"]]


# ---- the definition --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint16, np.uint8], ids=["uint16", "uint8"])
def test_definition_is_the_oracles_at_plain_lengths(oracle, dtype):
    for n in (1, 5, 15, 16, 17, 127, 128, 8191, 8192, 8193, 24663, 393, 65560):
        a = B.make("random", dtype, n, 40 + n)
        p = B.planes(a)
        assert p.dtype == a.dtype and p.size == n
        assert np.array_equal(p, oracle.bitswap1_encode(a)), (n, B.first_difference(p, oracle.bitswap1_encode(a)))
        assert np.array_equal(B.voxels(p), a) and np.array_equal(oracle.bitswap1_decode(p), a), n


def test_definition_by_hand():
    """one word of each width, written out: voxel j of the word sits at bit W - 1 - j, segment W - 1 - b carries bit b"""
    a = np.zeros(16 + 3, np.uint16)
    a[0], a[15], a[5] = 0x8000, 0x0001, 0x0180
    a[16:] = (0xBEEF, 7, 0x8000)
    want = np.zeros(19, np.uint16)
    want[0] = 0x8000                                        # bit 15 of voxel 0: segment 0, bit 15
    want[15] = 0x0001                                       # bit 0 of voxel 15: segment 15, bit 0
    want[7] = want[8] = 1 << (15 - 5)                       # bits 8 and 7 of voxel 5: segments 7 and 8, bit 10
    want[16:] = a[16:]
    assert np.array_equal(B.planes(a), want) and np.array_equal(B.voxels(want), a)
    b = np.zeros(8 + 2, np.uint8)
    b[0], b[7], b[8:] = 0x81, 0x10, (0xAB, 1)
    wantb = np.array([0x80, 0, 0, 0x01, 0, 0, 0, 0x80, 0xAB, 1], np.uint8)
    assert np.array_equal(B.planes(b), wantb) and np.array_equal(B.voxels(wantb), b)


@pytest.mark.parametrize("case", B.CASES, ids=B.case_id)
def test_definition_is_the_oracles_on_every_case(oracle, case):
    vol = B.volume(case)
    p = _p(case)
    want = oracle.bitswap1_encode(vol).reshape(-1)
    assert np.array_equal(p, want), B.failure(case, "encode", "planes() against the oracle", B.first_difference(p, want))
    assert np.array_equal(B.voxels(p), vol.reshape(-1)), B.describe(case)
    assert np.array_equal(oracle.bitswap1_decode(p), vol.reshape(-1)), B.describe(case)
    blob = oracle.pipeline_encode("bitswap1", vol, nthreads=2)
    got = np.frombuffer(_payload(blob), vol.dtype)
    assert np.array_equal(got, p), B.failure(case, "encode", "the oracle's blob payload", B.first_difference(got, p))
    assert np.array_equal(oracle.pipeline_decode(blob).reshape(-1), vol.reshape(-1)), B.describe(case)


@pytest.mark.parametrize("tiles", [1, 2, 3, 5, 7, 16, 33])
def test_definition_is_the_oracles_on_the_frames_volumes(oracle, tiles):
    for kind in B.KINDS:
        vol = B.frames_volume(tiles, kind)
        assert vol.shape == (tiles, 64, 128) and np.array_equal(B.planes(vol), oracle.bitswap1_encode(vol).reshape(-1)), (tiles, kind)
    holes = B.frames_volume(16, "random", (3, 4, 15))
    assert not holes.reshape(16, -1)[[3, 4, 15]].any() and holes.reshape(16, -1)[[0, 2, 5, 14]].any(axis=1).all()
    assert np.array_equal(B.planes(holes), oracle.bitswap1_encode(holes).reshape(-1))


QUANTISER_LENGTHS = sorted(set(B.QUANTISER_LENGTHS + [128, 8320, 8200, 1003, B.fused_length(256)]))


@pytest.mark.parametrize("n", QUANTISER_LENGTHS)
def test_quantiser_bitswap1_payload_is_planes_of_the_quantisers(oracle, n):
    vol = B.narrow_band(n, 7700 + n % 97)
    sink = np.frombuffer(_payload(oracle.pipeline_encode("quantiser", vol, nthreads=2)), np.uint8)
    both = np.frombuffer(_payload(oracle.pipeline_encode("quantiser->bitswap1", vol, nthreads=2)), np.uint8)
    assert sink.size == n and both.size == n
    assert len(np.unique(sink)) > 128 or n < 1000, "the sink's bytes leave the top plane empty"
    p = B.planes(sink)
    assert np.array_equal(p, both), (n, B.first_difference(both, p))
    assert np.array_equal(B.voxels(both), sink), n


# ---- the routes ------------------------------------------------------------------------------------------------------------------------------
T = B.TILE_VOXELS
# by hand, per length: encode (tiles, workgroups of two waves, idle wave, first_word, rest_words, tail, generic, generic workgroups) |
# decode behind lz4 (tiles, workgroups of four waves, w0, rest_words, generic, generic workgroups)
WANT_U16 = {
    T - 1: ((0, 0, False, 0, 511, 15, "whole", 2), (0, 0, 0, 511, "whole", 2)),
    T: ((1, 1, True, 512, 0, 0, "none", 0), (1, 1, 512, 0, "none", 1)),
    T + 1: ((1, 1, True, 512, 0, 1, "tail-only", 1), (1, 1, 512, 0, "tail-only", 1)),
    T + 16: ((0, 0, False, 0, 513, 0, "whole", 3), (0, 0, 0, 513, "whole", 3)),
    T + 128: ((1, 1, True, 512, 8, 0, "rest", 1), (1, 1, 512, 8, "rest", 1)),
    T + 133: ((1, 1, True, 512, 8, 5, "both", 1), (1, 1, 512, 8, "both", 1)),
    2 * T: ((2, 1, False, 1024, 0, 0, "none", 0), (2, 1, 1024, 0, "none", 1)),
    3 * T + 399: ((3, 2, True, 1536, 24, 15, "both", 1), (3, 1, 1536, 24, "both", 1)),
    5 * T + 8176: ((0, 0, False, 0, 3071, 0, "whole", 12), (0, 0, 0, 3071, "whole", 12)),
    5 * T + 8064: ((5, 3, True, 2560, 504, 0, "rest", 2), (5, 2, 2560, 504, "rest", 2)),
    33 * T: ((33, 17, True, 16896, 0, 0, "none", 0), (33, 9, 16896, 0, "none", 1)),
}
# encode (workgroups of 128, threads of the last, tail) | decode (workgroups of 256, threads of the last) | LUT decode possible
WANT_U8 = {
    7: ((1, 0, 7), (1, 0), False), 8: ((1, 1, 0), (1, 1), False), 9: ((1, 1, 1), (1, 1), False),
    1023: ((1, 127, 7), (1, 127), False), 1024: ((1, 128, 0), (1, 128), True), 1025: ((1, 128, 1), (1, 128), False),
    8064: ((8, 112, 0), (4, 240), True), 8192: ((8, 128, 0), (4, 256), True), 8320: ((9, 16, 0), (5, 16), True),
    8200: ((9, 1, 0), (5, 1), False), 32896: ((33, 16, 0), (17, 16), True),
}


def test_every_length_reaches_the_branch_it_is_named_for():
    assert len(B.BY_NAME) == len(B.CASES) == 4 * (len(B.U16_LENGTHS) + len(B.U8_LENGTHS))
    assert [n for n, _ in B.U16_LENGTHS] == list(WANT_U16) and [n for n, _ in B.U8_LENGTHS] == list(WANT_U8)
    assert max(c["n"] for c in B.CASES) == 33 * T < 300000
    for c in B.U16_CASES:
        enc, dec = WANT_U16[c["n"]]
        e, d = c["encode"], c["decode"]
        assert (e["tiles"], e["regs_blocks"], e["idle_wave"], e["first_word"], e["rest_words"], e["tail"], e["generic"], e["generic_blocks"]) == enc, B.describe(c)
        assert (d["tiles"], d["regs_blocks"], d["w0"], d["rest_words"], d["generic"], d["generic_blocks"]) == dec and d["tail"] == e["tail"], B.describe(c, "decode")
        # in front of lz4 the same kernels; piece hashes only for whole tiles
        el = c["encode_lz4"]
        assert {k: v for k, v in el.items() if k != "piece_hashes"} == {k: v for k, v in e.items() if k != "piece_hashes"}
        assert el["piece_hashes"] == (c["n"] % T == 0) and not e["piece_hashes"] and not el["in_place"], B.describe(c, "encode_lz4")
        # off the 16-byte grid: no tile, no hashes, everything generic -- for the encoder's source and for the decoder's planes behind the header
        for r in (c["encode_off_grid"], c["decode_off_grid"]):
            assert r["tiles"] == 0 and r["rest_words"] == c["n"] // 16 and r["generic"] == "whole", B.describe(c)
        assert not c["encode_off_grid"]["piece_hashes"]
    for c in B.U8_CASES:
        enc, dec, lut = WANT_U8[c["n"]]
        e, d = c["encode"], c["decode"]
        assert (e["blocks"], e["last_block_threads"], e["tail"]) == enc and (d["blocks"], d["last_block_threads"]) == dec and c["lut"] == lut, B.describe(c)
    assert [c["n"] for c in B.TILE_CASES if c["kind"] == "random"] == [T, T + 1, T + 128, T + 133, 2 * T, 3 * T + 399, 5 * T + 8064, 33 * T]
    # the LUT decode's waves: one lane idle, whole, whole + one lane, a second workgroup of one lane
    lut = {n: B.lut_decode_route(n) for n in (8064, 8192, 8320, 32896)}
    assert [(r["blocks"], r["whole_waves"], r["partial_wave_lanes"]) for r in lut.values()] == [(1, 0, 63), (1, 1, 0), (1, 1, 1), (2, 4, 1)]


def test_frames_in_place_routes():
    """bitswap1_u16_regs<true>: whole tiles, piece hashes, no generic launch; workgroups of two waves at one tile per wave"""
    for tiles, blocks in ((1, 1), (2, 1), (3, 2), (5, 3), (7, 4), (16, 8), (33, 17)):
        r = B.encode_route_u16(tiles * T, lz4_behind=True, in_place=True)
        assert (r["in_place"], r["tiles"], r["regs_blocks"], r["idle_wave"], r["generic"], r["piece_hashes"]) == (True, tiles, blocks, tiles % 2 == 1, "none", True)
        assert B.encode_route_u16(tiles * T, lz4_behind=True, in_place=True, tiles_per_wave=64)["regs_blocks"] == 1
    # no frames in place without whole tiles, without lz4 behind the stage or off the grid
    assert not B.encode_route_u16(T + 16, lz4_behind=True, in_place=True)["in_place"]
    assert not B.encode_route_u16(T, lz4_behind=False, in_place=True)["in_place"]
    assert not B.encode_route_u16(T, src_aligned=False, lz4_behind=True, in_place=True)["in_place"]


def test_fused_quantiser_trips():
    """a workgroup per 4096 plane bytes, at most 2 x CUs of them: below the cap 4 x step covers at least a quarter of the plane bytes, so the
    loop makes one to four trips, and the second starts at 1025 plane bytes already"""
    cus = 256
    want = {7: (0, 1, 0, 0, 0, 7), 8: (1, 1, 1, 1, 1, 0), 9: (1, 1, 1, 1, 1, 1), 1023: (127, 1, 1, 1, 127, 7), 1024: (128, 1, 1, 1, 128, 0),
            1025: (128, 1, 1, 1, 128, 1), 8064: (1008, 1, 1, 4, 240, 0), 8192: (1024, 1, 1, 4, 256, 0), 8320: (1040, 1, 2, 1, 16, 0),
            8200: (1025, 1, 2, 1, 1, 0), 32896: (4112, 2, 3, 1, 16, 0)}
    assert sorted(want) == sorted(B.QUANTISER_LENGTHS)
    for n, w in want.items():
        r = B.fused_quantiser_trips(n, cus)
        assert (r["seg"], r["blocks"], r["trips"], r["last_trip_slots"], r["last_slot_threads"], r["tail"]) == w and not r["capped"], (n, r)
    # the long case: 5 x (2 cus x 256) + 77 plane bytes.  The grid is NOT capped there (161 workgroups of 512 at 256 CUs): four trips, the
    # last with all four slots and the fourth of them partly live, and a tail of 5
    for c in (256, 304, 64):
        n = B.fused_length(c)
        r = B.fused_quantiser_trips(n, c)
        seg = 5 * 2 * c * 256 + 77
        assert r["seg"] == seg and r["tail"] == 5 and not r["capped"] and r["blocks"] == (seg + 4095) // 4096 < 2 * c
        assert r["trips"] == 4 and r["last_trip_slots"] == 4 and 0 < r["last_slot_threads"] < r["step"], r
    assert B.fused_length(256) == 5243501
    assert B.fused_quantiser_trips(8 * 4096 * 2 * cus + 8, cus)["capped"]                 # (16 Mi voxels: not a case of this table)


def test_every_route_value_is_claimed():
    u16 = [c for c in B.U16_CASES if c["kind"] == "random"]
    for route in ("encode", "decode"):
        assert {c[route]["generic"] for c in u16} == {"none", "rest", "tail-only", "both", "whole"}, route
        tiles = {c[route]["tiles"] for c in u16}
        assert 0 in tiles and 1 in tiles and any(t > 1 and t % 2 == 0 for t in tiles) and any(t > 1 and t % 2 for t in tiles), route
    assert {c["encode"]["idle_wave"] for c in u16} == {True, False}
    assert {c["encode_lz4"]["piece_hashes"] for c in u16} == {True, False}
    assert {c["encode"]["generic_blocks"] for c in u16} >= {0, 1, 2, 3} and {c["decode"]["regs_blocks"] for c in u16} >= {0, 1, 2}
    assert {c["encode"]["tail"] for c in u16} >= {0, 1, 5, 15}
    u8 = [c for c in B.U8_CASES if c["kind"] == "random"]
    assert {c["lut"] for c in u8} == {True, False}
    assert {c["encode"]["blocks"] > 1 for c in u8} == {True, False} and {c["decode"]["blocks"] > 1 for c in u8} == {True, False}
    assert {c["encode"]["tail"] > 0 for c in u8} == {True, False} and {c["encode"]["seg"] == 0 for c in u8} == {True, False}
    trips = {B.fused_quantiser_trips(n, 256)["trips"] for n in B.QUANTISER_LENGTHS + [B.fused_length(256)]}
    assert trips == {0, 1, 2, 3, 4}
    # every claim is what the route functions compute
    for c in B.CASES:
        if c["dtype"] == "uint16":
            assert c["encode"] == B.encode_route_u16(c["n"]) and c["decode"] == B.decode_route_u16(c["n"])
            assert c["encode_off_grid"] == B.encode_route_u16(c["n"], src_aligned=False, lz4_behind=True)
            assert c["decode_off_grid"] == B.decode_route_u16(c["n"], in_aligned=False)
        else:
            assert c["encode"] == B.encode_route_u8(c["n"]) and c["decode"] == B.decode_route_u8(c["n"]) and c["lut"] == B.lut_decode_possible(c["n"])


@pytest.mark.parametrize("case", B.U16_CASES, ids=B.case_id)
def test_plain_blobs_put_their_planes_off_the_16_byte_grid(oracle, case):
    """the decode of a `bitswap1` blob reads the planes behind the header: what the GPU test claims for it (all generic) rests on the
    header's length being no multiple of 16 for every case"""
    blob = oracle.pipeline_encode("bitswap1", B.volume(case), nthreads=2)
    assert (blob.index(HEADER_END) + len(HEADER_END)) % 16 != 0, B.describe(case, "decode_off_grid")


# ---- the data kinds --------------------------------------------------------------------------------------------------------------------------
def test_kinds_are_what_the_gpu_tests_take_them_for():
    for c in B.CASES:
        vol, p = B.volume(c).reshape(-1), _p(c)
        W = vol.dtype.itemsize * 8
        n, seg = c["n"], c["n"] // W
        segs = p[:seg * W].reshape(W, seg) if seg else np.zeros((W, 0), vol.dtype)
        full = (1 << W) - 1
        if c["kind"] == "random" and n >= 1000:
            assert int(vol.max()) >> (W - 1) == 1 and int(np.bitwise_or.reduce(vol)) == full and int(np.bitwise_and.reduce(vol)) == 0, c["name"]
            assert segs.any(axis=1).all(), c["name"]
        if c["kind"] == "ones":
            assert (p == full).all(), c["name"]
        if c["kind"] == "top" and seg:
            assert (segs[0] == full).all() and not segs[1:W - 1].any() and (segs[W - 1] == int("01" * (W // 2), 2)).all(), c["name"]
        if c["kind"] == "onehot":
            idx = B.onehot_indices(n, vol.dtype)
            assert np.array_equal(np.flatnonzero(vol), idx) and all(bin(int(vol[i])).count("1") == 1 for i in idx), c["name"]
            assert {int(vol[i]).bit_length() - 1 for i in idx} == ({b % W for b in B.ONEHOT_BITS} if len(idx) >= 4 else {int(vol[i]).bit_length() - 1 for i in idx})
            # every planted bit lands where the definition says, and nowhere else
            want = np.zeros_like(p)
            for i in idx:
                b = int(vol[i]).bit_length() - 1
                if i < seg * W:
                    want[(W - 1 - b) * seg + i // W] |= 1 << (W - 1 - i % W)
                else:
                    want[i] = vol[i]
            assert np.array_equal(p, want), (c["name"], B.first_difference(p, want))
    # the hand-over voxels of the 16-bit cases: the last the register kernel owns, the first of the rest, the last word's last, the first tail voxel
    assert B.onehot_indices(T + 133, np.uint16) == [0, 1, 15, 16, 127, 128, 2047, 2048, 8191, 8192, 8319, 8320]
    assert B.onehot_indices(3 * T + 399, np.uint16)[-4:] == [3 * T - 1, 3 * T, 3 * T + 383, 3 * T + 384]
    assert B.onehot_indices(7, np.uint8) == [0, 1] and B.onehot_indices(9, np.uint8) == [0, 1, 7, 8]


def test_onehot_pieces_have_one_busy_lane_in_one_plane():
    """in a tile of the in-place transposer a lone planted voxel makes a 1 KiB piece whose only non-zero 16 bytes are one lane's, in one plane:
    the hole decision of bitswap1_u16_regs<true> sees such pieces in every frames volume of two tiles and more, in its last tile among them
    (tile 0 holds nine planted voxels on four planes: its busy pieces have two and three busy lanes, the first and the last lane among them)"""
    for tiles in (1, 2, 3, 5, 7, 33):
        vol = B.frames_volume(tiles, "onehot")
        p = B.planes(vol).view(np.uint8).reshape(16, tiles, 64, 16)                 # plane, tile (piece), lane, the lane's bytes
        busy = p.any(axis=3)                                                        # (plane, tile, lane)
        lanes = busy.sum(axis=2)
        assert set(np.flatnonzero(lanes.any(axis=1)).tolist()) == {0, 7, 8, 15} and 2 <= lanes[:, 0].max() <= 3, tiles
        assert busy[:, 0, 63].any() and busy[:, 0, 0].any(), tiles
        if tiles > 1:
            assert (lanes[:, 1:] == 1).sum() >= 2 and lanes[:, 1:].max() == 1 and lanes[:, tiles - 1].sum() >= 1, tiles
            assert busy[:, tiles - 1, 63].any() and busy[:, 1, 0].any(), tiles


def test_first_difference_names_the_place():
    a = B.make("random", np.uint16, T + 133, 3)
    p = B.planes(a)
    assert B.first_difference(p, p) is None
    bad = a.copy()
    bad[8200] ^= 1 << 3                                      # voxel 8200 = word 512, j = 8; bit 3 lives in segment 12
    d = B.first_difference(B.planes(bad), p)
    assert (d["plane_segment"], d["word"], d["bit"], d["voxel"], d["voxel_bit"], d["differing"]) == (12, 512, 7, 8200, 3, 1), d
    bad = p.copy()
    bad[-1] ^= 0x100
    d = B.first_difference(bad, p)
    assert d["tail_voxel"] == T + 132 and "plane_segment" not in d
    b = B.make("random", np.uint8, 1025, 4)
    bad = b.copy()
    bad[9] ^= 0x80
    d = B.first_difference(B.planes(bad), B.planes(b))
    assert (d["plane_segment"], d["word"], d["bit"], d["voxel"], d["voxel_bit"]) == (0, 1, 6, 9, 7), d
    assert "streams" in B.first_difference(p[:-1], p)


# ---- numpy models of four value-only mistakes: which cases would notice ----------------------------------------------------------------------
def _regs_words(case):
    return case["encode"]["tiles"] * B.TILE_WORDS


def test_models_of_wrong_kernels_are_noticed():
    """(1) the register kernel stores the top plane where the bottom one belongs; (2) the generic kernel starts one word late; (3) the decode
    drops the last tail voxel.  Applied to the definition's output: every case with the branch notices, through first_difference"""
    for c in B.U16_CASES:
        vol, p = B.volume(c).reshape(-1), _p(c)
        n, seg, regs = c["n"], c["n"] // 16, _regs_words(c)
        segs = p[:16 * seg].reshape(16, seg)
        if regs and c["kind"] != "ones":
            bad = p.copy()
            bad[:16 * seg].reshape(16, seg)[15, :regs] = segs[0, :regs]              # bit 15's words stored into segment 15
            d = B.first_difference(bad, p)
            assert d is not None and d["word"] < regs, B.describe(c)
        if c["encode"]["rest_words"] and regs and c["kind"] in ("random", "ones", "top"):
            bad = p.copy()
            bad[:16 * seg].reshape(16, seg)[:, regs] = 0xA5A5                        # the first rest word never written
            d = B.first_difference(bad, p)
            assert d is not None and d["word"] == regs and d["voxel"] // 16 == regs, B.describe(c)
        if c["encode"]["tail"] and c["kind"] in ("random", "ones", "top"):          # (a decoder that leaves the last tail voxel as it found it)
            back = B.voxels(p).copy()
            back[n - 1] ^= 0xA5A5
            assert vol[n - 1] != 0 and not np.array_equal(back, vol), B.describe(c)
    # the onehot kind plants both sides of the hand-over to the rest and the first tail voxel
    vol = B.volume(B.BY_NAME["uint16-%d-onehot" % (T + 133)]).reshape(-1)
    assert vol[T - 1] and vol[T] and vol[T + 127] and vol[T + 128]
