"""Host side of the background-removal head filters rmestbkrd and rmbkrd_neighbor5x5x5 (no GPU): which pipelines are possible, the
configuration strings the header carries, the size bound, and the host_l2_bytes option."""
import ctypes

import numpy as np
import pytest

import bkrd_restate as R

POSSIBLE = ["rmestbkrd->bitswap1->lz4", "rmestbkrd", "rmbkrd_neighbor5x5x5", "rmbkrd_neighbor5x5x5->bitswap1->lz4",
            "rmbkrd_neighbor5x5x5(threshold=40,fraction=0.25)->diff3x3x1->bitswap1->lz4", "frame_shuffle->rmbkrd_neighbor5x5x5->lz4",
            "rmestbkrd->rmbkrd_neighbor5x5x5(threshold=3)->lz4", "rmbkrd_neighbor5x5x5(fraction=1)->lz4(accel=2)",
            "rmbkrd_neighbor5x5x5(threshold=70000)->lz4", "rmbkrd_neighbor5x5x5(threshold=-1,fraction=-2)->lz4", "rmestbkrd->pass_through"]

REFUSED = ["rmbkrd_neighbor5x5x5(fraction=nan)->lz4", "rmbkrd_neighbor5x5x5(fraction=inf)->lz4", "rmbkrd_neighbor5x5x5(fraction=-inf)->lz4",
           "rmbkrd_neighbor5x5x5(fraction=1e50)->lz4", "rmbkrd_neighbor5x5x5(fraction=abc)->lz4", "rmbkrd_neighbor5x5x5(fraction=)->lz4",
           "rmbkrd_neighbor5x5x5(threshold=abc)->lz4", "rmbkrd_neighbor5x5x5(threshold=3000000000)->lz4", "rmbkrd_neighbor5x5x5(threshold)->lz4",
           "rmbkrd_neighbor5x5x5(threshold=)->lz4", "remove_background->lz4", "remove_background(threshold=3)->bitswap1->lz4",
           "rmestbkrd->remove_background->lz4", "lz4->rmestbkrd", "bitswap1->lz4->rmbkrd_neighbor5x5x5"]


@pytest.mark.parametrize("pipeline", POSSIBLE + ["rmestbkrd->quantiser->bitswap1->lz4"])
def test_possible(sqy, pipeline):
    lib = sqy.lib()
    assert lib.SQY_Pipeline_Possible_UI16(pipeline.encode())
    assert lib.SQY_Pipeline_Possible(pipeline.encode(), 2)
    if "quantiser" not in pipeline:
        assert lib.SQY_Pipeline_Possible_UI8(pipeline.encode())
        assert lib.SQY_Pipeline_Possible(pipeline.encode(), 1)


@pytest.mark.parametrize("pipeline", REFUSED)
def test_refused(sqy, pipeline):
    lib = sqy.lib()
    assert not lib.SQY_Pipeline_Possible_UI16(pipeline.encode())
    assert not lib.SQY_Pipeline_Possible_UI8(pipeline.encode())
    vol = np.ones((8, 8, 8), np.uint16)
    assert sqy.encode(pipeline, vol)[0] == 1                                   # (refused before any device is looked for)


def _header_build(sqy, pipeline, dtype, shape, nbytes):
    lib = sqy.lib()
    shp = (ctypes.c_long * len(shape))(*shape)
    need = ctypes.c_long(0)
    rc = lib.SQYAMD_Header_Build(pipeline.encode(), ctypes.c_int(np.dtype(dtype).itemsize), shp, ctypes.c_uint(len(shape)),
                                 ctypes.c_long(nbytes), None, ctypes.byref(need))
    if rc:
        return rc, None
    buf = ctypes.create_string_buffer(need.value)
    rc = lib.SQYAMD_Header_Build(pipeline.encode(), ctypes.c_int(np.dtype(dtype).itemsize), shp, ctypes.c_uint(len(shape)),
                                 ctypes.c_long(nbytes), buf, ctypes.byref(need))
    return rc, buf.raw[:need.value]


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("pipeline", POSSIBLE)
def test_header_names(sqy, oracle, pipeline, dtype):
    shape = (16, 32, 48)
    rc, hdr = _header_build(sqy, pipeline, dtype, shape, 12345)
    assert rc == 0
    assert hdr == oracle.header_pack(dtype, shape, R.full_pipename(oracle, pipeline, dtype), 12345)


def test_header_config_strings(sqy, oracle):
    cases = [("rmbkrd_neighbor5x5x5->lz4", np.uint16, "rmbkrd_neighbor5x5x5(threshold=1,fraction=0.500000)"),
             ("rmbkrd_neighbor5x5x5(threshold=70000)", np.uint16, "rmbkrd_neighbor5x5x5(threshold=4464,fraction=0.500000)"),
             ("rmbkrd_neighbor5x5x5(threshold=70000)", np.uint8, "rmbkrd_neighbor5x5x5(threshold=112,fraction=0.500000)"),
             ("rmbkrd_neighbor5x5x5(threshold=-1,fraction=0.25)", np.uint16, "rmbkrd_neighbor5x5x5(threshold=65535,fraction=0.250000)"),
             ("rmbkrd_neighbor5x5x5(fraction=0.1)", np.uint8, "rmbkrd_neighbor5x5x5(threshold=1,fraction=0.100000)"),
             ("rmbkrd_neighbor5x5x5(fraction=1e-9,threshold=7)", np.uint8, "rmbkrd_neighbor5x5x5(threshold=7,fraction=0.000000)"),
             ("rmestbkrd", np.uint16, "rmestbkrd")]
    for pipeline, dtype, first in cases:
        rc, hdr = _header_build(sqy, pipeline, dtype, (8, 8, 8), 0)
        assert rc == 0
        name = oracle.header_unpack(hdr + b"\0")["pipename"]
        assert name.split("->")[0] == first, (pipeline, name)
        # the name parses back to itself
        rc2, hdr2 = _header_build(sqy, name, dtype, (8, 8, 8), 0)
        assert rc2 == 0 and hdr2 == hdr


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("pipeline", POSSIBLE)
def test_max_compressed_length(sqy, oracle, pipeline, dtype):
    for shape in ((16, 32, 48), (512, 1024, 1024), (3, 5, 7)):
        n = int(np.prod(shape))
        assert sqy.max_compressed_length(pipeline, shape, dtype) == R.max_encoded_size(oracle, pipeline, n * np.dtype(dtype).itemsize, dtype)


def test_host_l2_bytes_option(sqy):
    detected = sqy.get_option("host_l2_bytes")
    assert 0 <= detected < (1 << 32)
    for v in (1, 0, 12345, (1 << 32) - 1):
        with sqy.option("host_l2_bytes", v):
            assert sqy.get_option("host_l2_bytes") == v
        assert sqy.get_option("host_l2_bytes") == detected
    for bad in (-1, 1 << 32):
        with pytest.raises(ValueError):
            sqy.set_option("host_l2_bytes", bad)
    assert sqy.get_option("host_l2_bytes") == detected


def test_restatement_geometry():
    """the refusals the library shares with the restatement (sqy::neighbor5_geometry_defined)"""
    assert R.neighbor5_defined((10, 5, 6)) and R.neighbor5_defined((16, 16, 16)) and R.neighbor5_defined((2, 6, 9))
    for shape in ((3, 5, 6), (8, 5, 5), (8, 4, 9), (8, 9, 4), (5, 5, 5), (20, 5, 5)):
        assert not R.neighbor5_defined(shape), shape
    # an empty offset list is defined: all zeros
    v = np.full((2, 8, 8), 9, np.uint16)
    assert not R.neighbor5(v, 1, 0.5).any()


def _neighbor5_loops(vol, threshold, fraction):
    """flatten_to_neighborhood_scheme::encode written out as the reference's loops (offsets list, halo_size_x, count_neighbors_if)"""
    Z, Y, X = vol.shape
    flat = vol.reshape(-1)
    N = flat.size
    offsets = [z * Y * X + y * X + 2 for z in range(2, X - 2) for y in range(2, Y - 2) if z * Y * X + y * X + 2 < N]
    halo_size_x = X - 3                                          # non_halo_end(2) - non_halo_begin(2) + 1
    cut = np.float32(fraction) * np.float32(124)
    out = np.zeros_like(flat)
    for o in offsets:
        for index in range(halo_size_x):
            c = o + index
            if flat[c] < threshold:
                continue
            n = 0
            for dz in range(-2, 3):
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        i = c + dz * Y * X + dy * X + dx
                        if i != c and i < N and flat[i] < threshold:    # (past the end: not counted)
                            n += 1
            out[c] = 0 if np.float32(n) > cut else flat[c]
    return out.reshape(vol.shape)


@pytest.mark.parametrize("shape", [(7, 7, 7), (4, 6, 11), (9, 8, 6), (10, 5, 6), (6, 9, 9)])
def test_restatement_matches_the_reference_loops(shape):
    rng = np.random.default_rng(sum(shape))
    vol = rng.integers(0, 10, shape).astype(np.uint16)
    for t, f in ((5, 0.5), (3, 0.25), (8, 0.75), (5, 0.0)):
        assert np.array_equal(R.neighbor5(vol, t, np.float32(f)), _neighbor5_loops(vol, t, f)), (shape, t, f)


# ---- the constructions of tests/bkrd_seam_cases.py, held to what they claim (tests/test_gpu_background_seams.py runs them) ----------------
import bkrd_seam_cases as S                                                   # noqa: E402
from ref_stage_inputs import PLANTED_SEAMS, SPREAD_STARTS, planted_sites, stage_input  # noqa: E402

SEAM_SHAPES = [(72, 6, 70), (70, 20, 68), (129, 18, 70), (136, 18, 134)]


@pytest.mark.parametrize("shape", SEAM_SHAPES + S.CHUNK_END_SHAPES)
def test_direct_count_equals_the_box_sums(shape):
    """the 125 offsets added one by one against the separated sum the kernel shares with the restatement: equal at every voxel, the
    centres among them, on volumes of more than one tile and chunk"""
    centres = R.neighbor5_centres(shape)
    assert centres[64:].any() or shape in ((70, 6, 66),)                       # centres behind the first chunk (but for the zero-fill shape)
    for vol, t in ((stage_input("low80", np.uint16, shape, 1), 36), (stage_input("low80", np.uint8, shape, 2), 18),
                   (stage_input("planted", np.uint16, shape, 3), 100)):
        direct, box = R.neighbor5_counts_direct(vol, t), R.neighbor5_counts(vol, t)
        assert np.array_equal(direct[centres], box[centres]) and np.array_equal(direct, box), (shape, t)
        assert np.array_equal(S.neighbor5_direct(vol, t, 0.25)[0], R.neighbor5(vol, t, 0.25)), (shape, t)


def test_low80_cuts_every_chunk_of_the_largest_shape():
    """(136, 18, 134), fraction 0.5: each of the three z chunks has thousands of centres on both sides of the cut at threshold 40, and
    hundreds (the last chunk has four planes of centres) at the goldens' 36"""
    shape = (136, 18, 134)
    vol = stage_input("low80", np.uint16, shape, 5)
    for t in (40, 36):
        want, n = S.neighbor5_direct(vol, t, 0.5)
        at = R.neighbor5_centres(shape) & (vol >= t)
        for zs in (0, 64, 128):
            chunk = np.zeros(shape, bool)
            chunk[zs:zs + 64] = True
            least = 1000 if t == 40 else 400
            assert (at & chunk & (want != 0)).sum() > least and (at & chunk & (want == 0)).sum() > least, (t, zs)


@pytest.mark.parametrize("shape,seeds", S.PLANTED)
def test_planted_volumes_reach_every_seam(shape, seeds):
    Z, Y, X = shape
    seen = {f: set() for f in S.PLANTED_FRACTIONS}
    for seed in seeds:
        singles, pairs = planted_sites(shape, seed)
        for z, y, x in S.planted_voxels(shape, seed):                          # coordinates within 3 of a seam, in every axis
            assert min(abs(z + .5 - s) for s in PLANTED_SEAMS["z"]) < 3 and abs(y + .5 - 16) < 3 and min(abs(x + .5 - s) for s in PLANTED_SEAMS["x"]) < 3
        vol = stage_input("planted", np.uint16, shape, seed)
        assert (vol == 10).sum() == len(singles) + 2 * len(pairs)
        n = R.neighbor5_counts_direct(vol, S.PLANTED_THRESHOLD)
        assert n.max() == (2 if pairs else 1)                                    # neighbourhoods of different sites are disjoint
        lone = stage_input("planted", np.uint16, shape, seed)
        for p in pairs:
            lone[p[1]] = 200
        assert R.neighbor5_counts_direct(lone, S.PLANTED_THRESHOLD).max() == 1
        for f in S.PLANTED_FRACTIONS:
            seen[f] |= S.seam_outcomes(vol, seed, f)
    wanted = S.seam_outcomes_wanted(shape)
    assert {(a, s) for a, s, _, _ in wanted} >= ({("z", 64), ("x", 64), ("y", 16)} | ({("z", 128), ("x", 128)} if Z > 130 else set()))
    for f in S.PLANTED_FRACTIONS:
        assert seen[f] >= wanted, (f, sorted(wanted - seen[f]))


def test_planted_names_the_voxel_of_a_count_lost_between_chunks():
    """a model of the kernel's chunk walk whose ring starts empty at zs (frames zs-2 and zs-1 not loaded): the first voxel the planted
    test would name lies in the first plane of the second chunk"""
    shape, seed = (136, 18, 134), 0
    vol = stage_input("planted", np.uint16, shape, seed)
    want, n = S.neighbor5_direct(vol, S.PLANTED_THRESHOLD, 0.0)
    b = (vol < S.PLANTED_THRESHOLD).astype(np.int16)
    got = want.copy()
    for zs in (64, 128):                                                          # what the two lost planes would have added
        lost = np.zeros(shape, np.int16)
        for z in (zs, zs + 1):
            for p in range(z - 2, zs):
                only = np.zeros(shape, np.int16)
                only[p] = b[p]
                lost[z] += R.neighbor5_counts_direct(200 - 190 * only, S.PLANTED_THRESHOLD)[z]
        broken = n - lost
        keep = R.neighbor5_centres(shape) & (vol >= S.PLANTED_THRESHOLD) & ~(broken > 0)
        got[zs:zs + 2] = np.where(keep, vol, 0)[zs:zs + 2]
    diff = S.first_difference(got, want, n)
    assert diff is not None and diff[0] == 64 and diff[3:] == (200, 0, 1), diff


def test_spread_volumes_leave_the_window():
    vol = S.spread_volume(S.WINDOW_SHAPE, np.uint16)
    segs = S.face_segments(vol, S.L2_ALL)
    bases = {S.window_base(int(seg[0])) for _, _, seg in segs}
    assert bases >= {0, 1, 40000 - 8192, 57343 - 8192, 65536 - S.WIN}                # the switch, open bases, the clamp
    assert {int(seg[0]) for _, _, seg in segs} == set(SPREAD_STARTS)
    for (_, piece, seg), (_, piece2, seg2) in zip(segs, segs[1:]):
        if piece == piece2:
            assert seg[0] != seg2[0]                                                   # neighbours overlap in global bins, from different bases
    for _, _, seg in segs:
        if len(seg) < 8:
            continue
        v0, wb = int(seg[0]), S.window_base(int(seg[0]))
        assert ((seg >= wb) & (seg < wb + S.WIN)).sum() >= len(seg) // 2
        assert (seg < wb).any() == (v0 > 8192) and (seg >= wb + S.WIN).any() == (v0 + 8193 < 65536), v0
    assert sum(len(seg) for face, _, seg in segs if face == 2) == 3 * 520 and 520 > 2 * 256
    # the second pass of the 128 workgroups, on data like the above
    for shape, l2, portion in [(S.STRIDE_SHAPE, S.L2_ALL, 33800)] + [(S.PORTION_SHAPE, l2, p) for p, l2 in S.PORTION_L2.items()]:
        assert R.face_portion(shape[1] * shape[2], l2) == portion > 128 * 256 - 1
    for shape in (S.WINDOW_SHAPE, S.STRIDE_SHAPE, S.PORTION_SHAPE):
        for dtype in (np.uint16, np.uint8):
            v = S.spread_volume(shape, dtype)
            sup = [float(R.support(h)) for h in R.face_histograms(v, S.L2_ALL)]
            assert len(set(sup)) == 4 and min(sup) == sup[3], sup                      # four supports, the last decides
            out = R.rmestbkrd(v, S.L2_ALL)
            assert 0.2 < (out != 0).mean() < 0.8


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_support_volumes_stop_where_they_mean_to(dtype):
    cases = S.support_cases(dtype)
    stops = set()
    for lo, hi, k in cases:
        vol = S.support_volume(dtype, lo, hi, k)
        m, t = S.support_crossing(lo, hi, k), S.support_threshold(lo, hi, k)
        for h in R.face_histograms(vol, S.L2_ALL):
            assert int(h[lo]) + int(h[hi]) == h.sum() and int(h[hi]) in ((10, 3) if k == 10 else (9, 2))
            running = np.cumsum(h, dtype=np.uint64).astype(np.float64) / float(h.sum())
            assert int(np.nonzero(running > np.float64(np.float32(0.99)))[0][0]) == m, (lo, hi, k)
        assert R.rmestbkrd_threshold(vol, S.L2_ALL) == t, (lo, hi, k)
        inner = vol[1:-1, 1:-1]
        assert all((inner == x).any() for x in (t - 1, t, t + 1) if 0 <= x <= np.iinfo(dtype).max)
        stops.add(m)
    assert stops >= set(S.SUPPORT_BINS[dtype])
