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
