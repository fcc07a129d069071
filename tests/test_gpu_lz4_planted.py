"""The planted LZ4 streams (tests/lz4_planted.py; test_lz4_planted_host.py shows on the CPU what each of them contains) through every
instantiation of lz4_chunks_kernel: the lean kernel and the dense one (chunked layout, one volume per case), block-linked frames (the 256 KiB
cases as one volume, nthreads = 1, block-parallel and walked), the ACCEL instantiation (parity only: the features belong to acceleration 1),
frames in place behind bitswap1 (with and without the noise digest), the TABLE instantiations (one batch call over all cases) and the
device entry point on resident uint16 volumes.  Every blob is compared byte for byte with the oracle's and decoded back; a failure names the
case and, through lz4_planted.explain, the first sequence at which the block differs from liblz4's -- the case's name and its features
(lz4_planted.cases) say which boundary of the parse lies there."""
import numpy as np
import pytest

import lz4_planted as P
from test_gpu_encode_batch import _batch, _profile

pytestmark = pytest.mark.gpu

CASES = P.cases()
NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}
BIG = [c for c in CASES if len(c["data"]) == 262144]
DENSE_KERNEL = ("dense:whole", "dense:batch-ends") + tuple("dense:tail=%d" % t for t in P.DENSE_TAILS)
DENSE = [c["name"] for c in CASES if any(f in DENSE_KERNEL for f in c["features"])]


def _pipe(cfg):
    return "lz4(%s)" % cfg if cfg else "lz4"


def _same(oracle, got, want, what, names=None):
    if got != want:
        msg = P.explain(got, want, oracle.header_unpack(want)["size"])
        if names and msg.startswith("block "):
            i = int(msg.split(":")[0].split()[1])
            msg = "%s (%s)" % (msg, names[i] if i < len(names) else "?")
        pytest.fail("%s: %s" % (what, msg), pytrace=False)


def _roundtrip(sqy, oracle, pipe, vol, nthreads, what, names=None):
    want = oracle.pipeline_encode(pipe, vol, nthreads=nthreads)
    rc, blob = sqy.encode(pipe, vol, nthreads=nthreads)
    assert rc == 0, what
    _same(oracle, blob, want, what, names)
    rc, back = sqy.decode(blob)
    assert rc == 0 and np.array_equal(back, vol), what
    return want


@pytest.mark.parametrize("name", NAMES)
def test_chunked_one_volume_per_case(sqy, oracle, name):
    c = BY_NAME[name]
    vol = np.frombuffer(c["data"], np.uint8).reshape(1, 1, -1)
    _roundtrip(sqy, oracle, _pipe(c["config"]), vol, 2, (name, c["features"]))


@pytest.mark.parametrize("name", DENSE)
def test_dense_cases_reach_the_dense_kernel(sqy, oracle, name):
    c = BY_NAME[name]
    vol = np.frombuffer(c["data"], np.uint8).reshape(1, 1, -1)
    (_, p) = _profile(sqy, lambda: _roundtrip(sqy, oracle, _pipe(c["config"]), vol, 2, name))
    assert p.get("lz4_chunks_dense", (0, 0))[1] >= 1, (name, sorted(p))


@pytest.fixture(scope="module")
def big():
    return np.frombuffer(b"".join(c["data"] for c in BIG), np.uint8).reshape(1, 1, -1)


BIG_NAMES = [c["name"] for c in BIG]


def test_big_cases_as_one_volume_chunked(sqy, oracle, big):
    _roundtrip(sqy, oracle, "lz4", big, 2, "chunked", BIG_NAMES)


def test_big_cases_as_one_volume_linked(sqy, oracle, options, big):
    """one block-linked frame: offsets now reach into the case in front"""
    want = _roundtrip(sqy, oracle, "lz4", big, 1, "linked, block-parallel", BIG_NAMES)
    options("block_parallel", 0)
    rc, blob = sqy.encode("lz4", big, nthreads=1)
    assert rc == 0
    _same(oracle, blob, want, "linked, frame walk", BIG_NAMES)


@pytest.mark.parametrize("accel", [-1, -3])
@pytest.mark.parametrize("nthreads", [2, 1])
def test_big_cases_accelerated(sqy, oracle, big, accel, nthreads):
    _roundtrip(sqy, oracle, "lz4(accel=%d)" % accel, big, nthreads, ("accel", accel, nthreads), BIG_NAMES)


@pytest.mark.parametrize("digest", [1, 0])
@pytest.mark.parametrize("nthreads", [2, 1])
def test_big_cases_behind_bitswap1(sqy, oracle, options, big, nthreads, digest):
    """the same bytes as bit planes of a uint16 volume: frames in place with their stride, the noise digest, holes, the duplicate search"""
    stream = big.reshape(-1).view(np.uint16)
    vol = oracle.bitswap1_decode(stream).reshape(len(BIG), 256, 512)
    assert np.array_equal(np.ascontiguousarray(oracle.bitswap1_encode(vol)).reshape(-1).view(np.uint16), stream)
    if not digest:
        options("noise_digest", 0)
    _roundtrip(sqy, oracle, "bitswap1->lz4", vol, nthreads, ("bitswap1->lz4", nthreads, digest), BIG_NAMES)


def test_batch_all_cases_in_one_call(sqy, oracle):
    import torch
    dev = torch.device("cuda", 0)
    vols = [np.frombuffer(c["data"], np.uint8).reshape(1, 1, -1) for c in CASES]
    want = [oracle.pipeline_encode("lz4", v, 2) for v in vols]
    ((rc, blobs), p) = _profile(sqy, lambda: _batch(sqy, "lz4", vols, dev))
    assert rc == 0
    assert p["batch_lz4_chunks"][1] == 1 and p["batch_lz4_chunks_dense"][1] >= 1, p
    for c, v, b, w in zip(CASES, vols, blobs, want):
        _same(oracle, b, w, ("batch", c["name"], c["features"]))
        rc, back = sqy.decode(b)
        assert rc == 0 and np.array_equal(back, v), c["name"]


@pytest.mark.parametrize("name", ["star-262144-cut", "catch-up", "dense-whole-65536"])
def test_device_entry_point_resident_uint16(sqy, oracle, name):
    import torch
    dev = torch.device("cuda", 0)
    c = BY_NAME[name]
    vol = np.frombuffer(c["data"], np.uint8).view(np.uint16).reshape(1, 1, -1)
    pipe = _pipe(c["config"])
    want = oracle.pipeline_encode(pipe, vol, 2)
    d_vol = torch.from_numpy(vol.copy()).to(dev)
    cap = sqy.max_compressed_length(pipe, vol.shape, np.uint16)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    rc, n = sqy.encode_device(pipe, d_vol.data_ptr(), vol.shape, np.uint16, out.data_ptr(), cap)
    assert rc == 0
    _same(oracle, bytes(out[:n].cpu().numpy().tobytes()), want, (name, "device"))
    rc, back = sqy.decode(want)
    assert rc == 0 and np.array_equal(back, vol)
