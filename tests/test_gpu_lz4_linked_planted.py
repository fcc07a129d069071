"""The streams planted at block borders (tests/lz4_linked_planted.py; test_lz4_linked_planted_host.py shows on the CPU what each contains and
which wrong rule it would expose) through the block-linked encoder: the block-parallel guess with its verify and redo rounds, the same with
a worthless guess (warm-up 0: every block parsed again by the dense instantiation from the table on record), the one-wavefront frame walk,
the chunked layout of the multi-block-frame configurations, the ACCEL instantiation (parity only), every stream of a block size as one
volume (foreign history in front of every case), the same behind bitswap1, and the device entry point.  Every blob is compared byte for
byte with the oracle's BEFORE anything is decoded; a failure names the case, its features and, through lz4_planted.explain, the first block
and sequence that differ.  Then the blob goes back through the decoder (block-parallel and walked)."""
import numpy as np
import pytest

import lz4_planted as P
import lz4_linked_planted as L
from test_gpu_encode_batch import _profile

pytestmark = pytest.mark.gpu

CASES = L.cases()
NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}

# Block k begins with a match into block k - 1 (REDO_FEATURES).  The guess of block k's table is a parse of the 64 KiB in front of it from an
# empty table; where it differs from the table block k - 1 really left, block k is parsed again.  Stated per case and held against the
# first run on the MI355X:
#   * 64 KiB blocks: the warm-up is block k - 1 alone, the true table also holds what block k - 2 entered -- the guess fails and
#     lz4_linked_redo runs, in every such case;
#   * larger blocks (NO_REDO): the last 64 KiB of block k - 1 are quiet filler and the planted sources, which the warm-up enters exactly
#     as the real parse did, and nothing older is in reach -- the guess comes out right, so no redo is expected of them.  The byte
#     compare is the same; warm-up 0 sends the same blocks through the redo runs.
REDO_FEATURES = ("start:found-at-second-byte", "start:first-byte-not-searched", "start:first-byte-is-a-source", "prev:cut-at-border", "border:off=65535")
NO_REDO = ("off=65535-ext256", "off=1000-ext256", "first-byte-not-searched-ext256", "first-byte-is-a-source-ext256", "cut-at-border-ext256",
           "off=65535-ext1024", "off=65535-ext4096")
EXPECT_REDO = tuple(c["name"] for c in CASES if c["nthreads"] == 1 and any(f in REDO_FEATURES for f in c["features"]) and c["name"] not in NO_REDO)

_want = {}


def _vol(c):
    return np.frombuffer(c["data"], np.uint8).reshape(1, 1, -1)


def _oracle_blob(oracle, pipe, vol, nthreads, key):
    k = (key, pipe, nthreads)
    if k not in _want:
        _want[k] = oracle.pipeline_encode(pipe, vol, nthreads=nthreads)
    return _want[k]


def _same(oracle, got, want, what, names=None):
    if got != want:
        msg = P.explain(got, want, oracle.header_unpack(want)["size"])
        if names and msg.startswith("block "):
            i = int(msg.split(":")[0].split()[1])
            msg = "%s (in %s)" % (msg, names(i))
        pytest.fail("%s: %s" % (what, msg), pytrace=False)


def _encode(sqy, oracle, pipe, vol, nthreads, want, what, names=None):
    (rc, blob), prof = _profile(sqy, lambda: sqy.encode(pipe, vol, nthreads=nthreads))
    assert rc == 0, what
    _same(oracle, blob, want, what, names)
    return blob, set(prof)


def _decode(sqy, blob, vol, what):
    rc, back = sqy.decode(blob)
    assert rc == 0 and np.array_equal(back, vol), what


@pytest.mark.parametrize("name", NAMES)
def test_case_block_parallel_warmup0_and_walk(sqy, oracle, options, name):
    c = BY_NAME[name]
    vol, pipe, nt = _vol(c), L.pipe_of(c), c["nthreads"]
    what = (name, c["features"])
    want = _oracle_blob(oracle, pipe, vol, nt, name)
    blob, prof = _encode(sqy, oracle, pipe, vol, nt, want, what + ("default",))
    if nt == 1:
        assert "lz4_linked_blocks" in prof and "lz4_linked_verify" in prof, (name, sorted(prof))
        if name in EXPECT_REDO:
            assert "lz4_linked_redo" in prof, (name, "block k starts with a match into block k - 1: the guess was expected to fail")
    else:
        assert "lz4_linked" in prof and "lz4_linked_verify" not in prof, (name, sorted(prof))      # frames of two blocks are walked
    _decode(sqy, blob, vol, what)
    options("block_parallel_warmup", 0)
    _, prof = _encode(sqy, oracle, pipe, vol, nt, want, what + ("warm-up 0",))
    if nt == 1:
        assert "lz4_linked_redo" in prof and "lz4_linked_verify" in prof, (name, sorted(prof))
    options("block_parallel", 0)
    _, prof = _encode(sqy, oracle, pipe, vol, nt, want, what + ("walk",))
    assert "lz4_linked" in prof and "lz4_linked_verify" not in prof, (name, sorted(prof))
    _decode(sqy, blob, vol, what + ("decoded with block_parallel = 0",))


def test_redo_expectations_name_cases_of_the_right_kind():
    assert len(EXPECT_REDO) >= 6 and all(L.CLASS[BY_NAME[n]["cls"]][1] == 65536 for n in EXPECT_REDO)
    for name in NO_REDO:
        assert any(f in REDO_FEATURES for f in BY_NAME[name]["features"]) and L.CLASS[BY_NAME[name]["cls"]][1] > 65536, name


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["cls"] in ("prefix64", "prefix256", "pair64", "chunked64")])
def test_multi_block_frames_chunked(sqy, oracle, name):
    """the configurations whose frames hold several blocks, under nthreads = 2: a frame every framestep bytes, each a fresh stream"""
    c = BY_NAME[name]
    vol, pipe = _vol(c), L.pipe_of(c)
    want = _oracle_blob(oracle, pipe, vol, 2, name)
    blob, _ = _encode(sqy, oracle, pipe, vol, 2, want, (name, c["features"], "nthreads = 2"))
    _decode(sqy, blob, vol, name)


def test_frame_history_ends_at_a_frame(sqy, oracle):
    """the same bytes: one frame finds the copy at s_k + 1, a frame that starts at s_k does not -- the two blobs differ, each is its oracle's"""
    a, b = BY_NAME["frame-one-pair64"], BY_NAME["frame-no-history-chunked64"]
    assert a["data"] == b["data"] and L.pipe_of(a) == L.pipe_of(b)
    vol, pipe = _vol(a), L.pipe_of(a)
    w1, w2 = _oracle_blob(oracle, pipe, vol, 1, a["name"]), _oracle_blob(oracle, pipe, vol, 2, b["name"])
    hs = oracle.header_unpack(w1)["size"]
    assert P.frame_blocks(w1[hs:])[2] != P.frame_blocks(w2[hs:])[2]
    _encode(sqy, oracle, pipe, vol, 1, w1, "one frame")
    _encode(sqy, oracle, pipe, vol, 2, w2, "a frame per two blocks")


def test_catchup_stops_or_runs_on_by_configuration(sqy, oracle):
    """the same bytes under external-dictionary and under prefix mode: the catch-up stops at s_k or walks over it"""
    for ext, pre in (("stops-at-block-start-ext64", "through-block-start-prefix64"), ("stops-at-block-start-ext256", "through-block-start-prefix256")):
        a, b = BY_NAME[ext], BY_NAME[pre]
        assert a["data"] == b["data"]
        vol = _vol(a)
        w1, w2 = _oracle_blob(oracle, L.pipe_of(a), vol, 1, ext), _oracle_blob(oracle, L.pipe_of(b), vol, 1, pre)
        assert P.frame_blocks(w1[oracle.header_unpack(w1)["size"]:])[2] != P.frame_blocks(w2[oracle.header_unpack(w2)["size"]:])[2]
        _encode(sqy, oracle, L.pipe_of(a), vol, 1, w1, ext)
        _encode(sqy, oracle, L.pipe_of(b), vol, 1, w2, pre)


@pytest.mark.parametrize("accel", [-1, -3])
def test_256k_cases_accelerated(sqy, oracle, accel):
    """liblz4's acceleration through the ACCEL instantiation, nthreads = 1: parity only, the features belong to acceleration 1"""
    for c in CASES:
        if c["cls"] != "ext256":
            continue
        vol, pipe = _vol(c), "lz4(accel=%d)" % accel
        want = _oracle_blob(oracle, pipe, vol, 1, c["name"])
        blob, _ = _encode(sqy, oracle, pipe, vol, 1, want, (c["name"], "accel", accel))
        _decode(sqy, blob, vol, c["name"])


# ---- every stream of a block size as ONE volume: parity only, the features need not survive a foreign history ---------------------------
def _joined(B):
    """(bytes, names per block): the whole-block streams of block size B; the 64 KiB volume also takes 256 KiB streams, cut into its blocks"""
    parts = [c for c in CASES if L.CLASS[c["cls"]][1] == B and len(c["data"]) % B == 0]
    if B == 65536:
        parts += [c for c in CASES if c["cls"] == "ext256"][:8]
    names = [c["name"] for c in parts for _ in range(len(c["data"]) // B)]
    tail = BY_NAME["last-17-ext64"]["data"][-17:] if B == 65536 else b""
    return np.frombuffer(b"".join(c["data"] for c in parts) + tail, np.uint8).reshape(1, 1, -1), names


@pytest.fixture(scope="module")
def joined64():
    return _joined(65536)


@pytest.fixture(scope="module")
def joined256():
    return _joined(262144)


def _rounds(err):
    """the run counts of the verify / redo rounds that block_parallel_stats printed for two calls: the first call's, and both alike"""
    rounds = [ln for ln in err.splitlines() if "lz4 block-parallel: round" in ln]
    nruns = [int(ln.split(" runs")[0].split()[-1]) for ln in rounds]
    first = nruns[:len(nruns) // 2]
    assert first and first[-1] == 0 and all(x >= y for x, y in zip(first, first[1:])), (first, err[-300:])
    assert nruns[len(nruns) // 2:] == first, "both calls go through the same rounds"
    return first


def _joined_test(sqy, oracle, options, capfd, joined, pipe, key, guess_fails):
    """guess_fails: with 64 KiB blocks the default guess (block k - 1 alone) misses what block k - 2 entered and blocks are parsed again; with
    256 KiB blocks the first run on the MI355X showed every guess of this volume right (round 0: 0 of 65 blocks) -- there the redo runs are
    reached by warm-up 0 alone"""
    vol, names = joined

    def who(i):
        return names[i] if i < len(names) else "the tail"
    want = _oracle_blob(oracle, pipe, vol, 1, key)
    options("block_parallel_stats", 1)
    capfd.readouterr()
    for run in range(2):                                                # (the second call reuses the workspace: stale tables and lists in it)
        blob, prof = _encode(sqy, oracle, pipe, vol, 1, want, (key, "default", run), who)
        assert "lz4_linked_blocks" in prof and "lz4_linked_verify" in prof and ("lz4_linked_redo" in prof) == guess_fails, sorted(prof)
    first = _rounds(capfd.readouterr().err)
    assert (first[0] >= 1) == guess_fails, first
    _decode(sqy, blob, vol, key)
    options("block_parallel_warmup", 0)
    for run in range(2):
        _, prof = _encode(sqy, oracle, pipe, vol, 1, want, (key, "warm-up 0", run), who)
        assert "lz4_linked_redo" in prof, sorted(prof)
    first = _rounds(capfd.readouterr().err)
    assert first[0] >= 1, first
    options("block_parallel_stats", 0)
    options("block_parallel", 0)
    for run in range(2):
        _, prof = _encode(sqy, oracle, pipe, vol, 1, want, (key, "walk", run), who)
        assert "lz4_linked_verify" not in prof
    _decode(sqy, blob, vol, (key, "decoded with block_parallel = 0"))


def test_all_64k_streams_as_one_volume(sqy, oracle, options, capfd, joined64):
    assert len(joined64[1]) > 150 and joined64[0].size % 65536 == 17
    _joined_test(sqy, oracle, options, capfd, joined64, "lz4(blocksize_kb=64,framestep_kb=64)", "joined64", True)


def test_all_64k_streams_as_one_volume_prefix_mode(sqy, oracle, options, capfd, joined64):
    _joined_test(sqy, oracle, options, capfd, joined64, "lz4(blocksize_kb=64)", "joined64-prefix", True)


def test_all_256k_streams_as_one_volume(sqy, oracle, options, capfd, joined256):
    assert len(joined256[1]) >= 60
    _joined_test(sqy, oracle, options, capfd, joined256, "lz4", "joined256", False)


@pytest.mark.parametrize("digest", [1, 0])
def test_256k_volume_behind_bitswap1(sqy, oracle, options, joined256, digest):
    """the same bytes as the bit planes of a uint16 volume, nthreads = 1: linked blocks read with the planes' stride, with and without the
    noise digest"""
    stream = joined256[0].reshape(-1).view(np.uint16)
    vol = oracle.bitswap1_decode(stream).reshape(-1, 256, 512)
    assert np.array_equal(np.ascontiguousarray(oracle.bitswap1_encode(vol)).reshape(-1).view(np.uint16), stream)
    if not digest:
        options("noise_digest", 0)
    want = _oracle_blob(oracle, "bitswap1->lz4", vol, 1, "joined256-bitswap1")
    names = joined256[1]
    blob, _ = _encode(sqy, oracle, "bitswap1->lz4", vol, 1, want, ("bitswap1->lz4", digest), lambda i: names[i] if i < len(names) else "?")
    _decode(sqy, blob, vol, ("bitswap1->lz4", digest))


@pytest.mark.parametrize("name", ["off=65535-ext64", "stored-literals-ext256", "through-block-start=300-prefix256"])
def test_device_entry_point_resident_uint16(sqy, oracle, name):
    import torch
    dev = torch.device("cuda", 0)
    c = BY_NAME[name]
    vol = np.frombuffer(c["data"], np.uint8).view(np.uint16).reshape(1, 1, -1)
    pipe = L.pipe_of(c)
    want = _oracle_blob(oracle, pipe, vol, 1, name + "/u16")
    d_vol = torch.from_numpy(vol.copy()).to(dev)
    cap = sqy.max_compressed_length(pipe, vol.shape, np.uint16)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    rc, n = sqy.encode_device(pipe, d_vol.data_ptr(), vol.shape, np.uint16, out.data_ptr(), cap, nthreads=1)
    assert rc == 0
    _same(oracle, bytes(out[:n].cpu().numpy().tobytes()), want, (name, "device"))
    rc, back = sqy.decode(want)
    assert rc == 0 and np.array_equal(back, vol)
