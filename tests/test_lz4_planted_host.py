"""The planted LZ4 streams (tests/lz4_planted.py) on the CPU: every stream is shown, against the oracle's block, to contain the features it
claims, and the list as a whole to claim every feature -- in every chunk length class where a feature is starred.  This is the cap on what
the GPU test (test_gpu_lz4_planted.py) may leave out: nothing.  The streams and the oracle's blocks are pinned by digests
(tests/golden/lz4_planted.json, written by oracle/gen_golden.py --lz4-planted), so that a builder or an oracle that drifts fails here.

liblz4 searches position n - 12 and no further (mflimitPlusOne = n - 11 is the first position it does not probe), so the chunk-end
features are "found at n - 13", "found at n - 12: the last searched position" and "planted at n - 11: not searched"."""
import hashlib
import json
import os

import numpy as np
import pytest

import lz4_planted as P

CASES = P.cases()
NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4_planted.json")


def _block(oracle, data):
    return oracle.lz4_block_compress(data, cap=P.block_cap(len(data)))


@pytest.mark.parametrize("name", NAMES)
def test_case_holds_its_features(oracle, name):
    c = BY_NAME[name]
    data = c["data"]
    n = len(data)
    blk = _block(oracle, data)
    assert oracle.lz4_block_decompress(blk, n) == data
    fits = oracle.lz4_block_compress(data)                  # into n - 1 bytes, as a frame's block has them: the same block, or stored
    assert fits == (blk if len(blk) <= n - 1 else None)
    seqs = P.parse_block(blk)
    assert sum(s[1] + s[3] for s in seqs) == n and seqs[-1][2:] == (0, 0)
    tseqs, found, refused = P.greedy_trace(data)
    assert tseqs == seqs, next((i, a, b) for i, (a, b) in enumerate(zip(tseqs + [None], seqs + [None])) if a != b)
    ctx = P.Ctx(data, seqs, found, refused, c["marks"], len(blk))
    assert c["features"]
    missing = [f for f in c["features"] if not P.FEATURES[f](ctx)]
    assert not missing, (name, missing)


def test_every_feature_is_claimed():
    claimed = {f for c in CASES for f in c["features"]}
    assert claimed == set(P.FEATURES), sorted(set(P.FEATURES) - claimed)
    want = (["lit=%d" % v for v in (0, 1, 14, 15, 16, 63, 64, 65, 269, 270, 271, 524, 525, 2047, 2048, 2049, 5000)] + ["lit>=960probes"]
            + ["ml=%d" % v for v in (4, 5, 15, 16, 17, 18, 19, 20, 273, 274, 275, 1023, 1024, 1025, 1027, 1028, 1029, 8200, 33000)]
            + ["wrap:%s=8192k%+d" % (e, v) for e in ("start", "end") for v in (-1, 0, 1)] + ["ml>whi"]
            + ["off=%d" % v for v in (1, 2, 3, 4, 7, 8, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 7167, 8191, 8192, 8208, 32767, 32768, 65534, 65535)]
            + ["off=wlo-1", "off=wlo+0", "off=wlo+1", "no-match@65536", "no-match@65540"]
            + ["catchup=%d" % v for v in (1, 2, 3, 4, 5, 20)] + ["catchup>=300", "catchup:anchor", "catchup:first-byte"]
            + ["bucket:hazard", "bucket:collision", "bucket:4th-byte"]
            + ["end:n-5", "end:cut", "end:n-13", "end:last-searched", "end:not-searched"]
            + ["n=%d" % v for v in (1, 4, 12, 13, 14, 17, 31)] + ["csize=n-2", "csize=n-1", "csize=n+0"]
            + ["dense:whole", "dense:100-then-ordinary", "dense:leaky", "dense:batch-ends", "dense:tail=111", "dense:tail=112", "dense:tail=113"])
    assert not [f for f in want if f not in claimed], "a feature of the issue's list has no case"
    star = (["lit=%d" % v for v in (0, 1, 14, 15, 16, 63, 64, 65)] + ["ml=%d" % v for v in (4, 5, 15, 16, 17, 18, 19, 20)]
            + ["off=%d" % v for v in (1, 2, 3, 4, 7, 8, 15, 16, 17)] + ["end:n-5", "end:cut", "end:n-13", "end:last-searched", "end:not-searched"])
    assert set(star) == P.STAR
    classes = ["262144", "65536"] + ["%d+%d" % (b, r) for b in (4096, 40000) for r in (0, 1, 5, 11, 12, 13, 15)]
    assert classes == P.CLASSES
    for cls in classes:
        n = sum(int(x) for x in cls.split("+"))
        have = {f for c in CASES if c["cls"] == cls and len(c["data"]) == n for f in c["features"]}
        assert not [f for f in star if f not in have], (cls, [f for f in star if f not in have])
    assert 80 <= len(CASES) <= 120 and max(len(c["data"]) for c in CASES) == 262144
    assert all((c["config"] != "") == (len(c["data"]) == 65536) for c in CASES)


def test_cases_are_deterministic():
    P._cases = None
    again = P.cases()
    assert [(c["name"], c["data"]) for c in again] == [(c["name"], c["data"]) for c in CASES]


def test_golden_digests(oracle):
    with open(GOLDEN) as f:
        G = json.load(f)["cases"]
    assert sorted(G) == sorted(NAMES)
    for c in CASES:
        g, blk = G[c["name"]], _block(oracle, c["data"])
        got = {"n": len(c["data"]), "sha256": hashlib.sha256(c["data"]).hexdigest(), "block_bytes": len(blk), "block_sha256": hashlib.sha256(blk).hexdigest()}
        assert got == g, c["name"]


def test_helpers_on_a_handmade_block():
    blk = bytes([0x52]) + b"abcde" + bytes([5, 0]) + bytes([0x50]) + b"vwxyz"        # 5 literals, 6 bytes from 5 back, 5 literals
    assert P.parse_block(blk) == [(0, 5, 5, 6), (11, 5, 0, 0)]
    other = bytes([0x53]) + b"abcde" + bytes([5, 0]) + bytes([0x40]) + b"wxyz"
    msg = P.first_difference(blk, other)
    assert "sequence 0" in msg and "pos 0 lit 5 off 5 ml 6" in msg and "pos 0 lit 5 off 5 ml 7" in msg, msg
    assert "same 2 sequences" in P.first_difference(blk, blk)
    assert P.hash5(b"\x00\x00\x00\x00\x00") == 0 and P.hash5(b"\x01\x00\x00\x00\x00abc") == (((1 << 24) * 889523592379) & (2 ** 64 - 1)) >> 52
    assert P.hash5(b"abcdeXYZ") == P.hash5(b"abcde") == P.hash5(int.from_bytes(b"abcdeQ", "little"))
    assert P.probe_positions(10, 67)[-3:] == [75, 77, 79]          # 65 probes a byte apart, then every second byte


def _ref():
    from oracle import ref
    if not ref.available():
        pytest.skip("oracle/_ref/libsqy_ref.so not available here")
    return ref


def test_oracle_is_liblz4_on_every_case(oracle):
    ref = _ref()
    for c in CASES:
        d = np.frombuffer(c["data"], np.uint8)
        assert oracle.lz4_block_compress(d) == ref.lz4_block(d), P.first_difference(oracle.lz4_block_compress(d) or b"", ref.lz4_block(d) or b"", ("oracle", "liblz4"))
        if len(d) >= 13:
            assert _block(oracle, d) == ref.lz4_block(d, cap=P.block_cap(len(d))), c["name"]
        cfg = oracle.Lz4Config(c["config"])
        chunk = cfg.bytes_per_chunk(len(d))
        assert np.array_equal(oracle.lz4_encode_chunked(d, cfg), ref.lz4_encode_parallel(d, chunk=chunk, block_id=cfg.block_id)), c["name"]
        assert np.array_equal(oracle.lz4_encode_serial(d, cfg), ref.lz4_encode_serial(d, framestep=chunk, block_id=cfg.block_id)), c["name"]
    big = np.frombuffer(b"".join(c["data"] for c in CASES if len(c["data"]) == 262144), np.uint8)
    cfg = oracle.Lz4Config("")
    assert np.array_equal(oracle.lz4_encode_chunked(big, cfg), ref.lz4_encode_parallel(big))
    assert np.array_equal(oracle.lz4_encode_serial(big, cfg), ref.lz4_encode_serial(big))
