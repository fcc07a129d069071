"""The duplicate search's fixture (dedupe_collisions.py) on the CPU: every case is what it says -- equal keys under the restatement of the
kernels' hash and bytes that differ exactly in the vectors named, the all-zero pieces where they are named -- and the oracle gives the two
chunks of every rejected pair different frames, so an encoder that takes one chunk for the other cannot produce the oracle's blob.
(test_gpu_dedupe_collisions.py asserts that the restated keys are the kernels'.)  No case is skipped: one that does not collide is a bug
in the fixture."""
import numpy as np
import pytest

import dedupe_collisions as DC


@pytest.fixture(scope="module", params=DC.CHUNKS, ids=["%dk" % (c >> 10) for c in DC.CHUNKS])
def fixture(request):
    chunk = request.param
    stream, cases = DC.plane_streams(chunk)
    return chunk, stream, cases, DC.chunk_keys(stream, chunk)


def test_solvers_against_a_scalar_restatement():
    """the vectorised restatement and the solvers against the hash written out lane by lane in Python integers"""
    rng = np.random.default_rng(5)
    piece = rng.integers(0, 256, 1024, dtype=np.uint8)
    piece[256:512] = 0                                                  # row 1 all zero: its marker
    d = piece.view("<u4").reshape(64, 4)
    want = []
    for r in range(4):
        s = 0
        for lane in range(16 * r, 16 * r + 16):
            a = sum(int(d[lane, i]) * DC.C[i] for i in range(4)) & DC.M
            s = (s + (a ^ (a >> 15)) * (2 * lane + 1)) & DC.M
        want.append((s | 1) if d[16 * r:16 * r + 16].any() else 0)
    assert DC.piece_hashes(piece).tolist() == [want]
    for lane, slot, term in ((0, 0, 1), (5, 0, 0x1234567a), (37, 3, 0xffffffff), (63, 2, 0x80000000)):
        p = np.zeros(256, dtype="<u4")
        p[lane * 4 + slot] = DC.solve_dword(term, lane, slot)
        q = DC.piece_hashes(p.view(np.uint8))[0].tolist()
        assert q[lane // 16] == term | 1 and sum(q) == term | 1
    assert DC.piece_hashes(DC.vanishing_piece(range(1, 65))).tolist() == [[1, 1, 1, 1]]
    assert DC.chunk_keys(np.zeros(4096, np.uint8), 2048).tolist() == [1, 1]


def test_every_case_is_what_it_says(fixture):
    chunk, stream, cases, keys = fixture
    n = chunk >> 10
    per = DC.chunks_per_plane(chunk)
    assert stream.size == 16 * per * chunk and stream.size <= 8 << 20
    body = lambda c: stream[c * chunk:(c + 1) * chunk]
    for c in cases:
        k, r = c["k"], c["r"]
        a, b = body(k), body(r)
        assert r <= k and keys[k] == keys[r], (c["name"], "the keys differ: the case does not collide")
        assert r == int(np.flatnonzero(keys == keys[k])[0]), (c["name"], "r is not the first chunk with this key")
        differ = np.flatnonzero((a != b).reshape(-1, 16).any(axis=1)).tolist()
        assert differ == c["vectors"], (c["name"], "the bytes differ elsewhere than said")
        assert bool(differ) == (c["kind"] == "reject"), c["name"]
        for buf, zp in ((a, c["holes_k"]), (b, c["holes_r"])):
            assert [p for p in range(n) if not buf[p * 1024:(p + 1) * 1024].any()] == zp, c["name"]
        if c["kind"] == "zero":
            assert keys[k] == 1 and len(c["holes_k"]) == n
        if c["kind"] == "alone":
            assert r == k
        if c["name"].startswith("nearly zero"):
            assert keys[k] != 1 and len(c["holes_k"]) == n - 1 and int(np.unpackbits(a).sum()) == 1
    # the expected decisions: rejected chunks are their own, accepted ones their twin's -- whatever else shares the key
    dup = DC.expected_dup_of(stream, chunk)
    for c in cases:
        assert dup[c["k"]] == (c["k"] if c["kind"] in ("reject", "alone") else c["r"]), c["name"]


def test_the_fixture_holds_what_the_compares_need(fixture):
    chunk, stream, cases, keys = fixture
    n, per = chunk >> 10, DC.chunks_per_plane(chunk)
    rej = [c for c in cases if c["kind"] == "reject"]
    names = " | ".join(c["name"] for c in rej)
    for cls in ("class 0", "class 2", "class 3", "class 4 zero-sum piece against a hole, hole first", "class 4 zero-sum piece against a hole, zero sum first",
                "C == B", "noise+holes linear"):
        assert cls in names, cls
    # every edge of the two loops, by a chunk that differs from the first of its key in that one vector
    for family in ("noise+holes",) + (("soft+holes",) if per == 8 else ()):
        single = {c["vectors"][0] for c in rej if c["name"].startswith(family + " linear")}
        nvec = chunk >> 4
        want = {0, nvec - 1, 255, 256, 1023} | ({1024} if nvec > 1024 else set())
        want |= {p * 64 + lane for p, lane in DC.positions(chunk)}
        assert {v >> 6 for v in want} >= set(range(4)) | set(range(n - 4, n)) and single == want, family
    # holes next to a difference, holes that ARE the difference (one side only), and equal chunks with holes
    assert any(c["holes_k"] and c["holes_k"] == c["holes_r"] for c in rej)
    assert any(set(c["holes_k"]) - set(c["holes_r"]) for c in rej) and any(set(c["holes_r"]) - set(c["holes_k"]) for c in rej)
    assert any(c["kind"] == "accept" and c["holes_k"] and c["k"] - c["r"] > 1 for c in cases)
    # the two chunks of a pair next to each other in one bit plane, and in different planes
    assert any(c["k"] == c["r"] + 1 and c["k"] // per == c["r"] // per for c in rej)
    assert any(c["k"] // per != c["r"] // per for c in rej)
    spots = DC.nearly_zero_spots(chunk)
    assert len([c for c in cases if c["name"].startswith("nearly zero")]) == len(spots) == (64 if per == 8 else 4)
    for i, values in enumerate(((0, n - 1), None, (0, 3), (0, 31))):
        if values:
            assert {s[i] for s in spots} == set(values)
    assert {s[1] % 16 for s in spots} == {0, 15} and {s[1] // 16 for s in spots} == {0, 1, 2, 3}
    assert sum(c["kind"] == "zero" for c in cases) >= 2


@pytest.mark.parametrize("accel", [None, -1], ids=["accel1", "accel2"])
def test_a_false_duplicate_changes_the_blob(oracle, fixture, accel):
    """the frames of the two chunks of every rejected pair differ in the oracle's blob; stored and compressed frames both occur among them"""
    from digest_planes import frame_kinds
    chunk, stream, cases, keys = fixture
    pipe = "bitswap1->lz4" + DC.lz4_config(chunk, accel)
    vol = oracle.bitswap1_decode(stream.view(np.uint16)).reshape(1, 1, -1)
    assert np.array_equal(oracle.bitswap1_encode(vol).reshape(-1).view(np.uint8), stream)
    blob = oracle.pipeline_encode(pipe, vol, nthreads=2)
    payload = blob[oracle.header_unpack(blob)["size"]:]
    fr = DC.frames(payload)
    stored = frame_kinds(payload)
    assert len(fr) == stream.size // chunk
    seen = set()
    for c in cases:
        same = fr[c["k"]] == fr[c["r"]]
        assert same == (c["kind"] != "reject"), (c["name"], "the oracle's frames of chunks %d and %d" % (c["k"], c["r"]))
        if c["kind"] == "reject":
            seen.add(stored[c["k"]])
    assert seen == {True, False}
