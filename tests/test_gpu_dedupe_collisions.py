"""GPU: the duplicate-chunk search on chunks built to share a key (dedupe_collisions.py; the fixture's own claims: test_dedupe_fixture.py).
The search nominates by key and decides by a byte compare -- lz4_chunk_dedupe inside the parse wavefront (frames in place, acceleration 1),
lz4_dedupe_verify_kernel otherwise, with the holes map (frames in place: all-zero 1 KiB pieces are never written, their markers stand for
them) or without (the ordinary path).  Honest data never makes that compare say "different"; every rejected pair here does, with the
difference at each edge of the two loops, inside a hole, next to holes, and over whatever an earlier call left under the holes.
Per chunk size and path, with option dedupe_report on:
  1 the blob is the oracle's, byte for byte, and decodes to the voxels (a false duplicate swaps one chunk's frame for another's)
  2 the keys the GPU reports are the restated keys (or the fixture would stop colliding, and this test pass for nothing)
  3 the reported dup_of is the one computed from keys and bytes (a missed duplicate does not show in the blob)."""
import numpy as np
import pytest

import dedupe_collisions as DC

pytestmark = pytest.mark.gpu

PATHS = ("fused", "verify_holes", "verify_plain")


@pytest.fixture(scope="module", params=DC.CHUNKS, ids=["%dk" % (c >> 10) for c in DC.CHUNKS])
def planted(request, oracle):
    chunk = request.param
    stream, cases = DC.plane_streams(chunk)
    voxels = lambda s: oracle.bitswap1_decode(s.view(np.uint16)).reshape(1, 1, -1)      # voxels whose bit planes are that stream
    vol = voxels(stream)
    want = {accel: oracle.pipeline_encode("bitswap1->lz4" + DC.lz4_config(chunk, accel), vol, nthreads=2) for accel in (None, -1)}
    # what the destination holds before the call: another call's leftovers -- noise, and the bytes that would make a rejected pair look equal
    stale = (np.random.default_rng(3).integers(0, 65536, vol.shape, dtype=np.uint16), voxels(DC.stale_twin(stream, chunk, cases)))
    return dict(chunk=chunk, stream=stream, cases=cases, vol=vol, want=want, stale=stale, keys=DC.chunk_keys(stream, chunk),
                dup_of=DC.expected_dup_of(stream, chunk))


def _about(planted, chunks):
    """the cases that chunks `chunks` belong to: name, the two chunks, where they differ"""
    out = []
    for c in planted["cases"]:
        if c["k"] in chunks or c["r"] in chunks:
            where = ["piece %d lane %d" % (v >> 6, v & 63) for v in c["vectors"][:4]] + (["..."] if len(c["vectors"]) > 4 else [])
            out.append("%s: chunk %d against chunk %d, %s; differ in %s" % (c["name"], c["k"], c["r"], c["kind"], ", ".join(where) or "nothing"))
    return out[:12]


def _wrong_frames(got, want, oracle):
    """chunks whose frame in `got` is not the oracle's (None: `got` is no sequence of frames any more)"""
    try:
        a, b = DC.frames(got[oracle.header_unpack(got)["size"]:]), DC.frames(want[oracle.header_unpack(want)["size"]:])
    except Exception:
        return None
    return [k for k in range(max(len(a), len(b))) if k >= len(a) or k >= len(b) or a[k] != b[k]]


@pytest.mark.parametrize("path", PATHS)
def test_built_collisions(sqy, oracle, options, planted, path):
    import torch
    dev = torch.device("cuda", 0)
    chunk, vol = planted["chunk"], planted["vol"]
    accel = -1 if path == "verify_holes" else None
    pipe = "bitswap1->lz4" + DC.lz4_config(chunk, accel)
    want = planted["want"][accel]
    in_place = path != "verify_plain"
    cap = sqy.max_compressed_length(pipe, vol.shape, np.uint16) if in_place else len(want) + 64
    out = torch.full((cap,), 0xA5, dtype=torch.uint8, device=dev)
    d_vol = torch.from_numpy(vol.copy()).to(dev)
    options("dedupe_report", 1)
    for which, before in enumerate(planted["stale"] if in_place else (None,)):
        tag = "%d KiB, %s, destination used before by %s" % (chunk >> 10, path, ("noise", "the pairs' twins", "nobody")[which if in_place else 2])
        if before is not None:
            d_before = torch.from_numpy(before).to(dev)
            rc, off, n = sqy.encode_device_at(pipe, d_before.data_ptr(), vol.shape, np.uint16, out.data_ptr(), cap, nthreads=2)
            assert rc == 0 and off > 0, tag
        options("dedupe_report", 1)                                                  # (drops the record of the call before)
        rc, off, n = sqy.encode_device_at(pipe, d_vol.data_ptr(), vol.shape, np.uint16, out.data_ptr(), cap, nthreads=2)
        assert rc == 0 and 0 <= off and off + n <= cap, tag
        assert (off > 0) == in_place, (tag, "not the path this test is about")
        got = bytes(out[off:off + n].cpu().numpy().tobytes())
        keys, dup_of = sqy.dedupe_report()
        assert keys.size == dup_of.size == planted["keys"].size, (tag, "no report of this call")
        # 2: the fixture is tied to the kernels
        bad = np.flatnonzero(keys != planted["keys"]).tolist()
        assert not bad, (tag, "assertion 2: the reported keys are not the restated ones in chunks", bad[:16], _about(planted, bad))
        # 3: rejects and accepts alike
        bad = np.flatnonzero(dup_of != planted["dup_of"]).tolist()
        assert not bad, (tag, "assertion 3: dup_of (chunk, reported, expected)", [(k, int(dup_of[k]), int(planted["dup_of"][k])) for k in bad[:16]],
                         _about(planted, bad))
        # 1: the blob
        if got != want:
            bad = _wrong_frames(got, want, oracle)
            assert False, (tag, "assertion 1: the blob differs from the oracle's; frames of chunks", bad if bad is None else bad[:16],
                           _about(planted, bad or []))
        rc, back = sqy.decode(got)
        assert rc == 0 and np.array_equal(back, vol), (tag, "assertion 1: the blob does not decode to the voxels")
